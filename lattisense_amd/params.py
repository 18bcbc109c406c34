"""Default FHE parameter sets (data only).

Prime chains are the reference's published parameter data: frontend/parameter.json (BFV/CKKS default sets)
and frontend/custom_task.py:387-420 (CKKS bootstrap chain N16QP1546H192H32).  All moduli are prime and
== 1 (mod 2N) (checked in tests/test_params.py).
"""

BFV_DEFAULT = {
    4096: {'t': 65537, 'q': [549755731969, 549755904001], 'p': [1073750017]},
    8192: {'t': 65537, 'q': [18014398508400641, 18014398510645249, 18014398510661633], 'p': [36028797018652673]},
    16384: {'t': 65537, 'q': [72057594038321153, 36028797019389953, 36028797019488257, 18014398508400641, 18014398510661633, 18014398508138497], 'p': [36028797020209153, 36028797017456641]},
    32768: {'t': 65537, 'q': [576460752301785089, 576460752301391873, 576460752300015617, 288230376154267649, 288230376155185153, 288230376155250689, 288230376147582977, 288230376147386369, 288230376147320833, 288230376156758017, 288230376157413377, 288230376158396417], 'p': [1152921504606584833, 1152921504608747521, 1152921504614055937]},
}

CKKS_DEFAULT = {
    4096: {'scale': 4294967296.0, 'slots': 2048, 'q': [137439010817, 4294991873], 'p': [274877816833]},
    8192: {'scale': 1073741824.0, 'slots': 4096, 'q': [8589852673, 1073692673, 1073643521, 1073872897, 1073971201, 1073479681], 'p': [34359754753]},
    16384: {'scale': 17179869184.0, 'slots': 8192, 'q': [35184372121601, 17179967489, 17179672577, 17180262401, 17180295169, 17179410433, 17180393473, 17180557313, 17180950529, 17178525697], 'p': [8796092858369, 8796092792833]},
    32768: {'scale': 1099511627776.0, 'slots': 16384, 'q': [1125899908022273, 1099512938497, 1099510054913, 1099514314753, 1099507695617, 1099515691009, 1099516280833, 1099516542977, 1099506515969, 1099516870657, 1099518246913, 1099504549889, 1099503894529, 1099503370241, 1099502714881, 1099520606209, 1099502518273, 1099521458177], 'p': [1125899908612097, 1125899904679937, 1125899909398529]},
    65536: {'scale': 35184372088832.0, 'slots': 32768, 'q': [36028797019488257, 35184372744193, 35184373006337, 35184368025601, 35184376545281, 35184377331713, 35184378511361, 35184365273089, 35184379035649, 35184363569153, 35184380870657, 35184382967809, 35184383229953, 35184383754241, 35184388734977, 35184353083393, 35184351772673, 35184350330881, 35184394240001, 35184346267649, 35184398958593, 35184345088001, 35184399351809, 35184343908353, 35184404070401, 35184339320833, 35184337354753, 35184410361857, 35184333684737, 35184411279361], 'p': [36028797023420417, 36028797014376449, 36028797024206849, 36028797013327873]},
}

CKKS_BOOTSTRAP_65536 = {'scale': 1099511627776.0, 'q': [1152921504614055937, 1099512938497, 1099510054913, 1099507695617, 1099515691009, 1099506515969, 1099516870657, 1099504549889, 1099503894529, 1099503370241, 549754109953, 549753978881, 549753716737, 1152921504598720513, 1152921504615628801, 1152921504597016577, 1152921504616808449, 1152921504595968001, 1152921504618381313, 1152921504620347393, 1152921504592822273, 72057594038321153, 72057594036879361, 72057594035306497, 72057594040680449], 'p': [2305843009211596801, 2305843009210023937, 2305843009208713217, 2305843009202159617, 2305843009201242113]}


# ---- N = 2^17 deep chain (BASELINE configs[4]).  The reference ships no parameter set for it: its bootstrap primes are
# == 1 mod 2^17 only, so a chain with the same shape as CKKS_BOOTSTRAP_65536 (one 60-bit prime, 24 scale
# primes, five 61-bit special primes) is generated here: the largest NTT primes (== 1 mod 2^18) below 2^60, 2^45 and 2^61.
def _is_prime(n):
    if n < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in small:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in small:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def ntt_primes_below(bits, n, count, avoid=()):
    """the `count` largest primes p < 2^bits with p == 1 (mod 2n), skipping `avoid`"""
    out, step = [], 2 * n
    x = (1 << bits) + 1
    while len(out) < count:
        x -= step
        if x > 1 and x not in avoid and _is_prime(x):
            out.append(x)
    return out


def ckks_n17_chain():
    n = 1 << 17
    p = ntt_primes_below(61, n, 5)
    q0 = ntt_primes_below(60, n, 1)
    q = q0 + ntt_primes_below(45, n, 24)
    return {"n": n, "scale": float(1 << 45), "q": q, "p": p}


# ---- BFV at N = 2^16 (BASELINE north_star: BFV HMult + relin at N = 2^16).  The reference ships no BFV set above N = 2^15,
# so this chain is generated the same way: 24 Q primes of 59 bits and 4 special primes of 60 bits, all == 1 mod 2^17.
def bfv_n16_chain():
    """BFV chain for N = 2^16: Q = 24 x 59-bit primes (1416 bits), P = 4 x 60-bit primes, log QP = 1656 bits.

    Security: the 128-bit bound used is Lattigo's PN16QP1761 default set (log QP <= 1761 at N = 2^16, ternary secret),
    itself taken from the HomomorphicEncryption.org security standard tables; it was not re-derived here.
    t = 786433 = 3 * 2^18 + 1 is prime and == 1 mod 2N, so the plaintext ring batches (65537 does not at N = 2^16).
    The Q -> QMul extension of a multiply at the top level has 24 source limbs (the wide base conversion).
    """
    n = 1 << 16
    p = ntt_primes_below(60, n, 4)
    q = ntt_primes_below(59, n, 24, avoid=p)
    return {"n": n, "t": 786433, "q": q, "p": p}
