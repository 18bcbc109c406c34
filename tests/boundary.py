"""Test helpers for the modulus-size thresholds: chains whose primes sit on both sides of every bit length at which a kernel
switches its arithmetic (46, 47, 48, 57, 58 bits, and the 61-bit ceiling), and worst-case residue patterns for operands
and keys.  Used by tests/test_gpu_boundary.py and the CPU replay tests."""
import numpy as np

from lattisense_amd import params

THRESHOLD_BITS = (46, 47, 48, 57, 58)
ORDERS = ("ascending", "descending", "interleaved")
PATTERNS = ("zero", "max", "one", "half", "alt", "alt1", "delta", "top", "uniform")


def primes_above(bits, n, count, avoid=()):
    """the `count` smallest primes p > 2^bits with p == 1 (mod 2n), skipping `avoid`"""
    out, step = [], 2 * n
    x = (1 << bits) + 1
    while len(out) < count:
        x += step
        if x not in avoid and params._is_prime(x):
            out.append(x)
    return out


def fp_engine(q):
    """the FP64-FMA butterfly engine takes the limb (LSA_FP64_MAX_BITS = 47)"""
    return q >> 47 == 0


def head_flags(ql, qi):
    """(near, fp_lift) of the rescale / ModDown head for target prime qi and dropped prime ql (ntt_make_load_fix)"""
    return ql <= 2 * qi, fp_engine(qi) and ql >> 48 == 0


def straddle_chain(n, np_, order="ascending"):
    """Q: for every bit length in THRESHOLD_BITS the largest NTT prime below 2^bits and the smallest above it, plus the largest
    60-bit prime, one 30-bit and one 40-bit prime (13 primes); P: the np_ largest primes below 2^61.
    order: ascending / descending by size, or interleaved (small and large alternate), so that over the levels every size
    class is dropped onto both smaller and larger targets."""
    q = []
    for b in THRESHOLD_BITS:
        q += params.ntt_primes_below(b, n, 1) + primes_above(b, n, 1)
    q += params.ntt_primes_below(60, n, 1) + params.ntt_primes_below(30, n, 1) + params.ntt_primes_below(40, n, 1)
    q = sorted(q)
    assert len(set(q)) == 13
    if order == "descending":
        q = q[::-1]
    elif order == "interleaved":
        lo, hi = q[:7], q[7:][::-1]
        q = [x for pair in zip(lo, hi + [None]) for x in pair if x is not None]
    else:
        assert order == "ascending", order
    p = params.ntt_primes_below(61, n, np_)
    assert all((m - 1) % (2 * n) == 0 and params._is_prime(m) for m in q + p) and not set(q) & set(p)
    # every size class present
    for lo, hi in ((46, 47), (47, 48), (48, 49), (57, 58)):
        assert any((1 << lo) < m < (1 << hi) for m in q), (lo, hi)
    assert any(m > (1 << 58) for m in q)
    assert any(m < (1 << 46) and m.bit_length() == 46 for m in q)
    # both values of both head selectors over the levels, on both engines where the engine can take it
    seen = {head_flags(q[l], q[i]) + (fp_engine(q[i]),) for l in range(1, len(q)) for i in range(l)}
    if order == "descending":   # every dropped limb is the smallest: only near, and fp_lift wherever the target is FP64
        assert seen == {(True, True, True), (True, False, False)}
        return {"n": n, "q": q, "p": p}
    assert {s[0] for s in seen} == {True, False}, "near"
    assert {s[1] for s in seen} == {True, False}, "fp_lift"
    assert {s[1] for s in seen if s[2]} == {True, False}, "fp_lift on and off for FP64-engine targets"
    if order == "ascending":
        assert {(s[0], s[2]) for s in seen} == {(a, b) for a in (True, False) for b in (True, False)}, "near x engine"
    return {"n": n, "q": q, "p": p}


def is_ceiling(m):
    """eight products of residues fit under the lazy REDC's bound m 2^64, nine of the largest do not"""
    return 8 * (m - 1) ** 2 < (m << 64) < 9 * (m - 1) ** 2


def ceiling_chain(n, nq, np_):
    """P: the np_ largest NTT primes below 2^61, Q: the next nq largest.  Every prime is at the ceiling of the
    multiply-accumulate kernels: 8 (q - 1)^2 < q 2^64 < 9 (q - 1)^2, so a sum of nine products of the largest residues has
    left the range the lazy REDC is written for, and a fold that comes one term late shows."""
    pr = params.ntt_primes_below(61, n, nq + np_)
    p, q = pr[:np_], pr[np_:]
    assert len(set(pr)) == nq + np_ and all(params._is_prime(m) and (m - 1) % (2 * n) == 0 and m >> 61 == 0 for m in pr)
    assert all(is_ceiling(m) for m in pr), [m for m in pr if not is_ceiling(m)]
    return {"n": n, "q": q, "p": p}


def ceiling_mixed_chain(n, np_):
    """Q alternates ceiling primes with the 30-, 40-, 47- and 48-bit classes of straddle_chain (9 primes, a ceiling prime at
    every even position, the largest small primes first); P: the np_ largest primes below 2^61.  Over the levels a 61-bit limb
    is dropped onto 61-bit targets (near) and onto small ones (not near), and a small limb onto 61-bit targets."""
    pr = params.ntt_primes_below(61, n, np_ + 5)
    p, big = pr[:np_], pr[np_:]
    small = [params.ntt_primes_below(b, n, 1)[0] for b in (48, 47, 40, 30)]
    q = [x for pair in zip(big, small + [None]) for x in pair if x is not None]
    assert len(set(q + p)) == 9 + np_ and all(params._is_prime(m) and (m - 1) % (2 * n) == 0 for m in q + p)
    assert all(is_ceiling(m) for m in big + p) and [m.bit_length() for m in small] == [48, 47, 40, 30]
    drops = {(is_ceiling(q[l]), is_ceiling(q[i])) + head_flags(q[l], q[i]) for l in range(1, len(q)) for i in range(l)}
    assert (True, True, True, False) in drops, "a 61-bit limb dropped onto a 61-bit target: near"
    assert any(d[:3] == (True, False, False) for d in drops), "a 61-bit limb dropped onto a small target: not near"
    assert any(d[:2] == (False, True) and d[2] for d in drops), "a small limb dropped onto a 61-bit target"
    assert {d[3] for d in drops} == {True, False}, "fp_lift"
    return {"n": n, "q": q, "p": p}


# ---------------------------------------------------------------- BFV chains (tests/test_gpu_boundary.py, the operator-chain tests)

def bfv_mixed_chain(n):
    """FP64-size primes (46/47/48-bit) next to 57/58/59-bit ones: the narrow-split predicate of the base conversions is false
    although some sources are below 2^58; P: two 61-bit primes"""
    q = (params.ntt_primes_below(46, n, 1) + params.ntt_primes_below(59, n, 1) + params.ntt_primes_below(47, n, 1) +
         primes_above(57, n, 1) + primes_above(47, n, 1) + params.ntt_primes_below(58, n, 1) + params.ntt_primes_below(57, n, 1) +
         primes_above(46, n, 1))
    return q, params.ntt_primes_below(61, n, 2)


def bfv_fp_chain(n):
    """every limb on the FP64 butterfly engine.  Q: the two largest NTT primes below 2^47, the largest below 2^46 and the smallest
    above 2^45; P: the next two primes below 2^47"""
    top = params.ntt_primes_below(47, n, 4)
    q = top[:2] + params.ntt_primes_below(46, n, 1) + primes_above(45, n, 1)
    p = top[2:]
    assert len(set(q + p)) == 6 and all(fp_engine(m) and params._is_prime(m) and (m - 1) % (2 * n) == 0 for m in q + p), (q, p)
    assert [m.bit_length() for m in q] == [47, 47, 46, 46] and all(m.bit_length() == 47 for m in p), (q, p)
    return q, p


BFV_OPERATOR_CHAINS = ("fp", "mixed", "ceiling")
BFV_OPERATOR_T = 65537


def bfv_operator_chain(kind, n):
    """(q, p) of the three chains the BFV operators are held to (tests/test_gpu_bfv_operator_chains.py):
    fp       bfv_fp_chain: 4 Q + 2 P, all six on the FP64 engine;
    mixed    the first six Q limbs of bfv_mixed_chain (46, 59, 47, 58, 48 and 58 bits) with its two 61-bit P: both engines in
             every launch over Q u P;
    ceiling  ceiling_chain(n, 4, 2): six primes just below 2^61, none on the FP64 engine.
    The special primes come in pairs, so a level with an odd number of limbs ends its decomposition in a digit of one limb."""
    if kind == "fp":
        return bfv_fp_chain(n)
    if kind == "mixed":
        q, p = bfv_mixed_chain(n)
        q = q[:6]
        assert any(fp_engine(m) for m in q) and any((1 << 47) < m < (1 << 48) for m in q)
        assert any(m.bit_length() in (58, 59) for m in q) and all(m.bit_length() == 61 for m in p) and len(p) == 2
        return q, p
    assert kind == "ceiling", kind
    C = ceiling_chain(n, 4, 2)
    return C["q"], C["p"]


def digit_sizes(level, np_):
    """limbs per key-switch digit at `level` with np_ special primes"""
    L = level + 1
    return [min(np_, L - d) for d in range(0, L, np_)]


def lift_level(q, p):
    """the highest level below the top whose last digit is exactly one limb: the digit the ModUp lift applies to (when that limb
    is below 2^53)"""
    for level in range(len(q) - 2, -1, -1):
        if digit_sizes(level, len(p))[-1] == 1:
            return level
    raise AssertionError("no level with a single-limb last digit")


def pattern(name, q, n, rng):
    """one limb-polynomial of n residues modulo q"""
    q = int(q)
    h = q // 2
    v = np.zeros(n, dtype=np.uint64)
    if name == "zero":
        pass
    elif name == "max":
        v[:] = q - 1
    elif name == "one":
        v[:] = 1
    elif name == "half":          # floor(q/2), floor(q/2) + 1 interleaved: the centred-remainder compare of the rescale head
        v[0::2] = h
        v[1::2] = h + 1
    elif name == "alt":
        v[0::2] = q - 1
    elif name == "alt1":          # the shifted variant
        v[1::2] = q - 1
    elif name == "delta":
        v[[0, 1, n // 2, n - 1]] = q - 1
    elif name == "top":
        v[:] = np.uint64(q - 1) - rng.integers(0, 4, size=n, dtype=np.uint64)
    elif name == "uniform":
        v[:] = rng.integers(0, q, size=n, dtype=np.uint64)
    else:
        raise ValueError(name)
    return v


def pattern_ct(names, mods, polys, n, rng, oracle=None):
    """[len(names)][polys][len(mods)][n]: batch slot b carries pattern names[b] in every limb.  With `oracle`, the pattern
    is the coefficient-domain content and the words returned are its forward transform (limb i is oracle modulus i)."""
    out = np.empty((len(names), polys, len(mods), n), dtype=np.uint64)
    for b, name in enumerate(names):
        for pl in range(polys):
            for i, m in enumerate(mods):
                v = pattern(name, m, n, rng)
                out[b, pl, i] = oracle.ntt(i, v) if oracle is not None else v
    return out


def pattern_key(name, mods, beta, n, rng):
    """a switching key [beta][2][len(mods)][n] whose every limb carries the pattern"""
    return pattern_ct([name] * beta, mods, 2, n, rng)


# ---------------------------------------------------------------- the long sums at the ceiling (tests/test_gpu_ceiling.py, cases A and B)

CEILING_SLOTS = ("top", "uniform", "top")     # the batch: two worst-case slots around a uniform control
MAC_TERMS = (8, 9, 16, 17, 33)                # on both sides of the fold at 8, of the launch bound 16, and two launches + 1
DOT_TERMS = (4, 5, 8, 9, 16, 17, 33)          # ... and of d1's fold at 4
CEILING_LOGN = {8: 12, 9: 13, 16: 12, 17: 13, 33: 12, 4: 12, 5: 13}   # the ring each term count runs at


def ceiling_mac_operands(logn):
    """case A: ceiling_chain with 4 Q limbs; three ciphertext batches [3][2][4][N] and four plaintext batches [3][4][N] in the
    CEILING_SLOTS patterns, the addend all q - 1.  Term i of a sum multiplies ciphertext i % 3 by plaintext i % 4; every third
    plaintext (i % 3 == 2) is batch item 0 for the whole batch."""
    n = 1 << logn
    C = ceiling_chain(n, 4, 1)
    rng = np.random.default_rng(6100 + logn)
    cts = [pattern_ct(CEILING_SLOTS, C["q"], 2, n, rng) for _ in range(3)]
    pts = [pattern_ct(CEILING_SLOTS, C["q"], 1, n, rng)[:, 0] for _ in range(4)]
    addend = pattern_ct(("max",) * len(CEILING_SLOTS), C["q"], 2, n, rng)
    return C, cts, pts, addend


def mac_term(i):
    """(ciphertext, plaintext, shared) of term i"""
    return i % 3, i % 4, i % 3 == 2


def ceiling_dot_operands(logn):
    """case B: the same chain; three a and three b ciphertext batches; term i is a[i % 3] (x) b[(2 i + 1) % 3] (nine pairs)"""
    n = 1 << logn
    C = ceiling_chain(n, 4, 1)
    rng = np.random.default_rng(6200 + logn)
    As = [pattern_ct(CEILING_SLOTS, C["q"], 2, n, rng) for _ in range(3)]
    Bs = [pattern_ct(CEILING_SLOTS, C["q"], 2, n, rng) for _ in range(3)]
    addend = pattern_ct(("max",) * len(CEILING_SLOTS), C["q"], 2, n, rng)
    return C, As, Bs, addend


def dot_term(i):
    return i % 3, (2 * i + 1) % 3
