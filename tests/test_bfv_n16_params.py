"""The BFV chain for N = 2^16 (params.bfv_n16_chain): prime sizes, batching plaintext modulus, the security budget it is
quoted against, and the auxiliary basis of its multiply -- 24 limbs, so both base conversions of a top-level multiply have
24 sources (the wide conversion of kernels.hip)."""
from lattisense_amd import params
from oracle.pyoracle import Oracle, lib


def test_bfv_n16_chain_shape():
    c = params.bfv_n16_chain()
    n, q, p, t = c["n"], c["q"], c["p"], c["t"]
    assert n == 1 << 16
    assert len(q) == 24 and len(p) == 4
    assert len(set(q + p)) == 28
    L = lib()
    for m in q + p:
        assert L.ora_is_prime(m) and m % (1 << 17) == 1
    assert all(m.bit_length() == 59 for m in q)
    assert all(m.bit_length() == 60 for m in p)
    assert L.ora_is_prime(t) and t % (2 * n) == 1
    assert sum(m.bit_length() for m in q + p) == 1656 <= 1761


def test_bfv_n16_aux_basis():
    c = params.bfv_n16_chain()
    n, q, p, t = c["n"], c["q"], c["p"], c["t"]
    o = Oracle(n, q, p, t)
    # bfv_aux_count: (bits(Q) + log N + 60) // 61 limbs of 61-bit primes, the largest NTT primes below 2^61 not in Q or P
    qprod = 1
    for m in q:
        qprod *= m
    assert len(o.aux) == (qprod.bit_length() + 16 + 60) // 61 == 24
    assert o.aux == params.ntt_primes_below(61, n, 24, avoid=q + p)
    assert o.mod == q + p + o.aux
