"""CPU restatement of the BFV coefficient packing (lattisense_amd/csrc/bfv_pack.h and bfv_pack.hip; include/lattisense_amd.h:
lsa_bfv_pack_*) as the composition the header names: per node the numpy negacyclic shift by +s (tests/bfv_expand_model.py
mul_monomial), Oracle.vec add and sub on both polynomials, Oracle.bfv_rotate, and Oracle.vec add.  The plan is restated here as well
(levels_of, nodes_of, trace_elements_of, galois_elements_of, keyswitches_of)."""
import numpy as np

from tests.bfv_expand_model import _each, levels_of, mul_monomial


def nodes_of(n_ring, count):
    """[(g, s, nodes, paired nodes)] per level, j = k-1 down to 0"""
    k = levels_of(count)
    out = []
    for j in range(k - 1, -1, -1):
        l = k - j
        out.append(((1 << l) + 1, n_ring >> l, 1 << j, min(1 << j, count - (1 << j))))
    return out


def trace_elements_of(n_ring, count, trace):
    if not trace:
        return []
    return [(1 << l) + 1 for l in range(levels_of(count) + 1, n_ring.bit_length())]


def galois_elements_of(n_ring, count, trace):
    top = n_ring.bit_length() - 1 if trace else levels_of(count)
    return [(1 << l) + 1 for l in range(1, top + 1)]


def keyswitches_of(n_ring, count, trace):
    return (1 << levels_of(count)) - 1 + len(trace_elements_of(n_ring, count, trace))


def factor_of(n_ring, count, trace):
    return n_ring if trace else 1 << levels_of(count)


def pack(o, key_of, key_level, cts, level, trace):
    """cts [count][2][level+1][N] coefficient domain -> (the result [2][level+1][N], the list c after every level but the last ran
    in place: what the input array holds afterwards, entry 0 being the state before the last step); key_of(g): the Galois key of g
    exported at key_level"""
    count = len(cts)
    c = [np.array(x, dtype=np.uint64) for x in cts]
    steps = [(g, s, nodes, n_pair) for g, s, nodes, n_pair in nodes_of(o.n, count)] + [(g, 0, 1, 0) for g in trace_elements_of(o.n, count, trace)]
    before_last = c[0]
    for g, s, nodes, n_pair in steps:
        before_last = c[0]
        for a in range(nodes):
            if a < n_pair:
                xb = mul_monomial(o, c[a + nodes], s)
                u, v = _each(o, "add", c[a], xb), _each(o, "sub", c[a], xb)
            else:
                u = v = c[a]
            c[a] = _each(o, "add", u, o.bfv_rotate(level, v, g, key_of(g), key_level))
    left = [before_last] + c[1:]
    return c[0], left


def encrypt_constant_terms(client, values, level, rng):
    """one ciphertext per value: a random polynomial mod t whose coefficient 0 is the value -> (the coefficients, the ciphertext)"""
    from tests.bfv_expand_model import encrypt_coeffs
    t, n = client.o.t, client.o.n
    out = []
    for v in values:
        m = rng.integers(0, t, n)
        m[0] = int(v) % t
        out.append((m, encrypt_coeffs(client, m, level)))
    return out


def expected_positions(values, n_ring, count, trace, t):
    """(positions, what they hold): coefficient i * N / 2^k holds F * values[i]"""
    step = n_ring >> levels_of(count)
    f = factor_of(n_ring, count, trace)
    return np.arange(count) * step, np.array([int(v) * f % t for v in values], dtype=np.int64)
