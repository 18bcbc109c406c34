"""CPU restatement of the BFV oblivious expansion (lattisense_amd/csrc/bfv_expand.h and bfv_expand.hip; include/lattisense_amd.h:
lsa_bfv_expand_*) as the composition the header names: per node Oracle.bfv_rotate, Oracle.vec add and sub on both polynomials, and
the negacyclic shift by -s in numpy.  The plan is restated here as well (nodes_of, galois_elements_of, keyswitches_of)."""
import numpy as np


def levels_of(count):
    return max(0, (int(count) - 1).bit_length())


def nodes_of(n_ring, count):
    """[(g_j, s_j, nodes, nodes with an odd child)] per level"""
    out = []
    for j in range(levels_of(count)):
        s = 1 << j
        out.append((n_ring // s + 1, s, min(s, count), max(0, min(s, count - s))))
    return out


def galois_elements_of(n_ring, count):
    return sorted(g for g, _, _, _ in nodes_of(n_ring, count))


def keyswitches_of(n_ring, count):
    return sum(n for _, _, n, _ in nodes_of(n_ring, count))


def mul_monomial(o, data, exponent):
    """X^exponent * data over Z_q[X] / (X^N + 1), data [polys][L][N] (limb j at modulus j): coefficient y lands on (y + e) mod N,
    negated when (y + e) mod 2N >= N"""
    data = np.asarray(data, dtype=np.uint64)
    n = data.shape[-1]
    e = int(exponent) % (2 * n)
    t = (np.arange(n) + e) % (2 * n)
    out = np.empty_like(data)
    for pl in range(data.shape[0]):
        for j in range(data.shape[1]):
            q = np.uint64(o.mod[j])
            v = data[pl, j]
            neg = np.where(v == 0, v, q - v)
            out[pl, j, t % n] = np.where(t >= n, neg, v)
    return out


def _each(o, op, a, b):
    return np.stack([np.stack([o.vec(op, j, a[pl, j], b[pl, j]) for j in range(a.shape[1])]) for pl in range(2)])


def expand(o, key_of, key_level, ct, level, count):
    """ct [2][level+1][N] coefficient domain -> [count][2][level+1][N]; key_of(g): the Galois key of g exported at key_level"""
    n = o.n
    c = [None] * count
    c[0] = np.array(ct, dtype=np.uint64)
    for g, s, nodes, _ in nodes_of(n, count):
        for a in range(nodes):
            sigma = o.bfv_rotate(level, c[a], g, key_of(g), key_level)
            if a + s < count:
                c[a + s] = mul_monomial(o, _each(o, "sub", c[a], sigma), -s)
            c[a] = _each(o, "add", c[a], sigma)
    return np.stack(c)


def encrypt_coeffs(client, coeffs, level):
    """coefficient-domain BFV ciphertext of Delta * m(X), m given by its coefficients mod t"""
    o = client.o
    Q = 1
    for i in range(level + 1):
        Q *= o.mod[i]
    delta = Q // o.t
    m = [int(x) % o.t for x in coeffs]
    limbs = [np.array([(delta % o.mod[i]) * mx % o.mod[i] for mx in m], dtype=np.uint64) for i in range(level + 1)]
    return client._encrypt_limbs(limbs, level, ntt_domain=False)


def decrypt_coeffs(client, ct):
    """the coefficients mod t of a coefficient-domain ciphertext: the phase rounded to t"""
    ph, Q = client._phase_bigint(np.asarray(ct), ntt_domain=False)
    t = client.o.t
    return np.array([((2 * t * v + Q) // (2 * Q)) % t for v in ph], dtype=np.int64)


def prescale(coeffs, count, t):
    """m * 2^-k mod t: what the caller encrypts so that the outputs hold m_i itself"""
    inv = pow(pow(2, levels_of(count), t), -1, t)
    return np.array([int(x) * inv % t for x in coeffs], dtype=np.int64)


def expected_plain(coeffs, i, count, n_ring, t):
    """what output i holds when m * 2^-k was encrypted: sum_u m_(i + 2^k u) X^(2^k u)"""
    step = 1 << levels_of(count)
    out = np.zeros(n_ring, dtype=np.int64)
    idx = np.arange(i, n_ring, step)
    out[idx - i] = np.asarray(coeffs, dtype=np.int64)[idx] % t
    return out
