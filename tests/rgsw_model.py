"""CPU restatement of the BFV external product RLWE x RGSW, the CMux and the select-by-index operator (include/lattisense_amd.h:
lsa_bfv_external_product, lsa_bfv_cmux, lsa_bfv_select_*; lattisense_amd/csrc/bfv_select.h) on the oracle: Oracle.gadget_product twice,
Oracle.vec("add") on every row of both polynomials of the extended accumulator, ONE Oracle.moddown, the inverse transforms, and
Oracle.vec add / sub for the base and the CMux's difference.  The plan is restated here as well (levels_of, pairs_of)."""
import numpy as np


def levels_of(count):
    return max(0, (int(count) - 1).bit_length())


def pairs_of(count):
    """[(j, 2^j, n_pair)] for the levels j = k-1 down to 0"""
    return [(j, 1 << j, min(1 << j, count - (1 << j))) for j in range(levels_of(count) - 1, -1, -1)]


def products_of(count):
    return sum(n for _, _, n in pairs_of(count))


def first_unchanged(count):
    """the inputs from here on are only read"""
    return max(1, 1 << max(levels_of(count) - 1, 0))


def rgsw_encrypt(client, m_coeffs, klvl):
    """(R0, R1) of the small polynomial m (signed integer coefficients [N]): switching keys from m and from m * s to s, in the layout
    of lsa_key_upload"""
    o = client.o
    m_ntt = np.stack([o.ntt(i, client._lift(m_coeffs, o.mod[i])) for i in range(client.nqp)])
    ms_ntt = np.stack([o.vec("mul", i, m_ntt[i], client.s_ntt[i]) for i in range(client.nqp)])
    return client.gen_switching_key(m_ntt, client.s_ntt, klvl), client.gen_switching_key(ms_ntt, client.s_ntt, klvl)


def monomial(n, e):
    """the coefficients of X^e, 0 <= e < N"""
    m = np.zeros(n, dtype=np.int64)
    m[e] = 1
    return m


def constant(n, v):
    m = np.zeros(n, dtype=np.int64)
    m[0] = v
    return m


def _each(o, op, a, b):
    return np.stack([np.stack([o.vec(op, j, a[pl, j], b[pl, j]) for j in range(a.shape[1])]) for pl in range(2)])


def external_product(o, level, ct, rgsw, klvl, base=None):
    """ct, base: [2][level+1][N], coefficient domain; rgsw = (R0, R1) exported at klvl -> [2][level+1][N]"""
    ct = np.asarray(ct, dtype=np.uint64)
    L, T = level + 1, level + 1 + len(o.p)
    cx = [np.stack([o.ntt(j, ct[h, j]) for j in range(L)]) for h in range(2)]
    a0 = o.gadget_product(level, cx[0], rgsw[0], klvl)
    a1 = o.gadget_product(level, cx[1], rgsw[1], klvl)
    mi = lambda tl: tl if tl < L else o.nq + (tl - L)
    acc = np.stack([np.stack([o.vec("add", mi(tl), a0[h, tl], a1[h, tl]) for tl in range(T)]) for h in range(2)])
    md = o.moddown(level, acc)
    out = np.stack([np.stack([o.intt(j, md[h, j]) for j in range(L)]) for h in range(2)])
    return out if base is None else _each(o, "add", np.asarray(base, dtype=np.uint64), out)


def cmux(o, level, c0, c1, rgsw, klvl):
    c0, c1 = np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64)
    return external_product(o, level, _each(o, "sub", c1, c0), rgsw, klvl, base=c0)


def select(o, level, cts, selectors, klvl):
    """cts [count][2][level+1][N]; selectors[j] = (R0, R1) of index bit j -> (the result, the input array as the device leaves it when
    `out` is input 0)"""
    c = [np.array(x, dtype=np.uint64) for x in cts]
    for j, half, n_pair in pairs_of(len(c)):
        for a in range(n_pair):
            c[a] = cmux(o, level, c[a], c[a + half], selectors[j], klvl)
    return c[0], np.stack(c)
