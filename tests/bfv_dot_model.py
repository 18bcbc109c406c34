"""CPU restatement of the BFV encrypted inner product (lsa_bfv_mult_sum / lsa_bfv_dot; ops.hip bfv_mult_sum / bfv_dot) on the
oracle's primitives only -- Oracle.baseconv, ntt, intt, vec -- plus the same sum in exact Python integers.

The rule (include/lattisense_amd.h, "Headroom rule"): with bl = bitlen(Q_level), nmul = (bitlen(Q_full) + log N + 60) // 61,
    G = min(30, 61 nmul - bl - log N),   max_terms = 2^G,   M(m) = (bl + log N + ceil(log2 m) + 60) // 61;
the terms are cut into consecutive groups of max_terms, a group of m terms runs over Q_level and the first M(m) auxiliary primes
and is divided by Q on its own, the group results are added in Q, one relinearisation follows.

Ciphertexts are [2][level+1][N] uint64 arrays in the coefficient domain, as the oracle's bfv_mult takes them."""
import numpy as np


def product(vals):
    out = 1
    for v in vals:
        out *= int(v)
    return out


def ceil_log2(m):
    return (int(m) - 1).bit_length()


def plan(n, q, level, terms):
    """{G, max_terms, groups, aux_limbs}: the rule, stated independently of the library"""
    logn = n.bit_length() - 1
    nmul = (product(q).bit_length() + logn + 60) // 61
    bl = product(q[: level + 1]).bit_length()
    G = min(30, 61 * nmul - bl - logn)
    assert G >= 0
    mt = 1 << G
    return {"G": G, "max_terms": mt, "groups": -(-terms // mt), "aux_limbs": aux_limbs(n, q, level, min(terms, mt))}


def aux_limbs(n, q, level, m):
    return (product(q[: level + 1]).bit_length() + n.bit_length() - 1 + ceil_log2(m) + 60) // 61


def _aux_index(o, i):
    return o.nq + o.np_ + i


def group_d3(o, lvl, As, Bs, M):
    """t * round(sum_i As[i] (x) Bs[i] / Q) over Q_lvl and the first M auxiliary primes: [3][lvl+1][N]"""
    L, n = lvl + 1, o.n
    assert 1 <= M <= len(o.aux)
    qidx, aidx = list(range(L)), [_aux_index(o, i) for i in range(M)]
    tidx = qidx + aidx
    T = L + M

    def extend(poly):   # [L][N] coefficients -> [T][N] in the NTT domain
        e = np.concatenate([np.ascontiguousarray(poly), o.baseconv(qidx, aidx, poly, True)])
        return np.stack([o.ntt(tidx[j], e[j]) for j in range(T)])

    cache = {}

    def ext_ct(ct):
        key = id(ct)
        if key not in cache:
            cache[key] = (ct, extend(ct[0]), extend(ct[1]))
        return cache[key][1:]

    d = np.zeros((3, T, n), dtype=np.uint64)
    for a, b in zip(As, Bs):
        a0, a1 = ext_ct(a)
        b0, b1 = ext_ct(b)
        for j in range(T):
            mi = tidx[j]
            d[0, j] = o.vec("add", mi, d[0, j], o.vec("mul", mi, a0[j], b0[j]))
            d[1, j] = o.vec("add", mi, d[1, j], o.vec("add", mi, o.vec("mul", mi, a0[j], b1[j]), o.vec("mul", mi, a1[j], b0[j])))
            d[2, j] = o.vec("add", mi, d[2, j], o.vec("mul", mi, a1[j], b1[j]))
    out = np.empty((3, L, n), dtype=np.uint64)
    Q = product(o.mod[:L])
    for k in range(3):
        dk = np.stack([o.intt(tidx[j], d[k, j]) for j in range(T)])
        ext = o.baseconv(qidx, aidx, dk[:L], True)
        r = np.empty((M, n), dtype=np.uint64)
        for i in range(M):
            p = o.mod[aidx[i]]
            qinv = np.full(n, pow(Q % p, -1, p), dtype=np.uint64)
            r[i] = o.vec("mul", aidx[i], o.vec("sub", aidx[i], dk[L + i], ext[i]), qinv)
        back = o.baseconv(aidx, qidx, r, True)
        for i in range(L):
            out[k, i] = o.vec("mul", i, back[i], np.full(n, o.t % o.mod[i], dtype=np.uint64))
    return out


def mult_sum(o, lvl, As, Bs, addend=None, force_aux=None):
    """lsa_bfv_mult_sum on one batch item.  force_aux: run every group over that many auxiliary primes instead of M(m) (what
    the rule exists to prevent: the tests use it to show that they can fail)"""
    pl = plan(o.n, o.q, lvl, len(As))
    out = None
    for i0 in range(0, len(As), pl["max_terms"]):
        ga, gb = As[i0: i0 + pl["max_terms"]], Bs[i0: i0 + pl["max_terms"]]
        M = force_aux if force_aux is not None else aux_limbs(o.n, o.q, lvl, len(ga))
        g = group_d3(o, lvl, ga, gb, M)
        if out is None:
            out = g
        else:
            for k in range(3):
                for j in range(lvl + 1):
                    out[k, j] = o.vec("add", j, out[k, j], g[k, j])
    if addend is not None:
        for k in range(2):
            for j in range(lvl + 1):
                out[k, j] = o.vec("add", j, out[k, j], addend[k, j])
    return out


def dot(o, lvl, As, Bs, rlk, klvl, addend=None):
    """lsa_bfv_dot on one batch item"""
    return o.bfv_relin(lvl, mult_sum(o, lvl, As, Bs, addend), rlk, klvl)


# ---- exact integers
def centred_ints(o, lvl, poly):
    """[lvl+1][N] residues -> N Python integers in [-(Q-1)/2, (Q-1)/2]"""
    L = lvl + 1
    mods = [int(m) for m in o.mod[:L]]
    Q = product(mods)
    w = [(Q // m) * pow(Q // m, -1, m) for m in mods]
    out = []
    for x in range(o.n):
        v = sum(int(poly[i][x]) * w[i] for i in range(L)) % Q
        out.append(v - Q if v > Q // 2 else v)
    return out


def negacyclic(a, b):
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        if x == 0:
            continue
        for j, y in enumerate(b):
            k = i + j
            if k < n:
                out[k] += x * y
            else:
                out[k - n] -= x * y
    return out


def exact_tensor_sum(o, lvl, As, Bs):
    """the three integer polynomials sum_i a_i (x) b_i, operands lifted centred; equal operand objects are multiplied once"""
    ints, prods = {}, {}

    def lift(ct):
        if id(ct) not in ints:
            ints[id(ct)] = (ct, centred_ints(o, lvl, ct[0]), centred_ints(o, lvl, ct[1]))
        return ints[id(ct)][1:]

    d = [[0] * o.n for _ in range(3)]
    for a, b in zip(As, Bs):
        key = (id(a), id(b))
        if key not in prods:
            (a0, a1), (b0, b1) = lift(a), lift(b)
            x01, x10 = negacyclic(a0, b1), negacyclic(a1, b0)
            prods[key] = (negacyclic(a0, b0), [u + v for u, v in zip(x01, x10)], negacyclic(a1, b1))
        for k in range(3):
            d[k] = [u + v for u, v in zip(d[k], prods[key][k])]
    return d


def exact_d3(o, lvl, As, Bs):
    """t * (d - centred(d mod Q)) / Q per coefficient on Python integers, reduced to the limbs of Q_lvl: [3][lvl+1][N]"""
    L = lvl + 1
    Q = product(o.mod[:L])
    out = np.empty((3, L, o.n), dtype=np.uint64)
    for k, dk in enumerate(exact_tensor_sum(o, lvl, As, Bs)):
        for x, v in enumerate(dk):
            c = v % Q
            if c > Q // 2:
                c -= Q
            r = o.t * ((v - c) // Q)
            for i in range(L):
                out[k, i, x] = r % o.mod[i]
    return out


def exact_mult_sum(o, lvl, As, Bs):
    """exact_d3 per group of the plan, the groups added limb by limb: every group carries its own rounding"""
    mt = plan(o.n, o.q, lvl, len(As))["max_terms"]
    out = None
    for i0 in range(0, len(As), mt):
        g = exact_d3(o, lvl, As[i0: i0 + mt], Bs[i0: i0 + mt])
        if out is None:
            out = g
        else:
            for j in range(lvl + 1):
                out[:, j] = (out[:, j].astype(object) + g[:, j].astype(object)) % o.mod[j]
    return out


def constant_ct(o, lvl, v0, v1):
    """the ciphertext whose two polynomials have every coefficient v0 / v1 (integers, reduced to the limbs)"""
    ct = np.empty((2, lvl + 1, o.n), dtype=np.uint64)
    for h, v in enumerate((v0, v1)):
        for i in range(lvl + 1):
            ct[h, i, :] = v % o.mod[i]
    return ct
