"""CPU restatement of the BFV polynomial evaluator (lsa_bfv_poly_* / lsa_bfv_poly_eval; csrc/bfv_poly.h, bfv_poly.hip) and of
lsa_bfv_affine_const on the oracle's primitives only -- Oracle.bfv_mult_relin, vec, bfv_scale_up -- with tests/bfv_dot_model.dot
for the sum, plus a planner in plain Python that states the counts and the depth independently of the library.

The plan (include/lattisense_amd.h, "BFV polynomial evaluation"): m = 2^log_baby, G = ceil(n_coef / m), coefficients padded to
G * m; x^j = x^ceil(j/2) * x^floor(j/2); y = x^m = x^(m/2) * x^(m/2), y^g = y^ceil(g/2) * y^floor(g/2);
leaf_g = coef[g m] + sum_{1 <= j < m} coef[g m + j] x^j; out = leaf_0 + sum_{g >= 1} leaf_g * y^g with ONE scale-down and ONE
relinearisation.  Only what a non-zero coefficient needs is computed.

Ciphertexts are [2][level+1][N] uint64 arrays in the coefficient domain."""
import numpy as np

from tests import bfv_dot_model


def ceil_log2(x):
    return (int(x) - 1).bit_length()


def _halves(needed, lowest):
    """close a set of exponents under e -> ceil(e/2), floor(e/2) down to `lowest`"""
    todo = sorted(needed, reverse=True)
    out = set()
    while todo:
        e = todo.pop(0)
        if e < lowest or e in out:
            continue
        out.add(e)
        todo += [(e + 1) // 2, e // 2]
    return out


def plan_at(coeffs, log_baby):
    """the structure and the counts at one log_baby in 1..4"""
    m = 1 << log_baby
    n = len(coeffs)
    G = -(-n // m)
    cf = [int(c) for c in coeffs] + [0] * (G * m - n)
    rows = [cf[g * m: (g + 1) * m] for g in range(G)]
    leaves = [g for g in range(G) if any(rows[g])]
    used = {g: [j for j in range(1, m) if rows[g][j]] for g in leaves}
    pairs = [g for g in leaves if g >= 1]
    want_baby = {j for g in leaves for j in used[g]}
    if pairs:
        want_baby.add(m // 2)          # y = x^(m/2) * x^(m/2)
    babies = sorted(_halves(want_baby, 2))
    giants = sorted(_halves(set(pairs), 1))

    def d_leaf(g):
        return max([ceil_log2(j) for j in used[g]], default=0)

    depth = d_leaf(0) if 0 in leaves else 0
    for g in pairs:
        depth = max(depth, max(d_leaf(g), log_baby + ceil_log2(g)) + 1)
    return {"log_baby": log_baby, "m": m, "G": G, "coef": cf, "leaves": leaves, "used": used, "babies": babies, "giants": giants,
            "depth": depth, "n_mult": len(babies) + len(giants) + (1 if pairs else 0), "n_pairs": len(pairs),
            "n_leaves": len(leaves), "n_leaf_launches": -(-len(leaves) // 8)}


def plan(coeffs, log_baby=0):
    """log_baby 0: the least depth, then the fewest key switches, then the smaller value"""
    if log_baby:
        return plan_at(coeffs, log_baby)
    return min((plan_at(coeffs, b) for b in (1, 2, 3, 4)), key=lambda p: (p["depth"], p["n_mult"], p["log_baby"]))


COUNTS = ("log_baby", "depth", "n_mult", "n_leaves", "n_leaf_launches", "n_pairs")


def counts(coeffs, log_baby=0):
    p = plan(coeffs, log_baby)
    return {k: p[k] for k in COUNTS}


# ---- the leaf kernel
def centred(k, t):
    """k in [0, t) centred into (-t/2, t/2]"""
    k = int(k)
    return k - t if k > t // 2 else k


def lincomb(o, lvl, terms, c0):
    """sum_i K_i * src_i + scaleUp(c0): terms a list of (coefficient in [0, t), ciphertext); the constant is Lattigo's scaleUp of
    the constant polynomial, one word per limb on coefficient 0 of c0"""
    L, n = lvl + 1, o.n
    out = np.zeros((2, L, n), dtype=np.uint64)
    for k, ct in terms:
        for j in range(L):
            kv = np.full(n, centred(k, o.t) % o.mod[j], dtype=np.uint64)
            for h in range(2):
                out[h, j] = o.vec("add", j, out[h, j], o.vec("mul", j, kv, ct[h, j]))
    if c0:
        pt = np.zeros(n, dtype=np.uint64)
        pt[0] = c0
        up = o.bfv_scale_up(lvl, pt)
        assert not up[:, 1:].any()      # the constant polynomial scales to one coefficient
        for j in range(L):
            out[0, j] = o.vec("add", j, out[0, j], up[j])
    return out


def affine_const(o, lvl, ct, k, c):
    """lsa_bfv_affine_const on one batch item"""
    return lincomb(o, lvl, [(k, ct)] if k else [], c)


def evaluate(o, lvl, ct, coeffs, rlk, klvl, log_baby=0):
    """lsa_bfv_poly_eval on one batch item"""
    p = plan(coeffs, log_baby)
    m, cf = p["m"], p["coef"]
    X = {1: ct}
    for j in p["babies"]:
        X[j] = o.bfv_mult_relin(lvl, X[(j + 1) // 2], X[j // 2], rlk, klvl)
    Y = {}
    for g in p["giants"]:
        a, b = (X[m // 2], X[m // 2]) if g == 1 else (Y[(g + 1) // 2], Y[g // 2])
        Y[g] = o.bfv_mult_relin(lvl, a, b, rlk, klvl)
    leaf = {g: lincomb(o, lvl, [(cf[g * m + j], X[j]) for j in p["used"][g]], cf[g * m]) for g in p["leaves"]}
    pairs = [g for g in p["leaves"] if g >= 1]
    if not pairs:
        return leaf[0]
    return bfv_dot_model.dot(o, lvl, [leaf[g] for g in pairs], [Y[g] for g in pairs], rlk, klvl, leaf.get(0))


def polynomial_mod_t(coeffs, values, t):
    """p(values) mod t on Python integers"""
    out = np.zeros(len(values), dtype=object)
    for c in reversed([int(c) for c in coeffs]):
        out = (out * np.asarray(values).astype(object) + c) % t
    return out
