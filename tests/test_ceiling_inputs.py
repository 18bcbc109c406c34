"""The operands of tests/test_gpu_ceiling.py cases A and B discriminate: a Python-integer model of the multiply-accumulate
loop -- products summed in 128 bits, a lazy REDC (V 2^-64 mod q, in [0, 2q) only for V < q 2^64) with ONE conditional subtraction
at every fold, the fold cadence a parameter -- run on those exact arrays gives the true sum under the kernels' cadence and a
non-canonical or wrong word under every later one.  No GPU.

The second half models what k_mac_plain and k_tensor_sum do AFTER the loop (tests/test_ceiling_inputs.py is the only place that
records it): both finish with a Montgomery multiply by 2^128 mod q, which takes any 64-bit word and returns the canonical
residue, and the REDC itself is exact for every V with hi + q < 2^64.  Up to the launch bound of 16 terms (32 products for d1:
hi < 4q) a late or missing fold therefore leaves a non-canonical intermediate that the tail absorbs -- the stored word is still
the true sum.  The folds keep the documented [0, 2q) contract of mont_redc_lazy; at these term counts they do not decide the
result, and no output comparison can see them move."""
import numpy as np
import pytest

from tests.boundary import (CEILING_LOGN, CEILING_SLOTS, DOT_TERMS, MAC_TERMS, ceiling_dot_operands, ceiling_mac_operands, dot_term,
                            is_ceiling, mac_term)

W = 1 << 64
SLOT = CEILING_SLOTS.index("top")


def obj(a):
    return np.asarray(a).astype(object)


def redc_lazy(V, q):
    """mont_redc_lazy on whole 128-bit values: hi - mulhi(lo * qinv, q) + q"""
    qinv = pow(q, -1, W)
    m = (V % W) * qinv % W
    return (V >> 64) - ((m * q) >> 64) + q


def csub(x, q):
    x = np.asarray(x, dtype=object)
    return np.where((x >= q).astype(bool), x - q, x)


def loop_model(products, q, folds):
    """products: the per-coefficient products in the order the kernel adds them; folds: the set of product counts after which
    the loop folds.  Every segment leaves csub(redc(V)) and the segments join by add_mod.  Returns the joined word and
    whether every segment's word was a canonical residue (it is whenever the segment stayed below q 2^64; a later add_mod can
    happen to subtract the q a segment left behind, so the joined word alone understates what went wrong)"""
    r, V, clean = None, 0, True
    for k, p in enumerate(products, 1):
        V = V + p
        if k in folds or k == len(products):
            x = csub(redc_lazy(V, q), q)
            clean = clean & (x < q).astype(bool)
            r = x if r is None else csub(r + x, q)
            V = 0
    return r, clean


def right(model, want):
    r, clean = model
    return clean & (r == want).astype(bool)


def every(step, count, late=0):
    return {k + late for k in range(step, count + 1, step)}


def cadences(count, per_term=1):
    """(the kernel's cadence, the later ones) as product counts: a fold after every 8 products; per_term products per term"""
    wrong = {"one term late": every(8, count, late=per_term), "every 16 terms": every(16 * per_term, count), "none": set()}
    if per_term == 2:
        wrong["d1 every 8 terms instead of every 4"] = every(16, count)
    return every(8, count), wrong


def true_word(products, q):
    return sum(products) * pow(W, -1, q) % q


def _mac_products(n, limb, poly=0):
    C, cts, pts, _ = ceiling_mac_operands(CEILING_LOGN[n])
    out = []
    for i in range(n):
        ci, pi, shared = mac_term(i)
        out.append(obj(cts[ci][SLOT, poly, limb]) * obj(pts[pi][0 if shared else SLOT, limb]))
    return C["q"][limb], out


def _dot_products(n, limb):
    C, As, Bs, _ = ceiling_dot_operands(CEILING_LOGN[n])
    d0, d1, d2 = [], [], []
    for i in range(n):
        ai, bi = dot_term(i)
        a0, a1, b0, b1 = (obj(x[SLOT, h, limb]) for x in (As[ai], Bs[bi]) for h in (0, 1))
        d0.append(a0 * b0)
        d1 += [a0 * b1, a1 * b0]
        d2.append(a1 * b1)
    return C["q"][limb], d0, d1, d2


@pytest.mark.parametrize("n", MAC_TERMS)
def test_case_a_operands_show_a_late_fold(n):
    """k_mac_plain: one product per term, fold after 8"""
    for limb in (0, 3):
        q, prods = _mac_products(n, limb)
        assert is_ceiling(q)
        good, wrong = cadences(n)
        want = true_word(prods, q)
        assert np.all(right(loop_model(prods, q, good), want)), (n, limb)
        for name, folds in wrong.items():
            got = loop_model(prods, q, folds)
            if n <= 8:                                   # nothing to fold yet: every cadence is the same loop
                assert np.all(right(got, want)), (n, limb, name)
            else:
                assert not np.all(right(got, want)), (n, limb, name, "the operands do not show this cadence")


@pytest.mark.parametrize("n", DOT_TERMS)
def test_case_b_operands_show_a_late_fold(n):
    """k_tensor_sum: d0 and d2 one product per term (fold before term 8), d1 two (fold before term 4)"""
    q, d0, d1, d2 = _dot_products(n, 1)
    for tag, prods, per_term in (("d0", d0, 1), ("d2", d2, 1), ("d1", d1, 2)):
        good, wrong = cadences(len(prods), per_term)
        want = true_word(prods, q)
        assert np.all(right(loop_model(prods, q, good), want)), (n, tag)
        for name, folds in wrong.items():
            got = loop_model(prods, q, folds)
            if len(prods) <= 8:
                assert np.all(right(got, want)), (n, tag, name)
            else:
                assert not np.all(right(got, want)), (n, tag, name, "the operands do not show this cadence")


# ---------------------------------------------------------------- the kernels' tails

def mont_mul(a, b, q):
    """mont_mul for any 64-bit a and b < q: a b < q 2^64, the lazy REDC is in range"""
    assert np.all(a < W) and b < q
    return csub(redc_lazy(a * b, q), q)


def k_mac_plain_word(products, q, folds):
    """kernels.hip k_mac_plain: r = add_mod(r, csub(redc)) at every fold and once after the loop, then mont_mul(r, r2)"""
    r, V = 0, 0
    for k, p in enumerate(products, 1):
        V = V + p
        if k in folds:
            r = csub(r + csub(redc_lazy(V, q), q), q)
            V = 0
    r = csub(r + csub(redc_lazy(V, q), q), q)
    assert np.all(r < W), "a word left 64 bits"
    return mont_mul(r, W * W % q, q)


def k_tensor_sum_word(products, q, folds):
    """tensor_sum.h: ts_fold in place before the next product (hi -> hi 2^64 mod q, [0, 2q)), ts_finish = mont_mul(redc, r2)"""
    r2, V = W * W % q, 0
    for k, p in enumerate(products, 1):
        V = V + p
        if k in folds and k < len(products):
            V = redc_lazy((V >> 64) * r2, q) + V % W
    x = redc_lazy(V, q)
    assert np.all(V >> 64 < W - q) and np.all(x < W), "a word left 64 bits"
    return mont_mul(x, r2, q)


def test_the_tails_absorb_a_late_fold_up_to_the_launch_bound():
    """16 terms, the launch bound of both kernels (LSA_MAC_MAX_TERMS, LSA_DOT_MAX_TERMS): the stored word is the true sum under
    every cadence, the kernels' own included; see the module docstring"""
    q, prods = _mac_products(16, 0)
    want = sum(prods) % q
    good, wrong = cadences(16)
    for name, folds in [("kernel", good)] + list(wrong.items()):
        assert np.array_equal(k_mac_plain_word(prods, q, folds), want), ("k_mac_plain", name)
    q, d0, d1, _ = _dot_products(16, 1)
    for tag, prods, per_term in (("d0", d0, 1), ("d1", d1, 2)):
        want = sum(prods) % q
        good, wrong = cadences(len(prods), per_term)
        for name, folds in [("kernel", good)] + list(wrong.items()):
            assert np.array_equal(k_tensor_sum_word(prods, q, folds), want), ("k_tensor_sum", tag, name)
