"""The handle contract of the six operators that work through a plan (bootstrap, CKKS and BFV linear transform, CKKS and BFV slot
sum, polynomial evaluation), the same for each: a plan made on one context and run with another is refused (LSA_ERR_ARG, "another
context") before anything is queued, a sentinel-filled output unchanged; the destroy entry points take a null handle; close()
twice on the Python object is harmless; the Galois elements the handle reports are the host planner's.  Every refusal here is
decided on the host.  N = 2^12 (the bootstrap plan at N = 2^10), the small chains of the operators' own tests."""
import ctypes

import numpy as np
import pytest

from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu

SENTINEL = 7


class Pair:
    """two contexts A and B on the same parameters, a sentinel-filled output and a zero input on B"""

    def __init__(self, algo, n, q, p, t=0):
        from lattisense_amd.device import DeviceContext
        self.n, self.q, self.p = n, list(q), list(p)
        self.a = DeviceContext(algo, n, q, p, t)
        self.b = DeviceContext(algo, n, q, p, t)
        self.words = 2 * len(self.q) * n                      # a ciphertext at the top level: enough for every call below
        self.xin = self.b.upload(np.zeros(self.words, dtype=np.uint64))
        self.out = self.b.upload(np.full(self.words, SENTINEL, dtype=np.uint64))

    def zero_key(self, level):
        return self.b.upload_key(np.zeros(self.b.key_bytes(level) // 8, dtype=np.uint64), level)

    def refused_on_b(self, plan, run):
        """run(plan) with the plan's context swapped for B: the refusal, and the output untouched"""
        from lattisense_amd._native import LsaError
        plan.ctx = self.b
        try:
            with pytest.raises(LsaError) as e:
                run(plan)
        finally:
            plan.ctx = self.a
        assert e.value.code == 1 and "another context" in str(e.value), e.value
        assert np.all(self.b.download(self.out, (self.words,)) == SENTINEL)

    def close(self):
        self.a.close()
        self.b.close()


@pytest.fixture(scope="module")
def ckks():
    need_gpu()
    from lattisense_amd import params
    from lattisense_amd.device import ALGO_CKKS
    P = params.CKKS_DEFAULT[65536]
    pair = Pair(ALGO_CKKS, 1 << 12, P["q"][:4], P["p"])       # 4 Q + the P of the headline chain: one digit
    yield pair
    pair.close()


@pytest.fixture(scope="module")
def bfv():
    need_gpu()
    from lattisense_amd import params
    from lattisense_amd.device import ALGO_BFV
    B = params.BFV_DEFAULT[8192]
    pair = Pair(ALGO_BFV, 1 << 12, B["q"], B["p"], B["t"])    # 3 Q + 1 P
    yield pair
    pair.close()


def _closes_twice(plan):
    plan.close()
    assert plan.h is None
    plan.close()
    assert plan.h is None


def _elements(n, rotations):
    return sorted(pow(5, r, 2 * n) for r in rotations)


def test_destroy_takes_a_null_handle():
    need_gpu()
    from lattisense_amd._native import lib
    for name in ("lsa_bootstrap_destroy", "lsa_lt_destroy", "lsa_bfv_lt_destroy", "lsa_slot_sum_destroy", "lsa_bfv_slot_sum_destroy",
                 "lsa_poly_destroy"):
        getattr(lib(), name)(None)


def test_bootstrap():
    need_gpu()
    from lattisense_amd import params
    from lattisense_amd._native import LsaError, check, lib
    from lattisense_amd.device import ALGO_CKKS, BootstrapPlan, plan_rotations
    B = params.CKKS_BOOTSTRAP_65536
    pair = Pair(ALGO_CKKS, 1 << 10, B["q"], B["p"])
    n, top = pair.n, len(B["q"]) - 1
    plan = BootstrapPlan(pair.a, in_scale=2.0 ** 40, out_scale=2.0 ** 40)
    assert not plan.sparse
    # the host planner's list: the rotations of every matrix's diagonal set (lsa_lt_plan_rotations) and the conjugation
    want = {2 * n - 1}
    for i in range(plan.n_matrices):
        _, n1, ks, _ = plan.matrix(i)
        split, rot = plan_rotations(n // 2, ks)
        assert split == n1
        want |= set(_elements(n, rot))
    assert plan.galois_elements == sorted(want)
    rlk = pair.zero_key(top)
    with pytest.raises(LsaError) as e:
        check(lib().lsa_ckks_bootstrap(pair.b.h, plan.h, pair.xin.ptr, pair.out.ptr, 1, 2 * n, 2 * (plan.out_level + 1) * n, rlk, 0, None,
                                       None, None, None, None))
    assert e.value.code == 1 and "another context" in str(e.value), e.value
    assert np.all(pair.b.download(pair.out, (pair.words,)) == SENTINEL)
    pair.b.destroy_key(rlk)
    _closes_twice(plan)
    pair.close()


def test_ckks_linear_transform(ckks):
    from lattisense_amd.device import LinearTransformPlan, plan_rotations
    period, index = 8, [0, 1, 2, 5]
    plan = LinearTransformPlan(ckks.a, 2, {k: np.full(period, 0.5 + 0.25j) for k in index})
    n1, rot = plan_rotations(period, index)
    assert plan.n1 == n1 and plan.galois_elements == _elements(ckks.n, rot) and plan.galois_elements
    ckks.refused_on_b(plan, lambda p: p.run(ckks.xin, 1, {}, rescale=False, out=ckks.out))
    _closes_twice(plan)


def test_bfv_linear_transform(bfv):
    from lattisense_amd.device import BfvLinearTransformPlan
    plan = BfvLinearTransformPlan(bfv.a, 2, {k: np.arange(8, dtype=np.uint64) for k in (0, 1, 2, 5)})
    assert plan.h is None                                      # planned on the host; the handle comes with the first use
    assert plan.info()["galois_elements"] == plan.galois_elements == _elements(bfv.n, plan.rotations) and plan.galois_elements
    bfv.refused_on_b(plan, lambda p: p.run(bfv.xin, 1, {}, out=bfv.out))
    _closes_twice(plan)


def _handle_elements(fetch, handle, count):
    from lattisense_amd._native import check
    g = (ctypes.c_uint64 * max(count, 1))()
    check(fetch(handle, g, count))
    return [int(x) for x in g[:count]]


def test_ckks_slot_sum(ckks):
    from lattisense_amd._native import lib
    from lattisense_amd.device import SlotSumPlan
    plan = SlotSumPlan(ckks.a, 2, 3, 13, 4)                    # tail keys and a radix-4 step
    assert plan.h is None
    want = _elements(ckks.n, plan.rotations)
    assert plan.galois_elements == want and len(want) >= 3
    assert _handle_elements(lib().lsa_slot_sum_galois_elements, plan._handle(), len(want)) == want
    ckks.refused_on_b(plan, lambda p: p.run(ckks.xin, 1, {}, out=ckks.out))
    _closes_twice(plan)


def test_bfv_slot_sum(bfv):
    from lattisense_amd._native import lib
    from lattisense_amd.device import BfvSlotSumPlan, plan_slot_sum
    plan = BfvSlotSumPlan(bfv.a, 2, 3, 13, 4, rows=1)
    assert plan.h is None
    want = sorted(_elements(bfv.n, plan_slot_sum(bfv.n, 3, 13, 4)["rotations"]) + [2 * bfv.n - 1])   # the columns' plan and the row swap
    assert plan.galois_elements == want
    assert _handle_elements(lib().lsa_bfv_slot_sum_galois_elements, plan._handle(), len(want)) == want
    bfv.refused_on_b(plan, lambda p: p.run(bfv.xin, 1, {}, out=bfv.out))
    _closes_twice(plan)


def test_polynomial(ckks):
    from lattisense_amd.device import PolynomialPlan
    plan = PolynomialPlan(ckks.a, [0.5, 0.25, 0.125, 0.0625], 3, 2.0 ** 45)   # (a polynomial plan rotates nothing: no elements)
    rlk = ckks.zero_key(3)
    ckks.refused_on_b(plan, lambda p: p.run(ckks.xin, 1, rlk, out=ckks.out))
    ckks.b.destroy_key(rlk)
    _closes_twice(plan)
