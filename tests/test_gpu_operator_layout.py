"""Layout, aliasing and argument contract (include/lattisense_amd.h, "Layout and aliasing") of the second-generation operators,
through raw C calls: lsa_bfv_rotate_many, lsa_bfv_mult_plain_mul / _mac_plain_mul / _rotate_mac_plain_mul, lsa_ckks_slot_sum,
lsa_bfv_slot_sum, lsa_ckks_linear_transform, lsa_bfv_linear_transform, lsa_ckks_poly_eval, lsa_bfv_poly_eval,
lsa_bfv_affine_const, lsa_ckks_mult_sum / _dot and lsa_bfv_mult_sum / _dot.  Their tails gather, scatter or stage a limb in LDS
and store with the OUTPUT's stride, and they cut the batch into tiles at b0 * stride separately for every operand: a wrong
stride is invisible while every buffer is dense.

The reference of every result is the operator's CPU model on the same words -- tests/slot_sum_model.py, bfv_slot_sum_model.py,
bfv_lt_model.py, poly_model.py, bfv_poly_model.py, bfv_dot_model.py, oracle/ckks_bootstrap.py linear_transform, Oracle.bfv_rotate
and the pt_mul product INTT(NTT(ct) . pt . 2^-64) limb by limb -- never a dense call of the entry point, computed once per
operand set and shared by the layout variants.  Every comparison is word for word.

  padded layout   every input, plaintext, addend / partial and output inside its own sentinel-filled buffer, each with its own
                  16-byte aligned base (no multiple of N) and its own padded stride, the output's the largest: payload == model at
                  every batch position, every word of padding and of the guard zones still the sentinel, every input unchanged
  tiles           batch 5 in tiles of 2 (2, 2, 1) under both lsa_set_dual_stream settings, tile batch 0 once
  shared          stride 0 on plaintexts, on the b side and the addend of the inner products; as[i] == bs[i] (a square)
  in place        slot sums out == in, lsa_bfv_affine_const and lsa_bfv_mult_plain_mul out == ct, lsa_bfv_rotate_many with exactly
                  one output == in (tiled: that rotation must still see the intact input)
  interleaved     outputs between the items of the first input in one buffer: overlap is exact, padding belongs to nobody
  refusals        every refusal of the contract: return code, message prefix, nothing written, the context still usable

CKKS: N = 2^11, the first five primes of CKKS_DEFAULT[16384] with its two special primes, level 3, keys at level 4.  BFV: N = 2^11
on BFV_DEFAULT[8192] (three Q limbs, one special prime), top level.  Two-pass rings, N = 2^13 (CKKS: six Q and two P limbs of
CKKS_DEFAULT[65536]; BFV: BFV_DEFAULT[8192]) for the operators with a gathering or LDS-staged tail -- the slot sums,
lsa_bfv_rotate_many, lsa_bfv_rotate_mac_plain_mul and both linear transforms -- in the padded, tiled case only.  Plans are the
smallest with two key-switching steps: a slot sum of 4, four diagonals split 2 x 2 (one giant step), a degree-3 polynomial with
log_baby = 1, three inner-product terms, three rotations including 2N - 1.  Keys and ciphertexts are uniform words."""
import numpy as np
import pytest

from tests.gpu_util import need_gpu, rand_ct
from tests.layout_util import SENT, Field, invoke, last_error, padded_operands, padded_outputs

pytestmark = pytest.mark.gpu

ARG = 1                                                    # LSA_ERR_ARG
GAP = 30                                                   # words between neighbours in the interleaved layouts


def _lib():
    from lattisense_amd._native import lib
    return lib()


def _rand_key(rng, q, p, klvl, n):
    beta = (klvl + 1 + len(p) - 1) // len(p)
    key = np.empty((beta, 2, klvl + 1 + len(p), n), dtype=np.uint64)
    for j, m in enumerate(list(q[: klvl + 1]) + list(p)):
        key[:, :, j, :] = rng.integers(0, m, size=(beta, 2, n), dtype=np.uint64)
    return key


def _ok(rc):
    assert rc == 0, last_error()


class Case:
    """one operator on one set of operands.  arrays: the inputs [batch][...] in the adapter's order; fn(*items) -> the model's
    result for one batch item from that item of every input ([n_out][...] when n_out > 1); shared[i] / same[i]: input i may have
    stride 0 / the output may BE input i; nullable: inputs that may be absent (no null refusal); prefix: how every refusal begins"""

    def __init__(self, name, arrays, extra, wout, fn, prefix, shared=None, same=None, nullable=(), n_out=1, level_arg=True, bound=True,
                 min_level=0):
        self.name, self.arrays, self.extra, self.wout, self.fn, self.prefix = name, arrays, extra, wout, fn, prefix
        self.shared = shared or (False,) * len(arrays)
        self.same = same or (False,) * len(arrays)
        self.nullable, self.n_out, self.level_arg, self.bound, self.min_level = nullable, n_out, level_arg, bound, min_level


class Rig:
    """one context, its oracle and evaluator, operands made once and never written, model results computed once"""

    def __init__(self, algo, n, q, p, t, lvl, klvl, batch, seed):
        from lattisense_amd.device import DeviceContext
        from oracle.ckks_bootstrap import Evaluator
        from oracle.pyoracle import Oracle
        self.algo, self.n, self.q, self.p, self.t, self.lvl, self.klvl, self.batch = algo, n, list(q), list(p), t, lvl, klvl, batch
        self.L = lvl + 1
        self.ctx = DeviceContext(algo, n, q, p, t)
        self.o = Oracle(n, q, p, t)
        self.rng = np.random.default_rng(seed)
        ql = self.q[: lvl + 1]
        self.A = [rand_ct(self.rng, ql, 2, n, batch) for _ in range(3)]
        self.B = [rand_ct(self.rng, ql, 2, n, batch) for _ in range(3)]
        self.E = rand_ct(self.rng, ql, 2, n, batch)
        self.P = [rand_ct(self.rng, ql, 1, n, batch)[:, 0] for _ in range(3)]          # pt_mul plaintexts [batch][L][N]
        self.raw, self.key = {}, {}
        self.ev = Evaluator.__new__(Evaluator)             # the models take their keys from ev.glk / ev.rlk: uniform words
        self.ev.o, self.ev.c, self.ev.klvl, self.ev.n = self.o, None, klvl, n
        self.ev.glk, self.ev.counts = {}, {"rotate": 0, "mult": 0, "mul_plain": 0}
        self.ev.rlk = self.raw_key("rlk")
        self.plans, self._want, self._cases = {}, {}, {}

    def raw_key(self, what, klvl=None):
        if what not in self.raw:
            self.raw[what] = _rand_key(self.rng, self.q, self.p, self.klvl if klvl is None else klvl, self.n)
            self.key[what] = self.ctx.upload_key(self.raw[what], self.klvl if klvl is None else klvl)
        return self.raw[what]

    def glk(self, elements):
        """Galois keys of uniform words, on the device and in the evaluator the models read"""
        for g in elements:
            self.ev.glk[g] = self.raw_key(g)
        return {g: self.key[g] for g in elements}

    def low_key(self):
        self.raw_key("low", self.lvl - 1)
        return self.key["low"]

    def settings(self, dual, tile=2):
        lib = _lib()
        assert lib.lsa_set_dual_stream(self.ctx.h, dual) == 0 and lib.lsa_set_tile_batch(self.ctx.h, tile) == 0

    def want(self, tag, fn):
        """fn(i) -> the model's result for batch item i; stacked and cached under `tag`"""
        if tag not in self._want:
            self._want[tag] = np.stack([np.asarray(fn(i)) for i in range(self.batch)])
        return self._want[tag]

    def case(self, name):
        if name not in self._cases:
            self._cases[name] = CASES[name](self)
        return self._cases[name]


_RIGS = {}


def _rig(name):
    need_gpu()
    if name not in _RIGS:
        from lattisense_amd import params
        from lattisense_amd.device import ALGO_BFV, ALGO_CKKS
        B = params.BFV_DEFAULT[8192]
        if name == "ckks":
            P = params.CKKS_DEFAULT[16384]
            _RIGS[name] = Rig(ALGO_CKKS, 2048, P["q"][:5], P["p"], 0, 3, 4, 5, 11)
        elif name == "ckks2":
            P = params.CKKS_DEFAULT[65536]
            _RIGS[name] = Rig(ALGO_CKKS, 8192, P["q"][:6], P["p"][:2], 0, 3, 5, 5, 12)
        elif name == "bfv":
            _RIGS[name] = Rig(ALGO_BFV, 2048, B["q"], B["p"], B["t"], len(B["q"]) - 1, len(B["q"]) - 1, 5, 13)
        else:
            _RIGS[name] = Rig(ALGO_BFV, 8192, B["q"], B["p"], B["t"], len(B["q"]) - 1, len(B["q"]) - 1, 5, 14)
    return _RIGS[name]


@pytest.fixture(scope="module", autouse=True)
def _close_rigs():
    yield
    for r in _RIGS.values():
        for plan in r.plans.values():                      # a plan goes before its context
            plan.close()
        r.ctx.close()
    _RIGS.clear()


# ------------------------------------------------------------------------------------------------ the operators as cases
def _elements(r):
    return [5, pow(5, -7, 2 * r.n), 2 * r.n - 1]


def _ptmul_sum(o, lvl, cts, pts, partial=None):
    """sum_i INTT(NTT(ct_i) . pt_i . 2^-64) (+ partial), limb by limb: the words of the pt_mul entry points"""
    out = np.empty_like(cts[0])
    for j in range(lvl + 1):
        r = np.full(o.n, np.uint64(pow(2 ** 64, -1, int(o.q[j]))), dtype=np.uint64)
        for pl in range(2):
            acc = np.zeros(o.n, dtype=np.uint64)
            for ct, pt in zip(cts, pts):
                acc = o.vec("add", j, acc, o.vec("mul", j, o.ntt(j, np.ascontiguousarray(ct[pl, j])), o.vec("mul", j, np.ascontiguousarray(pt[j]), r)))
            v = o.intt(j, acc)
            out[pl, j] = o.vec("add", j, v, np.ascontiguousarray(partial[pl, j])) if partial is not None else v
    return out


def _bfv_rotate_many(r):
    g = _elements(r)
    r.glk(g)
    return Case("lsa_bfv_rotate_many", [r.A[0]], dict(g=g, key=[r.key[e] for e in g]), 2 * r.L * r.n,
                lambda x: np.stack([r.o.bfv_rotate(r.lvl, x, e, r.raw[e], r.klvl) for e in g]), "lsa_bfv_rotate_many", same=(True,), n_out=3)


def _bfv_mult_plain_mul(r):
    return Case("lsa_bfv_mult_plain_mul", [r.A[0], r.P[0]], {}, 2 * r.L * r.n, lambda ct, pt: _ptmul_sum(r.o, r.lvl, [ct], [pt]),
                "lsa_bfv_mult_plain_mul", shared=(False, True), same=(True, False))


def _bfv_mac_plain_mul(r):
    return Case("lsa_bfv_mac_plain_mul", r.A + r.P + [r.E], dict(n=3, partial=True), 2 * r.L * r.n,
                lambda a0, a1, a2, p0, p1, p2, e: _ptmul_sum(r.o, r.lvl, [a0, a1, a2], [p0, p1, p2], e), "lsa_bfv_mac_plain_mul",
                shared=(False,) * 3 + (True,) * 3 + (False,), nullable=(6,))


def _bfv_rotate_mac(r):
    g = [1] + _elements(r)[1:]                             # the identity term, one rotation, the row rotation
    r.glk(g[1:])
    keys = [None] + [r.key[e] for e in g[1:]]

    def fn(x, p0, p1, p2, e):
        rots = [x] + [r.o.bfv_rotate(r.lvl, x, el, r.raw[el], r.klvl) for el in g[1:]]
        return _ptmul_sum(r.o, r.lvl, rots, [p0, p1, p2], e)
    return Case("lsa_bfv_rotate_mac_plain_mul", [r.A[0]] + r.P + [r.E], dict(g=g, key=keys, partial=True), 2 * r.L * r.n, fn,
                "lsa_bfv_rotate_mac_plain_mul", shared=(False, True, True, True, False), nullable=(4,))


def _ckks_slot_sum(r):
    from lattisense_amd.device import SlotSumPlan
    from oracle.ckks_bootstrap import Ct
    from tests.slot_sum_model import slot_sum, steps_of
    plan = r.plans["slot"] = SlotSumPlan(r.ctx, r.lvl, 1, 4, 2)
    assert len(steps_of(r.n, 1, 4, 2)) == 2 and plan.keyswitches == 2                  # two key-switching steps
    glk = r.glk(plan.galois_elements)
    return Case("lsa_ckks_slot_sum", [r.A[0]], dict(plan=plan._handle(), glk=glk), 2 * r.L * r.n,
                lambda x: slot_sum(r.ev, Ct(x, r.lvl, 1.0), 1, 4, 2).data, "lsa_ckks_slot_sum", same=(True,), level_arg=False)


def _bfv_slot_sum(r):
    from lattisense_amd.device import BfvSlotSumPlan
    from tests.bfv_slot_sum_model import slot_sum
    plan = r.plans["slot"] = BfvSlotSumPlan(r.ctx, r.lvl, 1, 4, 2, rows=0)
    assert plan.keyswitches == 2 and plan.gather_in_force()                            # two steps, the gathering tail
    glk = r.glk(plan.galois_elements)
    return Case("lsa_bfv_slot_sum", [r.A[0]], dict(plan=plan._handle(), glk=glk), 2 * r.L * r.n,
                lambda x: slot_sum(r.ev, x, r.lvl, 1, 4, 2, 0), "lsa_bfv_slot_sum", same=(True,), level_arg=False)


def _ckks_lt(r):
    from lattisense_amd.device import LinearTransformPlan
    from oracle.ckks_bootstrap import Ct, linear_transform
    rng = np.random.default_rng(21)
    diags = {k: (rng.uniform(-1, 1, 8) + 1j * rng.uniform(-1, 1, 8)) / 4 for k in range(4)}
    plan = r.plans["lt"] = LinearTransformPlan(r.ctx, r.lvl, diags, ratio=1.0)
    assert plan.n1 == 2 and len(plan.diagonals) == 4 and plan.double_hoist           # 2 x 2: one baby rotation, one giant step
    glk = r.glk(plan.galois_elements)
    plains = plan.oracle_plains()
    return Case("lsa_ckks_linear_transform", [r.A[0]], dict(plan=plan.h, glk=glk, rescale=1), 2 * r.lvl * r.n,
                lambda x: linear_transform(r.ev, Ct(x, r.lvl, 1.0), diags, 1.0, plains=plains, rescale=True, n_slots=8, double_hoist=True).data,
                "linear transform", level_arg=False)


def _bfv_lt(r):
    from lattisense_amd.device import BfvLinearTransformPlan
    from tests.bfv_lt_model import linear_transform
    rng = np.random.default_rng(22)
    index = [0, 1, 2, 3]
    plan = r.plans["lt"] = BfvLinearTransformPlan(r.ctx, r.lvl, {k: rng.integers(0, r.t, (2, 8), dtype=np.uint64) for k in index}, ratio=1.0)
    assert plan.n1 == 2 and plan.moddowns == 2                                       # one giant step besides giant 0
    glk = r.glk(plan.galois_elements)
    plains = plan.oracle_plains()
    return Case("lsa_bfv_linear_transform", [r.A[0]], dict(plan=plan._handle(), glk=glk), 2 * r.L * r.n,
                lambda x: linear_transform(r.ev, x, r.lvl, 8, index, plains, 1.0), "lsa_bfv_linear_transform", level_arg=False)


def _ckks_poly(r):
    from lattisense_amd.device import PolynomialPlan
    from oracle.ckks_bootstrap import Ct
    from tests import poly_model as pm
    coeffs = [0.25, -0.5, 0.125, 0.375]
    scale = float(2 ** (int(r.q[r.lvl]).bit_length() - 1))
    plan = r.plans["poly"] = PolynomialPlan(r.ctx, coeffs, r.lvl, scale, log_baby=1)
    assert plan.log_baby == 1 and plan.mults >= 2
    consts = plan.constants()
    return Case("lsa_ckks_poly_eval", [r.A[0]], dict(plan=plan.h, key=r.key["rlk"]), 2 * (plan.level_out + 1) * r.n,
                lambda x: pm.evaluate(r.ev, Ct(x, r.lvl, scale), coeffs, "chebyshev", (-1, 1), None, 1, constants=consts)[0].data, "poly",
                level_arg=False)


def _bfv_poly(r):
    from lattisense_amd.device import BfvPolynomialPlan
    from tests import bfv_poly_model
    coeffs = [3, r.t - 1, 5, 7]
    plan = r.plans["poly"] = BfvPolynomialPlan(r.ctx, coeffs, r.lvl, 1)
    assert plan.log_baby == 1 and plan.n_mult >= 2
    return Case("lsa_bfv_poly_eval", [r.A[0]], dict(plan=plan.h, key=r.key["rlk"]), 2 * r.L * r.n,
                lambda x: bfv_poly_model.evaluate(r.o, r.lvl, x, coeffs, r.raw["rlk"], r.klvl, 1), "bfv_poly", level_arg=False)


def _bfv_affine(r):
    from tests import bfv_poly_model
    k, c = (r.t - 1) // 2, r.t - 1
    return Case("lsa_bfv_affine_const", [r.A[0]], dict(k=k, c=c), 2 * r.L * r.n, lambda x: bfv_poly_model.affine_const(r.o, r.lvl, x, k, c),
                "lsa_bfv_affine_const", same=(True,))


def _ckks_dot(which):
    def case(r):
        from tests.test_gpu_ckks_dot import oracle_d3, oracle_dot
        if which == "sum":
            return Case("lsa_ckks_mult_sum", r.A + r.B + [r.E], dict(n=3, addend=True), 3 * r.L * r.n,
                        lambda a0, a1, a2, b0, b1, b2, e: oracle_d3(r.o, r.lvl, [a0, a1, a2], [b0, b1, b2], e), "dot", shared=(True,) * 7,
                        nullable=(6,))
        return Case("lsa_ckks_dot", r.A + r.B + [r.E], dict(n=3, addend=True, key=r.key["rlk"], rescale=1), 2 * r.lvl * r.n,
                    lambda a0, a1, a2, b0, b1, b2, e: oracle_dot(r.o, r.lvl, [a0, a1, a2], [b0, b1, b2], r.raw["rlk"], r.klvl, True, e), "dot",
                    shared=(True,) * 7, nullable=(6,), min_level=1)
    return case


def _bfv_dot(which):
    def case(r):
        from tests import bfv_dot_model
        if which == "sum":
            return Case("lsa_bfv_mult_sum", r.A + r.B + [r.E], dict(n=3, addend=True), 3 * r.L * r.n,
                        lambda a0, a1, a2, b0, b1, b2, e: bfv_dot_model.mult_sum(r.o, r.lvl, [a0, a1, a2], [b0, b1, b2], e), "bfv_dot",
                        shared=(True,) * 7, nullable=(6,))
        return Case("lsa_bfv_dot", r.A + r.B + [r.E], dict(n=3, addend=True, key=r.key["rlk"]), 2 * r.L * r.n,
                    lambda a0, a1, a2, b0, b1, b2, e: bfv_dot_model.dot(r.o, r.lvl, [a0, a1, a2], [b0, b1, b2], r.raw["rlk"], r.klvl, e), "bfv_dot",
                    shared=(True,) * 7, nullable=(6,))
    return case


CASES = {"bfv_rotate_many": _bfv_rotate_many, "bfv_mult_plain_mul": _bfv_mult_plain_mul, "bfv_mac_plain_mul": _bfv_mac_plain_mul,
         "bfv_rotate_mac_plain_mul": _bfv_rotate_mac, "ckks_slot_sum": _ckks_slot_sum, "bfv_slot_sum": _bfv_slot_sum,
         "ckks_linear_transform": _ckks_lt, "bfv_linear_transform": _bfv_lt, "ckks_poly_eval": _ckks_poly, "bfv_poly_eval": _bfv_poly,
         "bfv_affine_const": _bfv_affine, "ckks_mult_sum": _ckks_dot("sum"), "ckks_dot": _ckks_dot("dot"),
         "bfv_mult_sum": _bfv_dot("sum"), "bfv_dot": _bfv_dot("dot")}
CKKS_CASES = ["ckks_slot_sum", "ckks_linear_transform", "ckks_poly_eval", "ckks_mult_sum", "ckks_dot"]
BFV_CASES = ["bfv_rotate_many", "bfv_mult_plain_mul", "bfv_mac_plain_mul", "bfv_rotate_mac_plain_mul", "bfv_slot_sum",
             "bfv_linear_transform", "bfv_poly_eval", "bfv_affine_const", "bfv_mult_sum", "bfv_dot"]
ALL_CASES = [("ckks", c) for c in CKKS_CASES] + [("bfv", c) for c in BFV_CASES]
# the gathering and LDS-staged tails once more where the transforms take two passes
TWO_PASS_CASES = [("ckks2", "ckks_slot_sum"), ("ckks2", "ckks_linear_transform"), ("bfv2", "bfv_slot_sum"), ("bfv2", "bfv_rotate_many"),
                  ("bfv2", "bfv_rotate_mac_plain_mul"), ("bfv2", "bfv_linear_transform")]
IDS = lambda cases: ["%s-%s" % c for c in cases]  # noqa: E731


def _args(r, c, ins, outs):
    a = dict(ptrs=[f.ptr for f in ins], strides=[f.stride for f in ins], out=[f.ptr for f in outs] if c.n_out > 1 else outs[0].ptr,
             so=outs[0].stride, batch=r.batch, level=r.lvl)
    a.update(c.extra)
    return a


def _model(r, case, c, item=None, tag=None):
    """the model on every batch item; item(i) -> that item's inputs (default: item i of every array)"""
    item = item or (lambda i: [a[i] for a in c.arrays])
    return r.want((case, tag), lambda i: c.fn(*[np.ascontiguousarray(x) for x in item(i)]))


def _expect(c, outs, want):
    for j, f in enumerate(outs):
        f.expect(want[:, j] if c.n_out > 1 else want)


def _padded(r, case):
    c = r.case(case)
    want = _model(r, case, c)
    ins = padded_operands(r.ctx, c.arrays, r.batch)
    outs = padded_outputs(r.ctx, c.wout, r.batch, ins, c.n_out)
    fields = ins + outs
    assert outs[0].stride > max(f.stride for f in ins) and all(f.base % r.n and f.base % 2 == 0 for f in fields)
    assert len({f.base for f in fields}) == len(fields) and len({f.stride for f in ins}) == len(ins)
    _ok(invoke(c.name, r.ctx.h, _args(r, c, ins, outs), r.ctx.stream))
    _expect(c, outs, want)
    for j, f in enumerate(outs):
        f.check("%s: output %d" % (case, j))
    for i, f in enumerate(ins):
        f.check("%s: input %d" % (case, i))


# ------------------------------------------------------------------------------------------------ padded layouts, tiles
@pytest.mark.parametrize("dual", [0, 1])
@pytest.mark.parametrize("rig,case", ALL_CASES, ids=IDS(ALL_CASES))
def test_padded_layout_in_tiles(rig, case, dual):
    r = _rig(rig)
    try:
        r.settings(dual)
        _padded(r, case)
    finally:
        r.settings(0, tile=0)


@pytest.mark.parametrize("rig,case", ALL_CASES, ids=IDS(ALL_CASES))
def test_padded_layout_automatic_tile(rig, case):
    r = _rig(rig)
    r.settings(0, tile=0)
    _padded(r, case)


@pytest.mark.parametrize("dual", [0, 1])
@pytest.mark.parametrize("rig,case", TWO_PASS_CASES, ids=IDS(TWO_PASS_CASES))
def test_two_pass_ring_padded_layout_in_tiles(rig, case, dual):
    r = _rig(rig)
    try:
        r.settings(dual)
        _padded(r, case)
    finally:
        r.settings(0, tile=0)


# ------------------------------------------------------------------------------------------------ shared operands, squares
def _shared(r, case, which, square=False):
    """stride 0 on the inputs `which` (item 1 of each for the whole batch); square: bs[0] IS as[0], pointer and stride"""
    c = r.case(case)
    assert all(c.shared[k] for k in which)

    def item(i):
        x = [a[1] if k in which else a[i] for k, a in enumerate(c.arrays)]
        if square:
            x[c.extra["n"]] = x[0]
        return x
    want = _model(r, case, c, item, ("shared", tuple(which), square))
    ins = padded_operands(r.ctx, c.arrays, r.batch)
    for k in which:                                        # one item at the operand's own base, stride 0
        ins[k] = Field(r.ctx, ins[k].words, r.batch, ins[k].base, 0, c.arrays[k][1])
    if square:
        ins[c.extra["n"]] = ins[0]
    outs = padded_outputs(r.ctx, c.wout, r.batch, ins, c.n_out)
    _ok(invoke(c.name, r.ctx.h, _args(r, c, ins, outs), r.ctx.stream))
    _expect(c, outs, want)
    outs[0].check("%s shared %s: output" % (case, which))
    for i, f in enumerate(ins):
        f.check("%s shared %s: input %d" % (case, which, i))


SHARED = [("bfv", "bfv_mult_plain_mul", (1,)), ("bfv", "bfv_mac_plain_mul", (3, 4, 5)), ("bfv", "bfv_rotate_mac_plain_mul", (1, 2, 3)),
          ("ckks", "ckks_mult_sum", (3, 4, 5, 6)), ("ckks", "ckks_dot", (3, 4, 5, 6)), ("bfv", "bfv_mult_sum", (3, 4, 5, 6)),
          ("bfv", "bfv_dot", (3, 4, 5, 6))]


@pytest.mark.parametrize("dual", [0, 1])
@pytest.mark.parametrize("rig,case,which", SHARED, ids=["%s-%s" % s[:2] for s in SHARED])
def test_shared_operands(rig, case, which, dual):
    """stride 0 on the plaintexts; on the b side and the addend of the inner products"""
    r = _rig(rig)
    try:
        r.settings(dual)
        _shared(r, case, which)
    finally:
        r.settings(0, tile=0)


@pytest.mark.parametrize("rig,case", [("ckks", "ckks_mult_sum"), ("ckks", "ckks_dot"), ("bfv", "bfv_mult_sum"), ("bfv", "bfv_dot")])
def test_square_term(rig, case):
    """as[0] == bs[0] with equal strides: the BFV runner extends that operand once"""
    r = _rig(rig)
    try:
        r.settings(1)
        _shared(r, case, (), square=True)
    finally:
        r.settings(0, tile=0)


# ------------------------------------------------------------------------------------------------ in place
IN_PLACE = [("ckks", "ckks_slot_sum", 0), ("bfv", "bfv_slot_sum", 0), ("bfv", "bfv_affine_const", 0), ("bfv", "bfv_mult_plain_mul", 0)]


@pytest.mark.parametrize("dual", [0, 1])
@pytest.mark.parametrize("rig,case,target", IN_PLACE, ids=["%s-%s" % s[:2] for s in IN_PLACE])
def test_in_place(rig, case, target, dual):
    r = _rig(rig)
    c = r.case(case)
    assert c.same[target] and c.wout == c.arrays[target][0].size
    want = _model(r, case, c)
    try:
        r.settings(dual)
        ins = padded_operands(r.ctx, c.arrays, r.batch)
        _ok(invoke(c.name, r.ctx.h, _args(r, c, ins, [ins[target]]), r.ctx.stream))
        ins[target].expect(want)
        for i, f in enumerate(ins):
            f.check("%s in place over input %d: operand %d" % (case, target, i))
    finally:
        r.settings(0, tile=0)


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("dual", [0, 1])
def test_bfv_rotate_many_one_output_is_the_input(dual, which):
    """exactly one output IS the input, first, middle or last in the list, in tiles of 2: every other rotation of every tile, and
    the in-place one itself, must still see the intact ciphertext"""
    r = _rig("bfv")
    c = r.case("bfv_rotate_many")
    want = _model(r, "bfv_rotate_many", c)
    try:
        r.settings(dual)
        w = c.wout
        src = Field(r.ctx, w, r.batch, 38, w + GAP, c.arrays[0])
        outs = [src if j == which else Field(r.ctx, w, r.batch, 74 + 36 * j, w + GAP) for j in range(3)]
        _ok(invoke(c.name, r.ctx.h, _args(r, c, [src], outs), r.ctx.stream))
        _expect(c, outs, want)
        for j, f in enumerate(outs):
            f.check("rotate_many, output %d is the input: output %d" % (which, j))
    finally:
        r.settings(0, tile=0)


# ------------------------------------------------------------------------------------------------ interleaved
@pytest.mark.parametrize("rig,case", ALL_CASES, ids=IDS(ALL_CASES))
def test_interleaved_operands(rig, case):
    """Overlap is exact, padding belongs to nobody: the outputs live BETWEEN the items of the first input, in the same buffer
    (item b | gap | output 0 of b | gap | output 1 of b ... | item b + 1), every other input in a padded buffer of its own."""
    r = _rig(rig)
    c = r.case(case)
    want = _model(r, case, c)
    try:
        r.settings(1)
        w = c.arrays[0][0].size
        slot = c.wout + GAP
        stride = w + GAP + c.n_out * slot
        f = Field(r.ctx, w, r.batch, 38, stride, c.arrays[0], room=stride)
        rest = padded_operands(r.ctx, c.arrays, r.batch)[1:]
        offs = [w + GAP + j * slot for j in range(c.n_out)]
        a = dict(ptrs=[f.ptr] + [x.ptr for x in rest], strides=[stride] + [x.stride for x in rest],
                 out=[f.ptr + 8 * o for o in offs] if c.n_out > 1 else f.ptr + 8 * offs[0], so=stride, batch=r.batch, level=r.lvl)
        a.update(c.extra)
        _ok(invoke(c.name, r.ctx.h, a, r.ctx.stream))
        for j, o in enumerate(offs):
            for b in range(r.batch):
                at = f.base + b * stride + o
                f.image[at:at + c.wout] = (want[b, j] if c.n_out > 1 else want[b]).ravel()
        f.check(case + ": interleaved")
        for i, x in enumerate(rest):
            x.check("%s: interleaved, input %d" % (case, i + 1))
    finally:
        r.settings(0, tile=0)


# ------------------------------------------------------------------------------------------------ refusals
def _refusals(r, other, case):
    """every refusal of the case's entry point that its argument checks make (lattisense_amd/csrc: EntryCheck for the BFV
    operators and the slot sums, dot_check, lt_run, poly_run, bfv_lt_run); other: a context of the other scheme"""
    c = r.case(case)
    # room behind every input: the overlapping outputs below stay inside the input's own allocation
    room = r.batch * (max([c.wout] + [a[0].size for a in c.arrays]) + 128)
    ins = padded_operands(r.ctx, c.arrays, r.batch, room=room)
    outs = padded_outputs(r.ctx, c.wout, r.batch, ins, c.n_out, room=room)
    out = outs[0]
    good = _args(r, c, ins, outs)
    bad = []                                               # (what, arguments, context handle)

    def mut(what, h=None, **kw):
        a = dict(good)
        a["ptrs"], a["strides"] = list(good["ptrs"]), list(good["strides"])
        for k, v in kw.items():
            if k in ("ptr", "stride"):
                a[k + "s"][v[0]] = v[1]
            elif k == "out" and c.n_out > 1:               # the middle output of several
                a["out"] = [good["out"][0], v, good["out"][2]]
            elif k in ("key", "g") and isinstance(good.get(k), list):
                a[k] = list(good[k])
                a[k][-1] = v
            else:
                a[k] = v
        bad.append((what, a, h if h is not None else r.ctx.h))

    for i, f in enumerate(ins):
        if i not in c.nullable:
            mut("input %d null" % i, ptr=(i, None))
        mut("input %d stride short" % i, stride=(i, f.words - 2))
        mut("input %d stride odd" % i, stride=(i, f.stride + 1))
        mut("input %d stride negative" % i, stride=(i, -f.stride))
        mut("input %d misaligned" % i, ptr=(i, f.ptr + 8))
        if not c.shared[i]:
            mut("input %d shared" % i, stride=(i, 0))
        mut("out one item into input %d" % i, out=f.ptr + 8 * f.stride)
        mut("out starting in the padding of input %d, reaching its next item" % i, out=f.ptr + 8 * f.words,
            so=f.stride if c.wout <= f.words else out.stride)
        if c.same[i]:
            mut("out == input %d with another stride" % i, out=f.ptr, so=f.stride + 2)
        else:
            mut("out == input %d" % i, out=f.ptr, so=max(f.stride, c.wout + 2))
    mut("out null", out=None)
    mut("out stride 0", so=0)
    mut("out stride short", so=c.wout - 2)
    mut("out stride odd", so=out.stride + 1)
    mut("out stride negative", so=-out.stride)
    mut("out misaligned", out=out.ptr + 8)
    if c.n_out > 1:                                        # the rule of the hoisted rotations
        o0, o1, o2 = good["out"]
        src = ins[0]
        bad.append(("two outputs equal", dict(good, out=[o0, o2, o2]), r.ctx.h))
        bad.append(("two outputs one item apart", dict(good, out=[o0, o2 + 8 * out.stride, o2]), r.ctx.h))
        bad.append(("an output starting in another's padding, reaching its next item", dict(good, out=[o0, o1, o1 + 8 * c.wout]), r.ctx.h))
        bad.append(("two outputs are the input", dict(good, out=[src.ptr, src.ptr, o2], so=src.stride), r.ctx.h))
        bad.append(("an output one item into the input, its stride", dict(good, out=[o0, src.ptr + 8 * src.stride, o2], so=src.stride), r.ctx.h))
        bad.append(("an output one word past the input, its stride", dict(good, out=[o0, o1, src.ptr + 16], so=src.stride), r.ctx.h))
    if c.level_arg:
        mut("level -1", level=-1)
        mut("level past the chain", level=len(r.q))
        if c.min_level == 1:
            mut("level 0", level=0)
        if c.bound:
            mut("context of the other scheme", h=other.ctx.h)
    if "key" in c.extra:
        mut("key null", key=None)
        mut("key below the level", key=r.low_key())
    if c.name == "lsa_bfv_rotate_mac_plain_mul":
        mut("Galois element even", g=4)
    if c.extra.get("n"):
        mut("no terms", n=0)
    for what, a, h in bad:
        rc = invoke(c.name, h, a, r.ctx.stream)
        assert rc == ARG, (case, what, rc, last_error())
        assert last_error().startswith(c.prefix), (case, what, last_error())
    for nb in (0, -1):                                     # a no-op, whatever else is passed
        _ok(invoke(c.name, r.ctx.h, dict(good, batch=nb), r.ctx.stream))
    for j, f in enumerate(outs):
        f.check("%s: a refused call or an empty batch wrote to output %d" % (case, j))
    for f in ins:
        f.check(case + ": a refused call wrote to an input")
    _ok(invoke(c.name, r.ctx.h, good, r.ctx.stream))      # the context still works
    _expect(c, outs, _model(r, case, c))
    for j, f in enumerate(outs):
        f.check("%s: the call after the refusals, output %d" % (case, j))


@pytest.mark.parametrize("rig,case", ALL_CASES, ids=IDS(ALL_CASES))
def test_refusals(rig, case):
    r, other = _rig(rig), _rig("bfv" if rig == "ckks" else "ckks")
    r.settings(1)
    try:
        _refusals(r, other, case)
    finally:
        r.settings(0, tile=0)
    assert SENT not in (int(x) for x in r.q + r.p)
