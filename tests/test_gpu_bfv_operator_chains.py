"""The BFV operators of the key-switch layer -- lsa_bfv_mult_sum / lsa_bfv_dot, lsa_bfv_slot_sum, lsa_bfv_encode,
lsa_bfv_linear_transform, lsa_bfv_poly_eval / lsa_bfv_affine_const -- on the three chains their own files never reach
(tests/boundary.py bfv_operator_chain, t = 65537):

  fp       4 Q + 2 P, every limb below 2^47: all six rows of Q u P on the FP64 butterfly engine;
  mixed    46, 59, 47, 58, 48 and 58-bit Q limbs with two 61-bit P: both engines inside every launch over Q u P;
  ceiling  six primes just below 2^61: no FP64-engine row, every product at the lazy reductions' bound;

at N = 2^11 (2^12 for the two operators on the multiply) -- single pass -- and at 2^13 and 2^14, the two two-pass plans.  The
relinearisation key is pattern_key("top"), the Galois keys rotate through max / top / half / uniform, all exported at the top
level; the ciphertexts are batch 3 of the patterns max / top / uniform (second operands alt / uniform / half) as the
coefficient-domain words the entry points take.  Every comparison is exact equality with the CPU model on every batch item.

Levels: `top` is the chain's top level (digits of two limbs each), `lift` the highest level below it with an odd number of limbs
(fp 2, mixed 4, ceiling 2): its last digit is one limb -- below 2^53 on fp and mixed, where the extension transform's load lifts it
instead of a base conversion, above 2^53 on ceiling, where the conversion is kept.  No operator refuses a level on these chains
(tests/test_bfv_operator_chains.py), so none is lowered.

On the two-pass rings every operator runs once more per chain with the integer engine forced (on fp and mixed this changes the
engine of real rows), without the ModUp lift, with unfused tails, in tiles of 1 and 2 on two streams and with 1 MiB transform
chunks, against the words already held to the model.  What is in force -- engine per row, the lifted digit, the fused second
pass + key MAC, the 29-bit split of the conversions -- is read back from the context and asserted, not assumed.

Run time: the slowest test of tests/test_gpu_bfv_slot_sum.py + tests/test_gpu_bfv_lt.py takes 0.8 s and bounds every test
here, and the time is the oracle's.  So the device words of a case are cached per (rig, case), each model walk runs once per
(rig, case, batch item), and the tests of the four key-switching operators are split by batch item (the inner product also
into n <= 3 and n = 17).  The two log_baby = 4 cases of the polynomial evaluator (14 oracle multiplications per item) stay
above the bound at N = 2^14 even so (0.96 s per item on the mixed chain) and run at 2^12 and 2^13 only; every other cell runs on all three rings."""
import numpy as np
import pytest

from tests import bfv_dot_model, bfv_poly_model
from tests.bfv_chain_cases import (AFFINE_VALUES, CHAINS, DENSE4, DOT_TERMS, LT_CASES, POLY_CASES, RINGS, RINGS_MULT, SLOT_CASES, T,
                                   TWO_PASS, levels, lt_diags)
from tests.bfv_lt_model import encode_ext, encode_pt_mul, linear_transform, model_plains
from tests.bfv_slot_sum_model import make_evaluator, slot_sum
from tests.boundary import bfv_operator_chain, fp_engine, pattern_ct, pattern_key
from tests.gpu_util import env, need_gpu

pytestmark = pytest.mark.gpu
BATCH = 3
ITEMS = (0, 1, 2)
A_PATTERNS, B_PATTERNS = ("max", "top", "uniform"), ("alt", "uniform", "half")
KEY_PATTERNS = ("max", "top", "half", "uniform")
FP_ROWS = {"fp": lambda k: k == 6, "mixed": lambda k: k >= 2, "ceiling": lambda k: k == 0}
_RIGS = {}


class Rig:
    """one context, oracle, relinearisation key and operand pool per (chain, ring); Galois keys are made on demand"""

    def __init__(self, kind, logn):
        from lattisense_amd.device import ALGO_BFV, DeviceContext
        from oracle.client import Client
        from oracle.pyoracle import Oracle
        self.kind, self.logn, self.n = kind, logn, 1 << logn
        n = self.n
        self.q, self.p = bfv_operator_chain(kind, n)
        self.top, self.lift = levels(kind, n)
        self.klvl = self.top
        self.o = Oracle(n, self.q, self.p, T)
        self.c = Client(self.o, seed=logn)
        self.ctx = DeviceContext(ALGO_BFV, n, self.q, self.p, T)
        assert self.ctx.moduli == self.o.mod                              # the same auxiliary primes on both sides
        self.rng = np.random.default_rng(1000 * logn + CHAINS.index(kind))
        self.beta = (self.klvl + 1 + len(self.p) - 1) // len(self.p)
        self.key = pattern_key("top", self.q + self.p, self.beta, n, self.rng)
        self.k = self.ctx.upload_key(self.key, self.klvl)
        self.ev = make_evaluator(self.o, self.c, self.klvl)
        self.dev_glk = {}
        self.A = [pattern_ct(A_PATTERNS, self.q, 2, n, self.rng) for _ in range(3)]
        self.B = [pattern_ct(B_PATTERNS, self.q, 2, n, self.rng) for _ in range(3)]
        self.E = pattern_ct(A_PATTERNS, self.q, 2, n, self.rng)
        self._host, self._dev, self.words, self.plans, self.held = {}, {}, {}, [], set()

    def level(self, which):
        return {"top": self.top, "lift": self.lift, "zero": 0}[which]

    def host(self, x, lvl):
        """the pool ciphertext x at `lvl`: (the batch [3][2][lvl+1][N], one stable view per item for the models' caches)"""
        key = (id(x), lvl)
        if key not in self._host:
            h = np.ascontiguousarray(x[:, :, : lvl + 1])
            self._host[key] = (h, [h[b] for b in range(BATCH)])
        return self._host[key]

    def dev(self, x, lvl):
        key = (id(x), lvl)
        if key not in self._dev:
            self._dev[key] = self.ctx.upload(self.host(x, lvl)[0])
        return self._dev[key]

    def keys_for(self, elements):
        """pattern Galois keys, in the evaluator (so the model walks use them) and on the device"""
        for g in elements:
            if g not in self.dev_glk:
                assert g not in self.ev.glk
                name = KEY_PATTERNS[len(self.dev_glk) % len(KEY_PATTERNS)]
                self.ev.glk[g] = pattern_key(name, self.q + self.p, self.beta, self.n, self.rng)
                self.dev_glk[g] = self.ctx.upload_key(self.ev.glk[g], self.klvl)
        return {g: self.dev_glk[g] for g in elements}

    def hold(self, key, lvl, items, got, model):
        """got[b] == model(b) for b in items, once per (case, item): a model walk is shared by every test of its case"""
        for b in items:
            if (key, b) not in self.held:
                want = model(b)
                assert np.array_equal(got[b], want), ("item %d differs from the model" % b, key, self.tag(lvl))
                self.held.add((key, b))

    def fused(self, lvl):
        return self.ctx.key_switch_fused(lvl, self.k)

    def tag(self, lvl):
        """what is in force at this level, for the assertion messages"""
        rows = self.q[: lvl + 1] + self.p
        return "%s N=2^%d level %d: %d/%d FP64 rows, last digit %d limb(s) of %d bits, fused key MAC %s" % (
            self.kind, self.logn, lvl, sum(fp_engine(m) for m in rows), len(rows), 2 - (lvl + 1) % 2, self.q[lvl].bit_length(),
            self.fused(lvl))

    def close(self):
        for plan in self.plans:                                          # a plan goes before its context
            plan.close()
        self.ctx.close()


def rig(kind, logn):
    need_gpu()
    if (kind, logn) not in _RIGS:
        _RIGS[(kind, logn)] = Rig(kind, logn)
    return _RIGS[(kind, logn)]


@pytest.fixture(scope="module", autouse=True)
def _close_rigs():
    yield
    for r in _RIGS.values():
        r.close()
    _RIGS.clear()


def variants(r, lvl, run, want, what):
    """run() under each setting must give `want` again; every setting is put back"""
    from lattisense_amd._native import check, lib
    ctx = r.ctx

    def same(name):
        got = run()
        assert np.array_equal(got, want), (what, name, r.tag(lvl), np.argwhere((got != want).any(axis=-1))[:8].tolist())

    ctx.set_fp64_ntt(0)
    try:
        assert not r.fused(lvl)
        same("integer engine")
    finally:
        ctx.set_fp64_ntt(1)
    ctx.set_modup_lift(0)
    try:
        same("no ModUp lift")
    finally:
        ctx.set_modup_lift(1)
    check(lib().lsa_set_fuse_tails(ctx.h, 0))
    try:
        same("unfused tails")
    finally:
        check(lib().lsa_set_fuse_tails(ctx.h, 1))
    check(lib().lsa_set_dual_stream(ctx.h, 1))
    try:
        for tile in (1, 2):
            ctx.set_tile_batch(tile)
            same("tile batch %d, dual stream" % tile)
    finally:
        ctx.set_tile_batch(0)
        check(lib().lsa_set_dual_stream(ctx.h, 0))
    ctx.set_ntt_chunk_mib(1)
    try:
        same("1 MiB chunks")
    finally:
        ctx.set_ntt_chunk_mib(0)


# ---------------------------------------------------------------- what is in force

@pytest.mark.parametrize("logn", (11, 12, 13, 14))
@pytest.mark.parametrize("kind", CHAINS)
def test_engines_lift_and_fused_key_mac_as_read_back(kind, logn):
    """the non-vacuity of everything below: FP64-engine rows of Q u P are 6 / at least 2 / 0; the lift level's last digit is one
    limb on the lifted side of 2^53 (fp, mixed) or on the converted side (ceiling); the fused key MAC is read back -- never on
    ceiling, never on a single-pass ring, on both levels of the fp and mixed chains at the two-pass rings"""
    r = rig(kind, logn)
    mods = r.q + r.p
    assert FP_ROWS[kind](sum(fp_engine(m) for m in mods)), r.tag(r.top)
    assert (r.top + 1) % 2 == 0 and (r.lift + 1) % 2 == 1 and len(r.p) == 2
    assert (r.q[r.lift] >> 53 == 0) == (kind != "ceiling"), r.tag(r.lift)
    for lvl in (r.top, r.lift):
        fused = r.fused(lvl)
        print("IN FORCE:", r.tag(lvl))
        if kind == "ceiling" or logn <= 12:
            assert not fused, r.tag(lvl)
        if kind != "ceiling" and logn >= 13:                       # some target row is an FP64-engine limb: those rows take it
            assert fused, r.tag(lvl)
        with env(LSA_KS_FUSED="0"):
            assert not r.fused(lvl)


def check_conversion_plans(r, lvl):
    """as tests/test_gpu_boundary.py test_bfv_operators: ModUp digits and ModDown have at most two sources and stay inside Q u P --
    split into 29-bit halves exactly where every prime of Q u P is below 2^58 (fp); the multiply's conversions to and from the
    61-bit auxiliary base have three or more sources and never qualify"""
    plans = r.ctx.baseconv_plans()
    assert any(ns <= len(r.p) for ns, _, _ in plans) and any(ns >= lvl + 1 for ns, _, _ in plans), plans
    for ns, nd, split in plans:
        assert split == (r.kind == "fp" and ns <= len(r.p)), (r.tag(lvl), ns, nd, split, plans)


# ---------------------------------------------------------------- lsa_bfv_mult_sum / lsa_bfv_dot

def _dot_operands(r, lvl, n):
    ia, ib = [i % 3 for i in range(n)], [(2 * i + 1) % 3 for i in range(n)]     # nine distinct pairs from 3 + 3 ciphertexts
    return ([r.host(r.A[i], lvl)[1] for i in ia], [r.host(r.B[i], lvl)[1] for i in ib],
            [r.dev(r.A[i], lvl) for i in ia], [r.dev(r.B[i], lvl) for i in ib])


def _dot_run(r, lvl, n, addend):
    _, _, dA, dB = _dot_operands(r, lvl, n)
    dE = r.dev(r.E, lvl) if addend else None
    return r.ctx.download(r.ctx.bfv_dot(lvl, dA, dB, r.k, BATCH, addend=dE), (BATCH, 2, lvl + 1, r.n))


def dot_words(r, lvl, n, addend, items=ITEMS):
    """dot == relin(mult_sum) on the batch; d3 and the dot against the model on `items`; returns the dot"""
    key = ("dot", lvl, n, addend)
    ctx, o = r.ctx, r.o
    vA, vB, dA, dB = _dot_operands(r, lvl, n)
    hE, dE = (r.host(r.E, lvl)[1], r.dev(r.E, lvl)) if addend else (None, None)
    if key not in r.words:
        d3 = ctx.bfv_mult_sum(lvl, dA, dB, BATCH, addend=dE)
        got3 = ctx.download(d3, (BATCH, 3, lvl + 1, r.n))
        got = _dot_run(r, lvl, n, addend)
        assert np.array_equal(got, ctx.download(ctx.bfv_relin(lvl, d3, r.k, BATCH), got.shape)), ("dot == relin(mult_sum)", key, r.tag(lvl))
        r.words[key] = (got3, got)
    got3, got = r.words[key]

    def model(b):
        want3 = bfv_dot_model.mult_sum(o, lvl, [a[b] for a in vA], [x[b] for x in vB], hE[b] if addend else None)
        assert np.array_equal(got3[b], want3), ("mult_sum: item %d differs from the model" % b, key, r.tag(lvl))
        return o.bfv_relin(lvl, want3, r.key, r.klvl)

    r.hold(key, lvl, items, got, model)
    return got


@pytest.mark.parametrize("item", ITEMS)
@pytest.mark.parametrize("terms", [DOT_TERMS[:3], DOT_TERMS[3:]], ids=["n1_2_3", "n%d" % DOT_TERMS[3]])
@pytest.mark.parametrize("addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("which", ["top", "lift"])
@pytest.mark.parametrize("logn", RINGS_MULT)
@pytest.mark.parametrize("kind", CHAINS)
def test_dot(kind, logn, which, addend, terms, item):
    """n in {1, 2, 3} and n = LSA_DOT_MAX_TERMS + 1 (two tensor launches), with and without an addend, at the top and at the
    lift level, one batch item per test; one term is bfv_mult_relin"""
    r = rig(kind, logn)
    lvl = r.level(which)
    for n in terms:
        dot_words(r, lvl, n, addend, (item,))
    if item == 0 and not addend and 1 in terms:
        one = r.ctx.download(r.ctx.bfv_mult_relin(lvl, r.dev(r.A[0], lvl), r.dev(r.B[1], lvl), r.k, BATCH), (BATCH, 2, lvl + 1, r.n))
        assert np.array_equal(r.words[("dot", lvl, 1, False)][1], one), ("n == 1 is bfv_mult_relin", r.tag(lvl))
    check_conversion_plans(r, lvl)


@pytest.mark.parametrize("logn", TWO_PASS)
@pytest.mark.parametrize("kind", CHAINS)
def test_dot_variants(kind, logn):
    r = rig(kind, logn)
    lvl = r.lift
    for n, addend in ((3, True), (DOT_TERMS[-1], False)):
        variants(r, lvl, lambda: _dot_run(r, lvl, n, addend), dot_words(r, lvl, n, addend), "dot n = %d" % n)


# ---------------------------------------------------------------- lsa_bfv_slot_sum

def _slot_level(r, case):
    return r.top if SLOT_CASES.index(case) % 2 else r.lift      # (7, 2, 0) with either step at the top level, the radix-4 shapes at lift


def slot_words(r, case, items=ITEMS):
    """(plan, keys, input, words): the gathering form, against the model on `items`"""
    from lattisense_amd.device import BfvSlotSumPlan
    key = ("slot", case)
    step, count, radix, rows = case
    lvl = _slot_level(r, case)
    if key not in r.words:
        plan = BfvSlotSumPlan(r.ctx, lvl, step, count, radix, rows)
        r.plans.append(plan)
        glk = r.keys_for(plan.galois_elements)                  # pattern keys into ev.glk before any model walk
        xin = r.dev(r.A[0], lvl)
        assert plan.gather_in_force()
        r.words[key] = (plan, glk, xin, r.ctx.download(plan.run(xin, BATCH, glk), (BATCH, 2, lvl + 1, r.n)))
    plan, glk, xin, got = r.words[key]
    _, host = r.host(r.A[0], lvl)

    def model(b):
        before = set(r.ev.glk)
        want = slot_sum(r.ev, host[b], lvl, step, count, radix, rows)
        assert set(r.ev.glk) == before, "the model asked for a key the plan did not list"
        return want

    r.hold(key, lvl, items, got, model)
    return plan, glk, xin, got


@pytest.mark.parametrize("item", ITEMS)
@pytest.mark.parametrize("case", SLOT_CASES, ids=["step%d_count%d_radix%d_rows%d" % c for c in SLOT_CASES])
@pytest.mark.parametrize("logn", RINGS)
@pytest.mark.parametrize("kind", CHAINS)
def test_slot_sum(kind, logn, case, item):
    """(count, radix, rows) in {(5, 4, 1), (21, 4, 1)} at the lift level and (7, 2, 0) with step 1 and -1 at the top level, one
    batch item per test; with item 0 the plain form and, on the first case, out == in"""
    r = rig(kind, logn)
    plan, glk, xin, got = slot_words(r, case, (item,))
    lvl = plan.level
    if item:
        return
    plan.gather = False
    try:
        assert np.array_equal(r.ctx.download(plan.run(xin, BATCH, glk), got.shape), got), ("plain form", case, r.tag(lvl))
        assert not plan.gather_in_force()
    finally:
        plan.gather = True
    if case == SLOT_CASES[0]:
        same = r.ctx.upload(r.host(r.A[0], lvl)[0])
        plan.run(same, BATCH, glk, out=same)
        assert np.array_equal(r.ctx.download(same, got.shape), got), ("out == in", case, r.tag(lvl))


@pytest.mark.parametrize("logn", TWO_PASS)
@pytest.mark.parametrize("kind", CHAINS)
def test_slot_sum_variants(kind, logn):
    r = rig(kind, logn)
    case = SLOT_CASES[2]                                         # 21 at radix 4 with the row step: a tail that is added to twice
    plan, glk, xin, got = slot_words(r, case)
    for gather in (True, False):
        plan.gather = gather
        try:
            variants(r, plan.level, lambda: r.ctx.download(plan.run(xin, BATCH, glk), got.shape), got, "slot sum %s gather %d" % (case, gather))
        finally:
            plan.gather = True


# ---------------------------------------------------------------- lsa_bfv_encode

def _encode_inputs(n, rng):
    rows = [np.zeros(n, dtype=np.uint64), np.full(n, T - 1, dtype=np.uint64)]
    for slot in (0, n // 2 - 1, n // 2, n - 1):
        v = np.zeros(n, dtype=np.uint64)
        v[slot] = 1
        rows.append(v)
    rows += [rng.integers(0, T, n).astype(np.uint64) for _ in range(2)]
    return np.stack(rows)


def encode_words(r, form, lvl):
    """(inputs, the device words held to the CPU client)"""
    key = ("encode", form, lvl)
    if key not in r.words:
        vals = _encode_inputs(r.n, np.random.default_rng(r.logn + form))
        if form == 0:
            want = np.stack([r.c.bfv_encode(v) for v in vals])[:, None]
            assert int(want.max()) < T
        else:
            want = np.stack([(encode_pt_mul if form == 1 else encode_ext)(r.o, r.c, lvl, v) for v in vals])
        rows = r.ctx.bfv_pt_rows(lvl, form)
        assert want.shape == (len(vals), rows, r.n)
        got = r.ctx.download(r.ctx.bfv_encode(lvl, form, vals), want.shape)
        for i in range(len(vals)):
            assert np.array_equal(got[i], want[i]), ("input %d, form %d" % (i, form), r.tag(lvl))
        r.words[key] = (vals, got)
    return r.words[key]


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("logn", RINGS)
@pytest.mark.parametrize("kind", CHAINS)
def test_encode(kind, logn, form):
    """all zeros, all t - 1, a single 1 in slot 0, N/2 - 1, N/2 and N - 1, two random vectors; at the top level and at level 0;
    once with a padded batch stride"""
    r = rig(kind, logn)
    for lvl in (r.top, 0):
        vals, got = encode_words(r, form, lvl)
    w = got.shape[1] * r.n                                        # level 0, batch 3, padded: the padding is nobody's
    sout = w + 64
    out = r.ctx.upload(np.full(3 * sout, 7, dtype=np.uint64))
    r.ctx.bfv_encode(0, form, vals[4:7], out=out, sout=sout)
    pad = r.ctx.download(out, (3, sout))
    assert np.array_equal(pad[:, :w].reshape(got[4:7].shape), got[4:7]) and np.all(pad[:, w:] == 7), (form, r.tag(0))


@pytest.mark.parametrize("logn", TWO_PASS)
@pytest.mark.parametrize("kind", CHAINS)
def test_encode_variants(kind, logn):
    r = rig(kind, logn)
    for form in (1, 2):
        vals, got = encode_words(r, form, r.top)
        variants(r, r.top, lambda: r.ctx.download(r.ctx.bfv_encode(r.top, form, vals), got.shape), got, "encode form %d" % form)


# ---------------------------------------------------------------- lsa_bfv_linear_transform

def _lt_level(r, name):
    return r.top if name == "D20" else r.lift


def lt_words(r, name, items=ITEMS):
    """(plan, keys, input, words): the plan's plaintexts are the model's; the transform against the model on `items`"""
    from lattisense_amd.device import BfvLinearTransformPlan
    key = ("lt", name)
    index = dict(LT_CASES)[name]
    lvl, period = _lt_level(r, name), r.n // 2
    if key not in r.words:
        diags = lt_diags(index, period, r.logn)
        plan = BfvLinearTransformPlan(r.ctx, lvl, diags, period)
        r.plans.append(plan)
        glk = r.keys_for(plan.galois_elements)
        xin = r.dev(r.A[0], lvl)
        got = r.ctx.download(plan.run(xin, BATCH, glk), (BATCH, 2, lvl + 1, r.n))
        plains = plan.oracle_plains()
        want_plains = model_plains(r.o, r.c, lvl, period, diags)
        assert sorted(plains) == sorted(want_plains) == sorted(k % period for k in index)
        for k in plains:
            assert np.array_equal(plains[k], want_plains[k]), ("plaintext of diagonal %d" % k, name, r.tag(lvl))
        r.words[key] = (plan, glk, xin, got, plains)
    plan, glk, xin, got, plains = r.words[key]
    _, host = r.host(r.A[0], lvl)

    def model(b):
        before = set(r.ev.glk)
        want = linear_transform(r.ev, host[b], lvl, period, index, plains)
        assert set(r.ev.glk) == before, "the model needed a key the plan did not list"
        return want

    r.hold(key, lvl, items, got, model)
    return plan, glk, xin, got


@pytest.mark.parametrize("item", ITEMS)
@pytest.mark.parametrize("name", [c[0] for c in LT_CASES])
@pytest.mark.parametrize("logn", RINGS)
@pytest.mark.parametrize("kind", CHAINS)
def test_linear_transform(kind, logn, name, item):
    """diagonals range(7) and the sparse set at the lift level, range(20) at the top level, period N/2; the second diagonal all
    t - 1, the third all 0; one batch item per test"""
    lt_words(rig(kind, logn), name, (item,))


@pytest.mark.parametrize("logn", TWO_PASS)
@pytest.mark.parametrize("kind", CHAINS)
def test_linear_transform_variants(kind, logn):
    r = rig(kind, logn)
    plan, glk, xin, got = lt_words(r, "D7")
    variants(r, plan.level, lambda: r.ctx.download(plan.run(xin, BATCH, glk), got.shape), got, "linear transform D7")


# ---------------------------------------------------------------- lsa_bfv_poly_eval / lsa_bfv_affine_const

def _poly_level(r, name):
    return r.top if name == "dense8" else r.lift


def _poly_run(r, lvl, coeffs, log_baby, d_in, batch=BATCH):
    from lattisense_amd.device import BfvPolynomialPlan
    plan = BfvPolynomialPlan(r.ctx, coeffs, lvl, log_baby)
    try:
        info = plan.info()
        counts = bfv_poly_model.counts(coeffs, log_baby)
        assert {k: info[k] for k in bfv_poly_model.COUNTS} == counts and info["level"] == lvl
        return r.ctx.download(plan.run(d_in, batch, r.k), (batch, 2, lvl + 1, r.n))
    finally:
        plan.close()


def poly_words(r, name, items=ITEMS):
    key = ("poly", name)
    _, coeffs, log_baby = [c for c in POLY_CASES if c[0] == name][0]
    lvl = _poly_level(r, name)
    if key not in r.words:
        r.words[key] = _poly_run(r, lvl, coeffs, log_baby, r.dev(r.A[0], lvl))
    _, host = r.host(r.A[0], lvl)
    r.hold(key, lvl, items, r.words[key], lambda b: bfv_poly_model.evaluate(r.o, lvl, host[b], coeffs, r.key, r.klvl, log_baby))
    return r.words[key]


# (the two log_baby = 4 cases at N = 2^14: see "Run time" above)
POLY_CELLS = [(kind, logn, c[0]) for kind in CHAINS for logn in RINGS_MULT for c in POLY_CASES if not (logn == 14 and c[2] == 4)]


@pytest.mark.parametrize("item", ITEMS)
@pytest.mark.parametrize("kind,logn,name", POLY_CELLS, ids=["%s-%d-%s" % c for c in POLY_CELLS])
def test_poly_eval(kind, logn, name, item):
    """dense 8 at the planner's choice (top level); at the lift level dense 16 at log_baby 2 and 4 and the 16 coefficients
    without x^9 at log_baby 4 (the leaf kernel's fold without a term); one batch item per test"""
    r = rig(kind, logn)
    if name == "no_x9_b4":
        coeffs = [c for c in POLY_CASES if c[0] == name][0][1]
        assert coeffs[9] == 0 and all(coeffs[:9]) and all(coeffs[10:]) and bfv_poly_model.counts(coeffs, 4)["n_pairs"] == 0
    poly_words(r, name, (item,))


@pytest.mark.parametrize("logn", RINGS_MULT)
@pytest.mark.parametrize("kind", CHAINS)
def test_affine_const(kind, logn):
    """k, c in {0, 1, t - 1, (t - 1) / 2, (t + 1) / 2} at the top level; item 0 is all q_j - 1: with k = (t - 1) / 2 the largest
    single product the leaf kernel is given"""
    r = rig(kind, logn)
    lvl = r.top
    _, items = r.host(r.A[0], lvl)
    d = r.dev(r.A[0], lvl)
    assert all(np.all(items[0][:, j] == r.q[j] - 1) for j in range(lvl + 1))
    for k in AFFINE_VALUES:
        for c in AFFINE_VALUES:
            got = r.ctx.download(r.ctx.bfv_affine_const(lvl, d, k, c, BATCH), (BATCH, 2, lvl + 1, r.n))
            for b in range(BATCH):
                assert np.array_equal(got[b], bfv_poly_model.affine_const(r.o, lvl, items[b], k, c)), (k, c, b, r.tag(lvl))


@pytest.mark.parametrize("logn", TWO_PASS)
@pytest.mark.parametrize("kind", CHAINS)
def test_poly_eval_variants(kind, logn):
    r = rig(kind, logn)
    name, coeffs, log_baby = POLY_CASES[1]
    lvl = _poly_level(r, name)
    variants(r, lvl, lambda: _poly_run(r, lvl, coeffs, log_baby, r.dev(r.A[0], lvl)), poly_words(r, name), "poly " + name)


# ---------------------------------------------------------------- the fused second pass + key MAC in force

def test_dot_and_poly_with_the_fused_key_mac_in_force():
    """the smallest ring from 2^13 up at which key_switch_fused reports the fused second pass + key MAC on the fp chain: lsa_bfv_dot
    (n = 2, with addend, batch 2) and lsa_bfv_poly_eval on a dense degree-3 polynomial against the model with the kernel in force
    (asserted), and the same words with LSA_KS_FUSED=0 (read per call; asserted off)"""
    r = None
    for logn in range(13, 17):
        r = rig("fp", logn)
        if r.fused(r.top):
            break
    lvl, batch = r.top, 2
    assert r.fused(lvl), ("no ring up to 2^16 runs the fused key MAC on the fp chain", r.tag(lvl))
    assert r.logn == 13, ("the fused key MAC starts at another ring than the first two-pass one", r.tag(lvl))
    vA, vB = [r.host(x, lvl)[1] for x in r.A[:2]], [r.host(x, lvl)[1] for x in r.B[:2]]
    dA, dB, dE = [r.dev(x, lvl) for x in r.A[:2]], [r.dev(x, lvl) for x in r.B[:2]], r.dev(r.E, lvl)
    hE, items = r.host(r.E, lvl)[1], r.host(r.A[0], lvl)[1]
    want_dot = [bfv_dot_model.dot(r.o, lvl, [a[b] for a in vA], [x[b] for x in vB], r.key, r.klvl, hE[b]) for b in range(batch)]
    want_poly = [bfv_poly_model.evaluate(r.o, lvl, items[b], DENSE4, r.key, r.klvl) for b in range(batch)]
    assert bfv_poly_model.counts(DENSE4)["n_pairs"] >= 1          # the evaluator ends in a dot: a key switch of its own
    for off in (None, "0"):
        with env(LSA_KS_FUSED=off):
            assert r.fused(lvl) == (off is None), (off, r.tag(lvl))
            got = r.ctx.download(r.ctx.bfv_dot(lvl, dA, dB, r.k, batch, addend=dE), (batch, 2, lvl + 1, r.n))
            poly = _poly_run(r, lvl, DENSE4, 0, r.dev(r.A[0], lvl), batch)
            for b in range(batch):
                assert np.array_equal(got[b], want_dot[b]), ("dot", off, b, r.tag(lvl))
                assert np.array_equal(poly[b], want_poly[b]), ("poly", off, b, r.tag(lvl))
