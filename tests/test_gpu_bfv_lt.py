"""BFV linear transform on the device (lsa_bfv_lt_* / lsa_bfv_linear_transform; linear_transform.hip bfv_lt_create / bfv_lt_run)
against its CPU model (tests/bfv_lt_model.py on oracle/ckks_bootstrap.py), fed the plan's own plaintexts: identical word for word
for every batch item -- on a one-pass ring (one to seven diagonals, 16 x 10 steps beyond one 8 x 8 block, a sparse set with
negative indices, a short period), on two-pass rings, with two special primes and two digit counts, at N = 2^15; with padded batch
strides; under the rotation, inner-sum and giant-step switches and on the integer engine.  The plan's plaintexts are the public
encoder's form 2 of rot_{-giant}(d_k).  At the (level, D) pairs tests/test_bfv_lt_api.py shows safe the output decrypts to the plain
matrix product mod t, as does lsa_bfv_rotate_mac_plain_mul over form-1 plaintexts of the same diagonals.  Refusals leave the
output and the plan untouched; a plan runs again with another batch size after a second plan ran on the same context.

Each model walk is computed once per (rig, case) and shared by the variants."""
import ctypes

import numpy as np
import pytest

from lattisense_amd import params
from tests.bfv_lt_model import linear_transform, model_plains, plain_lt, plan_of, rolled_slots
from tests.bfv_slot_sum_model import make_evaluator
from tests.gpu_util import env, need_gpu

pytestmark = pytest.mark.gpu
SPARSE = [-5, 0, 3, 64, 70, 1000]


def _message(err):
    return str(err).split(": ", 1)[1]


class Rig:
    def __init__(self, n, level, seed):
        from lattisense_amd.device import ALGO_BFV, DeviceContext
        from oracle.client import Client
        from oracle.pyoracle import Oracle
        B = params.BFV_DEFAULT[n]
        self.N, self.level, self.t = n, level, B["t"]
        self.q = B["q"]
        self.p = B["p"]
        self.klvl = len(self.q) - 1
        self.o = Oracle(n, self.q, self.p, self.t)
        self.c = Client(self.o, seed=seed)
        self.ctx = DeviceContext(ALGO_BFV, n, self.q, self.p, self.t)
        self.ev = make_evaluator(self.o, self.c, self.klvl)
        self.rng = np.random.default_rng(seed)
        self.dev_keys = {}

    def keys_for(self, elements):
        for e in elements:
            if e not in self.dev_keys:
                self.dev_keys[e] = self.ctx.upload_key(self.ev._key(e), self.klvl)
        return {e: self.dev_keys[e] for e in elements}

    def encrypt(self, level=None):
        vals = self.rng.integers(0, self.t, self.N)
        return vals, self.c.bfv_encrypt(vals, self.level if level is None else level)

    def diags(self, index, period):
        return {k: self.rng.integers(0, self.t, (2, period)).astype(np.uint64) for k in index}

    def close(self):
        self.ctx.close()


def _case(rig, index, period, items, order, level=None, decrypt=False):
    """items: [(values, ct)]; order: the batch as indices into items.  Returns (plan, glk, device input, words, diagonals)."""
    from lattisense_amd.device import BfvLinearTransformPlan
    N = rig.N
    level = rig.level if level is None else level
    diags = rig.diags(index, period)
    plan = BfvLinearTransformPlan(rig.ctx, level, diags, period)
    want = plan_of(period, list(index))
    assert (plan.n1, plan.rotations, plan.babies, plan.giants) == (want["n1"], want["rotations"], want["babies"], want["giants"])
    info = plan.info()
    assert (info["n1"], info["n_baby"], info["n_giant"], info["n_moddown"]) == (want["n1"], len(want["babies"]), len(want["giants"]), want["moddowns"])
    assert info["galois_elements"] == plan.galois_elements and info["diagonals"] == plan.diagonals
    assert info["rows"] == level + 1 + len(rig.p) and info["level"] == level and info["period"] == period
    glk = rig.keys_for(plan.galois_elements)
    batch = len(order)
    xin = rig.ctx.upload(np.stack([items[i][1][:, : level + 1] for i in order]))
    got = rig.ctx.download(plan.run(xin, batch, glk), (batch, 2, level + 1, N))
    plains = plan.oracle_plains()
    before = set(rig.ev.glk)
    model = [linear_transform(rig.ev, ct[:, : level + 1], level, period, list(index), plains) for _, ct in items]
    assert set(rig.ev.glk) == before, "the model needed a key the plan did not list"
    for b, i in enumerate(order):
        assert np.array_equal(got[b], model[i]), "batch item %d differs from the model (D = %d, period %d, level %d)" % (b, len(index), period, level)
    if decrypt:
        assert np.array_equal(rig.c.bfv_decrypt(got[0]).astype(np.int64), plain_lt(items[order[0]][0], diags, period, N, rig.t))
    return plan, glk, xin, got, diags


@pytest.fixture(scope="module")
def rig12():
    need_gpu()
    r = Rig(4096, 1, 41)
    yield r
    r.close()


def test_plan_plaintexts_are_the_encoders_form_2(rig12):
    from lattisense_amd.device import BfvLinearTransformPlan
    rig, period = rig12, 4096 // 2
    diags = rig.diags(range(7), period)
    plan = BfvLinearTransformPlan(rig.ctx, 1, diags, period)
    got = plan.oracle_plains()
    want = model_plains(rig.o, rig.c, 1, period, diags)
    split = plan.n1
    assert split and sorted(got) == list(range(7))
    for k in range(7):
        assert np.array_equal(got[k], want[k]), k
        dev = rig.ctx.bfv_encode(1, 2, rolled_slots(diags[k], (k // split) * split, period, rig.N)[None])
        assert np.array_equal(rig.ctx.download(dev, (1, 3, rig.N))[0], got[k]), k
    plan.close()


@pytest.mark.parametrize("index, period", [([0], 2048), ([0, 1], 2048), ([0, 1, 2], 2048), (list(range(7)), 2048), (list(range(160)), 2048),
                                           (SPARSE, 2048), ([-1, 0, 5, 17, 40, 62], 64)],
                         ids=["D1", "D2", "D3", "D7", "D160", "sparse", "period64"])
def test_one_pass_ring(rig12, index, period):
    """N = 2^12, level 1, L = 2, k = 1; batch (a, b, a): batch positions are independent; decrypts to the plain product"""
    items = [rig12.encrypt(), rig12.encrypt()]
    plan, _, _, got, _ = _case(rig12, index, period, items, [0, 1, 0], decrypt=True)
    assert np.array_equal(got[0], got[2]) and not np.array_equal(got[0], got[1])
    if len(index) == 160:
        assert (plan.n1, len(plan.babies), len(plan.giants)) == (16, 16, 10)
    plan.close()


@pytest.mark.parametrize("n, level, D", [(8192, 2, 7), (8192, 0, 7), (16384, 5, 20), (16384, 1, 20), (32768, 11, 3)],
                         ids=["N13-l2", "N13-l0", "N14-l5", "N14-l1", "N15-l11"])
def test_two_pass_rings(n, level, D):
    need_gpu()
    rig = Rig(n, level, n + level)
    try:
        _case(rig, list(range(D)), n // 2, [rig.encrypt()], [0], decrypt=level >= 2)[0].close()
    finally:
        rig.close()


def test_padded_strides_and_layout_refusals(rig12):
    from lattisense_amd._native import LsaError, check, lib
    rig, N, lvl = rig12, 4096, 1
    ctx = rig.ctx
    w = 2 * (lvl + 1) * N
    items = [rig.encrypt(), rig.encrypt(), rig.encrypt()]
    plan, glk, xin, got, _ = _case(rig, list(range(7)), N // 2, items, [0, 1, 2])
    sin, sout = w + 2 * N, w + 64
    src = np.full((3, sin), 5, dtype=np.uint64)
    for b in range(3):
        src[b, :w] = items[b][1].reshape(-1)
    dsrc = ctx.upload(src)
    dout = ctx.upload(np.full(3 * sout, 7, dtype=np.uint64))
    plan.run(dsrc, 3, glk, out=dout, sin=sin, sout=sout)
    pad = ctx.download(dout, (3, sout))
    assert np.array_equal(pad[:, :w].reshape(got.shape), got) and np.all(pad[:, w:] == 7)
    assert np.array_equal(ctx.download(dsrc, src.shape), src), "the input was written"

    def fails(fn, needle):
        with pytest.raises(LsaError) as e:
            fn()
        assert e.value.code == 1 and _message(e.value).startswith("lsa_bfv_linear_transform") and needle in _message(e.value), e.value
        assert np.array_equal(ctx.download(dout, (3, sout)), pad)
    elts = (ctypes.c_uint64 * len(glk))(*glk.keys())
    keys = (ctypes.c_void_p * len(glk))(*[k.value for k in glk.values()])
    call = lambda c, i, o, b, si, so: check(lib().lsa_bfv_linear_transform(c, plan._handle(), i, o, b, si, so, len(glk), elts, keys, ctx.stream))
    fails(lambda: call(ctx.h, dsrc.ptr, dout.ptr, 2, 0, sout), "stride of in")              # a shared input is not accepted
    fails(lambda: call(ctx.h, dsrc.ptr, dout.ptr, 2, sin, w - 2), "stride of out")
    fails(lambda: call(ctx.h, dsrc.ptr, dout.ptr, 2, sin + 1, sout), "even")
    fails(lambda: call(ctx.h, dsrc.ptr + 8, dout.ptr, 1, sin, sout), "16-byte")
    fails(lambda: call(ctx.h, None, dout.ptr, 1, sin, sout), "null")
    fails(lambda: call(ctx.h, dout.ptr, dout.ptr, 1, sout, sout), "overlaps")
    fails(lambda: call(ctx.h, dout.ptr, dout.ptr + 8 * (w // 2), 1, sout, sout), "overlaps")
    plan.run(dsrc, 0, glk, out=dout, sin=sin, sout=sout)                                  # batch <= 0: a no-op
    assert np.array_equal(ctx.download(dout, (3, sout)), pad)
    plan.close()


@pytest.mark.parametrize("D", [7, 160])
def test_same_words_under_the_switches(rig12, D):
    rig, N = rig12, 4096
    items = [rig.encrypt(), rig.encrypt()]
    plan, glk, xin, got, _ = _case(rig, list(range(D)), N // 2, items, [0, 1])
    run = lambda: rig.ctx.download(plan.run(xin, 2, glk), got.shape)
    for sw in ({"LSA_ROT_SCATTER": "0"}, {"LSA_LT_BLOCKED_MAC": "0"}, {"LSA_LT_GIANT_SCATTER": "1"}):
        with env(**sw):
            assert np.array_equal(run(), got), sw
    rig.ctx.set_fp64_ntt(0)
    try:
        assert np.array_equal(run(), got), "integer engine"
    finally:
        rig.ctx.set_fp64_ntt(1)
    rig.ctx.set_tile_batch(1)
    try:
        assert np.array_equal(run(), got), "batch split into tiles"
    finally:
        rig.ctx.set_tile_batch(0)
    plan.close()


def test_decrypts_like_the_single_hoisted_composition(rig12):
    """the same seven diagonals through lsa_bfv_rotate_mac_plain_mul over form-1 plaintexts: other words (one division per
    rotation), the same slots"""
    rig, N, lvl = rig12, 4096, 1
    period = N // 2
    vals, ct = rig.encrypt()
    plan, glk, xin, got, diags = _case(rig, list(range(7)), period, [(vals, ct)], [0], decrypt=True)
    ks = sorted(diags)
    elements = [pow(5, k, 2 * N) for k in ks]
    keys = rig.keys_for([e for e in elements if e != 1])
    pts = [rig.ctx.bfv_encode(lvl, 1, rolled_slots(diags[k], 0, period, N)[None]) for k in ks]
    out = rig.ctx.bfv_rotate_mac_plain_mul(lvl, xin, [(e, keys.get(e), pt) for e, pt in zip(elements, pts)], 1)
    comp = rig.ctx.download(out, (1, 2, lvl + 1, N))[0]
    assert not np.array_equal(comp, got[0])
    assert np.array_equal(rig.c.bfv_decrypt(comp).astype(np.int64), plain_lt(vals, diags, period, N, rig.t))
    plan.close()


def test_key_and_plan_refusals_and_plan_reuse(rig12):
    from lattisense_amd._native import LsaError
    from lattisense_amd.device import ALGO_CKKS, BfvLinearTransformPlan, DeviceContext
    rig, N, lvl = rig12, 4096, 1
    ctx = rig.ctx
    w = 2 * (lvl + 1) * N
    items = [rig.encrypt(), rig.encrypt(), rig.encrypt()]
    plan, glk, xin, got, diags = _case(rig, list(range(7)), N // 2, items, [0, 1, 2])
    sentinel = ctx.upload(np.full(3 * w, 7, dtype=np.uint64))

    def fails(fn, prefix, needle):
        with pytest.raises(LsaError) as e:
            fn()
        assert e.value.code == 1 and _message(e.value).startswith(prefix) and needle in _message(e.value), e.value
        assert np.all(ctx.download(sentinel, (3 * w,)) == 7)                           # refused before anything was queued
    for missing in (plan.galois_elements[0], plan.galois_elements[-1]):
        fails(lambda: plan.run(xin, 3, {e: k for e, k in glk.items() if e != missing}, out=sentinel), "lsa_bfv_linear_transform",
              "element %d missing" % missing)
    low = dict(glk)
    e0 = plan.galois_elements[0]
    low[e0] = ctx.upload_key(rig.c.gen_galois_key(e0, lvl - 1), lvl - 1)
    fails(lambda: plan.run(xin, 3, low, out=sentinel), "lsa_bfv_linear_transform", "lower level")
    # the plan is still usable; it runs again with other batch sizes (pool reuse), a second plan in between
    other, g2, x2, got2, _ = _case(rig, SPARSE, N // 2, items[:1], [0])
    assert np.array_equal(ctx.download(plan.run(xin, 1, glk), (1, 2, lvl + 1, N)), got[:1])
    assert np.array_equal(ctx.download(other.run(x2, 1, g2), got2.shape), got2)
    assert np.array_equal(ctx.download(plan.run(xin, 3, glk), got.shape), got)
    other.close()
    # creation refusals
    mk = lambda c, level, d, period=None: BfvLinearTransformPlan(c, level, d, period)._handle()
    z = lambda p: np.zeros(p, dtype=np.uint64)
    fails(lambda: mk(ctx, lvl + 1, {0: z(64)}), "lsa_bfv_lt_create", "level")
    fails(lambda: mk(ctx, -1, {0: z(64)}), "lsa_bfv_lt_create", "level")
    fails(lambda: mk(ctx, lvl, {0: np.full(64, rig.t, dtype=np.uint64)}), "lsa_bfv_lt_create", "below t")
    P = params.CKKS_DEFAULT[4096]
    ckks = DeviceContext(ALGO_CKKS, N, P["q"], P["p"])
    fails(lambda: mk(ckks, 0, {0: z(64)}), "lsa_bfv_lt_create", "not BFV")
    ckks.close()
    B = params.BFV_DEFAULT[4096]
    nop = DeviceContext(0, N, B["q"], [], B["t"])
    fails(lambda: mk(nop, lvl, {0: z(64)}), "lsa_bfv_lt_create", "special prime")
    nop.close()
    import lattisense_amd.device as dev
    idx = (ctypes.c_int * 2)(1, 65)
    h = ctypes.c_void_p()
    v = np.zeros((2, 2, 64), dtype=np.uint64)
    vp = v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    create = lambda period, n_diag: dev.check(dev.lib().lsa_bfv_lt_create(ctx.h, lvl, period, n_diag, idx, vp, 0.0, ctx.stream, ctypes.byref(h)))
    fails(lambda: create(64, 2), "lsa_bfv_lt_create", "repeats")
    fails(lambda: create(48, 1), "lsa_bfv_lt_create", "period")
    fails(lambda: create(4096, 1), "lsa_bfv_lt_create", "period")
    fails(lambda: create(64, 0), "lsa_bfv_lt_create", "diagonal")
    second = Rig(4096, 1, 43)
    try:
        elts = (ctypes.c_uint64 * len(glk))(*glk.keys())
        keys = (ctypes.c_void_p * len(glk))(*[k.value for k in glk.values()])
        fails(lambda: dev.check(dev.lib().lsa_bfv_linear_transform(second.ctx.h, plan._handle(), xin.ptr, sentinel.ptr, 1, w, w, len(glk), elts, keys,
                                                                   None)), "lsa_bfv_linear_transform", "another context")
    finally:
        second.close()
    assert np.array_equal(ctx.download(plan.run(xin, 3, glk), got.shape), got)
    plan.close()
