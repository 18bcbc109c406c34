"""BFV slot sum on the device (lsa_bfv_slot_sum_*; slot_sum.hip bfv_slot_sum_run and k_bfv_slot_tail) against its CPU model
(tests/bfv_slot_sum_model.py slot_sum on oracle/ckks_bootstrap.py): identical word for word, for every batch item, on a one-pass
ring (every count that takes another plan shape, both radices, with and without the row step, three steps), with keys above the
plan's level, on 60/61-bit special primes (integer engine), on the full N = 2^14 ring (two-pass transforms, the 128 KiB LDS row) and
above the LDS limit (the plain form); the same words with the gathering tail off, under lsa_set_fp64_ntt(0), with unfused tails,
with the batch split into tiles, with chunked transforms and in place; the message by equality mod t; refusals that leave the
context usable.  No chain here has an FP64-engine limb: the two engines are compared in tests/test_gpu_bfv_operator_chains.py.

Each model walk is computed once per distinct ciphertext and case and shared by the variants."""
import ctypes

import numpy as np
import pytest

from tests.bfv_slot_sum_model import galois_elements_of, make_evaluator, plain_slot_sum, slot_sum, steps_of
from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu


def _message(err):
    """the library's message without the binding's "lattisense_amd error <code>: " in front"""
    return str(err).split(": ", 1)[1]


def _chain(name):
    from lattisense_amd import params
    if name == "d8192":                       # 3 Q + 1 P: three digits of one limb
        B = params.BFV_DEFAULT[8192]
        return B["q"], B["p"], B["t"]
    if name == "d16384":                      # 6 Q + 2 P
        B = params.BFV_DEFAULT[16384]
        return B["q"], B["p"], B["t"]
    assert name == "d32768_4"                 # the first 4 Q + 3 P of the 2^15 set: 60/61-bit special primes, integer engine
    B = params.BFV_DEFAULT[32768]
    return B["q"][:4], B["p"], B["t"]


class Rig:
    def __init__(self, log_n, chain, seed, key_level=None):
        from lattisense_amd.device import ALGO_BFV, DeviceContext
        from oracle.client import Client
        from oracle.pyoracle import Oracle
        self.N = 1 << log_n
        self.q, self.p, self.t = _chain(chain)
        self.top = len(self.q) - 1
        self.klvl = self.top if key_level is None else key_level
        self.o = Oracle(self.N, self.q, self.p, self.t)
        self.c = Client(self.o, seed=seed)
        self.ctx = DeviceContext(ALGO_BFV, self.N, self.q, self.p, self.t)
        self.ev = make_evaluator(self.o, self.c, self.klvl)
        self.dev_keys = {}
        self.models = {}

    def keys_for(self, elements):
        for e in elements:
            if e not in self.dev_keys:
                self.dev_keys[e] = self.ctx.upload_key(self.ev._key(e), self.klvl)
        return {e: self.dev_keys[e] for e in elements}

    def encrypt(self, rng, level, values=None):
        if values is None:
            values = rng.integers(0, self.t, self.N)
        return np.asarray(values, dtype=np.int64), self.c.bfv_encrypt(values, level)

    def model(self, tag, ct, level, step, count, radix, rows):
        key = (tag, level, step, count, radix, rows)
        if key not in self.models:
            self.models[key] = slot_sum(self.ev, ct, level, step, count, radix, rows)
        return self.models[key]


def _case(rig, level, step, count, radix, rows, items, order, message=True):
    """items: [(values, ct)] distinct ciphertexts; order: the batch as indices into items.  Returns (plan, glk, device input, words)."""
    from lattisense_amd.device import BfvSlotSumPlan
    N = rig.N
    plan = BfvSlotSumPlan(rig.ctx, level, step, count, radix, rows)
    want_steps = steps_of(N, step, count, radix, rows)
    assert plan.galois_elements == galois_elements_of(N, step, count, radix, rows)
    assert plan.steps == len(want_steps) and plan.keyswitches == sum(len(k) for k in want_steps)
    glk = rig.keys_for(plan.galois_elements)
    batch = len(order)
    xin = rig.ctx.upload(np.stack([items[i][1] for i in order]))
    got = rig.ctx.download(plan.run(xin, batch, glk), (batch, 2, level + 1, N))
    before = set(rig.ev.glk)
    model = [rig.model(id(ct), ct, level, step, count, radix, rows) for _, ct in items]
    assert set(rig.ev.glk) == before                                  # the model needed no other key
    what = "(count %d, radix %d, rows %d, step %d)" % (count, radix, rows, step)
    for b, i in enumerate(order):
        assert np.array_equal(got[b], model[i]), "batch item %d differs from the model %s" % (b, what)
    if message:
        want = plain_slot_sum(items[order[0]][0], N, step, count, rows, rig.t)
        assert np.array_equal(rig.c.bfv_decrypt(got[0]).astype(np.int64), want), "decryption is not the slot sum mod t " + what
    return plan, glk, xin, got


@pytest.mark.parametrize("step", [1, -1, 8])
def test_one_pass_ring_every_plan_shape(step):
    """N = 2^11, 3 Q + 1 P, top level: copy, the row step alone, one key, tail only at the end, radix-4 steps with three and four
    keys, a tail that is added to twice (21 at radix 4); batch 3 = (a, b, a): batch positions are independent"""
    need_gpu()
    rig = Rig(11, "d8192", 100 + step)
    rng = np.random.default_rng(7 + step)
    items = [rig.encrypt(rng, 2), rig.encrypt(rng, 2)]
    for count in (1, 2, 3, 4, 5, 7, 8, 12, 16, 21):
        for radix in (2, 4):
            for rows in (0, 1):
                plan, _, _, got = _case(rig, 2, step, count, radix, rows, items, [0, 1, 0], message=count in (1, 5, 21))
                assert plan.gather_in_force()
                assert np.array_equal(got[0], got[2]) and not np.array_equal(got[0], got[1])
                plan.close()


@pytest.mark.parametrize("level,key_level", [(3, 5), (5, 5)])
def test_keys_above_the_level_and_two_special_primes(level, key_level):
    """N = 2^12, 6 Q + 2 P: level 3 with keys exported at level 5, and level 5; count 5 at radix 4 with the row step (two steps, five
    keys) and count 7 at radix 2 (tails in two steps)"""
    need_gpu()
    rig = Rig(12, "d16384", 12 + level, key_level)
    rng = np.random.default_rng(12 + level)
    items = [rig.encrypt(rng, level), rig.encrypt(rng, level)]
    _case(rig, level, 1, 5, 4, 1, items, [0, 1])[0].close()
    _case(rig, level, 1, 7, 2, 0, items, [0, 1])[0].close()


@pytest.mark.parametrize("count", [5, 16])
def test_integer_engine_large_special_primes(count):
    """N = 2^11 on the first 4 Q + 3 P of the 2^15 set: 59/60-bit Q limbs, 61-bit special primes, the integer butterflies"""
    need_gpu()
    rig = Rig(11, "d32768_4", 61)
    rng = np.random.default_rng(61 + count)
    for radix in (2, 4):
        _case(rig, 3, 1, count, radix, 1, [rig.encrypt(rng, 3)], [0, 0])[0].close()


def test_full_ring_with_the_largest_lds_row():
    """N = 2^14, BFV_DEFAULT[16384] at level 3: two-pass transforms and a c0 row of 128 KiB in LDS; count 5 at radix 4 with the row
    step, batch 2; once more in 1 MiB chunks"""
    need_gpu()
    rig = Rig(14, "d16384", 14, key_level=3)
    rng = np.random.default_rng(14)
    plan, glk, xin, got = _case(rig, 3, 1, 5, 4, 1, [rig.encrypt(rng, 3), rig.encrypt(rng, 3)], [0, 1])
    assert plan.gather_in_force()
    rig.ctx.set_ntt_chunk_mib(1)
    try:
        alt = rig.ctx.download(plan.run(xin, 2, glk), got.shape)
    finally:
        rig.ctx.set_ntt_chunk_mib(0)
    assert np.array_equal(alt, got)
    plan.close()


def test_above_the_lds_limit_runs_the_plain_form():
    """N = 2^15, 4 Q + 3 P: a limb does not fit in LDS, `gather` reports 0, asking for it is refused and the plain form runs"""
    need_gpu()
    from lattisense_amd._native import LsaError
    rig = Rig(15, "d32768_4", 15)
    rng = np.random.default_rng(15)
    plan, glk, xin, got = _case(rig, 3, 1, 5, 4, 0, [rig.encrypt(rng, 3)], [0])
    assert not plan.gather_in_force()
    plan.gather = True
    with pytest.raises(LsaError) as e:
        plan.run(xin, 1, glk)
    assert e.value.code == 1 and _message(e.value).startswith("lsa_bfv_slot_sum_set_gather") and "enable" in _message(e.value), e.value
    plan.gather = None
    assert not plan.gather_in_force()
    assert np.array_equal(rig.ctx.download(plan.run(xin, 1, glk), got.shape), got)
    plan.close()


def test_same_words_across_variants():
    """count 21 at radix 4 with the row step (the second column step adds to a live tail) and count 7 at radix 2, batch 3: the
    plain form, lsa_set_fp64_ntt(0), unfused tails, tiles of 2 + 1, chunked transforms, and out == in.  This chain (54 / 55-bit Q,
    55-bit P) has no FP64-engine limb, so "integer engine" below is the engine of every row already: the run shows that the
    setting itself changes nothing.  The comparison of the two engines lives in tests/test_gpu_bfv_operator_chains.py
    (test_slot_sum_variants on the fp and mixed chains)."""
    need_gpu()
    from lattisense_amd._native import check, lib
    rig = Rig(11, "d8192", 200)
    ctx = rig.ctx
    rng = np.random.default_rng(200)
    items = [rig.encrypt(rng, 2), rig.encrypt(rng, 2), rig.encrypt(rng, 2)]
    for count, radix, rows in ((21, 4, 1), (7, 2, 0)):
        plan, glk, xin, got = _case(rig, 2, -1, count, radix, rows, items, [0, 1, 2])
        run = lambda: ctx.download(plan.run(xin, 3, glk), got.shape)
        plan.gather = False
        assert np.array_equal(run(), got), "plain form"
        assert not plan.gather_in_force()
        for gather in (True, False):
            plan.gather = gather
            ctx.set_fp64_ntt(0)
            try:
                assert np.array_equal(run(), got), "integer engine, gather %d" % gather
            finally:
                ctx.set_fp64_ntt(1)
            check(lib().lsa_set_fuse_tails(ctx.h, 0))
            try:
                assert np.array_equal(run(), got), "unfused tails, gather %d" % gather
            finally:
                check(lib().lsa_set_fuse_tails(ctx.h, 1))
            ctx.set_tile_batch(2)
            try:
                assert np.array_equal(run(), got), "batch split into tiles, gather %d" % gather
            finally:
                ctx.set_tile_batch(0)
            ctx.set_ntt_chunk_mib(1)
            try:
                assert np.array_equal(run(), got), "chunked transforms, gather %d" % gather
            finally:
                ctx.set_ntt_chunk_mib(0)
            same = ctx.upload(np.stack([ct for _, ct in items]))
            plan.run(same, 3, glk, out=same)
            assert np.array_equal(ctx.download(same, got.shape), got), "out == in, gather %d" % gather
        plan.close()


def test_message_total_in_every_slot_replicate_and_the_eager_chain():
    """N = 2^11: count = N/2 with the row step leaves the total of all N slots in every slot; a replicate (step -1, count 8) of a
    vector that is non-zero in one slot; the operator's words differ from the chain of lsa_bfv_rotate + lsa_poly_addsub (one
    division per rotation) while both decrypt to the same sums"""
    need_gpu()
    from lattisense_amd.device import BfvSlotSumPlan
    rig = Rig(11, "d8192", 300)
    ctx, N, t = rig.ctx, rig.N, rig.t
    h = N // 2
    rng = np.random.default_rng(300)
    vals, ct = rig.encrypt(rng, 2)
    for radix in (2, 4):
        plan = BfvSlotSumPlan(ctx, 2, 1, h, radix, 1)
        glk = rig.keys_for(plan.galois_elements)
        got = ctx.download(plan.run(ctx.upload(ct[None]), 1, glk), (1, 2, 3, N))[0]
        assert np.array_equal(rig.c.bfv_decrypt(got).astype(np.int64), np.full(N, int(vals.sum()) % t))
        plan.close()
    one = np.zeros(N, dtype=np.int64)
    one[0] = 12345
    _, ct1 = rig.encrypt(None, 2, one)
    plan = BfvSlotSumPlan(ctx, 2, -1, 8)
    glk = rig.keys_for(plan.galois_elements)
    got = ctx.download(plan.run(ctx.upload(ct1[None]), 1, glk), (1, 2, 3, N))[0]
    want = np.zeros(N, dtype=np.int64)
    want[:8] = 12345
    assert np.array_equal(rig.c.bfv_decrypt(got).astype(np.int64), want)
    plan.close()
    # count 5 at radix 4: four rotations divided by P together (three NEXT) and alone (the TAIL); the chain divides each on its own
    plan = BfvSlotSumPlan(ctx, 2, 1, 5, 4)
    glk = rig.keys_for(plan.galois_elements)
    xin = ctx.upload(ct[None])
    got = ctx.download(plan.run(xin, 1, glk), (1, 2, 3, N))[0]
    chain = xin
    for r in (1, 2, 3, 4):
        e = pow(5, r, 2 * N)
        chain = ctx.addsub(0, 2, 2, chain, ctx.bfv_rotate(2, xin, e, glk[e], 1), 1)
    eager = ctx.download(chain, (2, 3, N))
    assert not np.array_equal(eager, got)
    want = plain_slot_sum(vals, N, 1, 5, 0, t)
    assert np.array_equal(rig.c.bfv_decrypt(got).astype(np.int64), want)
    assert np.array_equal(rig.c.bfv_decrypt(eager).astype(np.int64), want)
    plan.close()


def test_refusals_leave_the_context_usable():
    need_gpu()
    from lattisense_amd import params
    from lattisense_amd._native import LsaError, check, lib
    from lattisense_amd.device import ALGO_CKKS, BfvSlotSumPlan, DeviceContext
    rig = Rig(11, "d8192", 400)
    ctx, N, lvl = rig.ctx, rig.N, 2
    rng = np.random.default_rng(400)
    _, ct = rig.encrypt(rng, lvl)
    words = 2 * (lvl + 1) * N
    plan = BfvSlotSumPlan(ctx, lvl, 1, 5, 4, 1)
    glk = rig.keys_for(plan.galois_elements)
    xin = ctx.upload(np.stack([ct, ct]))
    ref = ctx.download(plan.run(xin, 2, glk), (2, 2, lvl + 1, N))

    def fails(fn, needle):
        with pytest.raises(LsaError) as e:
            fn()
        assert e.value.code == 1 and _message(e.value).startswith("lsa_bfv_slot_sum") and needle in _message(e.value), e.value

    def intact():
        assert np.array_equal(ctx.download(plan.run(xin, 2, glk), ref.shape), ref)
    sentinel = ctx.upload(np.full(2 * words, 7, dtype=np.uint64))

    def untouched():
        assert np.all(ctx.download(sentinel, (2 * words,)) == 7)      # refused before anything was queued
        intact()
    for missing in (plan.galois_elements[1], 2 * N - 1):
        fails(lambda: plan.run(xin, 2, {e: k for e, k in glk.items() if e != missing}, out=sentinel), "element %d missing" % missing)
        untouched()
    low = dict(glk)                                                   # a key exported below the plan's level
    low[2 * N - 1] = ctx.upload_key(rig.c.gen_galois_key(2 * N - 1, lvl - 1), lvl - 1)
    fails(lambda: plan.run(xin, 2, low, out=sentinel), "lower level")
    untouched()
    big = ctx.upload(np.zeros(3 * words, dtype=np.uint64))           # out = in shifted by half a ciphertext: overlapping, unequal
    elts = (ctypes.c_uint64 * len(glk))(*glk.keys())
    keys = (ctypes.c_void_p * len(glk))(*[k.value for k in glk.values()])
    call = lambda c, i, o, b, si, so: check(lib().lsa_bfv_slot_sum(c, plan._handle(), i, o, b, si, so, len(glk), elts, keys, ctx.stream))
    fails(lambda: call(ctx.h, big.ptr, big.ptr + 8 * (words // 2), 2, words, words), "not overlap")
    fails(lambda: call(ctx.h, xin.ptr + 8, sentinel.ptr, 1, words, words), "16-byte")
    fails(lambda: call(ctx.h, xin.ptr, sentinel.ptr, 2, words, words + 1), "even")
    fails(lambda: call(ctx.h, None, sentinel.ptr, 2, words, words), "null")
    untouched()
    plan.run(xin, 0, glk, out=sentinel)                               # batch <= 0: a no-op
    untouched()
    fails(lambda: BfvSlotSumPlan(ctx, lvl + 1, 1, 4).run(xin, 1, {}), "level")
    fails(lambda: BfvSlotSumPlan(ctx, -1, 1, 4).run(xin, 1, {}), "level")
    fails(lambda: BfvSlotSumPlan(ctx, lvl, 1, 0), "count")
    fails(lambda: BfvSlotSumPlan(ctx, lvl, 1, N // 2 + 1), "count")
    fails(lambda: BfvSlotSumPlan(ctx, lvl, 1, 4, radix=3), "radix")
    fails(lambda: BfvSlotSumPlan(ctx, lvl, N // 2, 2), "step")
    P = params.CKKS_DEFAULT[65536]
    ckks = DeviceContext(ALGO_CKKS, N, P["q"][:4], P["p"][:2])
    fails(lambda: BfvSlotSumPlan(ckks, lvl, 1, 4).run(xin, 1, {}), "not BFV")      # wrong algorithm
    ckks.close()
    other = Rig(11, "d8192", 401)
    fails(lambda: call(other.ctx.h, xin.ptr, sentinel.ptr, 1, words, words), "another context")
    untouched()
    copy = BfvSlotSumPlan(ctx, lvl, 1, 1)                             # count 1, no rows: a copy, no key
    assert np.array_equal(ctx.download(copy.run(xin, 2, {}), ref.shape), np.stack([ct, ct]))
    copy.close()
    plan.close()
