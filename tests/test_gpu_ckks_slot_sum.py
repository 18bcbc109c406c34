"""CKKS slot sum on the device (lsa_slot_sum_* / lsa_ckks_slot_sum; slot_sum.hip slot_sum_run, k_ks_mac_multi / k_ext_sum)
against its CPU model (tests/slot_sum_model.py on oracle/ckks_bootstrap.py): identical word for word, for every batch item, on a
one-pass ring (every count that takes another plan shape, both radices, three steps), on 61-bit primes (integer engine, unfused
MAC), with more than eight digits (the streaming instantiation), on a whole-limb ring with a partial last batch group and on a
two-pass ring; the same words with the multi-key MAC switched off, on the integer engine, with the batch split into tiles, with
chunked transforms and in place; the message by the project's criterion; refusals that leave the context usable.

Each model walk is computed once per distinct ciphertext and shared by the variants of its case."""
import ctypes

import numpy as np
import pytest

from tests.gpu_util import need_gpu
from tests.slot_sum_model import rotations_of, slot_sum, steps_of

pytestmark = pytest.mark.gpu

D40 = float(2 ** 40)


def _chain(name, n):
    from lattisense_amd import params
    P = params.CKKS_DEFAULT[65536]
    if name == "fp4":                         # 4 Q + 2 P of the headline chain: the FP64 engine but q_0, two digits
        return P["q"][:4], P["p"][:2]
    if name == "ceiling":                     # 60/61-bit primes: integer engine, unfused MAC
        from tests.boundary import ceiling_chain
        C = ceiling_chain(n, 4, 2)
        return C["q"], C["p"]
    if name == "beta9":                       # 9 Q + 1 P: nine digits, the streaming instantiation of the multi-key MAC
        return P["q"][:9], P["p"][:1]
    if name == "beta8":                       # 8 Q + 1 P: eight digits -- <8, 2>, and the streamed form for three and four keys
        return P["q"][:8], P["p"][:1]
    if name == "headline13":                  # 13 Q + 4 P: 17 target limbs, four digits
        return P["q"][:13], P["p"]
    assert name == "headline4"                # the first 4 Q + the P of the headline chain: one digit
    return P["q"][:4], P["p"]


class Rig:
    def __init__(self, log_n, chain, seed):
        from lattisense_amd.device import ALGO_CKKS, DeviceContext
        from oracle.ckks_bootstrap import Evaluator
        from oracle.client import Client
        from oracle.pyoracle import Oracle
        self.N = 1 << log_n
        self.q, self.p = _chain(chain, self.N)
        self.top = len(self.q) - 1
        self.o = Oracle(self.N, self.q, self.p, 0)
        self.c = Client(self.o, seed=seed)
        self.ctx = DeviceContext(ALGO_CKKS, self.N, self.q, self.p)
        self.ev = Evaluator.__new__(Evaluator)          # no relinearisation key needed
        self.ev.o, self.ev.c, self.ev.klvl, self.ev.n = self.o, self.c, self.top, self.N
        self.ev.glk, self.ev.counts = {}, {"rotate": 0, "mult": 0, "mul_plain": 0}
        self.dev_keys = {}

    def keys_for(self, elements):
        for e in elements:
            if e not in self.ev.glk:
                self.ev.glk[e] = self.c.gen_galois_key(e, self.top)
            if e not in self.dev_keys:
                self.dev_keys[e] = self.ctx.upload_key(self.ev.glk[e], self.top)
        return {e: self.dev_keys[e] for e in elements}

    def encrypt(self, rng, level, z=None):
        n = self.N // 2
        if z is None:
            z = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
        return z, self.c.ckks_encrypt(z, level, D40)


def _plain_sum(z, step, count):
    return sum(np.roll(z, -i * step) for i in range(count))


def _case(rig, level, step, count, radix, items, order, message=True):
    """items: [(z, ct)] distinct ciphertexts; order: the batch as indices into items.  Returns (plan, glk, device input, words)."""
    from lattisense_amd.device import SlotSumPlan
    from oracle.ckks_bootstrap import Ct
    from oracle.client import galois_element_for_col_rotation, mean_precision_bits
    N = rig.N
    plan = SlotSumPlan(rig.ctx, level, step, count, radix)
    want_steps = steps_of(N, step, count, radix)
    assert plan.rotations == rotations_of(N, step, count, radix)
    assert plan.steps == len(want_steps) and plan.keyswitches == sum(len(k) for k in want_steps)
    assert plan.galois_elements == sorted(galois_element_for_col_rotation(r, N) for r in plan.rotations)
    glk = rig.keys_for(plan.galois_elements)
    batch = len(order)
    xin = rig.ctx.upload(np.stack([items[i][1] for i in order]))
    assert plan.multi_mac is False                                    # the default: one single-key MAC launch per key
    seq = rig.ctx.download(plan.run(xin, batch, glk), (batch, 2, level + 1, N))
    plan.multi_mac = True                                             # k_ks_mac_multi + k_ext_sum: held to the model below
    got = rig.ctx.download(plan.run(xin, batch, glk), (batch, 2, level + 1, N))
    assert np.array_equal(seq, got), "multi-key MAC and single-key MACs differ (count %d, radix %d, step %d)" % (count, radix, step)
    before = set(rig.ev.glk)
    model = [slot_sum(rig.ev, Ct(ct, level, D40), step, count, radix).data for _, ct in items]
    assert set(rig.ev.glk) == before                                  # the model needed no other key
    for b, i in enumerate(order):
        assert np.array_equal(got[b], model[i]), "batch item %d differs from the model (count %d, radix %d, step %d)" % (b, count, radix, step)
    if message:
        z = items[order[0]][0]
        re, im = mean_precision_bits(_plain_sum(z, step, count), rig.c.ckks_decrypt(got[0], D40))
        assert re >= 10 and im >= 10, (re, im, count, radix, step)
    return plan, glk, xin, got


@pytest.mark.parametrize("step", [1, -1, 8])
def test_one_pass_ring_every_plan_shape(step):
    """N = 2^11, 4 Q + 2 P, level 3: copy, one key, tail only at the end, radix-4 steps with three and four keys, a tail that is
    added to twice (21 at radix 4); batch 3 = (a, b, a): batch positions are independent"""
    need_gpu()
    rig = Rig(11, "fp4", 100 + step)
    rng = np.random.default_rng(7 + step)
    items = [rig.encrypt(rng, 3), rig.encrypt(rng, 3)]
    for count in (1, 2, 3, 4, 5, 7, 8, 12, 16, 21):
        for radix in (2, 4):
            plan, _, _, got = _case(rig, 3, step, count, radix, items, [0, 1, 0])
            assert np.array_equal(got[0], got[2]) and (count == 1 or not np.array_equal(got[0], got[1]))
            plan.close()


@pytest.mark.parametrize("count", [5, 16])
def test_integer_engine_at_the_ceiling(count):
    """N = 2^11, every prime within 2^23 of 2^61: the integer butterflies, the unfused MAC, sums of products at the REDC bound"""
    need_gpu()
    rig = Rig(11, "ceiling", 61)
    rng = np.random.default_rng(61 + count)
    for radix in (2, 4):
        _case(rig, 3, 1, count, radix, [rig.encrypt(rng, 3)], [0, 0])[0].close()


def test_streaming_instantiation_nine_digits():
    """9 Q + 1 P at the top level: beta = 9 > 8 digits, keys and digits streamed, one fold inside the sum; count 5 at radix 4 is
    one launch with four keys"""
    need_gpu()
    rig = Rig(11, "beta9", 9)
    rng = np.random.default_rng(9)
    plan, glk, xin, got = _case(rig, 8, 3, 5, 4, [rig.encrypt(rng, 8), rig.encrypt(rng, 8)], [0, 1])
    assert plan.steps == 1 and plan.keyswitches == 4
    plan.multi_mac = False
    assert np.array_equal(rig.ctx.download(plan.run(xin, 2, glk), got.shape), got)
    plan.close()


def test_eight_digits_every_key_count():
    """8 Q + 1 P at the top level: beta = 8, the fold falls on the last digit and nothing is left for the finish.  Count 3 at
    radix 2 is one launch with two keys (k_ks_mac_multi<8, 2>, eight prefetched digits); counts 4 and 5 at radix 4 are launches
    with three and four keys, which from five digits on take the streamed form (<0, 3>, <0, 4>)"""
    need_gpu()
    rig = Rig(11, "beta8", 8)
    rng = np.random.default_rng(8)
    items = [rig.encrypt(rng, 7), rig.encrypt(rng, 7)]
    for count, radix, keys in ((3, 2, 2), (4, 4, 3), (5, 4, 4)):
        plan, _, _, _ = _case(rig, 7, 1, count, radix, items, [0, 1])
        assert plan.steps == 1 and plan.keyswitches == keys
        plan.close()


@pytest.mark.parametrize("count", [6, 16])
def test_whole_limb_ring_partial_last_group(count):
    """N = 2^13, 13 Q + 4 P at level 12: 17 target limbs x 16 chunks = 272 workgroups per item, so the key MAC walks
    ceil(2048 / 272) = 8 groups: batch 11 gives bpt = 2 and a last group of one item"""
    need_gpu()
    T, chunks, batch = 17, (1 << 13) // 512, 11
    groups = max(1, min(batch, -(-2048 // (T * chunks))))
    bpt = -(-batch // groups)
    assert bpt == 2 and batch % bpt == 1                              # launch_ks_mac's grouping rule
    rig = Rig(13, "headline13", 13)
    rng = np.random.default_rng(13 + count)
    items = [rig.encrypt(rng, 12), rig.encrypt(rng, 12), rig.encrypt(rng, 12)]
    order = [0, 1, 2, 1, 0, 2, 2, 0, 1, 0, 2]
    for radix in (2, 4):
        plan, glk, xin, got = _case(rig, 12, 1, count, radix, items, order)
        plan.multi_mac = False
        assert np.array_equal(rig.ctx.download(plan.run(xin, batch, glk), got.shape), got)
        plan.close()


def test_two_pass_ring():
    """N = 2^15, 4 Q + 4 P of the headline chain: two-pass transforms; count 5 at radix 4, batch 2; once more in 1 MiB chunks"""
    need_gpu()
    rig = Rig(15, "headline4", 15)
    rng = np.random.default_rng(15)
    plan, glk, xin, got = _case(rig, 3, 1, 5, 4, [rig.encrypt(rng, 3), rig.encrypt(rng, 3)], [0, 1])
    rig.ctx.set_ntt_chunk_mib(1)
    try:
        alt = rig.ctx.download(plan.run(xin, 2, glk), got.shape)
    finally:
        rig.ctx.set_ntt_chunk_mib(0)
    assert np.array_equal(alt, got)
    plan.close()


def test_same_words_across_variants():
    """count 21 at radix 4 (two steps of four keys, the second adding to a live tail) and count 7 at radix 2, batch 3: the
    single-key MAC per key, the integer engine, tiles of 2 + 1, chunked transforms, and out == in"""
    need_gpu()
    rig = Rig(11, "fp4", 200)
    ctx = rig.ctx
    rng = np.random.default_rng(200)
    items = [rig.encrypt(rng, 3), rig.encrypt(rng, 3), rig.encrypt(rng, 3)]
    for count, radix in ((21, 4), (7, 2)):
        plan, glk, xin, got = _case(rig, 3, -1, count, radix, items, [0, 1, 2])
        run = lambda: ctx.download(plan.run(xin, 3, glk), got.shape)
        plan.multi_mac = False
        assert np.array_equal(run(), got), "single-key MAC per key"
        plan.multi_mac = True
        ctx.set_fp64_ntt(0)
        try:
            assert np.array_equal(run(), got), "integer engine"
        finally:
            ctx.set_fp64_ntt(1)
        ctx.set_tile_batch(2)
        try:
            assert np.array_equal(run(), got), "batch split into tiles"
            plan.multi_mac = False
            assert np.array_equal(run(), got), "tiles, single-key MAC"
            plan.multi_mac = True
        finally:
            ctx.set_tile_batch(0)
        ctx.set_ntt_chunk_mib(1)
        try:
            assert np.array_equal(run(), got), "chunked transforms"
        finally:
            ctx.set_ntt_chunk_mib(0)
        same = ctx.upload(np.stack([ct for _, ct in items]))
        plan.run(same, 3, glk, out=same)
        assert np.array_equal(ctx.download(same, got.shape), got), "out == in"
        plan.close()


def test_replicate_fills_the_slots():
    """a vector that is non-zero in slot 0 only, step -1, count 8: slots 0..7 hold the value, the others nothing"""
    need_gpu()
    from lattisense_amd.device import SlotSumPlan
    from oracle.client import mean_precision_bits
    rig = Rig(11, "fp4", 300)
    n = rig.N // 2
    z = np.zeros(n, dtype=np.complex128)
    z[0] = 0.75 - 0.5j
    _, ct = rig.encrypt(None, 3, z)
    plan = SlotSumPlan(rig.ctx, 3, -1, 8)
    glk = rig.keys_for(plan.galois_elements)
    got = rig.ctx.download(plan.run(rig.ctx.upload(ct[None]), 1, glk), (1, 2, 4, rig.N))[0]
    want = np.zeros(n, dtype=np.complex128)
    want[:8] = z[0]
    dec = rig.c.ckks_decrypt(got, D40)
    re, im = mean_precision_bits(want, dec)
    assert re >= 10 and im >= 10, (re, im)
    assert np.max(np.abs(dec[:8] - z[0])) < 1e-3 and np.max(np.abs(dec[8:])) < 1e-3
    plan.close()


def test_refusals_leave_the_context_usable():
    need_gpu()
    from lattisense_amd import params
    from lattisense_amd._native import LsaError, check, lib
    from lattisense_amd.device import ALGO_BFV, DeviceContext, SlotSumPlan
    rig = Rig(11, "fp4", 400)
    ctx, N, lvl = rig.ctx, rig.N, 3
    rng = np.random.default_rng(400)
    _, ct = rig.encrypt(rng, lvl)
    words = 2 * (lvl + 1) * N
    plan = SlotSumPlan(ctx, lvl, 1, 5, 4)
    glk = rig.keys_for(plan.galois_elements)
    xin = ctx.upload(np.stack([ct, ct]))
    ref = ctx.download(plan.run(xin, 2, glk), (2, 2, lvl + 1, N))

    def fails(fn, needle):
        with pytest.raises(LsaError) as e:
            fn()
        assert e.value.code == 1 and needle in str(e.value), e.value

    def intact():
        assert np.array_equal(ctx.download(plan.run(xin, 2, glk), ref.shape), ref)
    missing = plan.galois_elements[1]
    sentinel = ctx.upload(np.full(2 * words, 7, dtype=np.uint64))
    fails(lambda: plan.run(xin, 2, {e: k for e, k in glk.items() if e != missing}, out=sentinel), "element %d missing" % missing)
    assert np.all(ctx.download(sentinel, (2 * words,)) == 7)          # refused before anything was queued
    intact()
    low = dict(glk)                                                   # a key exported below the ciphertext's level
    low[missing] = ctx.upload_key(rig.c.gen_galois_key(missing, lvl - 1), lvl - 1)
    fails(lambda: plan.run(xin, 2, low, out=sentinel), "lower level")
    assert np.all(ctx.download(sentinel, (2 * words,)) == 7)
    intact()
    big = ctx.upload(np.zeros(3 * words, dtype=np.uint64))           # out = in shifted by half a ciphertext: overlapping, unequal
    elts = (ctypes.c_uint64 * len(glk))(*glk.keys())
    keys = (ctypes.c_void_p * len(glk))(*[k.value for k in glk.values()])
    fails(lambda: check(lib().lsa_ckks_slot_sum(ctx.h, plan._handle(), big.ptr, big.ptr + 8 * (words // 2), 2, words, words, len(glk), elts,
                                                keys, ctx.stream)), "not overlap")
    intact()
    plan.run(xin, 0, glk, out=sentinel)                               # batch <= 0: a no-op
    assert np.all(ctx.download(sentinel, (2 * words,)) == 7)
    B = params.BFV_DEFAULT[8192]
    bfv = DeviceContext(ALGO_BFV, 8192, B["q"], B["p"], B["t"])
    fails(lambda: SlotSumPlan(bfv, 0, 1, 4).run(xin, 1, {}), "CKKS")  # wrong algorithm
    bfv.close()
    fails(lambda: SlotSumPlan(ctx, lvl + 1, 1, 4).run(xin, 1, {}), "level")
    other = Rig(11, "fp4", 401)
    fails(lambda: check(lib().lsa_ckks_slot_sum(other.ctx.h, plan._handle(), xin.ptr, sentinel.ptr, 1, words, words, len(glk), elts, keys,
                                                None)), "another context")
    intact()
    plan.close()
