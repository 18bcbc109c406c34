"""BFV oblivious expansion on the device (lsa_bfv_expand_*, lsa_bfv_mul_monomial; bfv_expand.hip) against its CPU model
(tests/bfv_expand_model.py: per node Oracle.bfv_rotate, Oracle.vec add / sub, the numpy shift): identical word for word, for every
output of every batch item -- every plan shape on a one-pass ring, keys above the plan's level with two special primes, the full
expansion of N = 2^10, the 128 KiB LDS row at N = 2^14, the two-step form above the LDS limit; the same words with the gather off,
under lsa_set_fp64_ntt(0), with unfused tails, with the batch split into tiles on two streams and with chunked transforms; both
engines on the fp and ceiling operator chains with the fused key MAC read back; the device's own composition of lsa_bfv_rotate,
lsa_poly_addsub and lsa_bfv_mul_monomial; the layout rules; the launch count of a level; the monomial against numpy; refusals that
leave the context usable.

Each model walk is computed once per distinct ciphertext and case and shared by the variants."""
import ctypes

import numpy as np
import pytest

from tests.bfv_expand_model import (decrypt_coeffs, encrypt_coeffs, expand, expected_plain, galois_elements_of, keyswitches_of,
                                    levels_of, mul_monomial, nodes_of, prescale)
from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu


def _message(err):
    """the library's message without the binding's "lattisense_amd error <code>: " in front"""
    return str(err).split(": ", 1)[1]


def _chain(name):
    from lattisense_amd import params
    if name == "d8192":                       # 3 Q + 1 P
        B = params.BFV_DEFAULT[8192]
        return B["q"], B["p"], B["t"]
    if name == "d16384":                      # 6 Q + 2 P
        B = params.BFV_DEFAULT[16384]
        return B["q"], B["p"], B["t"]
    assert name == "d32768_4"                 # the first 4 Q + 3 P of the 2^15 set
    B = params.BFV_DEFAULT[32768]
    return B["q"][:4], B["p"], B["t"]


class Rig:
    def __init__(self, log_n, chain, seed, key_level=None, mods=None):
        from lattisense_amd.device import ALGO_BFV, DeviceContext
        from oracle.client import Client
        from oracle.pyoracle import Oracle
        self.N = 1 << log_n
        self.q, self.p, self.t = mods if mods is not None else _chain(chain)
        self.top = len(self.q) - 1
        self.klvl = self.top if key_level is None else key_level
        self.o = Oracle(self.N, self.q, self.p, self.t)
        self.c = Client(self.o, seed=seed)
        self.ctx = DeviceContext(ALGO_BFV, self.N, self.q, self.p, self.t)
        self.host_keys, self.dev_keys, self.models = {}, {}, {}

    def key_of(self, g):
        if g not in self.host_keys:
            self.host_keys[g] = self.c.gen_galois_key(g, self.klvl)
        return self.host_keys[g]

    def keys_for(self, elements):
        for e in elements:
            if e not in self.dev_keys:
                self.dev_keys[e] = self.ctx.upload_key(self.key_of(e), self.klvl)
        return {e: self.dev_keys[e] for e in elements}

    def encrypt(self, rng, level, count):
        """(m, a ciphertext of m * 2^-k mod t)"""
        m = rng.integers(0, self.t, self.N)
        return m, encrypt_coeffs(self.c, prescale(m, count, self.t), level)

    def model(self, ct, level, count):
        key = (id(ct), level, count)
        if key not in self.models:
            self.models[key] = expand(self.o, self.key_of, self.klvl, ct, level, count)
        return self.models[key]

    def close(self):
        self.ctx.close()


def _case(rig, level, count, items, order, decrypt=()):
    """items: [(m, ct)] distinct ciphertexts; order: the batch as indices into items.  Returns (plan, glk, device input, the words
    [count][batch][2][level+1][N])."""
    from lattisense_amd.device import BfvExpandPlan
    N = rig.N
    plan = BfvExpandPlan(rig.ctx, level, count)
    assert plan.galois_elements == galois_elements_of(N, count)
    assert plan.levels == levels_of(count) and plan.keyswitches == keyswitches_of(N, count)
    glk = rig.keys_for(plan.galois_elements)
    batch = len(order)
    xin = rig.ctx.upload(np.stack([items[i][1] for i in order]))
    got = rig.ctx.download(plan.run(xin, batch, glk), (count, batch, 2, level + 1, N))
    model = [rig.model(ct, level, count) for _, ct in items]
    for b, i in enumerate(order):
        for o in range(count):
            assert np.array_equal(got[o, b], model[i][o]), "output %d of batch item %d differs from the model (count %d)" % (o, b, count)
    for o in decrypt:
        want = expected_plain(items[order[0]][0], o, count, N, rig.t)
        assert np.array_equal(decrypt_coeffs(rig.c, got[o, 0]), want), "output %d does not decrypt to its coefficients (count %d)" % (o, count)
    return plan, glk, xin, got


def test_one_pass_ring_every_plan_shape():
    """N = 2^11, 3 Q + 1 P, top level: the copy, one level, odd children missing at the last level (3, 5, 11), full levels (2, 4, 8,
    16); batch 3 = (a, b, a): batch positions are independent"""
    need_gpu()
    rig = Rig(11, "d8192", 100)
    rng = np.random.default_rng(7)
    for count in (1, 2, 3, 4, 5, 8, 11, 16):
        items = [rig.encrypt(rng, 2, count), rig.encrypt(rng, 2, count)]
        plan, _, _, got = _case(rig, 2, count, items, [0, 1, 0], decrypt=range(count) if count in (5, 16) else ())
        assert plan.gather_in_force()
        assert np.array_equal(got[:, 0], got[:, 2]) and not np.array_equal(got[:, 0], got[:, 1])
        plan.close()
        rig.models.clear()
    rig.close()


@pytest.mark.parametrize("level,key_level", [(3, 5), (5, 5)])
def test_keys_above_the_level_and_two_special_primes(level, key_level):
    """N = 2^12, 6 Q + 2 P: level 3 with keys exported at level 5, and level 5; count 6"""
    need_gpu()
    rig = Rig(12, "d16384", 12 + level, key_level)
    rng = np.random.default_rng(12 + level)
    items = [rig.encrypt(rng, level, 6), rig.encrypt(rng, level, 6)]
    _case(rig, level, 6, items, [0, 1], decrypt=(0, 5))[0].close()
    rig.close()


def test_full_expansion():
    """N = 2^10, level 1, count 1024: ten levels down to g = 3, s = 512, 1023 key switches; every output against the model, and the
    checked ones decrypt to m_i in coefficient 0 and zero elsewhere"""
    need_gpu()
    rig = Rig(10, "d8192", 10)
    rng = np.random.default_rng(10)
    m, ct = rig.encrypt(rng, 1, 1024)
    plan, _, _, got = _case(rig, 1, 1024, [(m, ct)], [0])
    assert (plan.levels, plan.keyswitches) == (10, 1023) and plan.galois_elements[0] == 3
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 511, 512, 1023):
        dec = decrypt_coeffs(rig.c, got[i, 0])
        assert dec[0] == m[i] and not dec[1:].any(), i
    plan.close()
    rig.close()


@pytest.fixture(scope="module")
def full_ring():
    """N = 2^14, BFV_DEFAULT[16384] at level 1, count 4, batch 2: two-pass transforms and a 128 KiB row in LDS"""
    need_gpu()
    rig = Rig(14, "d16384", 14, key_level=1)
    rng = np.random.default_rng(14)
    items = [rig.encrypt(rng, 1, 4), rig.encrypt(rng, 1, 4)]
    yield rig, items
    rig.close()


def test_full_ring_with_the_largest_lds_row(full_ring):
    rig, items = full_ring
    plan = _case(rig, 1, 4, items, [0, 1], decrypt=(0, 3))[0]
    assert plan.gather_in_force()
    plan.close()


def test_above_the_lds_limit_runs_the_two_step_form():
    """N = 2^15, 4 Q + 3 P, level 1, count 3: a limb does not fit in LDS, `gather` reports 0, asking for it is refused"""
    need_gpu()
    from lattisense_amd._native import LsaError
    rig = Rig(15, "d32768_4", 15, key_level=1)
    rng = np.random.default_rng(15)
    plan, glk, xin, got = _case(rig, 1, 3, [rig.encrypt(rng, 1, 3)], [0], decrypt=(0, 2))
    assert not plan.gather_in_force()
    with pytest.raises(LsaError) as e:
        plan.set_gather(True)
    assert e.value.code == 1 and _message(e.value).startswith("lsa_bfv_expand_set_gather") and "enable" in _message(e.value), e.value
    assert not plan.gather_in_force()
    plan.gather = None
    assert np.array_equal(rig.ctx.download(plan.run(xin, 1, glk), got.shape), got)
    plan.close()
    rig.close()


def _variants(ctx, plan, run, got, fused_off=None):
    """run() under each setting must give `got` again; every setting is put back"""
    from lattisense_amd._native import check, lib
    plan.gather = False
    assert np.array_equal(run(), got), "two-step form"
    assert not plan.gather_in_force()
    for gather in (True, False):
        plan.gather = gather
        ctx.set_fp64_ntt(0)
        try:
            if fused_off is not None:
                assert not fused_off()
            assert np.array_equal(run(), got), "integer engine, gather %d" % gather
        finally:
            ctx.set_fp64_ntt(1)
        check(lib().lsa_set_fuse_tails(ctx.h, 0))
        try:
            assert np.array_equal(run(), got), "unfused tails, gather %d" % gather
        finally:
            check(lib().lsa_set_fuse_tails(ctx.h, 1))
        check(lib().lsa_set_dual_stream(ctx.h, 1))
        try:
            for tile in (1, 2):
                ctx.set_tile_batch(tile)
                assert np.array_equal(run(), got), "tile batch %d on two streams, gather %d" % (tile, gather)
        finally:
            ctx.set_tile_batch(0)
            check(lib().lsa_set_dual_stream(ctx.h, 0))
        ctx.set_ntt_chunk_mib(1)
        try:
            assert np.array_equal(run(), got), "chunked transforms, gather %d" % gather
        finally:
            ctx.set_ntt_chunk_mib(0)
    plan.gather = True
    assert np.array_equal(run(), got) and plan.gather_in_force()


def test_same_words_across_variants_one_pass_ring():
    need_gpu()
    rig = Rig(11, "d8192", 200)
    rng = np.random.default_rng(200)
    for count in (5, 16):
        items = [rig.encrypt(rng, 2, count), rig.encrypt(rng, 2, count)]
        plan, glk, xin, got = _case(rig, 2, count, items, [0, 1, 0])
        _variants(rig.ctx, plan, lambda: rig.ctx.download(plan.run(xin, 3, glk), got.shape), got)
        plan.close()
    rig.close()


def test_same_words_across_variants_full_ring(full_ring):
    rig, items = full_ring
    plan, glk, xin, got = _case(rig, 1, 4, items, [0, 1])
    _variants(rig.ctx, plan, lambda: rig.ctx.download(plan.run(xin, 2, glk), got.shape), got)
    plan.close()


@pytest.mark.parametrize("kind", ["fp", "ceiling"])
def test_both_engines(kind):
    """tests/boundary.py bfv_operator_chain at N = 2^13, count 5, at the top level and at the lift level, the operands the `max`
    and `uniform` patterns, pattern keys: fp has every row on the FP64 engine and takes the fused second pass + key MAC (read back
    and asserted: the path hoisted rotations never take), ceiling has none"""
    need_gpu()
    from lattisense_amd.device import BfvExpandPlan
    from tests import boundary
    n = 1 << 13
    q, p = boundary.bfv_operator_chain(kind, n)
    rig = Rig(13, None, 13, mods=(q, p, boundary.BFV_OPERATOR_T))
    rng = np.random.default_rng(13)
    beta = (rig.klvl + 1 + len(p) - 1) // len(p)
    names = ("top", "uniform", "max", "half")
    for lvl in (rig.top, boundary.lift_level(q, p)):
        plan = BfvExpandPlan(rig.ctx, lvl, 5)
        for i, g in enumerate(plan.galois_elements):
            if g not in rig.host_keys:
                rig.host_keys[g] = boundary.pattern_key(names[i % len(names)], q + p, beta, n, rng)
        glk = rig.keys_for(plan.galois_elements)
        fused = lambda: all(rig.ctx.key_switch_fused(lvl, k) for k in glk.values())
        assert fused() == (kind == "fp"), (kind, lvl)
        cts = boundary.pattern_ct(("max", "uniform"), q[: lvl + 1], 2, n, rng)
        xin = rig.ctx.upload(cts)
        got = rig.ctx.download(plan.run(xin, 2, glk), (5, 2, 2, lvl + 1, n))
        for b in range(2):
            want = expand(rig.o, rig.key_of, rig.klvl, cts[b], lvl, 5)
            assert np.array_equal(got[:, b], want), (kind, lvl, b)
        _variants(rig.ctx, plan, lambda: rig.ctx.download(plan.run(xin, 2, glk), got.shape), got, fused_off=fused)
        plan.close()
    rig.close()


def test_against_the_devices_own_composition():
    """lsa_bfv_rotate + lsa_poly_addsub + lsa_bfv_mul_monomial per node, count 7 at N = 2^12, word for word"""
    need_gpu()
    from lattisense_amd.device import BfvExpandPlan
    rig = Rig(12, "d16384", 77)
    ctx, N, lvl, count = rig.ctx, rig.N, 5, 7
    rng = np.random.default_rng(77)
    cts = np.stack([rig.encrypt(rng, lvl, count)[1] for _ in range(2)])
    plan = BfvExpandPlan(ctx, lvl, count)
    glk = rig.keys_for(plan.galois_elements)
    xin = ctx.upload(cts)
    got = ctx.download(plan.run(xin, 2, glk), (count, 2, 2, lvl + 1, N))
    c = [None] * count
    c[0] = xin
    for g, s, nodes, _ in nodes_of(N, count):
        for a in range(nodes):
            sigma = ctx.bfv_rotate(lvl, c[a], g, glk[g], 2)
            if a + s < count:
                c[a + s] = ctx.bfv_mul_monomial(lvl, ctx.addsub(1, lvl, 2, c[a], sigma, 2), -s, 2)
            c[a] = ctx.addsub(0, lvl, 2, c[a], sigma, 2)
    for i in range(count):
        assert np.array_equal(ctx.download(c[i], (2, 2, lvl + 1, N)), got[i]), i
    plan.close()
    rig.close()


def test_layout_in_place_gaps_and_unused_outputs():
    """`in` is output 0; a non-dense s_index with sentinel words in every gap and behind the last output; the outputs >= count of a
    buffer sized for 2^k are untouched"""
    need_gpu()
    rig = Rig(11, "d8192", 300)
    ctx, N, lvl, count, batch = rig.ctx, rig.N, 2, 5, 2
    rng = np.random.default_rng(300)
    items = [rig.encrypt(rng, lvl, count), rig.encrypt(rng, lvl, count)]
    plan, glk, xin, got = _case(rig, lvl, count, items, [0, 1])
    words = 2 * (lvl + 1) * N
    cts = np.stack([ct for _, ct in items])
    SENT = np.uint64(0x5EA75EA75EA75EA7)
    for s_index in (batch * words, batch * words + 6):
        host = np.full(8 * s_index + 4, SENT, dtype=np.uint64)          # room for 2^k = 8 outputs and a trailing guard
        host[: batch * words] = cts.reshape(-1)                          # `in` in the place of output 0
        buf = ctx.upload(host)
        plan.run(buf, batch, glk, out=buf, s_index=s_index)
        back = ctx.download(buf, host.shape)
        for i in range(count):
            assert np.array_equal(back[i * s_index: i * s_index + batch * words], got[i].reshape(-1)), (s_index, i)
            assert np.all(back[i * s_index + batch * words: (i + 1) * s_index] == SENT), (s_index, i)
        assert np.all(back[count * s_index:] == SENT), s_index
        # and from an input of its own into the same layout
        buf2 = ctx.upload(np.full(8 * s_index + 4, SENT, dtype=np.uint64))
        plan.run(xin, batch, glk, out=buf2, s_index=s_index)
        assert np.array_equal(ctx.download(buf2, host.shape), back), s_index
    assert np.array_equal(ctx.download(xin, cts.shape), cts)            # the input of its own is not written
    plan.close()
    rig.close()


def test_a_level_is_one_batched_key_switch():
    """dense layout, N = 2^11, batch 1: count 16 and count 9 both have four levels, and launch the same number of kernels"""
    need_gpu()
    from lattisense_amd._native import lib
    from lattisense_amd.device import BfvExpandPlan
    rig = Rig(11, "d8192", 400)
    ctx, L = rig.ctx, lib()
    rng = np.random.default_rng(400)
    _, ct = rig.encrypt(rng, 2, 16)
    xin = ctx.upload(ct[None])

    def launches(count, gather):
        plan = BfvExpandPlan(ctx, 2, count)
        plan.gather = gather
        glk = rig.keys_for(plan.galois_elements)
        plan.run(xin, 1, glk)                                            # tables uploaded outside the count
        ctx.sync()
        assert L.lsa_profile_begin(ctx.h, 1) == 0
        try:
            plan.run(xin, 1, glk)
            ctx.sync()
        finally:
            assert L.lsa_profile_end(ctx.h) == 0
        total = 0
        for kind in range(5):
            n = ctypes.c_longlong()
            assert L.lsa_profile_read(ctx.h, kind, None, None, None, ctypes.byref(n)) == 0
            total += n.value
        plan.close()
        return total
    for gather in (True, False):
        n16, n9, n8 = launches(16, gather), launches(9, gather), launches(8, gather)
        assert n16 == n9 and n16 > 0, (gather, n16, n9)
        assert n16 * 3 == n8 * 4, (gather, n16, n8)                      # four levels against three, the same launches per level
    rig.close()


def test_mul_monomial_against_numpy():
    need_gpu()
    rig = Rig(11, "d8192", 500)
    ctx, N, lvl = rig.ctx, rig.N, 2
    rng = np.random.default_rng(500)
    for polys in (1, 2, 3):
        words, stride = polys * (lvl + 1) * N, polys * (lvl + 1) * N + 10       # batch 2 with padding
        data = np.stack([np.stack([np.stack([rng.integers(0, rig.q[j], N, dtype=np.uint64) for j in range(lvl + 1)]) for _ in range(polys)])
                         for _ in range(2)])
        host = np.full(2 * stride, 3, dtype=np.uint64)
        for b in range(2):
            host[b * stride: b * stride + words] = data[b].reshape(-1)
        src = ctx.upload(host)

        def mono(buf, e):
            out = ctx.upload(np.full(2 * stride, 5, dtype=np.uint64))
            from lattisense_amd._native import check, lib
            check(lib().lsa_bfv_mul_monomial(ctx.h, lvl, polys, e, buf.ptr, out.ptr, 2, stride, stride, ctx.stream))
            return out
        for e in (0, 1, -1, 2, N - 1, N, N + 1, 2 * N - 1, -(2 * N + 3)):
            fwd = mono(src, e)
            back = ctx.download(fwd, (2 * stride,))
            for b in range(2):
                assert np.array_equal(back[b * stride: b * stride + words].reshape(polys, lvl + 1, N), mul_monomial(rig.o, data[b], e)), (polys, e, b)
                assert np.all(back[b * stride + words: (b + 1) * stride] == 5), (polys, e, b)
            rt = ctx.download(mono(fwd, -e), (2 * stride,))
            for b in range(2):
                assert np.array_equal(rt[b * stride: b * stride + words], host[b * stride: b * stride + words]), (polys, e, b)
    rig.close()


def test_refusals_leave_the_context_usable():
    need_gpu()
    from lattisense_amd import params
    from lattisense_amd._native import LsaError, check, lib
    from lattisense_amd.device import ALGO_BFV, ALGO_CKKS, BfvExpandPlan, DeviceContext
    rig = Rig(11, "d8192", 600)
    ctx, N, lvl, count = rig.ctx, rig.N, 2, 5
    rng = np.random.default_rng(600)
    _, ct = rig.encrypt(rng, lvl, count)
    words = 2 * (lvl + 1) * N
    plan = BfvExpandPlan(ctx, lvl, count)
    glk = rig.keys_for(plan.galois_elements)
    xin = ctx.upload(np.stack([ct, ct]))
    ref = ctx.download(plan.run(xin, 2, glk), (count, 2, 2, lvl + 1, N))

    def fails(fn, needle, who="lsa_bfv_expand"):
        with pytest.raises(LsaError) as e:
            fn()
        assert e.value.code == 1 and _message(e.value).startswith(who) and needle in _message(e.value), e.value

    sentinel = ctx.upload(np.full(count * 2 * words + 2 * words, 7, dtype=np.uint64))

    def untouched():
        assert np.all(ctx.download(sentinel, (sentinel.nwords,)) == 7)    # refused before anything was queued
        assert np.array_equal(ctx.download(plan.run(xin, 2, glk), ref.shape), ref)   # a good call on the same context
    for missing in (plan.galois_elements[0], N + 1):
        fails(lambda: plan.run(xin, 2, {e: k for e, k in glk.items() if e != missing}, out=sentinel), "element %d missing" % missing)
        untouched()
    low = dict(glk)                                                       # a key exported below the plan's level
    low[N + 1] = ctx.upload_key(rig.c.gen_galois_key(N + 1, lvl - 1), lvl - 1)
    fails(lambda: plan.run(xin, 2, low, out=sentinel), "lower level")
    untouched()
    elts = (ctypes.c_uint64 * len(glk))(*glk.keys())
    keys = (ctypes.c_void_p * len(glk))(*[k.value for k in glk.values()])
    call = lambda c, i, si, o, so, sx, b: check(lib().lsa_bfv_expand(c, plan._handle(), i, si, o, so, sx, b, len(glk), elts, keys, ctx.stream))
    S = sentinel.ptr
    fails(lambda: call(ctx.h, None, words, S, words, 2 * words, 2), "null")
    fails(lambda: call(ctx.h, xin.ptr, words, None, words, 2 * words, 2), "null")
    fails(lambda: call(ctx.h, xin.ptr + 8, words, S, words, 2 * words, 1), "16-byte")
    fails(lambda: call(ctx.h, xin.ptr, words, S + 8, words, 2 * words, 1), "16-byte")
    fails(lambda: call(ctx.h, xin.ptr, words, S, words + 1, 2 * words + 2, 2), "even")
    fails(lambda: call(ctx.h, xin.ptr, words - 2, S, words, 2 * words, 2), "stride")
    fails(lambda: call(ctx.h, xin.ptr, words, S, words - 2, 2 * words, 2), "stride")
    fails(lambda: call(ctx.h, xin.ptr, words, S, words, 2 * words + 1, 2), "s_index")
    fails(lambda: call(ctx.h, xin.ptr, words, S, words, 2 * words - 2, 2), "s_index")
    untouched()
    big = ctx.upload(np.full(count * 2 * words + 2 * words, 7, dtype=np.uint64))
    B = big.ptr
    fails(lambda: call(ctx.h, B + 8 * (words // 2), words, B, words, 2 * words, 2), "overlap")          # in across outputs 0
    fails(lambda: call(ctx.h, B + 8 * 2 * words, words, B, words, 2 * words, 2), "overlap")             # in is output 1
    fails(lambda: call(ctx.h, B, words + 2, B, words, 2 * words + 4, 2), "overlap")                     # same pointer, another stride
    assert np.all(ctx.download(big, (big.nwords,)) == 7)
    untouched()
    plan.run(xin, 0, glk, out=sentinel)                                   # batch <= 0: a no-op
    untouched()
    fails(lambda: BfvExpandPlan(ctx, lvl + 1, 4).run(xin, 1, {}), "level")
    fails(lambda: BfvExpandPlan(ctx, -1, 4).run(xin, 1, {}), "level")
    fails(lambda: BfvExpandPlan(ctx, lvl, 0), "count")
    fails(lambda: BfvExpandPlan(ctx, lvl, N + 1), "count")
    P = params.CKKS_DEFAULT[65536]
    ckks = DeviceContext(ALGO_CKKS, N, P["q"][:4], P["p"][:2])
    fails(lambda: BfvExpandPlan(ckks, lvl, 4).run(xin, 1, {}), "not BFV")
    ckks.close()
    nop = DeviceContext(ALGO_BFV, N, rig.q, [], rig.t)                    # a chain without a special prime
    fails(lambda: BfvExpandPlan(nop, lvl, 4).run(xin, 1, {}), "special prime")
    one = BfvExpandPlan(nop, lvl, 1)                                      # ... still copies
    nin = nop.upload(ct[None])
    assert np.array_equal(nop.download(one.run(nin, 1, {}), (1, 2, lvl + 1, N))[0], ct)
    one.close()
    nop.close()
    other = Rig(11, "d8192", 601)
    fails(lambda: call(other.ctx.h, xin.ptr, words, S, words, 2 * words, 1), "another context")
    other.close()
    untouched()
    # the monomial's own refusals
    mono = lambda c, l, pl, i, o, b, si, so: check(lib().lsa_bfv_mul_monomial(c, l, pl, 1, i, o, b, si, so, ctx.stream))
    fails(lambda: mono(ctx.h, lvl, 0, xin.ptr, S, 1, words, words), "polys", "lsa_bfv_mul_monomial")
    fails(lambda: mono(ctx.h, lvl, 4, xin.ptr, S, 1, words, words), "polys", "lsa_bfv_mul_monomial")
    fails(lambda: mono(ctx.h, lvl + 1, 2, xin.ptr, S, 1, words, words), "level", "lsa_bfv_mul_monomial")
    fails(lambda: mono(ctx.h, lvl, 2, None, S, 1, words, words), "null", "lsa_bfv_mul_monomial")
    fails(lambda: mono(ctx.h, lvl, 2, xin.ptr, S, 2, words, words - 2), "stride", "lsa_bfv_mul_monomial")
    fails(lambda: mono(ctx.h, lvl, 2, xin.ptr, xin.ptr, 1, words, words), "overlap", "lsa_bfv_mul_monomial")
    untouched()
    copy = BfvExpandPlan(ctx, lvl, 1)                                     # count 1: a copy, no key
    assert np.array_equal(ctx.download(copy.run(xin, 2, {}), (2, 2, lvl + 1, N)), np.stack([ct, ct]))
    copy.close()
    plan.close()
    rig.close()
