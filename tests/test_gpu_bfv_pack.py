"""BFV coefficient packing on the device (lsa_bfv_pack_*; bfv_pack.hip) against its CPU model (tests/bfv_pack_model.py: per node the
numpy shift, Oracle.vec add / sub, Oracle.bfv_rotate, Oracle.vec add): identical word for word for every batch item -- every plan
shape on a one-pass ring with and without the trace, keys above the plan's level with two special primes, the full pack of N = 2^10
(the s = 1 loads), the device round trip lsa_bfv_expand then lsa_bfv_pack, the 128 KiB LDS row at N = 2^14, the two-step form above
the LDS limit; the same words with the gather off, under lsa_set_fp64_ntt(0), with unfused tails, with the batch split into tiles on
two streams and with chunked transforms; both engines on the fp and ceiling operator chains with the fused key MAC read back; the
device's own composition of the five entry points; the layout rules; the launch count of a level; refusals that leave the context
usable.

Each model walk is computed once per distinct input set and case and shared by the variants."""
import ctypes

import numpy as np
import pytest

from tests.bfv_expand_model import decrypt_coeffs, encrypt_coeffs, levels_of
from tests.bfv_pack_model import (encrypt_constant_terms, expected_positions, galois_elements_of, keyswitches_of, nodes_of, pack,
                                  trace_elements_of)
from tests.gpu_util import need_gpu
from tests.test_gpu_bfv_expand import Rig as ExpandRig
from tests.test_gpu_bfv_expand import _message

pytestmark = pytest.mark.gpu


class Rig(ExpandRig):
    def inputs(self, rng, level, count):
        """(the values in coefficient 0, [count][2][level+1][N]): one input set, random coefficients everywhere"""
        values = rng.integers(0, self.t, count)
        return values, np.stack([ct for _, ct in encrypt_constant_terms(self.c, values, level, rng)])

    def pack_model(self, cts, level, trace):
        key = (id(cts), level, trace)
        if key not in self.models:
            self.models[key] = pack(self.o, self.key_of, self.klvl, cts, level, trace)
        return self.models[key]


def first_unchanged(count):
    return max(1, 1 << max(levels_of(count) - 1, 0))


def _run(ctx, plan, host, batch, glk, in_place=False, s_index=None):
    """host: the input array as the device is to hold it.  Returns (the result [batch][2][L][N], the input array afterwards)."""
    words = 2 * (plan.level + 1) * ctx.n
    buf = ctx.upload(host)
    out = plan.run(buf, batch, glk, out=buf if in_place else None, s_index=s_index)
    res = ctx.download(out, (batch, 2, plan.level + 1, ctx.n)) if not in_place else None
    after = ctx.download(buf, host.shape)
    if in_place:
        res = after.reshape(-1)[: batch * words].reshape(batch, 2, plan.level + 1, ctx.n).copy()
    return res, after


def _case(rig, level, count, trace, sets, order, decrypt=False):
    """sets: [(values, cts)] distinct input sets; order: the batch as indices into sets.  Returns (plan, glk, the host input array
    [count][batch][2][level+1][N], the result words [batch][2][level+1][N])."""
    from lattisense_amd.device import BfvPackPlan
    N = rig.N
    plan = BfvPackPlan(rig.ctx, level, count, trace)
    assert plan.galois_elements == galois_elements_of(N, count, trace)
    assert plan.levels == levels_of(count) and plan.trace_levels == len(trace_elements_of(N, count, trace))
    assert plan.keyswitches == keyswitches_of(N, count, trace)
    glk = rig.keys_for(plan.galois_elements)
    batch = len(order)
    host = np.stack([sets[i][1] for i in order], axis=1)
    got, after = _run(rig.ctx, plan, host, batch, glk)
    for b, i in enumerate(order):
        want, _ = rig.pack_model(sets[i][1], level, trace)
        assert np.array_equal(got[b], want), "batch item %d differs from the model (count %d, trace %d)" % (b, count, trace)
    assert np.array_equal(after[first_unchanged(count):], host[first_unchanged(count):]), "an input that is only read was written"
    if decrypt:
        dec = decrypt_coeffs(rig.c, got[0])
        pos, want = expected_positions(sets[order[0]][0], N, count, trace, rig.t)
        assert np.array_equal(dec[pos], want), "the result does not decrypt to its coefficients (count %d, trace %d)" % (count, trace)
        if trace:
            rest = np.ones(N, dtype=bool)
            rest[pos] = False
            assert not dec[rest].any(), "the trace left something beside the packed coefficients (count %d)" % count
    return plan, glk, host, got


def test_one_pass_ring_every_plan_shape():
    """N = 2^11, 3 Q + 1 P, top level: the copy, one level, unpaired nodes at the first level (3, 5, 11), full levels (2, 4, 8, 16),
    the trace for 1, 5 and 16; batch 3 = (a, b, a): batch positions are independent"""
    need_gpu()
    rig = Rig(11, "d8192", 100)
    rng = np.random.default_rng(7)
    cases = [(count, 0) for count in (1, 2, 3, 4, 5, 8, 11, 16)] + [(count, 1) for count in (1, 5, 16)]
    for count, trace in cases:
        sets = [rig.inputs(rng, 2, count), rig.inputs(rng, 2, count)]
        plan, _, _, got = _case(rig, 2, count, trace, sets, [0, 1, 0], decrypt=count in (5, 16))
        assert plan.gather_in_force()
        assert np.array_equal(got[0], got[2]) and not np.array_equal(got[0], got[1])
        plan.close()
        rig.models.clear()
    rig.close()


@pytest.mark.parametrize("level,key_level", [(3, 5), (5, 5)])
def test_keys_above_the_level_and_two_special_primes(level, key_level):
    """N = 2^12, 6 Q + 2 P: level 3 with keys exported at level 5, and level 5; count 6 with the trace"""
    need_gpu()
    rig = Rig(12, "d16384", 12 + level, key_level)
    rng = np.random.default_rng(12 + level)
    sets = [rig.inputs(rng, level, 6), rig.inputs(rng, level, 6)]
    _case(rig, level, 6, 1, sets, [0, 1], decrypt=True)[0].close()
    rig.close()


def test_full_pack_and_the_round_trip_with_the_expansion():
    """N = 2^10, level 1, count 1024: ten levels down to s = 1 (single-word loads of the partner), 1023 key switches; every
    coefficient decrypts to 2^10 times its input's constant term.  Then the device round trip: lsa_bfv_expand of one ciphertext
    into 1024 and lsa_bfv_pack of those back into one, which decrypts to 2^20 m_i at coefficient i"""
    need_gpu()
    from lattisense_amd.device import BfvExpandPlan, BfvPackPlan
    rig = Rig(10, "d8192", 10)
    rng = np.random.default_rng(10)
    n, t = rig.N, rig.t
    sets = [rig.inputs(rng, 1, n)]
    plan, glk, _, got = _case(rig, 1, n, 0, sets, [0])
    assert (plan.levels, plan.keyswitches) == (10, 1023) and plan.galois_elements[-1] == n + 1
    assert np.array_equal(decrypt_coeffs(rig.c, got[0]), sets[0][0] * 1024 % t)
    m = rng.integers(0, t, n)
    ex = BfvExpandPlan(rig.ctx, 1, n)
    eglk = rig.keys_for(ex.galois_elements)
    mid = ex.run(rig.ctx.upload(encrypt_coeffs(rig.c, m, 1)[None]), 1, eglk)
    res = rig.ctx.download(plan.run(mid, 1, glk), (2, 2, n))
    assert np.array_equal(decrypt_coeffs(rig.c, res), m * pow(2, 20, t) % t)
    ex.close()
    plan.close()
    rig.close()


@pytest.fixture(scope="module")
def full_ring():
    """N = 2^14, BFV_DEFAULT[16384] at level 5, count 4, batch 2: two-pass transforms, a 128 KiB row in LDS, all eight register
    pairs of a thread of the tail"""
    need_gpu()
    rig = Rig(14, "d16384", 14)
    rng = np.random.default_rng(14)
    sets = [rig.inputs(rng, 5, 4), rig.inputs(rng, 5, 4)]
    yield rig, sets
    rig.close()


def test_full_ring_with_the_largest_lds_row(full_ring):
    rig, sets = full_ring
    plan = _case(rig, 5, 4, 0, sets, [0, 1], decrypt=True)[0]
    assert plan.gather_in_force()
    plan.close()


def test_above_the_lds_limit_runs_the_two_step_form():
    """N = 2^15, 4 Q + 3 P, level 1, count 3: a limb does not fit in LDS, `gather` reports 0, asking for it is refused"""
    need_gpu()
    from lattisense_amd._native import LsaError
    rig = Rig(15, "d32768_4", 15, key_level=1)
    rng = np.random.default_rng(15)
    plan, glk, host, got = _case(rig, 1, 3, 0, [rig.inputs(rng, 1, 3)], [0], decrypt=True)
    assert not plan.gather_in_force()
    with pytest.raises(LsaError) as e:
        plan.set_gather(True)
    assert e.value.code == 1 and _message(e.value).startswith("lsa_bfv_pack_set_gather") and "enable" in _message(e.value), e.value
    assert not plan.gather_in_force()
    plan.gather = None
    assert np.array_equal(_run(rig.ctx, plan, host, 1, glk)[0], got)
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
    for count, trace in ((5, 1), (16, 0)):
        sets = [rig.inputs(rng, 2, count), rig.inputs(rng, 2, count)]
        plan, glk, host, got = _case(rig, 2, count, trace, sets, [0, 1, 0])
        _variants(rig.ctx, plan, lambda: _run(rig.ctx, plan, host, 3, glk)[0], got)
        plan.close()
    rig.close()


def test_same_words_across_variants_full_ring(full_ring):
    rig, sets = full_ring
    plan, glk, host, got = _case(rig, 5, 4, 0, sets, [0, 1])
    _variants(rig.ctx, plan, lambda: _run(rig.ctx, plan, host, 2, glk)[0], got)
    plan.close()


@pytest.mark.parametrize("kind", ["fp", "ceiling"])
def test_both_engines(kind):
    """tests/boundary.py bfv_operator_chain at N = 2^13, count 5 with the trace, at the top level and at the lift level, the operands
    the `max` and `uniform` patterns, pattern keys: fp has every row on the FP64 engine and takes the fused second pass + key MAC
    (read back and asserted), ceiling has none"""
    need_gpu()
    from lattisense_amd.device import BfvPackPlan
    from tests import boundary
    n = 1 << 13
    q, p = boundary.bfv_operator_chain(kind, n)
    rig = Rig(13, None, 13, mods=(q, p, boundary.BFV_OPERATOR_T))
    rng = np.random.default_rng(13)
    beta = (rig.klvl + 1 + len(p) - 1) // len(p)
    names = ("top", "uniform", "max", "half")
    for lvl in (rig.top, boundary.lift_level(q, p)):
        plan = BfvPackPlan(rig.ctx, lvl, 5, True)
        for i, g in enumerate(plan.galois_elements):
            if g not in rig.host_keys:
                rig.host_keys[g] = boundary.pattern_key(names[i % len(names)], q + p, beta, n, rng)
        glk = rig.keys_for(plan.galois_elements)
        fused = lambda: all(rig.ctx.key_switch_fused(lvl, k) for k in glk.values())
        assert fused() == (kind == "fp"), (kind, lvl)
        host = boundary.pattern_ct(("max", "uniform") * 5, q[: lvl + 1], 2, n, rng).reshape(5, 2, 2, lvl + 1, n)
        got = _run(rig.ctx, plan, host, 2, glk)[0]
        for b in range(2):
            want, _ = pack(rig.o, rig.key_of, rig.klvl, host[:, b], lvl, 1)
            assert np.array_equal(got[b], want), (kind, lvl, b)
        _variants(rig.ctx, plan, lambda: _run(rig.ctx, plan, host, 2, glk)[0], got, fused_off=fused)
        plan.close()
    rig.close()


def test_against_the_devices_own_composition():
    """lsa_bfv_mul_monomial, lsa_poly_addsub (add, sub), lsa_bfv_rotate, lsa_poly_addsub (add) per node, count 7 with the trace at
    N = 2^12, word for word"""
    need_gpu()
    from lattisense_amd.device import BfvPackPlan
    rig = Rig(12, "d16384", 77)
    ctx, N, lvl, count = rig.ctx, rig.N, 5, 7
    rng = np.random.default_rng(77)
    host = np.stack([rig.inputs(rng, lvl, count)[1] for _ in range(2)], axis=1)
    plan = BfvPackPlan(ctx, lvl, count, True)
    glk = rig.keys_for(plan.galois_elements)
    got = _run(ctx, plan, host, 2, glk)[0]
    c = [ctx.upload(host[i]) for i in range(count)]
    steps = nodes_of(N, count) + [(g, 0, 1, 0) for g in trace_elements_of(N, count, 1)]
    for g, s, nodes, n_pair in steps:
        for a in range(nodes):
            u = v = c[a]
            if a < n_pair:
                xb = ctx.bfv_mul_monomial(lvl, c[a + nodes], s, 2)
                u, v = ctx.addsub(0, lvl, 2, c[a], xb, 2), ctx.addsub(1, lvl, 2, c[a], xb, 2)
            c[a] = ctx.addsub(0, lvl, 2, u, ctx.bfv_rotate(lvl, v, g, glk[g], 2), 2)
    assert np.array_equal(ctx.download(c[0], (2, 2, lvl + 1, N)), got)
    plan.close()
    rig.close()


def test_layout_in_place_gaps_and_unchanged_inputs():
    """`out` is input 0, and `out` elsewhere; a non-dense s_index with sentinel words in every gap and behind the last input; the
    inputs i >= max(1, 2^(k-1)) are unchanged"""
    need_gpu()
    rig = Rig(11, "d8192", 300)
    ctx, N, lvl, count, batch = rig.ctx, rig.N, 2, 5, 2
    rng = np.random.default_rng(300)
    sets = [rig.inputs(rng, lvl, count), rig.inputs(rng, lvl, count)]
    for trace in (0, 1):
        plan, glk, dense, got = _case(rig, lvl, count, trace, sets, [0, 1])
        words = 2 * (lvl + 1) * N
        SENT = np.uint64(0x5EA75EA75EA75EA7)
        for s_index in (batch * words, batch * words + 6):
            host = np.full(count * s_index + 4, SENT, dtype=np.uint64)          # a trailing guard behind the last input
            for i in range(count):
                host[i * s_index: i * s_index + batch * words] = dense[i].reshape(-1)
            for in_place in (True, False):
                res, after = _run(ctx, plan, host, batch, glk, in_place=in_place, s_index=s_index)
                assert np.array_equal(res, got), (trace, s_index, in_place)
                for i in range(count):
                    assert np.all(after[i * s_index + batch * words: (i + 1) * s_index] == SENT), (trace, s_index, in_place, i)
                assert np.all(after[count * s_index:] == SENT), (trace, s_index, in_place)
                lo = first_unchanged(count) * s_index
                assert np.array_equal(after[lo:], host[lo:]), (trace, s_index, in_place)
        plan.close()
    rig.close()


def test_a_level_is_one_head_and_one_batched_key_switch():
    """dense layout, N = 2^11, batch 1: count 16 and count 9 both have four levels and launch the same number of kernels, 4/3 of what
    the three levels of count 8 launch -- a level's launches do not grow with its nodes"""
    need_gpu()
    from lattisense_amd._native import lib
    from lattisense_amd.device import BfvPackPlan
    rig = Rig(11, "d8192", 400)
    ctx, L = rig.ctx, lib()
    rng = np.random.default_rng(400)
    host = rig.inputs(rng, 2, 16)[1][:, None]
    xin = ctx.upload(host)

    def launches(count, gather):
        plan = BfvPackPlan(ctx, 2, count)
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
    per_level = {}
    for gather in (True, False):
        n16, n9, n8 = launches(16, gather), launches(9, gather), launches(8, gather)
        assert n16 == n9 and n16 > 0, (gather, n16, n9)
        assert n16 * 3 == n8 * 4, (gather, n16, n8)                      # four levels against three, the same launches per level
        per_level[gather] = n16 // 4
    assert per_level[False] == per_level[True] + 1                       # the two-step form's combine kernel, and nothing else
    rig.close()


def test_refusals_leave_the_context_usable():
    need_gpu()
    from lattisense_amd import params
    from lattisense_amd._native import LsaError, check, lib
    from lattisense_amd.device import ALGO_BFV, ALGO_CKKS, BfvPackPlan, DeviceContext
    rig = Rig(11, "d8192", 600)
    ctx, N, lvl, count = rig.ctx, rig.N, 2, 5
    rng = np.random.default_rng(600)
    _, cts = rig.inputs(rng, lvl, count)
    host = np.stack([cts, cts], axis=1)
    words = 2 * (lvl + 1) * N
    plan = BfvPackPlan(ctx, lvl, count, True)
    glk = rig.keys_for(plan.galois_elements)
    ref = _run(ctx, plan, host, 2, glk)[0]

    def fails(fn, needle, who="lsa_bfv_pack"):
        with pytest.raises(LsaError) as e:
            fn()
        assert e.value.code == 1 and _message(e.value).startswith(who) and needle in _message(e.value), e.value

    xin = ctx.upload(host)
    sentinel = ctx.upload(np.full(2 * words + 4, 7, dtype=np.uint64))

    def untouched():
        assert np.all(ctx.download(sentinel, (sentinel.nwords,)) == 7)    # refused before anything was queued
        assert np.array_equal(ctx.download(xin, host.shape), host)
        assert np.array_equal(_run(ctx, plan, host, 2, glk)[0], ref)      # a good call on the same context
    for missing in (plan.galois_elements[0], N + 1):
        fails(lambda: plan.run(xin, 2, {e: k for e, k in glk.items() if e != missing}, out=sentinel), "element %d missing" % missing)
        untouched()
    low = dict(glk)                                                       # a key exported below the plan's level
    low[3] = ctx.upload_key(rig.c.gen_galois_key(3, lvl - 1), lvl - 1)
    fails(lambda: plan.run(xin, 2, low, out=sentinel), "lower level")
    untouched()
    elts = (ctypes.c_uint64 * len(glk))(*glk.keys())
    keys = (ctypes.c_void_p * len(glk))(*[k.value for k in glk.values()])
    call = lambda c, i, si, sx, o, so, b: check(lib().lsa_bfv_pack(c, plan._handle(), i, si, sx, o, so, b, len(glk), elts, keys, ctx.stream))
    S = sentinel.ptr
    fails(lambda: call(ctx.h, None, words, 2 * words, S, words, 2), "null")
    untouched()
    fails(lambda: call(ctx.h, xin.ptr, words, 2 * words, None, words, 2), "null")
    untouched()
    fails(lambda: call(ctx.h, xin.ptr + 8, words, 2 * words, S, words, 1), "16-byte")
    untouched()
    fails(lambda: call(ctx.h, xin.ptr, words, 2 * words, S + 8, words, 1), "16-byte")
    untouched()
    fails(lambda: call(ctx.h, xin.ptr, words + 1, 2 * words + 2, S, words, 2), "even")
    untouched()
    fails(lambda: call(ctx.h, xin.ptr, words - 2, 2 * words, S, words, 2), "stride")
    untouched()
    fails(lambda: call(ctx.h, xin.ptr, words, 2 * words, S, words - 2, 2), "stride")
    untouched()
    fails(lambda: call(ctx.h, xin.ptr, words, 2 * words + 1, S, words, 2), "s_index")
    untouched()
    fails(lambda: call(ctx.h, xin.ptr, words, 2 * words - 2, S, words, 2), "s_index")
    untouched()
    X = xin.ptr
    fails(lambda: call(ctx.h, X, words, 2 * words, X + 8 * (words // 2), words, 2), "overlap")          # out across inputs 0
    untouched()
    fails(lambda: call(ctx.h, X, words, 2 * words, X + 8 * 2 * words, words, 2), "overlap")             # out is input 1
    untouched()
    fails(lambda: call(ctx.h, X, words, 2 * words + 4, X, words + 2, 2), "overlap")                     # same pointer, another stride
    untouched()
    plan.run(xin, 0, glk, out=sentinel)                                   # batch <= 0: a no-op
    untouched()
    fails(lambda: BfvPackPlan(ctx, lvl + 1, 4).run(xin, 1, {}), "level")
    fails(lambda: BfvPackPlan(ctx, -1, 4).run(xin, 1, {}), "level")
    fails(lambda: BfvPackPlan(ctx, lvl, 0), "count")
    fails(lambda: BfvPackPlan(ctx, lvl, N + 1), "count")
    untouched()
    P = params.CKKS_DEFAULT[65536]
    ckks = DeviceContext(ALGO_CKKS, N, P["q"][:4], P["p"][:2])
    fails(lambda: BfvPackPlan(ckks, lvl, 4).run(xin, 1, {}), "not BFV")
    ckks.close()
    untouched()
    nop = DeviceContext(ALGO_BFV, N, rig.q, [], rig.t)                    # a chain without a special prime
    fails(lambda: BfvPackPlan(nop, lvl, 4).run(xin, 1, {}), "special prime")
    fails(lambda: BfvPackPlan(nop, lvl, 1, True).run(xin, 1, {}), "special prime")
    one = BfvPackPlan(nop, lvl, 1)                                        # ... still copies
    nin = nop.upload(cts[0][None])
    assert np.array_equal(nop.download(one.run(nin, 1, {}), (1, 2, lvl + 1, N))[0], cts[0])
    one.close()
    nop.close()
    untouched()
    other = Rig(11, "d8192", 601)
    fails(lambda: call(other.ctx.h, xin.ptr, words, 2 * words, S, words, 1), "another context")
    other.close()
    untouched()
    copy = BfvPackPlan(ctx, lvl, 1)                                       # count 1 without the trace: a copy, no key
    assert np.array_equal(ctx.download(copy.run(xin, 2, {}), (2, 2, lvl + 1, N)), host[0])
    copy.close()
    plan.close()
    rig.close()
