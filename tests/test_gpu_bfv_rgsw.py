"""BFV external product RLWE x RGSW, CMux and select by an encrypted index on the device (lsa_bfv_external_product, lsa_bfv_cmux,
lsa_bfv_select_*; bfv_select.hip, key_switch.hip external_product) against their CPU model (tests/rgsw_model.py: Oracle.gadget_product
twice, Oracle.vec add on every row, one Oracle.moddown): identical word for word for every batch item -- a one-pass ring with and
without base and the outputs decrypted, keys above the level with two special primes and a last digit of one limb, one digit at
N = 2^15, the full ring with two-pass transforms, both engines on the fp / mixed / ceiling operator chains with pattern operands, the
fold of the long sum at the 61-bit ceiling on both sides of eight products and in the streaming instantiation; the select tree for every
plan shape, dense and gapped layouts, in place and elsewhere; the same words under lsa_set_rgsw_pair_mac(0), lsa_set_fp64_ntt(0),
unfused tails, tiles on two streams and chunked transforms; the launch count of a level; refusals that leave the context usable.

Each model is computed once per distinct input and shared by the variants."""
import ctypes

import numpy as np
import pytest

from tests.bfv_expand_model import decrypt_coeffs, encrypt_coeffs, mul_monomial
from tests.gpu_util import need_gpu
from tests.rgsw_model import cmux, constant, external_product, first_unchanged, levels_of, monomial, rgsw_encrypt, select
from tests.test_gpu_bfv_expand import Rig as ExpandRig
from tests.test_gpu_bfv_expand import _message

pytestmark = pytest.mark.gpu


class Rig(ExpandRig):
    def rgsw(self, m_coeffs):
        """(host (R0, R1), device (r0, r1)) of the small polynomial m"""
        host = rgsw_encrypt(self.c, m_coeffs, self.klvl)
        return host, self.upload_rgsw(host)

    def upload_rgsw(self, host):
        return tuple(self.ctx.upload_key(k, self.klvl) for k in host)

    def bits(self):
        """the RGSW ciphertexts of 0 and 1, made once"""
        if not hasattr(self, "_bits"):
            self._bits = [self.rgsw(constant(self.N, b)) for b in (0, 1)]
        return self._bits

    def message(self, rng, level):
        m = rng.integers(0, self.t, self.N)
        return m, encrypt_coeffs(self.c, m, level)


def _ep(rig, level, cts, R, base=None):
    ctx = rig.ctx
    batch = len(cts)
    out = ctx.bfv_external_product(level, ctx.upload(np.stack(cts)), R, batch, base=ctx.upload(np.stack(base)) if base is not None else None)
    return ctx.download(out, (batch, 2, level + 1, rig.N))


def _cmux(rig, level, c0s, c1s, R):
    ctx = rig.ctx
    batch = len(c0s)
    out = ctx.bfv_cmux(level, ctx.upload(np.stack(c0s)), ctx.upload(np.stack(c1s)), R, batch)
    return ctx.download(out, (batch, 2, level + 1, rig.N))


def _variants(ctx, run, got):
    """run() under each setting must give `got` again; every setting is put back"""
    from lattisense_amd._native import check, lib
    for pair in (0, 1):
        ctx.set_rgsw_pair_mac(pair)
        try:
            assert np.array_equal(run(), got), "pair MAC %d" % pair
            ctx.set_fp64_ntt(0)
            try:
                assert np.array_equal(run(), got), "integer engine, pair MAC %d" % pair
            finally:
                ctx.set_fp64_ntt(1)
            check(lib().lsa_set_fuse_tails(ctx.h, 0))
            try:
                assert np.array_equal(run(), got), "unfused tails, pair MAC %d" % pair
            finally:
                check(lib().lsa_set_fuse_tails(ctx.h, 1))
            check(lib().lsa_set_dual_stream(ctx.h, 1))
            try:
                for tile in (1, 2):
                    ctx.set_tile_batch(tile)
                    assert np.array_equal(run(), got), "tile batch %d on two streams, pair MAC %d" % (tile, pair)
            finally:
                ctx.set_tile_batch(0)
                check(lib().lsa_set_dual_stream(ctx.h, 0))
            ctx.set_ntt_chunk_mib(1)
            try:
                assert np.array_equal(run(), got), "chunked transforms, pair MAC %d" % pair
            finally:
                ctx.set_ntt_chunk_mib(0)
        finally:
            ctx.set_rgsw_pair_mac(1)


def _both_forms(ctx, run, got):
    ctx.set_rgsw_pair_mac(0)
    try:
        assert np.array_equal(run(), got), "two-step form"
    finally:
        ctx.set_rgsw_pair_mac(1)


def test_one_pass_ring_product_cmux_and_decryption():
    """N = 2^11, 3 Q + 1 P, level 2, batch 3 = (a, b, a): the external product with and without base, from a dense and from a gapped
    ct (one decomposition sequence and two), in place over ct and over base; the CMux with R(0), R(1) and R(X^e); everything decrypted"""
    need_gpu()
    from lattisense_amd._native import check, lib
    rig = Rig(11, "d8192", 100)
    ctx, N, t, lvl = rig.ctx, rig.N, rig.t, 2
    rng = np.random.default_rng(100)
    (ma, a), (mb, b), (mz, z) = rig.message(rng, lvl), rig.message(rng, lvl), rig.message(rng, lvl)
    e = 5
    Rh, R = rig.rgsw(monomial(N, e))
    want = {id(x): external_product(rig.o, lvl, x, Rh, rig.klvl) for x in (a, b)}
    got = _ep(rig, lvl, [a, b, a], R)
    for i, x in enumerate((a, b, a)):
        assert np.array_equal(got[i], want[id(x)]), i
    assert np.array_equal(decrypt_coeffs(rig.c, got[0]), decrypt_coeffs(rig.c, mul_monomial(rig.o, a, e)))
    _both_forms(ctx, lambda: _ep(rig, lvl, [a, b, a], R), got)
    want_b = {id(x): external_product(rig.o, lvl, x, Rh, rig.klvl, base=z) for x in (a, b)}
    got_b = _ep(rig, lvl, [a, b, a], R, base=[z, z, z])
    for i, x in enumerate((a, b, a)):
        assert np.array_equal(got_b[i], want_b[id(x)]), i
    shifted = np.roll(ma, e)
    shifted[:e] = (-shifted[:e]) % t
    assert np.array_equal(decrypt_coeffs(rig.c, got_b[0]), (shifted + mz) % t)
    # a gapped ct takes two decomposition sequences; out over base, then out over ct
    words = 2 * (lvl + 1) * N
    SENT = np.uint64(0x5EA75EA75EA75EA7)
    for pair in (1, 0):
        ctx.set_rgsw_pair_mac(pair)
        host = np.full(3 * (words + 6), SENT, dtype=np.uint64)
        for i, x in enumerate((a, b, a)):
            host[i * (words + 6): i * (words + 6) + words] = x.reshape(-1)
        xin, bs = ctx.upload(host), ctx.upload(np.stack([z, z, z]))
        check(lib().lsa_bfv_external_product(ctx.h, lvl, xin.ptr, words + 6, R[0], R[1], bs.ptr, words, bs.ptr, words, 3, ctx.stream))
        assert np.array_equal(ctx.download(bs, (3, 2, lvl + 1, N)), got_b), pair
        assert np.array_equal(ctx.download(xin, host.shape), host)
        check(lib().lsa_bfv_external_product(ctx.h, lvl, xin.ptr, words + 6, R[0], R[1], None, 0, xin.ptr, words + 6, 3, ctx.stream))
        after = ctx.download(xin, host.shape).reshape(3, words + 6)
        assert np.array_equal(after[:, :words].reshape(3, 2, lvl + 1, N), got) and np.all(after[:, words:] == SENT), pair
    ctx.set_rgsw_pair_mac(1)
    # CMux
    (h0, r0), (h1, r1) = rig.bits()
    for Rh_, R_, plain in ((h0, r0, (ma, mb, ma)), (h1, r1, (mb, ma, mz)), (Rh, R, None)):
        c0s, c1s = [a, b, a], [b, a, z]
        res = _cmux(rig, lvl, c0s, c1s, R_)
        models = {}
        for i in range(3):
            key = (id(c0s[i]), id(c1s[i]))
            if key not in models:
                models[key] = cmux(rig.o, lvl, c0s[i], c1s[i], Rh_, rig.klvl)
            assert np.array_equal(res[i], models[key]), i
            if plain is not None:
                assert np.array_equal(decrypt_coeffs(rig.c, res[i]), plain[i]), i
        _both_forms(ctx, lambda: _cmux(rig, lvl, c0s, c1s, R_), res)
        c0d, c1d = ctx.upload(np.stack(c0s)), ctx.upload(np.stack(c1s))   # out over c0, then over c1
        assert np.array_equal(ctx.download(ctx.bfv_cmux(lvl, c0d, c1d, R_, 3, out=c0d), res.shape), res)
        c0d = ctx.upload(np.stack(c0s))
        assert np.array_equal(ctx.download(ctx.bfv_cmux(lvl, c0d, c1d, R_, 3, out=c1d), res.shape), res)
    rig.close()


@pytest.mark.parametrize("level,key_level", [(3, 5), (5, 5), (4, 5)])
def test_two_special_primes_keys_above_the_level_and_a_one_limb_digit(level, key_level):
    """N = 2^12, 6 Q + 2 P: level 3 with keys exported at level 5, level 5 (two-limb digits), level 4 (a last digit of one limb)"""
    need_gpu()
    rig = Rig(12, "d16384", 12 + level, key_level)
    rng = np.random.default_rng(12 + level)
    (ma, a), (mb, b) = rig.message(rng, level), rig.message(rng, level)
    Rh, R = rig.rgsw(monomial(rig.N, 3))
    got = _ep(rig, level, [a, b], R, base=[b, a])
    assert np.array_equal(got[0], external_product(rig.o, level, a, Rh, rig.klvl, base=b))
    assert np.array_equal(got[1], external_product(rig.o, level, b, Rh, rig.klvl, base=a))
    sh = np.roll(ma, 3)
    sh[:3] = (-sh[:3]) % rig.t
    assert np.array_equal(decrypt_coeffs(rig.c, got[0]), (sh + mb) % rig.t)
    _both_forms(rig.ctx, lambda: _ep(rig, level, [a, b], R, base=[b, a]), got)
    h1, r1 = rig.bits()[1]
    res = _cmux(rig, level, [a, b], [b, a], r1)
    assert np.array_equal(res[0], cmux(rig.o, level, a, b, h1, rig.klvl)) and np.array_equal(decrypt_coeffs(rig.c, res[0]), mb)
    rig.close()


def test_one_digit_is_a_sum_of_two_products():
    """N = 2^15, the first 4 Q + 3 P, level 1: beta = 1, the k_ks_mac_pair<1> instantiation on a two-pass ring"""
    need_gpu()
    rig = Rig(15, "d32768_4", 15, key_level=1)
    rng = np.random.default_rng(15)
    (ma, a), (mb, b) = rig.message(rng, 1), rig.message(rng, 1)
    h1, r1 = rig.bits()[1]
    got = _cmux(rig, 1, [a], [b], r1)
    assert np.array_equal(got[0], cmux(rig.o, 1, a, b, h1, rig.klvl))
    assert np.array_equal(decrypt_coeffs(rig.c, got[0]), mb)
    _both_forms(rig.ctx, lambda: _cmux(rig, 1, [a], [b], r1), got)
    rig.close()


def test_full_ring_and_its_variants():
    """N = 2^14, BFV_DEFAULT[16384] at level 5, batch 2: two-pass transforms, three two-limb digits; every variant"""
    need_gpu()
    rig = Rig(14, "d16384", 14)
    rng = np.random.default_rng(14)
    (ma, a), (mb, b) = rig.message(rng, 5), rig.message(rng, 5)
    h1, r1 = rig.bits()[1]
    got = _cmux(rig, 5, [a, b], [b, a], r1)
    assert np.array_equal(got[0], cmux(rig.o, 5, a, b, h1, rig.klvl))
    assert np.array_equal(got[1], cmux(rig.o, 5, b, a, h1, rig.klvl))
    assert np.array_equal(decrypt_coeffs(rig.c, got[0]), mb)
    _variants(rig.ctx, lambda: _cmux(rig, 5, [a, b], [b, a], r1), got)
    rig.close()


@pytest.mark.parametrize("kind", ["fp", "mixed", "ceiling"])
def test_both_engines_on_the_operator_chains(kind):
    """tests/boundary.py bfv_operator_chain at N = 2^13, at the top level and at the lift level (a last digit of one limb: on fp it is
    below 2^53 and lifted by the extension transform's load), pattern keys (max, top, uniform) and pattern ciphertexts"""
    need_gpu()
    from tests import boundary
    n = 1 << 13
    q, p = boundary.bfv_operator_chain(kind, n)
    rig = Rig(13, None, 13, mods=(q, p, boundary.BFV_OPERATOR_T))
    rng = np.random.default_rng(13)
    beta = (rig.klvl + 1 + len(p) - 1) // len(p)
    lift = boundary.lift_level(q, p)
    assert boundary.digit_sizes(lift, len(p))[-1] == 1
    if kind == "fp":
        assert q[lift] >> 53 == 0                                          # the lifted single-limb digit is reached
    for lvl in (rig.top, lift):
        for k0, k1 in (("max", "top"), ("uniform", "max")):
            Rh = (boundary.pattern_key(k0, q + p, beta, n, rng), boundary.pattern_key(k1, q + p, beta, n, rng))
            R = rig.upload_rgsw(Rh)
            cts = boundary.pattern_ct(("max", "top", "uniform", "max"), q[: lvl + 1], 2, n, rng)
            got = _cmux(rig, lvl, [cts[0], cts[2]], [cts[1], cts[3]], R)
            assert np.array_equal(got[0], cmux(rig.o, lvl, cts[0], cts[1], Rh, rig.klvl)), (kind, lvl, k0)
            assert np.array_equal(got[1], cmux(rig.o, lvl, cts[2], cts[3], Rh, rig.klvl)), (kind, lvl, k0)
            if k0 == "max":
                _variants(rig.ctx, lambda: _cmux(rig, lvl, [cts[0], cts[2]], [cts[1], cts[3]], R), got)
            else:
                _both_forms(rig.ctx, lambda: _cmux(rig, lvl, [cts[0], cts[2]], [cts[1], cts[3]], R), got)
    rig.close()


@pytest.mark.parametrize("nq", [4, 5, 9])
def test_the_fold_of_the_long_sum_at_the_ceiling(nq):
    """tests/boundary.py ceiling_chain(4096, nq, 1) at the top level: beta = nq digits, 2 nq products of residues next to 2^61 --
    8 (the last count that needs no fold inside), 10, and 18 (beta > 8: the streaming instantiation, folds at 8 and 16).  Pattern keys
    top / max, ciphertexts (max, uniform, top)"""
    need_gpu()
    from tests import boundary
    n = 4096
    C = boundary.ceiling_chain(n, nq, 1)
    q, p = C["q"], C["p"]
    assert all(boundary.is_ceiling(m) for m in q + p)
    rig = Rig(12, None, nq, mods=(q, p, boundary.BFV_OPERATOR_T))
    rng = np.random.default_rng(nq)
    lvl = rig.top
    Rh = (boundary.pattern_key("top", q + p, nq, n, rng), boundary.pattern_key("max", q + p, nq, n, rng))
    R = rig.upload_rgsw(Rh)
    cts = boundary.pattern_ct(("max", "uniform", "top"), q, 2, n, rng)
    got = _ep(rig, lvl, list(cts), R)
    for b in range(3):
        want = external_product(rig.o, lvl, cts[b], Rh, rig.klvl)
        assert all(int(want[:, j].max()) < q[j] for j in range(nq))            # canonical
        assert np.array_equal(got[b], want), (nq, b)
    _both_forms(rig.ctx, lambda: _ep(rig, lvl, list(cts), R), got)
    rig.close()


def _run_select(ctx, plan, host, batch, sel, in_place=False, s_index=None):
    """host: the input array as the device is to hold it.  Returns (the result [batch][2][L][N], the input array afterwards)."""
    words = 2 * (plan.level + 1) * ctx.n
    buf = ctx.upload(host)
    out = plan.run(buf, batch, sel, out=buf if in_place else None, s_index=s_index)
    res = ctx.download(out, (batch, 2, plan.level + 1, ctx.n)) if not in_place else None
    after = ctx.download(buf, host.shape)
    if in_place:
        res = after.reshape(-1)[: batch * words].reshape(batch, 2, plan.level + 1, ctx.n).copy()
    return res, after


@pytest.fixture(scope="module")
def select_rig():
    need_gpu()
    rig = Rig(11, "d8192", 200)
    rng = np.random.default_rng(200)
    sets = [[rig.message(rng, 2) for _ in range(16)] for _ in range(2)]
    rig.bits()
    yield rig, sets
    rig.close()


def _selectors(rig, count, idx):
    """(host, device) selectors of index idx: bit j is the RGSW ciphertext of (idx >> j) & 1"""
    bits = rig.bits()
    k = levels_of(count)
    return [bits[(idx >> j) & 1][0] for j in range(k)], [bits[(idx >> j) & 1][1] for j in range(k)]


def _select_model(rig, sets_i, cts, count, idx):
    key = ("select", sets_i, count, idx)
    if key not in rig.models:
        rig.models[key] = select(rig.o, 2, cts, _selectors(rig, count, idx)[0], rig.klvl)[0]
    return rig.models[key]


@pytest.mark.parametrize("count,indices", [(1, (0,)), (2, (0, 1)), (3, (2,)), (5, (0, 1, 2, 3, 4)), (8, (5,)), (16, (0, 6, 15))])
def test_select_every_plan_shape(select_rig, count, indices):
    """N = 2^11, level 2, batch 2 = (set 0, set 1): the copy, one level, unpaired nodes at the first level (3, 5), full levels; the
    result decrypts to input idx; the inputs that are only read are unchanged"""
    from lattisense_amd.device import BfvSelectPlan
    rig, sets = select_rig
    plan = BfvSelectPlan(rig.ctx, 2, count)
    assert (plan.levels, plan.products) == (levels_of(count), count - 1)
    host = np.stack([np.stack([sets[s][i][1] for s in range(2)]) for i in range(count)])       # [count][batch][2][L][N]
    for idx in indices:
        _, sel = _selectors(rig, count, idx)
        got, after = _run_select(rig.ctx, plan, host, 2, sel)
        for s in range(2):
            want = _select_model(rig, s, host[:, s], count, idx)
            assert np.array_equal(got[s], want), (count, idx, s)
            assert np.array_equal(decrypt_coeffs(rig.c, got[s]), sets[s][idx][0]), (count, idx, s)
        lo = first_unchanged(count)
        assert np.array_equal(after[lo:], host[lo:]), "an input that is only read was written"
    plan.close()


def test_select_layouts_in_place_gaps_and_variants(select_rig):
    """count 5 and 16: `out` is input 0 and `out` elsewhere; a non-dense s_index with sentinel words in every gap and behind the last
    input; the read-only inputs unchanged; then every variant on the dense layout"""
    from lattisense_amd.device import BfvSelectPlan
    rig, sets = select_rig
    ctx, N, lvl, batch = rig.ctx, rig.N, 2, 2
    words = 2 * (lvl + 1) * N
    SENT = np.uint64(0x5EA75EA75EA75EA7)
    for count, idx in ((5, 3), (16, 6)):
        plan = BfvSelectPlan(ctx, lvl, count)
        dense = np.stack([np.stack([sets[s][i][1] for s in range(2)]) for i in range(count)])
        _, sel = _selectors(rig, count, idx)
        want = np.stack([_select_model(rig, s, dense[:, s], count, idx) for s in range(2)])
        for s_index in (batch * words, batch * words + 6):
            host = np.full(count * s_index + 4, SENT, dtype=np.uint64)              # a trailing guard behind the last input
            for i in range(count):
                host[i * s_index: i * s_index + batch * words] = dense[i].reshape(-1)
            for in_place in (True, False):
                res, after = _run_select(ctx, plan, host, batch, sel, in_place=in_place, s_index=s_index)
                assert np.array_equal(res, want), (count, s_index, in_place)
                for i in range(count):
                    assert np.all(after[i * s_index + batch * words: (i + 1) * s_index] == SENT), (count, s_index, in_place, i)
                assert np.all(after[count * s_index:] == SENT), (count, s_index, in_place)
                lo = first_unchanged(count) * s_index
                assert np.array_equal(after[lo:], host[lo:]), (count, s_index, in_place)
        _variants(ctx, lambda: _run_select(ctx, plan, dense, batch, sel)[0], want)
        plan.close()


def test_a_level_is_one_difference_and_one_batched_product(select_rig):
    """dense layout, batch 1: count 16 launches 4/3 of what the three levels of count 8 launch -- a level's launches do not grow with
    its nodes -- and the two-step form launches exactly one more kernel per level than the pair MAC"""
    from lattisense_amd._native import lib
    from lattisense_amd.device import BfvSelectPlan
    rig, sets = select_rig
    ctx, L = rig.ctx, lib()
    host = np.stack([sets[0][i][1] for i in range(16)])[:, None]
    xin = ctx.upload(host)

    def launches(count, pair):
        plan = BfvSelectPlan(ctx, 2, count)
        sel = _selectors(rig, count, count - 1)[1]
        ctx.set_rgsw_pair_mac(pair)
        try:
            plan.run(xin, 1, sel)                                            # tables uploaded outside the count
            ctx.sync()
            assert L.lsa_profile_begin(ctx.h, 1) == 0
            try:
                plan.run(xin, 1, sel)
                ctx.sync()
            finally:
                assert L.lsa_profile_end(ctx.h) == 0
        finally:
            ctx.set_rgsw_pair_mac(1)
        total = 0
        for kind in range(5):
            n = ctypes.c_longlong()
            assert L.lsa_profile_read(ctx.h, kind, None, None, None, ctypes.byref(n)) == 0
            total += n.value
        plan.close()
        return total
    per_level = {}
    for pair in (1, 0):
        n16, n9, n8 = launches(16, pair), launches(9, pair), launches(8, pair)
        assert n16 == n9 and n16 > 0, (pair, n16, n9)
        assert n16 * 3 == n8 * 4, (pair, n16, n8)
        per_level[pair] = n16 // 4
    assert per_level[0] == per_level[1] + 1


def test_refusals_leave_the_context_usable():
    need_gpu()
    from lattisense_amd import params
    from lattisense_amd._native import LsaError, check, lib
    from lattisense_amd.device import ALGO_BFV, ALGO_CKKS, BfvSelectPlan, DeviceContext
    rig = Rig(11, "d8192", 600)
    ctx, N, lvl, count = rig.ctx, rig.N, 2, 5
    rng = np.random.default_rng(600)
    cts = np.stack([rig.message(rng, lvl)[1] for _ in range(count)])
    host = np.stack([cts, cts], axis=1)
    words = 2 * (lvl + 1) * N
    plan = BfvSelectPlan(ctx, lvl, count)
    (_, r0), (_, r1) = rig.bits()
    sel = [r1, r0, r0]
    ref = _run_select(ctx, plan, host, 2, sel)[0]
    L = lib()

    def fails(fn, needle, who):
        with pytest.raises(LsaError) as e:
            fn()
        assert e.value.code == 1 and _message(e.value).startswith(who) and needle in _message(e.value), e.value

    xin = ctx.upload(host)
    sentinel = ctx.upload(np.full(2 * words + 4, 7, dtype=np.uint64))

    def untouched():
        assert np.all(ctx.download(sentinel, (sentinel.nwords,)) == 7)    # refused before anything was queued
        assert np.array_equal(ctx.download(xin, host.shape), host)
        assert np.array_equal(_run_select(ctx, plan, host, 2, sel)[0], ref)   # a good call on the same context
    X, S = xin.ptr, sentinel.ptr
    low = tuple(ctx.upload_key(k, lvl - 1) for k in rgsw_encrypt(rig.c, constant(N, 1), lvl - 1))   # exported below the level
    K0, K1 = r1
    # ---- external product
    ep = lambda c, lv, ct, sct, k0, k1, base, sb, o, so, b: check(L.lsa_bfv_external_product(c, lv, ct, sct, k0, k1, base, sb, o, so, b, ctx.stream))
    who = "lsa_bfv_external_product"
    for fn, needle in ((lambda: ep(ctx.h, lvl + 1, X, words, K0, K1, None, 0, S, words, 1), "level"),
                       (lambda: ep(ctx.h, -1, X, words, K0, K1, None, 0, S, words, 1), "level"),
                       (lambda: ep(ctx.h, lvl, None, words, K0, K1, None, 0, S, words, 1), "ct is null"),
                       (lambda: ep(ctx.h, lvl, X, words, K0, K1, None, 0, None, words, 1), "null"),
                       (lambda: ep(ctx.h, lvl, X, words, None, K1, None, 0, S, words, 1), "r0 is null"),
                       (lambda: ep(ctx.h, lvl, X, words, K0, None, None, 0, S, words, 1), "r1 is null"),
                       (lambda: ep(ctx.h, lvl, X + 8, words, K0, K1, None, 0, S, words, 1), "16-byte"),
                       (lambda: ep(ctx.h, lvl, X, words, K0, K1, X + 8, words, S, words, 1), "16-byte"),
                       (lambda: ep(ctx.h, lvl, X, words, K0, K1, None, 0, S + 8, words, 1), "16-byte"),
                       (lambda: ep(ctx.h, lvl, X, words + 1, K0, K1, None, 0, S, words, 2), "even"),
                       (lambda: ep(ctx.h, lvl, X, words - 2, K0, K1, None, 0, S, words, 2), "stride"),
                       (lambda: ep(ctx.h, lvl, X, words, K0, K1, None, 0, S, words - 2, 2), "stride"),
                       (lambda: ep(ctx.h, lvl, X, words, K0, K1, None, 0, X + 8 * (words // 2), words, 2), "ct"),      # partial overlap
                       (lambda: ep(ctx.h, lvl, X, words, K0, K1, X + 8 * 2 * words, words, X + 8 * 2 * words + 16, words, 1), "base"),
                       (lambda: ep(ctx.h, lvl, X, words + 2, K0, K1, None, 0, X, words, 2), "ct"),                      # same pointer, another stride
                       (lambda: ep(ctx.h, lvl, X, words, low[0], K1, None, 0, S, words, 1), "r0 was exported at a lower level"),
                       (lambda: ep(ctx.h, lvl, X, words, K0, low[1], None, 0, S, words, 1), "r1 was exported at a lower level")):
        fails(fn, needle, who)
        untouched()
    ep(ctx.h, lvl, X, words, K0, K1, None, 0, S, words, 0)                # batch <= 0: a no-op
    untouched()
    # ---- CMux
    cm = lambda c, lv, a, sa, b, sb, k0, k1, o, so, n: check(L.lsa_bfv_cmux(c, lv, a, sa, b, sb, k0, k1, o, so, n, ctx.stream))
    who = "lsa_bfv_cmux"
    Y = X + 8 * 2 * words
    for fn, needle in ((lambda: cm(ctx.h, lvl + 1, X, words, Y, words, K0, K1, S, words, 1), "level"),
                       (lambda: cm(ctx.h, lvl, None, words, Y, words, K0, K1, S, words, 1), "c0 is null"),
                       (lambda: cm(ctx.h, lvl, X, words, None, words, K0, K1, S, words, 1), "c1 is null"),
                       (lambda: cm(ctx.h, lvl, X, words, Y, words, K0, K1, None, words, 1), "null"),
                       (lambda: cm(ctx.h, lvl, X, words, Y, words, None, K1, S, words, 1), "r0 is null"),
                       (lambda: cm(ctx.h, lvl, X, words, Y + 8, words, K0, K1, S, words, 1), "16-byte"),
                       (lambda: cm(ctx.h, lvl, X, words + 1, Y, words, K0, K1, S, words, 2), "even"),
                       (lambda: cm(ctx.h, lvl, X, words, Y, words - 2, K0, K1, S, words, 2), "stride"),
                       (lambda: cm(ctx.h, lvl, X, words, Y, words, K0, K1, X + 16, words, 1), "c0"),
                       (lambda: cm(ctx.h, lvl, X, words, Y, words, K0, K1, Y + 16, words, 1), "c1"),
                       (lambda: cm(ctx.h, lvl, X, words, Y, words, K0, low[1], S, words, 1), "lower level")):
        fails(fn, needle, who)
        untouched()
    cm(ctx.h, lvl, X, words, Y, words, K0, K1, S, words, 0)
    untouched()
    # ---- select
    r0s = (ctypes.c_void_p * 3)(*[s[0].value for s in sel])
    r1s = (ctypes.c_void_p * 3)(*[s[1].value for s in sel])
    call = lambda c, i, si, sx, o, so, b, n=3, a0=r0s, a1=r1s: check(L.lsa_bfv_select(c, plan._handle(), i, si, sx, o, so, b, n, a0, a1, ctx.stream))
    who = "lsa_bfv_select"
    lows = (ctypes.c_void_p * 3)(r0s[0], low[0].value, r0s[2])
    nulls = (ctypes.c_void_p * 3)(r0s[0], None, r0s[2])
    for fn, needle in ((lambda: call(ctx.h, None, words, 2 * words, S, words, 2), "null"),
                       (lambda: call(ctx.h, X, words, 2 * words, None, words, 2), "null"),
                       (lambda: call(ctx.h, X + 8, words, 2 * words, S, words, 1), "16-byte"),
                       (lambda: call(ctx.h, X, words, 2 * words, S + 8, words, 1), "16-byte"),
                       (lambda: call(ctx.h, X, words + 1, 2 * words + 2, S, words, 2), "even"),
                       (lambda: call(ctx.h, X, words - 2, 2 * words, S, words, 2), "stride"),
                       (lambda: call(ctx.h, X, words, 2 * words, S, words - 2, 2), "stride"),
                       (lambda: call(ctx.h, X, words, 2 * words + 1, S, words, 2), "s_index"),
                       (lambda: call(ctx.h, X, words, 2 * words - 2, S, words, 2), "s_index"),
                       (lambda: call(ctx.h, X, words, 2 * words, X + 8 * (words // 2), words, 2), "overlap"),      # out across inputs 0
                       (lambda: call(ctx.h, X, words, 2 * words, X + 8 * 2 * words, words, 2), "overlap"),         # out is input 1
                       (lambda: call(ctx.h, X, words, 2 * words + 4, X, words + 2, 2), "overlap"),                 # same pointer, another stride
                       (lambda: call(ctx.h, X, words, 2 * words, S, words, 2, n=2), "n_sel"),
                       (lambda: call(ctx.h, X, words, 2 * words, S, words, 2, a0=None), "null"),
                       (lambda: call(ctx.h, X, words, 2 * words, S, words, 2, a0=nulls), "r0 is null"),
                       (lambda: call(ctx.h, X, words, 2 * words, S, words, 2, a0=lows), "lower level")):
        fails(fn, needle, who)
        untouched()
    plan.run(xin, 0, sel, out=sentinel)                                   # batch <= 0: a no-op
    untouched()
    fails(lambda: BfvSelectPlan(ctx, lvl + 1, 4).run(xin, 1, sel), "level", "lsa_bfv_select")
    fails(lambda: BfvSelectPlan(ctx, -1, 4).run(xin, 1, sel), "level", "lsa_bfv_select")
    fails(lambda: BfvSelectPlan(ctx, lvl, 0), "count", "lsa_bfv_select")
    untouched()
    P = params.CKKS_DEFAULT[65536]
    ckks = DeviceContext(ALGO_CKKS, N, P["q"][:4], P["p"][:2])
    fails(lambda: BfvSelectPlan(ckks, lvl, 4).run(xin, 1, sel), "not BFV", "lsa_bfv_select")
    fails(lambda: ep(ckks.h, lvl, X, words, K0, K1, None, 0, S, words, 1), "not BFV", "lsa_bfv_external_product")
    fails(lambda: cm(ckks.h, lvl, X, words, Y, words, K0, K1, S, words, 1), "not BFV", "lsa_bfv_cmux")
    ckks.close()
    untouched()
    nop = DeviceContext(ALGO_BFV, N, rig.q, [], rig.t)                    # a chain without a special prime
    fails(lambda: BfvSelectPlan(nop, lvl, 4).run(xin, 1, sel), "special prime", "lsa_bfv_select")
    fails(lambda: ep(nop.h, lvl, X, words, K0, K1, None, 0, S, words, 1), "special prime", "lsa_bfv_external_product")
    fails(lambda: cm(nop.h, lvl, X, words, Y, words, K0, K1, S, words, 1), "special prime", "lsa_bfv_cmux")
    one = BfvSelectPlan(nop, lvl, 1)                                      # ... still copies
    nin = nop.upload(cts[0][None])
    assert np.array_equal(nop.download(one.run(nin, 1, []), (1, 2, lvl + 1, N))[0], cts[0])
    one.close()
    nop.close()
    untouched()
    with pytest.raises(LsaError):                                         # N < 512: no context of that size exists to refuse on
        DeviceContext(ALGO_BFV, 256, params.ntt_primes_below(50, 256, 2), params.ntt_primes_below(51, 256, 1), 65537)
    untouched()
    other = Rig(11, "d8192", 601)
    fails(lambda: call(other.ctx.h, X, words, 2 * words, S, words, 1), "another context", who)
    other.close()
    untouched()
    copy = BfvSelectPlan(ctx, lvl, 1)                                     # count 1: a copy, no selector
    assert np.array_equal(ctx.download(copy.run(xin, 2, []), (2, 2, lvl + 1, N)), host[0])
    copy.close()
    plan.close()
    rig.close()
