"""Parity under NTT batch chunking (lsa_set_ntt_chunk_mib, include/lattisense_amd.h): with a positive setting launch_ntt runs both
passes of a two-pass transform over chunks of the batch, every chunk's workgroups count their batch index from 0 again, and the
fused operands of the load / store fix-ups have to follow the chunk (lattisense_amd/csrc/ntt_chunk.h).  A misdirected operand
stays inside the buffers, so nothing faults: only a word-for-word comparison sees it.

Every expected value is oracle.pyoracle.Oracle's on the same words (the rigs, cases and padded layouts of
tests/test_gpu_entry_layout.py, the plaintext-product oracles of tests/test_gpu_bfv_ptmul.py / _rotmac.py); every comparison
is exact; every test puts chunk 0, tile batch 0, dual stream 0, fused tails 1 and the ModUp lift 1 back.

Shapes: the smallest at which 1 MiB (the smallest setting) still cuts a tile, differently for the launches of one operator.
  ckks13  N = 8192 (a row is 64 KiB: floor(16 / active rows) items per chunk), six primes of CKKS_DEFAULT[65536] + two special
          primes, level 3, keys at level 5, batch 5: rescale (6 rows) and the ModDown tail (8 rows) run chunks 2, 2, 1, the
          extension transform one item per chunk.  LSA_NTT_WIDE=0: the plan is two-pass whatever the launch size
  ckks16  N = 2^16 (8 + 8 stages, a single row is half a chunk): three primes + one special prime, level 2, batch 3, relin and
          rescale
  bfv13   N = 8192 on the four-prime chain of tests/test_gpu_bfv.py, level 3, batch 3
The plain transforms also run at N = 2^15 and 2^17 (7 + 8 stages; the nine-stage second pass)."""
import contextlib
import ctypes

import numpy as np
import pytest

from tests.gpu_util import env, need_gpu, rand_ct
from tests.test_gpu_entry_layout import Rig, _padded, _padded_call, _rotate_many

pytestmark = pytest.mark.gpu

ARG = 1                                                    # LSA_ERR_ARG
PROF_NTT = 0
SKIP = 0xFF


def _lib():
    from lattisense_amd._native import lib
    return lib()


def chunk_sizes(n, active_rows, batch, mib):
    """the rule of ntt_chunk_items (ntt_chunk.h), restated: the items of every chunk of a two-pass launch"""
    c = batch if mib <= 0 else max(1, min(batch, (mib << 20) // (8 * n * max(active_rows, 1))))
    return [min(c, batch - b0) for b0 in range(0, batch, c)]


@contextlib.contextmanager
def settings(ctx, mib=1, tile=0, dual=0, fuse=1, lift=1):
    L, h = _lib(), ctx.h
    try:
        ctx.set_ntt_chunk_mib(mib)
        assert L.lsa_set_tile_batch(h, tile) == 0 and L.lsa_set_dual_stream(h, dual) == 0
        assert L.lsa_set_fuse_tails(h, fuse) == 0 and L.lsa_set_modup_lift(h, lift) == 0
        yield
    finally:
        ctx.set_ntt_chunk_mib(0)
        assert L.lsa_set_tile_batch(h, 0) == 0 and L.lsa_set_dual_stream(h, 0) == 0
        assert L.lsa_set_fuse_tails(h, 1) == 0 and L.lsa_set_modup_lift(h, 1) == 0


def ntt_launches(ctx, fn):
    """(launches, algorithmic bytes) of the NTT kind while fn() runs, every launch sampled"""
    L = _lib()
    assert L.lsa_profile_begin(ctx.h, 1) == 0
    try:
        fn()
        ctx.sync()
    finally:
        assert L.lsa_profile_end(ctx.h) == 0
    by, n = ctypes.c_double(), ctypes.c_longlong()
    assert L.lsa_profile_read(ctx.h, PROF_NTT, None, ctypes.byref(by), None, ctypes.byref(n)) == 0
    return n.value, by.value


_RIGS = {}


def _rig(name, monkeypatch):
    need_gpu()
    if name not in _RIGS:
        from lattisense_amd import params
        from lattisense_amd.device import ALGO_BFV, ALGO_CKKS
        monkeypatch.setenv("LSA_NTT_WIDE", "0")           # read when the context is made: two-pass plans at every launch size
        if name == "ckks13":
            P, n = params.CKKS_DEFAULT[65536], 8192
            _RIGS[name] = Rig(ALGO_CKKS, n, P["q"][:6], P["p"][:2], 0, 3, 5, 5, (5, 2 * n - 1), 21)
        elif name == "ckks16":
            P, n = params.CKKS_DEFAULT[65536], 65536
            _RIGS[name] = Rig(ALGO_CKKS, n, P["q"][:3], P["p"][:1], 0, 2, 2, 3, (5,), 22)
        else:
            P, n = params.BFV_DEFAULT[16384], 8192
            _RIGS[name] = Rig(ALGO_BFV, n, P["q"][:4], P["p"], P["t"], 3, 3, 3, (5, 2 * n - 1), 23)
    return _RIGS[name]


# ------------------------------------------------------------------------------------------------ 1. plain transforms
def _plain_mods(n):
    from lattisense_amd import params
    return params.ntt_primes_below(60, n, 1) + params.ntt_primes_below(45, n, 2), params.ntt_primes_below(61, n, 1)


def _plain(logn, wide, maps, monkeypatch):
    """forward == oracle row by row (skipped rows untouched), inverse == the input, the launch count == passes x chunks"""
    need_gpu()
    monkeypatch.setenv("LSA_NTT_WIDE", wide)
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    n, batch = 1 << logn, 5
    q, p = _plain_mods(n)
    mods = q + p
    ctx, o = DeviceContext(ALGO_CKKS, n, q, p), Oracle(n, q, p, 0)
    rng = np.random.default_rng(130 + logn)
    passes = 1 if (logn <= 12 or wide == "1") else 2
    try:
        for rows, mod_of in maps:
            row_mod = [mod_of[r % len(mod_of)] for r in range(rows)]
            active = sum(m != SKIP for m in row_mod)
            data = np.empty((batch, rows, n), dtype=np.uint64)
            for r, m in enumerate(row_mod):
                data[:, r] = rng.integers(0, mods[m if m != SKIP else 0], size=(batch, n), dtype=np.uint64)
            want = np.stack([np.stack([data[b, r] if m == SKIP else o.ntt(m, data[b, r]) for r, m in enumerate(row_mod)])
                             for b in range(batch)])
            sizes = chunk_sizes(n, active, batch, 1) if passes == 2 else [batch]
            buf = ctx.upload(data)
            with settings(ctx, mib=1):
                got_n, _ = ntt_launches(ctx, lambda: ctx.ntt(buf, batch, rows, mod_of))
                got = ctx.download(buf, data.shape)
                assert np.array_equal(got, want), (logn, rows, mod_of, np.argwhere((got != want).any(axis=-1)))
                assert got_n == passes * len(sizes), (logn, rows, mod_of, got_n, sizes)
                ctx.ntt(buf, batch, rows, mod_of, inverse=True)
                assert np.array_equal(ctx.download(buf, data.shape), data), (logn, rows, mod_of, "inverse")
            buf.free()
    finally:
        ctx.close()


FULL, HOLES = [0, 1, 2, 3], [0, SKIP, 2, SKIP]


@pytest.mark.parametrize("logn", [13, 15, 16, 17])
def test_plain_transforms_chunked(logn, monkeypatch):
    """batch 5 under 1 MiB chunks: at 2^13 eight rows give chunks 2, 2, 1, two active rows of four one chunk, twenty rows one item
    per chunk (more rows than a chunk holds); at 2^15 two active rows give 2, 2, 1; from 2^16 on every item is a chunk"""
    maps = [(8 if logn <= 15 else 4, FULL), (4, HOLES)] + ([(20, FULL)] if logn == 13 else [])
    n = 1 << logn
    if logn == 13:
        assert [chunk_sizes(n, a, 5, 1) for a in (8, 2, 20)] == [[2, 2, 1], [5], [1] * 5]
    else:
        assert chunk_sizes(n, 2, 5, 1) == ([2, 2, 1] if logn == 15 else [1] * 5)
    _plain(logn, "0", maps, monkeypatch)


def test_plain_transform_whole_limb_plan_ignores_the_chunk(monkeypatch):
    """LSA_NTT_WIDE=1 at N = 2^13: one pass with the limb in LDS, so the setting is a no-op (one launch, the same words)"""
    _plain(13, "1", [(8, FULL), (4, HOLES), (20, FULL)], monkeypatch)


# ------------------------------------------------------------------------------------------------ 2. CKKS entry points
def _ckks_case(r, case):
    """the cases of tests/test_gpu_entry_layout.py, plus the rotation by 2N - 1 and the hoisted rotations with one output in
    place"""
    if case == "lsa_ckks_rotate_many":
        _rotate_many(r, True)
    elif case == "lsa_ckks_rotate:conj":
        g = r.galois[1]
        _padded_call(r, case, [r.A], dict(g=g, key=r.key[g]), 2 * r.L * r.n, lambda x: r.o.ckks_rotate(r.lvl, x, g, r.raw[g], r.klvl))
    else:
        _padded(r, case)


CKKS_CASES = ["lsa_ckks_relin", "lsa_ckks_rescale", "lsa_ckks_rescale:3", "lsa_ckks_rotate", "lsa_ckks_rotate:conj",
              "lsa_ckks_rotate_many", "lsa_ckks_mult_relin_rescale"]


def test_shapes_cut_the_launches(monkeypatch):
    """the premise of every case below, from the rule alone: at N = 8192 and batch 5 a 1 MiB chunk cuts the rescale transform (6
    rows) and the ModDown tail (8 rows) into 2, 2, 1 and the extension transform into single items; a tile of two is cut again
    only where more than 8 rows are active; at N = 2^16 and on the BFV ring every launch with two rows or more is cut"""
    r = _rig("ckks13", monkeypatch)
    assert (r.n, r.batch, r.lvl, len(r.p)) == (8192, 5, 3, 2)
    assert chunk_sizes(r.n, 2 * r.lvl, r.batch, 1) == [2, 2, 1] and chunk_sizes(r.n, 2 * (r.lvl + 1), r.batch, 1) == [2, 2, 1]
    assert chunk_sizes(r.n, 9, r.batch, 1) == [1] * 5 and chunk_sizes(r.n, 9, 2, 1) == [1, 1] and chunk_sizes(r.n, 8, 2, 1) == [2]
    assert chunk_sizes(65536, 2, 3, 1) == [1, 1, 1] and chunk_sizes(8192, 9, 3, 1) == [1, 1, 1]


@pytest.mark.parametrize("dual", [0, 1])
@pytest.mark.parametrize("tile", [0, 2])
@pytest.mark.parametrize("case", CKKS_CASES)
def test_ckks_entry_points_chunked(case, tile, dual, monkeypatch):
    r = _rig("ckks13", monkeypatch)
    with settings(r.ctx, mib=1, tile=tile, dual=dual):
        _ckks_case(r, case)


@pytest.mark.parametrize("switch", ["LSA_HMULT_FOLD=0", "LSA_KS_FUSED=0", "fuse_tails=0", "modup_lift=0"])
@pytest.mark.parametrize("case", ["lsa_ckks_relin", "lsa_ckks_mult_relin_rescale"])
def test_ckks_key_switch_forms_chunked(case, switch, monkeypatch):
    """each switch moves a fusion to another transform or takes it away: the tensor product out of the inverse transform's load,
    the key MAC out of the extension transform's second pass, the tails into kernels of their own, the single-limb digits back to
    the conversion kernel"""
    r = _rig("ckks13", monkeypatch)
    name, value = switch.split("=")
    kw = {name: int(value)} if name in ("fuse_tails", "modup_lift") else {}
    ev = {} if kw else {name: value}
    with settings(r.ctx, mib=1, tile=0, dual=1, fuse=kw.get("fuse_tails", 1), lift=kw.get("modup_lift", 1)), env(**ev):
        _ckks_case(r, case)


@pytest.mark.parametrize("case", ["lsa_ckks_relin", "lsa_ckks_rescale"])
def test_ckks_n65536_chunked(case, monkeypatch):
    """8 + 8 stages (the radix-16-squared passes), one special prime: every digit has one source limb (the lift prologue)"""
    r = _rig("ckks16", monkeypatch)
    for tile, dual in ((0, 0), (2, 1)):
        with settings(r.ctx, mib=1, tile=tile, dual=dual):
            _padded(r, case)


# ------------------------------------------------------------------------------------------------ 3. BFV
@pytest.mark.parametrize("case", ["lsa_bfv_mult", "lsa_bfv_relin", "lsa_bfv_rotate", "lsa_bfv_rescale", "lsa_bfv_mult_relin"])
def test_bfv_entry_points_chunked(case, monkeypatch):
    r = _rig("bfv13", monkeypatch)
    for tile, dual in ((0, 0), (2, 1)):
        with settings(r.ctx, mib=1, tile=tile, dual=dual):
            _padded(r, case)


def _bfv_plain_operands(r):
    """two pt_mul plaintexts, a second ciphertext and a partial sum, made once per rig"""
    if not hasattr(r, "pts"):
        rng = np.random.default_rng(77)
        ql = r.q[: r.L]
        r.pts = [rand_ct(rng, ql, 1, r.n, r.batch)[:, 0] for _ in range(2)]
        r.partial = rand_ct(rng, ql, 2, r.n, r.batch)
    return r.pts, r.partial


@pytest.mark.parametrize("fused", ["1", "0"])
def test_bfv_plain_products_chunked(fused, monkeypatch):
    """ct x pt_mul and a two-term MAC onto a partial sum: the pt_mul epilogue of the inverse transform, and its unfused form"""
    from tests.test_gpu_bfv_ptmul import _want_mac
    r = _rig("bfv13", monkeypatch)
    pts, partial = _bfv_plain_operands(r)
    ctx, lvl, L, shape = r.ctx, r.lvl, r.L, (r.batch, 2, r.L, r.n)
    want1 = r.want("ptmul", lambda i: _want_mac(r.o, L, [r.A[i]], [pts[0][i]]))
    want2 = r.want("ptmac", lambda i: _want_mac(r.o, L, [r.A[i], r.B[i]], [pts[0][i], pts[1][i]], partial[i]))
    da, db, dp, dpa = ctx.upload(r.A), ctx.upload(r.B), [ctx.upload(p) for p in pts], ctx.upload(partial)
    for tile in (0, 2):
        with settings(ctx, mib=1, tile=tile), env(LSA_PTMUL_FUSED=fused):
            got = ctx.download(ctx.bfv_mult_plain_mul(lvl, da, dp[0], r.batch), shape)
            assert np.array_equal(got, want1), ("mult_plain_mul", tile, np.argwhere((got != want1).any(axis=-1)))
            got = ctx.download(ctx.bfv_mac_plain_mul(lvl, [da, db], dp, r.batch, partial=dpa), shape)
            assert np.array_equal(got, want2), ("mac_plain_mul", tile, np.argwhere((got != want2).any(axis=-1)))


@pytest.mark.parametrize("fused", ["1", "0"])
def test_bfv_hoisted_rotations_chunked(fused, monkeypatch):
    """lsa_bfv_rotate_many and the two-term rotate-and-MAC onto a partial sum (the fz_epi = 4 store), and its unfused form"""
    from tests.test_gpu_bfv_rotmac import _Ring
    r = _rig("bfv13", monkeypatch)
    pts, partial = _bfv_plain_operands(r)
    ctx, lvl, shape = r.ctx, r.lvl, (r.batch, 2, r.L, r.n)
    els = list(r.galois)
    want_rot = {g: r.want(("rot", g), lambda i, g=g: r.o.bfv_rotate(lvl, r.A[i], g, r.raw[g], r.klvl)) for g in els}
    want_mac = r.want("rotmac", lambda i: _Ring.want(r, lvl, r.A[i], els, [p[i] for p in pts], partial[i]))
    da, dp, dpa = ctx.upload(r.A), [ctx.upload(p) for p in pts], ctx.upload(partial)
    for tile in (0, 2):
        with settings(ctx, mib=1, tile=tile), env(LSA_ROTMAC_FUSED=fused):
            outs = ctx.bfv_rotate_many(lvl, da, {g: r.key[g] for g in els}, r.batch)
            for g in els:
                got = ctx.download(outs[g], shape)
                assert np.array_equal(got, want_rot[g]), ("rotate_many", g, tile, np.argwhere((got != want_rot[g]).any(axis=-1)))
            terms = [(g, r.key[g], d) for g, d in zip(els, dp)]
            got = ctx.download(ctx.bfv_rotate_mac_plain_mul(lvl, da, terms, r.batch, partial=dpa), shape)
            assert np.array_equal(got, want_mac), ("rotate_mac", tile, np.argwhere((got != want_mac).any(axis=-1)))


# ------------------------------------------------------------------------------------------------ 5. the chunking happened
@pytest.mark.parametrize("case", ["lsa_ckks_relin", "lsa_ckks_rescale", "lsa_ckks_mult_relin_rescale"])
def test_chunking_happened_and_costs_the_same_bytes(case, monkeypatch):
    """more NTT launches under 1 MiB chunks, the same algorithmic bytes (the byte model does not depend on how the batch is cut)"""
    r = _rig("ckks13", monkeypatch)
    sizes = chunk_sizes(r.n, 2 * r.lvl, r.batch, 1)        # the rescale transform's launch: 2 polys x lvl limbs
    assert len(sizes) >= 2 and sizes[-1] != sizes[0], sizes   # (a later change of shapes must not make this test vacuous)
    with settings(r.ctx, mib=0):
        n0, b0 = ntt_launches(r.ctx, lambda: _padded(r, case))
    with settings(r.ctx, mib=1):
        n1, b1 = ntt_launches(r.ctx, lambda: _padded(r, case))
    assert n1 > n0 > 0 and b1 == b0 > 0, (case, n0, n1, b0, b1)


def test_single_pass_ring_is_not_chunked():
    """N = 2048: one pass per transform, the setting changes nothing (the header promises N > 2^12)"""
    from tests.test_gpu_entry_layout import _rig as small_rig
    r = small_rig("ckks")
    assert r.n == 2048
    for case in ("lsa_ckks_relin", "lsa_ckks_rescale", "lsa_ckks_mult_relin_rescale"):
        with settings(r.ctx, mib=0):
            n0, b0 = ntt_launches(r.ctx, lambda: _padded(r, case))
        with settings(r.ctx, mib=1):
            n1, b1 = ntt_launches(r.ctx, lambda: _padded(r, case))
        assert n1 == n0 > 0 and b1 == b0, (case, n0, n1)


# ------------------------------------------------------------------------------------------------ 6. the setter's contract
def test_setter_contract(monkeypatch):
    r = _rig("ckks13", monkeypatch)
    L, h = _lib(), r.ctx.h
    count = lambda: ntt_launches(r.ctx, lambda: _padded(r, "lsa_ckks_rescale"))[0]
    with settings(r.ctx, mib=0):
        whole = count()
        assert L.lsa_set_ntt_chunk_mib(h, 1) == 0
        cut = count()
        assert cut > whole
        assert L.lsa_set_ntt_chunk_mib(h, -1) == ARG
        assert count() == cut                              # a refused value leaves the setting in force
        assert L.lsa_set_ntt_chunk_mib(h, 256) == 0
        assert count() == whole                            # five items of 6 x 64 KiB fit 256 MiB: one chunk
        assert L.lsa_set_ntt_chunk_mib(h, 1) == 0 and L.lsa_set_ntt_chunk_mib(h, 0) == 0
        assert count() == whole
        # one launch per pass: a plain two-pass transform of the whole batch
        buf = r.ctx.upload(r.A)
        plain = lambda: r.ctx.ntt(buf, r.batch, 2 * r.L, list(range(r.L)))
        assert ntt_launches(r.ctx, plain)[0] == 2
        assert L.lsa_set_ntt_chunk_mib(h, 1) == 0
        assert ntt_launches(r.ctx, plain)[0] == 2 * len(chunk_sizes(r.n, 2 * r.L, r.batch, 1)) == 6
