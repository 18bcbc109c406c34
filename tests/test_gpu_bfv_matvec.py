"""BFV plaintext matrix x ciphertext vector product on the device (lsa_bfv_matvec_plain_mul, lsa_set_bfv_matvec_block; bfv_matvec.hip)
against its CPU model (tests/bfv_matvec_model.py: every query ciphertext transformed once, Oracle.vec mul / add, Oracle.intt) and
against the device composition, `rows` calls of lsa_bfv_mac_plain_mul: identical word for word for every batch item -- every plan shape
on a one-pass ring with and without a partial and with a shared and a per-item database, the FP64 engine on and off, N = 2^14, pattern
operands on the fp / mixed / ceiling operator chains, the fold of the long sum at the 61-bit ceiling on both sides of eight columns and
across an accumulating column block, every row block crossed with column blocks and the launch count, gapped layouts with sentinels,
tiles on two streams and chunked transforms, expand -> matvec -> select on the device with no copy, refusals that leave the context
usable.

Each model is computed once per distinct input and shared by the variants."""
import ctypes

import numpy as np
import pytest

from tests.bfv_expand_model import decrypt_coeffs
from tests.bfv_matvec_model import descale, matvec_ntt, pt_mul_of, transform
from tests.boundary import BFV_OPERATOR_T, CEILING_SLOTS, MAC_TERMS, bfv_operator_chain, ceiling_chain, is_ceiling, pattern_ct
from tests.gpu_util import need_gpu, rand_ct
from tests.rgsw_model import levels_of, select
from tests.test_bfv_matvec_api import PAIRS, pir_database, pir_query
from tests.test_gpu_bfv_expand import _message
from tests.test_gpu_bfv_rgsw import Rig

pytestmark = pytest.mark.gpu

SENT = np.uint64(0x5EA75EA75EA75EA7)


def _ctx(n, q, p, t):
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    from oracle.pyoracle import Oracle
    return DeviceContext(ALGO_BFV, n, q, p, t), Oracle(n, q, p, t)


def _run(ctx, level, cts, pts, shared, partial=None):
    """cts [cols][batch][2][L][N], pts [rows][cols][L][N] (shared) or [batch][rows][cols][L][N], partial [rows][batch][2][L][N]
    -> the device's [rows][batch][2][L][N]"""
    cols, batch = cts.shape[:2]
    rows = pts.shape[0] if shared else pts.shape[1]
    out = ctx.bfv_matvec_plain_mul(level, ctx.upload(cts), ctx.upload(pts), rows, cols, batch,
                                   partial=ctx.upload(partial) if partial is not None else None, shared=shared)
    return ctx.download(out, (rows, batch, 2, level + 1, ctx.n))


def _compose(ctx, level, cts, pts, shared, partial=None):
    """the same product as `rows` calls of bfv_mac_plain_mul"""
    cols, batch = cts.shape[:2]
    rows = pts.shape[0] if shared else pts.shape[1]
    dc = [ctx.upload(cts[c]) for c in range(cols)]
    out = []
    for r in range(rows):
        dp = [ctx.upload(np.repeat(pts[r, c][None], batch, axis=0) if shared else pts[:, r, c]) for c in range(cols)]
        res = ctx.bfv_mac_plain_mul(level, dc, dp, batch, partial=ctx.upload(partial[r]) if partial is not None else None)
        out.append(ctx.download(res, (batch, 2, level + 1, ctx.n)))
        for b in dp:
            b.free()
    for b in dc:
        b.free()
    return np.stack(out)


def _add(o, a, b):
    return np.stack([np.stack([np.stack([o.vec("add", j, x[pl, j], y[pl, j]) for j in range(x.shape[1])]) for pl in range(2)])
                     for x, y in zip(a, b)])


def _check(ctx, o, level, cts, pts, shared, partial, want, what):
    """want[b]: the model's [rows][2][L][N] of batch item b without the partial"""
    got = _run(ctx, level, cts, pts, shared, partial)
    for b in range(cts.shape[1]):
        w = want[b] if partial is None else _add(o, want[b], partial[:, b])
        assert np.array_equal(got[:, b], w), "batch item %d differs from the model (%s)" % (b, what)
    assert np.array_equal(got, _compose(ctx, level, cts, pts, shared, partial)), "differs from the composition (%s)" % what
    return got


@pytest.fixture(scope="module")
def small():
    """N = 2^11, 3 Q + 1 P, level 2"""
    need_gpu()
    from lattisense_amd import params
    B = params.BFV_DEFAULT[8192]
    ctx, o = _ctx(1 << 11, B["q"], B["p"], B["t"])
    yield ctx, o, B["q"]
    ctx.close()


def _items(rng, q, L, n, cols, order):
    """distinct query vectors a, b, ... and the batch [cols][len(order)][2][L][N] that `order` makes of them"""
    distinct = [rand_ct(rng, q[:L], 2, n, cols) for _ in range(max(order) + 1)]
    return distinct, np.stack([distinct[i] for i in order], axis=1)


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 3), (3, 1), (5, 9), (8, 8), (9, 17)])
def test_plan_shapes_with_and_without_a_partial(small, rows, cols):
    """batch 3 = (a, b, a) with one database for the batch; at (5, 9) also one database per item"""
    ctx, o, q = small
    lvl, L, n = 2, 3, 1 << 11
    rng = np.random.default_rng(100 * rows + cols)
    order = [0, 1, 0]
    distinct, cts = _items(rng, q, L, n, cols, order)
    ctn = [transform(o, L, d) for d in distinct]
    pts = rand_ct(rng, q[:L], rows, n, cols).transpose(1, 0, 2, 3)          # [rows][cols][L][N]
    ptd = descale(o, L, pts)
    model = [matvec_ntt(o, L, c, ptd) for c in ctn]
    want = [model[i] for i in order]
    partial = rand_ct(rng, q[:L], 2, n, rows * 3).reshape(rows, 3, 2, L, n)
    got = _check(ctx, o, lvl, cts, pts, True, None, want, "shared database")
    assert np.array_equal(got[:, 0], got[:, 2]) and not np.array_equal(got[:, 0], got[:, 1])
    _check(ctx, o, lvl, cts, pts, True, partial, want, "shared database, partial")
    if (rows, cols) == (5, 9):
        other = rand_ct(rng, q[:L], rows, n, cols).transpose(1, 0, 2, 3)
        per_item = np.stack([pts, other, pts])
        model_other = matvec_ntt(o, L, ctn[1], descale(o, L, other))
        want = [model[0], model_other, model[0]]
        _check(ctx, o, lvl, cts, per_item, False, None, want, "database per item")
        _check(ctx, o, lvl, cts, per_item, False, partial, want, "database per item, partial")


@pytest.mark.parametrize("level", [1, 0])
def test_fp64_engine_on_and_off(level):
    """N = 2^12 on BFV_DEFAULT[4096] (39- and 40-bit limbs: the FP64 butterfly engine), (3, 5), batch 2"""
    need_gpu()
    from lattisense_amd import params
    B = params.BFV_DEFAULT[4096]
    n, L, rows, cols = 1 << 12, level + 1, 3, 5
    ctx, o = _ctx(n, B["q"], B["p"], B["t"])
    rng = np.random.default_rng(4096 + level)
    distinct, cts = _items(rng, B["q"], L, n, cols, [0, 1])
    pts = rand_ct(rng, B["q"][:L], rows, n, cols).transpose(1, 0, 2, 3)
    ptd = descale(o, L, pts)
    want = [matvec_ntt(o, L, transform(o, L, d), ptd) for d in distinct]
    partial = rand_ct(rng, B["q"][:L], 2, n, rows * 2).reshape(rows, 2, 2, L, n)
    for fp in (1, 0):
        ctx.set_fp64_ntt(fp)
        try:
            _check(ctx, o, level, cts, pts, True, None, want, "fp64 %d" % fp)
            _check(ctx, o, level, cts, pts, True, partial, want, "fp64 %d, partial" % fp)
        finally:
            ctx.set_fp64_ntt(1)
    ctx.close()


def test_ring_of_2_14():
    """N = 2^14 on BFV_DEFAULT[16384] (6 Q + 2 P), level 5, (3, 2), batch 2"""
    need_gpu()
    from lattisense_amd import params
    B = params.BFV_DEFAULT[16384]
    n, lvl, L, rows, cols = 1 << 14, 5, 6, 3, 2
    ctx, o = _ctx(n, B["q"], B["p"], B["t"])
    rng = np.random.default_rng(16384)
    distinct, cts = _items(rng, B["q"], L, n, cols, [0, 1])
    pts = rand_ct(rng, B["q"][:L], rows, n, cols).transpose(1, 0, 2, 3)
    ptd = descale(o, L, pts)
    want = [matvec_ntt(o, L, transform(o, L, d), ptd) for d in distinct]
    partial = rand_ct(rng, B["q"][:L], 2, n, rows * 2).reshape(rows, 2, 2, L, n)
    _check(ctx, o, lvl, cts, pts, True, partial, want, "N = 2^14")
    ctx.set_fp64_ntt(0)
    try:
        _check(ctx, o, lvl, cts, pts, True, None, want, "N = 2^14, integer engine")
    finally:
        ctx.set_fp64_ntt(1)
    ctx.close()


@pytest.mark.parametrize("kind", ["fp", "mixed", "ceiling"])
def test_operator_chains_with_pattern_operands(kind):
    """N = 2^13, top level, (2, 3); batch slots carry the patterns max / top / uniform in the ciphertexts and in a database per item"""
    need_gpu()
    n, rows, cols = 1 << 13, 2, 3
    q, p = bfv_operator_chain(kind, n)
    lvl, L = len(q) - 1, len(q)
    ctx, o = _ctx(n, q, p, BFV_OPERATOR_T)
    rng = np.random.default_rng(8192 + len(kind))
    names = ("max", "top", "uniform")
    cts = np.stack([pattern_ct(names, q, 2, n, rng) for _ in range(cols)])                                    # [cols][3][2][L][N]
    pts = np.stack([np.stack([pattern_ct(names, q, 1, n, rng)[:, 0] for _ in range(cols)]) for _ in range(rows)]).transpose(2, 0, 1, 3, 4)
    want = [matvec_ntt(o, L, transform(o, L, cts[:, b]), descale(o, L, pts[b])) for b in range(3)]
    partial = pattern_ct(("max",) * (rows * 3), q, 2, n, rng).reshape(rows, 3, 2, L, n)
    _check(ctx, o, lvl, cts, pts, False, None, want, kind)
    _check(ctx, o, lvl, cts, pts, False, partial, want, kind + ", partial")
    ctx.close()


@pytest.fixture(scope="module")
def ceiling():
    """ceiling_chain(4096, 4, 1), top level, rows = 3, the 33 columns the term counts take their first `cols` of.  The ciphertexts are the
    inverse transforms of the patterns, so what meets the plaintexts is the pattern itself: the worst-case residues."""
    need_gpu()
    n, rows, top = 4096, 3, max(MAC_TERMS)
    C = ceiling_chain(n, 4, 1)
    assert all(is_ceiling(m) for m in C["q"])
    ctx, o = _ctx(n, C["q"], C["p"], BFV_OPERATOR_T)
    rng = np.random.default_rng(6129)
    L = 4
    ctn = np.stack([pattern_ct(CEILING_SLOTS, C["q"], 2, n, rng) for _ in range(top)])                        # [33][3][2][4][N]
    cts = np.stack([np.stack([np.stack([np.stack([o.intt(j, ctn[c, b, pl, j]) for j in range(L)]) for pl in range(2)])
                              for b in range(len(CEILING_SLOTS))]) for c in range(top)])
    pts = np.stack([np.stack([pattern_ct(CEILING_SLOTS, C["q"], 1, n, rng)[:, 0] for _ in range(top)]) for _ in range(rows)])
    pts = pts.transpose(2, 0, 1, 3, 4)                                                                        # [3][rows][33][4][N]
    ptd = [descale(o, L, pts[b]) for b in range(len(CEILING_SLOTS))]
    partial = pattern_ct(("max",) * (rows * len(CEILING_SLOTS)), C["q"], 2, n, rng).reshape(rows, len(CEILING_SLOTS), 2, L, n)
    yield ctx, o, ctn, cts, pts, ptd, partial
    ctx.close()


@pytest.mark.parametrize("cols", MAC_TERMS)
def test_fold_at_the_ceiling(ceiling, cols):
    """on both sides of the fold after eight columns; once with the default blocks, once with column blocks of 4 and of 8, so that a
    fold and an accumulating launch meet at the block's edge"""
    ctx, o, ctn, cts, pts, ptd, partial = ceiling
    lvl, L = 3, 4
    want = [matvec_ntt(o, L, ctn[:cols, b], ptd[b][:, :cols]) for b in range(len(CEILING_SLOTS))]
    c, p = np.ascontiguousarray(cts[:cols]), np.ascontiguousarray(pts[:, :, :cols])
    got = _check(ctx, o, lvl, c, p, False, partial, want, "default blocks")
    for cb in (4, 8):
        ctx.set_bfv_matvec_block(0, cb)
        try:
            assert np.array_equal(_run(ctx, lvl, c, p, False, partial), got), "col_block %d" % cb
        finally:
            ctx.set_bfv_matvec_block(0, 0)


def _launches(ctx, fn):
    """the launches of each profile kind that fn() makes, counted as tests/test_gpu_bfv_rgsw.py counts a level's"""
    from lattisense_amd._native import lib
    L = lib()
    fn()                                                                       # tables uploaded outside the count
    ctx.sync()
    assert L.lsa_profile_begin(ctx.h, 1) == 0
    try:
        fn()
        ctx.sync()
    finally:
        assert L.lsa_profile_end(ctx.h) == 0
    out = []
    for kind in range(5):
        k = ctypes.c_longlong()
        assert L.lsa_profile_read(ctx.h, kind, None, None, None, ctypes.byref(k)) == 0
        out.append(k.value)
    return out


def test_every_row_block_and_column_block(small):
    """(9, 17): every row_block crossed with col_block 1, 4, 16, 17 gives the same words; the kernel's launches (the element-wise
    kind; no partial) are what lsa_bfv_matvec_plan says for a workspace of col_block columns"""
    from lattisense_amd.device import bfv_matvec_plan
    ctx, o, q = small
    lvl, L, n, rows, cols = 2, 3, 1 << 11, 9, 17
    rng = np.random.default_rng(917)
    distinct, cts = _items(rng, q, L, n, cols, [0, 1, 0])
    pts = rand_ct(rng, q[:L], rows, n, cols).transpose(1, 0, 2, 3)
    ptd = descale(o, L, pts)
    model = [matvec_ntt(o, L, transform(o, L, d), ptd) for d in distinct]
    partial = rand_ct(rng, q[:L], 2, n, rows * 3).reshape(rows, 3, 2, L, n)
    ref = _check(ctx, o, lvl, cts, pts, True, partial, [model[0], model[1], model[0]], "default blocks")
    dc, dp, d1 = ctx.upload(cts), ctx.upload(pts), ctx.upload(cts[:, :1])
    col_bytes = 2 * L * n * 8
    try:
        for rb in (1, 2, 4, 8):
            for cb in (1, 4, 16, 17):
                ctx.set_bfv_matvec_block(rb, cb)
                assert np.array_equal(_run(ctx, lvl, cts, pts, True, partial), ref), (rb, cb)
                plan = bfv_matvec_plan(n, L, rows, cols, 1, workspace_bytes=cb * col_bytes)
                assert plan["col_block"] == cb and plan["launches"] == -(-cols // cb)
                counts = _launches(ctx, lambda: ctx.bfv_matvec_plain_mul(lvl, d1, dp, rows, cols, 1).free())
                assert counts[4] == plan["launches"] and counts[0] > 0 and counts[1] == counts[2] == counts[3] == 0, (rb, cb, counts)
    finally:
        ctx.set_bfv_matvec_block(0, 0)
    # the default: one launch for all 17 columns, and one forward and one inverse transform on the dense layouts
    counts = _launches(ctx, lambda: ctx.bfv_matvec_plain_mul(lvl, dc, dp, rows, cols, 3).free())
    assert counts[4] == bfv_matvec_plan(n, L, rows, cols, 3)["launches"] == 1, counts


def test_gapped_layouts_keep_sentinels_and_inputs(small):
    """gaps in s_col, sct, s_row, sout, s_prow, s_pcol, spartial and s_partial_row, sentinel words in every gap: the output's gaps
    survive, the inputs are unchanged, the words are the dense call's.  (5, 9), batch 2, shared database, then one per item."""
    from lattisense_amd._native import check, lib
    ctx, o, q = small
    lvl, L, n, rows, cols, batch = 2, 3, 1 << 11, 5, 9, 2
    wct, wpt = 2 * L * n, L * n
    rng = np.random.default_rng(59)
    cts = rand_ct(rng, q[:L], 2, n, cols * batch).reshape(cols, batch, 2, L, n)
    per_item = rand_ct(rng, q[:L], batch * rows, n, cols).transpose(1, 0, 2, 3).reshape(batch, rows, cols, L, n)
    partial = rand_ct(rng, q[:L], 2, n, rows * batch).reshape(rows, batch, 2, L, n)
    for shared in (True, False):
        pts = per_item[0] if shared else per_item
        ref = _run(ctx, lvl, cts, pts, shared, partial)
        sct, sout, spa = wct + 2, wct + 4, wct + 6
        s_col, s_row, s_par = batch * sct + 4, batch * sout + 2, batch * spa + 8
        s_pcol = wpt + 2
        s_prow = cols * s_pcol + 6
        spt = 0 if shared else rows * s_prow + 8
        hc = np.full(cols * s_col, SENT, dtype=np.uint64)
        for c in range(cols):
            for b in range(batch):
                hc[c * s_col + b * sct: c * s_col + b * sct + wct] = cts[c, b].reshape(-1)
        hp = np.full((1 if shared else batch) * (rows * s_prow + 8), SENT, dtype=np.uint64)
        for b in range(1 if shared else batch):
            for r in range(rows):
                for c in range(cols):
                    at = b * spt + r * s_prow + c * s_pcol
                    hp[at: at + wpt] = (pts[r, c] if shared else pts[b, r, c]).reshape(-1)
        ha = np.full(rows * s_par, SENT, dtype=np.uint64)
        for r in range(rows):
            for b in range(batch):
                ha[r * s_par + b * spa: r * s_par + b * spa + wct] = partial[r, b].reshape(-1)
        ho = np.full(rows * s_row, SENT, dtype=np.uint64)
        dc, dp, da, do = ctx.upload(hc), ctx.upload(hp), ctx.upload(ha), ctx.upload(ho)
        check(lib().lsa_bfv_matvec_plain_mul(ctx.h, lvl, rows, cols, dc.ptr, s_col, sct, dp.ptr, s_prow, s_pcol, spt, da.ptr, s_par, spa, do.ptr,
                                             s_row, sout, batch, ctx.stream))
        after = ctx.download(do, ho.shape)
        mask = np.ones(ho.shape, dtype=bool)
        for r in range(rows):
            for b in range(batch):
                at = r * s_row + b * sout
                assert np.array_equal(after[at: at + wct].reshape(2, L, n), ref[r, b]), (shared, r, b)
                mask[at: at + wct] = False
        assert np.all(after[mask] == SENT), "a word between the outputs was written"
        assert np.array_equal(ctx.download(dc, hc.shape), hc) and np.array_equal(ctx.download(dp, hp.shape), hp)
        assert np.array_equal(ctx.download(da, ha.shape), ha)
        for buf in (dc, dp, da, do):
            buf.free()


def test_tiles_on_two_streams_and_chunked_transforms(small):
    """tile batch 1 and 2 on two streams (a tile is then not the whole batch: one transform per column and per row) and 1 MiB
    transform chunks give the same words; every setting is put back"""
    from lattisense_amd._native import check, lib
    ctx, o, q = small
    lvl, L, n, rows, cols = 2, 3, 1 << 11, 5, 9
    rng = np.random.default_rng(77)
    distinct, cts = _items(rng, q, L, n, cols, [0, 1, 0])
    pts = rand_ct(rng, q[:L], rows, n, cols).transpose(1, 0, 2, 3)
    ptd = descale(o, L, pts)
    model = [matvec_ntt(o, L, transform(o, L, d), ptd) for d in distinct]
    partial = rand_ct(rng, q[:L], 2, n, rows * 3).reshape(rows, 3, 2, L, n)
    ref = _check(ctx, o, lvl, cts, pts, True, partial, [model[0], model[1], model[0]], "default")
    check(lib().lsa_set_dual_stream(ctx.h, 1))
    try:
        for tile in (1, 2):
            ctx.set_tile_batch(tile)
            assert np.array_equal(_run(ctx, lvl, cts, pts, True, partial), ref), "tile batch %d on two streams" % tile
            ctx.set_bfv_matvec_block(2, 4)
            assert np.array_equal(_run(ctx, lvl, cts, pts, True, partial), ref), "tile batch %d, blocks 2 x 4" % tile
            ctx.set_bfv_matvec_block(0, 0)
    finally:
        ctx.set_bfv_matvec_block(0, 0)
        ctx.set_tile_batch(0)
        check(lib().lsa_set_dual_stream(ctx.h, 0))
    ctx.set_ntt_chunk_mib(1)
    try:
        assert np.array_equal(_run(ctx, lvl, cts, pts, True, partial), ref), "chunked transforms"
    finally:
        ctx.set_ntt_chunk_mib(0)
    assert np.array_equal(_run(ctx, lvl, cts, pts, True, partial), ref)


def test_expand_matvec_select_on_the_device():
    """N = 2^11, rows = 4, cols = 8, batch 3 (the queries of PAIRS): the output of bfv_expand is the matvec's `cts` and the matvec's
    output is bfv_select's input, by pointer, with no copy in between; word for word against the chained models, and decrypted to the
    database entry"""
    need_gpu()
    from lattisense_amd.device import BfvExpandPlan, BfvSelectPlan
    rig = Rig(11, "d8192", 29)
    ctx, o, c, n, t, lvl = rig.ctx, rig.o, rig.c, rig.N, rig.t, 2
    L, rows, cols, batch = lvl + 1, 4, 8, len(PAIRS)
    rng = np.random.default_rng(29)
    db = pir_database(rng, t, n, rows, cols)
    pts = np.stack([np.stack([pt_mul_of(o, L, db[r, k]) for k in range(cols)]) for r in range(rows)])
    ptd = descale(o, L, pts)
    queries = [pir_query(c, n, t, lvl, cols, col) for _, col in PAIRS]
    expand, pick = BfvExpandPlan(ctx, lvl, cols), BfvSelectPlan(ctx, lvl, rows)
    glk = rig.keys_for(expand.galois_elements)
    expanded = expand.run(ctx.upload(np.stack(queries)), batch, glk)          # [cols][batch][2][L][N]
    want_expanded = [rig.model(qy, lvl, cols) for qy in queries]
    got_expanded = ctx.download(expanded, (cols, batch, 2, L, n))
    for b in range(batch):
        assert np.array_equal(got_expanded[:, b], want_expanded[b]), b
    dp = ctx.upload(pts)
    want_scanned = [matvec_ntt(o, L, transform(o, L, want_expanded[b]), ptd) for b in range(batch)]
    bits = rig.bits()
    for b, (row, col) in enumerate(PAIRS):
        scanned = ctx.bfv_matvec_plain_mul(lvl, expanded, dp, rows, cols, batch)   # [rows][batch][2][L][N]; the select consumes it
        got_scanned = ctx.download(scanned, (rows, batch, 2, L, n))
        for i in range(batch):
            assert np.array_equal(got_scanned[:, i], want_scanned[i]), i
        sel = [bits[(row >> j) & 1] for j in range(levels_of(rows))]
        res = ctx.download(pick.run(scanned, batch, [s[1] for s in sel]), (batch, 2, L, n))
        want, _ = select(o, lvl, want_scanned[b], [s[0] for s in sel], rig.klvl)
        assert np.array_equal(res[b], want), (row, col)
        assert np.array_equal(decrypt_coeffs(c, res[b]), db[row, col]), (row, col)
        scanned.free()
    assert np.array_equal(ctx.download(expanded, (cols, batch, 2, L, n)), got_expanded)   # the query is only read
    expand.close()
    pick.close()
    rig.close()


def test_refusals_leave_the_context_usable(small):
    from lattisense_amd import params
    from lattisense_amd._native import LsaError, check, lib
    from lattisense_amd.device import ALGO_BFV, ALGO_CKKS, DeviceContext
    ctx, o, q = small
    lvl, L, n, rows, cols, batch = 2, 3, 1 << 11, 3, 2, 2
    wct, wpt = 2 * L * n, L * n
    rng = np.random.default_rng(600)
    cts = rand_ct(rng, q[:L], 2, n, cols * batch).reshape(cols, batch, 2, L, n)
    pts = rand_ct(rng, q[:L], rows, n, cols).transpose(1, 0, 2, 3)
    partial = rand_ct(rng, q[:L], 2, n, rows * batch).reshape(rows, batch, 2, L, n)
    ref = _run(ctx, lvl, cts, pts, True, partial)
    dc, dp, da = ctx.upload(cts), ctx.upload(pts), ctx.upload(partial)
    sentinel = ctx.upload(np.full(rows * batch * wct + 16, 7, dtype=np.uint64))
    who = "lsa_bfv_matvec_plain_mul"
    Lb = lib()

    def call(h=None, level=lvl, r=rows, k=cols, C=dc.ptr, s_col=batch * wct, sct=wct, P=dp.ptr, s_prow=cols * wpt, s_pcol=wpt, spt=0,
             A=da.ptr, s_par=batch * wct, spa=wct, O=sentinel.ptr, s_row=batch * wct, sout=wct, b=batch):
        check(Lb.lsa_bfv_matvec_plain_mul(ctx.h if h is None else h, level, r, k, C, s_col, sct, P, s_prow, s_pcol, spt, A, s_par, spa, O,
                                          s_row, sout, b, ctx.stream))

    def untouched():
        assert np.all(ctx.download(sentinel, (sentinel.nwords,)) == 7)        # refused before anything was queued
        assert np.array_equal(ctx.download(dc, cts.shape), cts) and np.array_equal(ctx.download(dp, pts.shape), pts)
        assert np.array_equal(_run(ctx, lvl, cts, pts, True, partial), ref)   # a good call on the same context

    for kw, needle in (({"level": lvl + 1}, "level"), ({"level": -1}, "level"), ({"r": 0}, "rows"), ({"k": 0}, "cols"), ({"k": -2}, "cols"),
                       ({"C": None}, "cts is null"), ({"P": None}, "pts is null"), ({"O": None}, "out is null"),
                       ({"C": dc.ptr + 8}, "16-byte"), ({"P": dp.ptr + 8}, "16-byte"), ({"A": da.ptr + 8}, "16-byte"),
                       ({"O": sentinel.ptr + 8}, "16-byte"),
                       ({"sct": wct + 1, "s_col": batch * (wct + 1) + 2}, "even"), ({"spt": wpt * rows * cols + 1}, "even"),
                       ({"sout": wct + 1, "s_row": batch * (wct + 1) + 2}, "even"), ({"spa": wct + 1, "s_par": batch * (wct + 1) + 2}, "even"),
                       ({"s_col": batch * wct + 1}, "s_col"), ({"s_row": batch * wct + 1}, "s_row"), ({"s_prow": cols * wpt + 1}, "s_prow"),
                       ({"s_pcol": wpt + 1}, "s_pcol"), ({"s_par": batch * wct + 1}, "s_partial_row"),
                       ({"sct": wct - 2}, "stride"), ({"sout": wct - 2}, "stride"), ({"spa": wct - 2}, "stride"), ({"spt": wpt - 2}, "stride"),
                       ({"s_col": batch * wct - 2}, "s_col"), ({"s_row": batch * wct - 2}, "s_row"), ({"s_par": batch * wct - 2}, "s_partial_row"),
                       ({"s_prow": wpt - 2}, "s_prow"), ({"s_pcol": wpt - 2}, "s_pcol"), ({"s_col": 0}, "s_col"), ({"s_row": -2}, "s_row"),
                       ({"O": dc.ptr}, "overlaps cts"), ({"O": dc.ptr + 8 * (wct // 2)}, "overlaps cts"),
                       ({"O": dc.ptr + 8 * (cols * batch - 1) * wct, "r": 1}, "overlaps cts"),
                       ({"O": dp.ptr, "r": 1, "b": 1}, "overlaps pts"), ({"O": da.ptr}, "overlaps partial"),
                       ({"O": da.ptr + 8 * (wct // 2)}, "overlaps partial")):
        with pytest.raises(LsaError) as e:
            call(**kw)
        assert e.value.code == 1 and _message(e.value).startswith(who) and needle in _message(e.value), (kw, str(e.value))
        untouched()
    call(b=0)                                                                 # batch <= 0: a no-op after the checks
    call(b=-1)
    untouched()
    with pytest.raises(LsaError) as e:
        call(b=0, C=None)
    assert "cts is null" in _message(e.value)
    for rb, cb, needle in ((3, 0, "row_block"), (16, 0, "row_block"), (-1, 0, "row_block"), (0, -1, "col_block")):
        with pytest.raises(LsaError) as e:
            ctx.set_bfv_matvec_block(rb, cb)
        assert _message(e.value).startswith("lsa_set_bfv_matvec_block") and needle in _message(e.value)
    untouched()
    P = params.CKKS_DEFAULT[65536]
    ckks = DeviceContext(ALGO_CKKS, n, P["q"][:4], P["p"][:2])
    with pytest.raises(LsaError) as e:
        call(h=ckks.h)
    assert _message(e.value).startswith(who) and "not BFV" in _message(e.value)
    ckks.close()
    with pytest.raises(LsaError):                                             # N < 512: no context of that size exists to refuse on
        DeviceContext(ALGO_BFV, 256, params.ntt_primes_below(50, 256, 2), params.ntt_primes_below(51, 256, 1), 65537)
    untouched()
    call(O=sentinel.ptr + 64)                                                 # a good call into the sentinel buffer itself
    got = ctx.download(sentinel, (sentinel.nwords,))
    assert np.array_equal(got[8: 8 + rows * batch * wct].reshape(ref.shape), ref) and np.all(got[:8] == 7) and np.all(got[8 + rows * batch * wct:] == 7)
