"""GPU parity at the modulus-size thresholds and on worst-case residues.

Every kernel on the hot path picks its arithmetic from the size of the limb's prime (46 / 47 / 48 / 57 / 58 / 61 bits, and the
ratio q_l / q_i of the rescale head).  The chains of tests/boundary.py put a prime on each side of every threshold, and the
operands and keys are the extreme patterns (all q-1, the half point, alternating, deltas, top of the range) next to a uniform
control.  Every assertion is exact equality with the CPU oracle; where a switch selects another form of an operator, that
form must give the same words.  Rings are real sizes: 2^12 (single pass), 2^13, 2^14 (whole-limb and radix-16-squared),
2^16 (8 + 8) and 2^17 (8 + 9).

Patterns are spread over batch slots and levels rather than crossed with everything: batch slot j of level l carries combo
(3 l + j + 5 order) mod 18 of the 9 patterns x {applied to the NTT-form words, applied to the coefficients}.  Dropped to bound
the run time (most of which is the oracle): pattern x switch crosses beyond that rotation; tile batches 1 / 2 only with fused
tails; the operator tests at N = 2^17 run the ascending order at seven levels (levels 1, 2, 5, 6, 7, 8, 12: both sides of the
q_l < 2^48 cut, both values of near, every prime a target at level 12); rotations run at levels 12, 7, 2, with the integer engine forced only at level 12, and at N = 2^16 on
the interleaved order only; the BFV operators run at the top level of their chains; the child process with
LSA_KS_FUSED_ENGINES=3 runs the np = 1 edge (L = 13, 14), np = 2, np = 4 and two levels of the interleaved chain.  No
threshold class is dropped.  Which base conversions run the 29-bit split, and which key switches run the fused key MAC, is
read back from the context (DeviceContext.baseconv_plans, key_switch_fused) and asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest

from lattisense_amd import params
from tests.boundary import (ORDERS, PATTERNS, bfv_mixed_chain, fp_engine, head_flags, pattern_ct, pattern_key, primes_above,
                            straddle_chain)
from tests.gpu_util import env, need_gpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [(p, dom) for dom in (0, 1) for p in PATTERNS]   # dom 1: the pattern is the coefficient-domain content
KEY_PATTERN = {"ascending": "max", "descending": "top", "interleaved": "half"}


def _combo_ct(o, mods, n, rng, first, batch=3):
    """[batch][2][len(mods)][n], slot j carrying combo first + j (limb i of mods is oracle modulus i)"""
    out = np.empty((batch, 2, len(mods), n), dtype=np.uint64)
    for j in range(batch):
        name, dom = COMBOS[(first + j) % len(COMBOS)]
        out[j] = pattern_ct([name], mods, 2, n, rng, oracle=o if dom else None)[0]
    return out


def _key(name, q, p, klvl, n, rng):
    mods = q[: klvl + 1] + p
    beta = (klvl + 1 + len(p) - 1) // len(p)
    return pattern_key(name, mods, beta, n, rng)


# ---------------------------------------------------------------- plain transforms

@pytest.mark.parametrize("logn,wide", [(12, 0), (13, 0), (13, 1), (14, 0), (14, 1), (16, 0), (17, 0)])
def test_plain_transforms(logn, wide, monkeypatch):
    """forward and inverse transform of every pattern on every prime of the straddling chain, both engines: oracle on every
    row and the round trip"""
    need_gpu()
    monkeypatch.setenv("LSA_NTT_WIDE", str(wide))
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    n = 1 << logn
    C = straddle_chain(n, 1)
    q, p = C["q"], C["p"]
    mods = q + p
    o = Oracle(n, q, p, 0)
    rng = np.random.default_rng(logn)
    data = pattern_ct(PATTERNS, mods, 1, n, rng)                       # [9][1][14][N]
    want_f = np.stack([np.stack([o.ntt(i, data[b, 0, i]) for i in range(len(mods))]) for b in range(len(PATTERNS))])[:, None]
    want_i = np.stack([np.stack([o.intt(i, data[b, 0, i]) for i in range(len(mods))]) for b in range(len(PATTERNS))])[:, None]
    mod_of = list(range(len(mods)))
    for fp64 in (1, 0):
        ctx = DeviceContext(ALGO_CKKS, n, q, p)
        try:
            ctx.set_fp64_ntt(fp64)
            for b0 in range(0, len(PATTERNS), 3):                          # batches of three patterns
                sl = slice(b0, b0 + 3)
                buf = ctx.upload(data[sl])
                ctx.ntt(buf, 3, len(mods), mod_of, inverse=False)
                got = ctx.download(buf, data[sl].shape)
                assert np.array_equal(got, want_f[sl]), (fp64, PATTERNS[sl], np.argwhere((got != want_f[sl]).any(axis=-1))[:8])
                ctx.ntt(buf, 3, len(mods), mod_of, inverse=True)
                assert np.array_equal(ctx.download(buf, data[sl].shape), data[sl]), (fp64, PATTERNS[sl])
                buf = ctx.upload(data[sl])
                ctx.ntt(buf, 3, len(mods), mod_of, inverse=True)
                got = ctx.download(buf, data[sl].shape)
                assert np.array_equal(got, want_i[sl]), (fp64, "inverse", PATTERNS[sl], np.argwhere((got != want_i[sl]).any(axis=-1))[:8])
        finally:
            ctx.close()


@pytest.mark.parametrize("logn", [14, 16])
def test_plain_transform_skip_rows(logn):
    """the skip-row map of test_ntt_skip_rows_and_strides on the straddling primes and the max / half / top patterns"""
    need_gpu()
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    n = 1 << logn
    C = straddle_chain(n, 1, "interleaved")
    q, p = C["q"], C["p"]
    o = Oracle(n, q, p, 0)
    rng = np.random.default_rng(3)
    mod_of = [i if i % 3 != 1 else 0xFF for i in range(len(q))]
    data = pattern_ct(("max", "half", "top"), q, 1, n, rng)
    ctx = DeviceContext(ALGO_CKKS, n, q, p)
    try:
        buf = ctx.upload(data)
        ctx.ntt(buf, 3, len(q), mod_of, inverse=False)
        got = ctx.download(buf, data.shape)
        for b in range(3):
            for i, m in enumerate(mod_of):
                want = data[b, 0, i] if m == 0xFF else o.ntt(i, data[b, 0, i])
                assert np.array_equal(got[b, 0, i], want), (b, i)
    finally:
        ctx.close()


# ---------------------------------------------------------------- CKKS rescale, three steps, fused operator

def _ckks_levels(n, order, levels, seed, np_=3, tiles=(1, 2), chain=None):
    """chain: another {"q", "p"} than straddle_chain(n, np_, order); `order` then only picks the key pattern and the combos"""
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    C = chain if chain is not None else straddle_chain(n, np_, order)
    q, p = C["q"], C["p"]
    o = Oracle(n, q, p, 0)
    rng = np.random.default_rng(seed)
    klvl = len(q) - 1
    key = _key(KEY_PATTERN[order], q, p, klvl, n, rng)
    oi = ORDERS.index(order)
    ctxs = []
    try:
        for fp64 in (1, 0):
            ctx = DeviceContext(ALGO_CKKS, n, q, p)
            ctx.set_fp64_ntt(fp64)
            ctxs.append((fp64, ctx, ctx.upload_key(key, klvl)))
        for lvl in levels:
            mods = q[: lvl + 1]
            first = 3 * lvl + 5 * oi
            A = _combo_ct(o, mods, n, rng, first)
            B = _combo_ct(o, mods, n, rng, first + 4)
            # the rescale head alone: the dropped limb's coefficients are exactly the pattern {0, h, h+1, q_l-1, ...}
            R = pattern_ct([PATTERNS[(lvl + j + oi) % len(PATTERNS)] for j in range(3)], mods, 2, n, rng, oracle=o)
            want_r = np.stack([o.ckks_rescale(lvl, R[b]) for b in range(3)])
            want = np.stack([o.ckks_mult_relin_rescale(lvl, A[b], B[b], key, klvl) for b in range(3)])
            want_d3 = np.stack([o.ckks_mult(lvl, A[b], B[b]) for b in range(3)])
            for fp64, ctx, k in ctxs:
                da, db, dr = ctx.upload(A), ctx.upload(B), ctx.upload(R)
                for tails in (1, 0):
                    check(lib().lsa_set_fuse_tails(ctx.h, tails))
                    tag = (order, lvl, "fp64=%d tails=%d" % (fp64, tails))
                    got = ctx.download(ctx.ckks_rescale(lvl, 2, dr, 3), want_r.shape)
                    assert np.array_equal(got, want_r), tag + ("rescale", np.argwhere((got != want_r).any(axis=-1))[:8])
                    d3 = ctx.ckks_mult(lvl, da, db, 3)
                    assert np.array_equal(ctx.download(d3, want_d3.shape), want_d3), tag + ("mult",)
                    three = ctx.download(ctx.ckks_rescale(lvl, 2, ctx.ckks_relin(lvl, d3, k, 3), 3), want.shape)
                    assert np.array_equal(three, want), tag + ("three steps", np.argwhere((three != want).any(axis=-1))[:8])
                    for fold in ("1", "0"):
                        for tile in (0,) + (tiles if tails else ()):
                            ctx.set_tile_batch(tile)
                            with env(LSA_HMULT_FOLD=None if fold == "1" else "0"):
                                got = ctx.download(ctx.ckks_mult_relin_rescale(lvl, da, db, k, 3), want.shape)
                            assert np.array_equal(got, want), tag + ("fold=" + fold, tile, np.argwhere((got != want).any(axis=-1))[:8])
                        ctx.set_tile_batch(0)
                check(lib().lsa_set_fuse_tails(ctx.h, 1))
    finally:
        for _, ctx, _k in ctxs:
            ctx.close()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("logn", [13, 14, 16])
def test_ckks_rescale_three_steps_and_fused(logn, order):
    """every level >= 1 of each chain order: ckks_rescale on pattern coefficients, ckks_mult, mult -> relin -> rescale and
    ckks_mult_relin_rescale against the oracle, under fused tails 0/1, LSA_HMULT_FOLD 0/1, tile batch 0/1/2, both engines"""
    need_gpu()
    _ckks_levels(1 << logn, order, range(1, 13), 100 * logn + ORDERS.index(order))


def test_ckks_rescale_three_steps_and_fused_n17():
    """N = 2^17 (8 + 9 stages), the ascending order (both values of near and fp_lift on both engines)"""
    need_gpu()
    _ckks_levels(1 << 17, "ascending", (1, 2, 5, 6, 7, 8, 12), 1717, tiles=(1,))


# ---------------------------------------------------------------- CKKS rotations

@pytest.mark.parametrize("logn,order", [(ln, od) for ln in (13, 14) for od in ORDERS] + [(16, "interleaved")])
def test_ckks_rotate_rotate_many_conjugate(logn, order):
    need_gpu()
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    n = 1 << logn
    C = straddle_chain(n, 3, order)
    q, p = C["q"], C["p"]
    o = Oracle(n, q, p, 0)
    oi = ORDERS.index(order)
    rng = np.random.default_rng(7 * logn + oi)
    klvl = len(q) - 1
    gs = [5, int(pow(5, 77, 2 * n)), 2 * n - 1]
    keys = {g: _key(PATTERNS[(1 + 2 * i + oi) % len(PATTERNS)] if i else KEY_PATTERN[order], q, p, klvl, n, rng) for i, g in enumerate(gs)}
    for fp64 in (1, 0):
        ctx = DeviceContext(ALGO_CKKS, n, q, p)
        try:
            ctx.set_fp64_ntt(fp64)
            hk = {g: ctx.upload_key(keys[g], klvl) for g in gs}
            for lvl in (12, 7, 2):
                if fp64 == 0 and lvl != 12:
                    continue
                A = _combo_ct(o, q[: lvl + 1], n, np.random.default_rng(lvl), 3 * lvl + 5 * oi + 1)
                da = ctx.upload(A)
                want = {g: np.stack([o.ckks_rotate(lvl, A[b], g, keys[g], klvl) for b in range(3)]) for g in gs}
                for scatter in (None, "0"):
                    with env(LSA_ROT_SCATTER=scatter):
                        for g in gs:
                            got = ctx.download(ctx.ckks_rotate(lvl, da, g, hk[g], 3), want[g].shape)
                            assert np.array_equal(got, want[g]), (order, lvl, fp64, scatter, g)
                        outs = ctx.ckks_rotate_many(lvl, da, hk, 3)
                        for g in gs:
                            assert np.array_equal(ctx.download(outs[g], want[g].shape), want[g]), (order, lvl, fp64, scatter, g, "many")
        finally:
            ctx.close()


# ---------------------------------------------------------------- digit-structure edges of the key MAC

def fp_size_chain(n, L, np_):
    """L primes alternating just below 2^47 and just below 2^46 (all FP64-engine limbs), np_ 61-bit special primes"""
    a, b = params.ntt_primes_below(47, n, (L + 1) // 2), params.ntt_primes_below(46, n, L // 2)
    q = [x for pair in zip(a, b + [None]) for x in pair if x is not None][:L]
    return q, params.ntt_primes_below(61, n, np_)


def _digit_edges(n, cases, seed):
    """cases: (np, list of L): HMult+relin+rescale and rotate at level L - 1 with the key of that level, against the oracle
    (first and last batch slot) and fused == LSA_KS_FUSED=0 (every slot); which of the two paths a level takes is read back
    from the context (DeviceContext.key_switch_fused), so the comparison is never between two runs of the same path"""
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    rng = np.random.default_rng(seed)
    for np_, Ls in cases:
        q, p = fp_size_chain(n, max(Ls), np_)
        assert all(fp_engine(m) for m in q) and any(m.bit_length() == 47 for m in q)
        o = Oracle(n, q, p, 0)
        ctx = DeviceContext(ALGO_CKKS, n, q, p)
        try:
            for L in Ls:
                lvl = klvl = L - 1
                mods = q[:L]
                key = _key(("max", "top", "half", "uniform")[L % 4], q, p, klvl, n, rng)
                k = ctx.upload_key(key, klvl)
                beta, T = (L + np_ - 1) // np_, L + np_
                assert ctx.key_switch_fused(lvl, k) == (beta * T <= 192), (np_, L, "fused key MAC expected up to beta T = 192")
                assert (np_, L) not in FUSED_EXPECTED or ctx.key_switch_fused(lvl, k) == FUSED_EXPECTED[(np_, L)], (np_, L)
                with env(LSA_KS_FUSED="0"):
                    assert not ctx.key_switch_fused(lvl, k), (np_, L, "LSA_KS_FUSED=0 must take the unfused path")
                A = _combo_ct(o, mods, n, rng, L)
                B = _combo_ct(o, mods, n, rng, L + 9)
                A[0], B[0] = pattern_ct(["max"], mods, 2, n, rng)[0], pattern_ct(["max"], mods, 2, n, rng)[0]
                da, db = ctx.upload(A), ctx.upload(B)
                g = int(pow(5, 77, 2 * n))
                outs = {}
                for fused in (None, "0"):
                    with env(LSA_KS_FUSED=fused):
                        outs[fused] = (ctx.download(ctx.ckks_mult_relin_rescale(lvl, da, db, k, 3), (3, 2, lvl, n)),
                                       ctx.download(ctx.ckks_rotate(lvl, da, g, k, 3), (3, 2, L, n)))
                assert np.array_equal(outs[None][0], outs["0"][0]), (np_, L, "hmult fused != unfused")
                assert np.array_equal(outs[None][1], outs["0"][1]), (np_, L, "rotate fused != unfused")
                for b in (0, 2):
                    assert np.array_equal(outs[None][0][b], o.ckks_mult_relin_rescale(lvl, A[b], B[b], key, klvl)), (np_, L, b, "hmult")
                    assert np.array_equal(outs[None][1][b], o.ckks_rotate(lvl, A[b], g, key, klvl)), (np_, L, b, "rotate")
                ctx.destroy_key(k)
        finally:
            ctx.close()


DIGIT_CASES = ((1, (2, 7, 8, 9, 13, 14)), (2, (9,)), (4, (13,)))
FUSED_EXPECTED = {(1, 13): True, (1, 14): False, (2, 9): True, (4, 13): True}   # np = 1: beta T = 182 / 210


@pytest.mark.parametrize("logn", [14, 16])
def test_digit_structure_edges(logn):
    """np = 1: beta = L up to the last fused shape (L = 13: beta T = 182) and the first unfused one (L = 14: 210);
    np = 2 with an odd L (short last digit); np = 4, L = 13 (the headline's shape) -- all on 46/47-bit primes"""
    need_gpu()
    _digit_edges(1 << logn, DIGIT_CASES, logn)


def test_digit_structure_edges_fused_on_both_engines_in_a_child():
    """LSA_KS_FUSED_ENGINES=3 (read once per process): integer-engine target limbs (the 61-bit P here) through the fused kernel"""
    need_gpu()
    code = ("from tests.test_gpu_boundary import _digit_edges, _ckks_levels; "
            "_digit_edges(1 << 16, ((1, (13, 14)), (2, (9,)), (4, (13,))), 5); "
            "_ckks_levels(1 << 16, 'interleaved', (4, 9), 6, tiles=())")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, LSA_KS_FUSED_ENGINES="3"),
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------- the bootstrap chain's 60 -> 40-bit drops on a two-pass ring

def test_bootstrap_chain_drops_n16():
    """params.CKKS_BOOTSTRAP_65536 q[:16] at N = 2^16: levels 13..15 drop a 60-bit limb onto 39-41-bit FP64-engine targets
    (near == false, fp_lift == false), bit-exact on the radix-16-squared kernels; max and half patterns"""
    need_gpu()
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    P = params.CKKS_BOOTSTRAP_65536
    n, q, p = 1 << 16, P["q"][:16], P["p"]
    assert all(head_flags(q[l], q[1]) == (False, False) for l in (13, 14, 15))
    o = Oracle(n, q, p, 0)
    rng = np.random.default_rng(65)
    klvl = 15
    key = _key("max", q, p, klvl, n, rng)
    g = int(pow(5, 77, 2 * n))
    ctx = DeviceContext(ALGO_CKKS, n, q, p)
    try:
        k = ctx.upload_key(key, klvl)
        for lvl in (13, 14, 15):
            mods = q[: lvl + 1]
            A = np.concatenate([pattern_ct(("max", "half"), mods, 2, n, rng), pattern_ct(("max", "half"), mods, 2, n, rng, oracle=o)])
            B = A[::-1].copy()
            da, db = ctx.upload(A), ctx.upload(B)
            got = ctx.download(ctx.ckks_mult_relin_rescale(lvl, da, db, k, 4), (4, 2, lvl, n))
            rot = ctx.download(ctx.ckks_rotate(lvl, da, g, k, 4), (4, 2, lvl + 1, n))
            res = ctx.download(ctx.ckks_rescale(lvl, 2, da, 4), (4, 2, lvl, n))
            for b in range(4):
                assert np.array_equal(got[b], o.ckks_mult_relin_rescale(lvl, A[b], B[b], key, klvl)), (lvl, b, "hmult")
                assert np.array_equal(rot[b], o.ckks_rotate(lvl, A[b], g, key, klvl)), (lvl, b, "rotate")
                assert np.array_equal(res[b], o.ckks_rescale(lvl, A[b])), (lvl, b, "rescale")
    finally:
        ctx.close()


# ---------------------------------------------------------------- BFV

def bfv_small_chain(n):
    """every Q and P prime below 2^58, with the largest ones (57.99 bits) among them: the split predicate true at its edge"""
    big = params.ntt_primes_below(58, n, 5)
    q = big[2:] + params.ntt_primes_below(47, n, 2) + params.ntt_primes_below(57, n, 1)
    return q, big[:2]


@pytest.mark.parametrize("chain", ["mixed", "small"])
@pytest.mark.parametrize("logn", [14, 16])
def test_bfv_operators(logn, chain, monkeypatch):
    """bfv_mult_relin, bfv_rotate, bfv_rotate_many, the pt_mul MAC and the hoisted rotate-and-MAC on FP64-engine and
    57-59-bit limbs at two-pass rings; LSA_BC_NO_SPLIT=1 must give the same words"""
    need_gpu()
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    from oracle.pyoracle import Oracle
    from tests.test_gpu_bfv_ptmul import _want_mac
    n, t = 1 << logn, 65537
    q, p = bfv_mixed_chain(n) if chain == "mixed" else bfv_small_chain(n)
    if chain == "small":   # ModUp / ModDown (sources and destinations within Q u P) take the split; the 61-bit auxiliary base never
        assert all(m >> 58 == 0 for m in q + p) and max(q + p) > (1 << 58) - (1 << 40)
    else:
        assert any(m >> 58 for m in q) and any(fp_engine(m) for m in q) and any((1 << 47) < m < (1 << 48) for m in q)
    o = Oracle(n, q, p, t)
    rng = np.random.default_rng(logn + len(chain))
    lvl = klvl = len(q) - 1
    L = lvl + 1
    names = ("max", "half", "top")
    key = _key("max", q, p, klvl, n, rng)
    gs = [5, 2 * n - 1]
    gkeys = {5: _key("top", q, p, klvl, n, rng), 2 * n - 1: _key("uniform", q, p, klvl, n, rng)}
    A = pattern_ct(names, q, 2, n, rng)
    B = pattern_ct(("alt", "max", "uniform"), q, 2, n, rng)
    pts = [pattern_ct(("max", "delta", "uniform"), q, 1, n, rng)[:, 0], pattern_ct(("half", "max", "top"), q, 1, n, rng)[:, 0]]
    want_mul = np.stack([o.bfv_mult_relin(lvl, A[b], B[b], key, klvl) for b in range(3)])
    want_rot = {g: np.stack([o.bfv_rotate(lvl, A[b], g, gkeys[g], klvl) for b in range(3)]) for g in gs}
    want_mac = np.stack([_want_mac(o, L, [A[b], B[b]], [pts[0][b], pts[1][b]]) for b in range(3)])
    want_rmac = np.stack([_want_mac(o, L, [want_rot[g][b] for g in gs], [pts[i][b] for i in range(2)]) for b in range(3)])
    for no_split in (None, "1"):
        if no_split is None:
            monkeypatch.delenv("LSA_BC_NO_SPLIT", raising=False)
        else:
            monkeypatch.setenv("LSA_BC_NO_SPLIT", no_split)
        ctx = DeviceContext(ALGO_BFV, n, q, p, t)
        try:
            assert ctx.moduli == o.mod
            k = ctx.upload_key(key, klvl)
            hk = {g: ctx.upload_key(gkeys[g], klvl) for g in gs}
            da, db = ctx.upload(A), ctx.upload(B)
            dp = [ctx.upload(x) for x in pts]
            tag = (chain, logn, no_split)
            for fold in (None, "0"):
                with env(LSA_BFV_FOLD=fold):
                    got = ctx.download(ctx.bfv_mult_relin(lvl, da, db, k, 3), want_mul.shape)
                assert np.array_equal(got, want_mul), tag + ("mult_relin", fold)
            outs = ctx.bfv_rotate_many(lvl, da, hk, 3)
            for g in gs:
                assert np.array_equal(ctx.download(ctx.bfv_rotate(lvl, da, g, hk[g], 3), want_rot[g].shape), want_rot[g]), tag + ("rotate", g)
                assert np.array_equal(ctx.download(outs[g], want_rot[g].shape), want_rot[g]), tag + ("rotate_many", g)
            got = ctx.download(ctx.bfv_mac_plain_mul(lvl, [da, db], dp, 3), want_mac.shape)
            assert np.array_equal(got, want_mac), tag + ("pt_mul MAC",)
            for fused in (None, "0"):
                with env(LSA_ROTMAC_FUSED=fused):
                    got = ctx.download(ctx.bfv_rotate_mac_plain_mul(lvl, da, [(g, hk[g], dp[i]) for i, g in enumerate(gs)], 3), want_rmac.shape)
                assert np.array_equal(got, want_rmac), tag + ("rotate-and-MAC", fused)
            # which conversions ran split: ModUp digits and ModDown have at most np sources and stay inside Q u P; the
            # multiply's conversions to and from the 61-bit auxiliary base have L or more sources and never qualify
            plans = ctx.baseconv_plans()
            assert any(ns <= len(p) for ns, _, _ in plans) and any(ns >= L for ns, _, _ in plans), plans
            for ns, nd, split in plans:
                want_split = chain == "small" and no_split is None and ns <= len(p)
                assert split == want_split, tag + (ns, nd, split, plans)
        finally:
            ctx.close()


@pytest.mark.parametrize("nq", [16, 17])
def test_bfv_conversion_with_16_and_17_sources_on_58_bit_primes(nq):
    """the multiply's Q -> auxiliary-base conversion with exactly LSA_BC_NARROW_SRC (16) source limbs (the narrow kernel) and
    with 17 (the wide kernel), on the largest primes below 2^58 and all-max operands.  Its destinations are 61-bit, so it
    never runs the 29-bit split (asserted); the split's own term limits are test_split_accumulate_with_8_and_16_terms"""
    need_gpu()
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    from oracle.pyoracle import Oracle
    n, t = 1 << 14, 65537
    pr = params.ntt_primes_below(58, n, nq + 2)
    q, p = pr[2:], pr[:2]
    o = Oracle(n, q, p, t)
    rng = np.random.default_rng(nq)
    lvl = klvl = nq - 1
    key = _key("max", q, p, klvl, n, rng)
    A = pattern_ct(("max", "half", "top"), q, 2, n, rng)
    B = pattern_ct(("max", "alt", "uniform"), q, 2, n, rng)
    want = np.stack([o.bfv_mult_relin(lvl, A[b], B[b], key, klvl) for b in range(3)])
    for no_split in (None, "1"):
        with env(LSA_BC_NO_SPLIT=no_split):
            ctx = DeviceContext(ALGO_BFV, n, q, p, t)
            try:
                k = ctx.upload_key(key, klvl)
                got = ctx.download(ctx.bfv_mult_relin(lvl, ctx.upload(A), ctx.upload(B), k, 3), want.shape)
                assert np.array_equal(got, want), (nq, no_split)
                plans = ctx.baseconv_plans()
                assert any(ns == nq for ns, _, _ in plans), plans
                assert all(not split for ns, _, split in plans if ns >= nq), plans
            finally:
                ctx.close()


@pytest.mark.parametrize("np_", [8, 16])
def test_split_accumulate_with_8_and_16_terms(np_):
    """every Q and P prime at 57.99 bits and np = 8 / 16 special primes: ModDown (np sources) and a full ModUp digit (np
    sources) run the narrow kernel's 29-bit split accumulate with 8 terms (the three-product form at its limit) and with 16
    (the four-product form at its limit), on all-max, half and top operands and an all-max key; against the oracle and
    against LSA_BC_NO_SPLIT=1, CKKS HMult+relin+rescale and rotate, and BFV multiply+relin (whose auxiliary-base
    conversions stay unsplit)"""
    need_gpu()
    from lattisense_amd.device import ALGO_BFV, ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    n, t = 1 << 14, 65537
    nq = np_ + 2                                   # digits of np_ and of 2 limbs
    pr = params.ntt_primes_below(58, n, nq + np_)
    assert min(pr) > (1 << 58) - (1 << 40)
    q, p = pr[np_:], pr[:np_]
    lvl = klvl = nq - 1
    rng = np.random.default_rng(np_)
    key = _key("max", q, p, klvl, n, rng)
    g = int(pow(5, 77, 2 * n))
    A = pattern_ct(("max", "half", "top"), q, 2, n, rng)
    B = pattern_ct(("max", "max", "uniform"), q, 2, n, rng)
    oc, ob = Oracle(n, q, p, 0), Oracle(n, q, p, t)
    want_mul = np.stack([oc.ckks_mult_relin_rescale(lvl, A[b], B[b], key, klvl) for b in range(3)])
    want_rot = np.stack([oc.ckks_rotate(lvl, A[b], g, key, klvl) for b in range(3)])
    want_bfv = np.stack([ob.bfv_mult_relin(lvl, A[b], B[b], key, klvl) for b in range(3)])
    for no_split in (None, "1"):
        with env(LSA_BC_NO_SPLIT=no_split):
            ctx = DeviceContext(ALGO_CKKS, n, q, p)
            try:
                k = ctx.upload_key(key, klvl)
                da, db = ctx.upload(A), ctx.upload(B)
                got = ctx.download(ctx.ckks_mult_relin_rescale(lvl, da, db, k, 3), want_mul.shape)
                assert np.array_equal(got, want_mul), (np_, no_split, "hmult")
                got = ctx.download(ctx.ckks_rotate(lvl, da, g, k, 3), want_rot.shape)
                assert np.array_equal(got, want_rot), (np_, no_split, "rotate")
                plans = ctx.baseconv_plans()
                assert sum(ns == np_ for ns, _, _ in plans) >= 2 and any(ns == 2 for ns, _, _ in plans), plans   # ModUp digit and ModDown; the short digit
                assert all(split == (no_split is None) for _, _, split in plans), (np_, no_split, plans)
            finally:
                ctx.close()
            ctx = DeviceContext(ALGO_BFV, n, q, p, t)
            try:
                k = ctx.upload_key(key, klvl)
                got = ctx.download(ctx.bfv_mult_relin(lvl, ctx.upload(A), ctx.upload(B), k, 3), want_bfv.shape)
                assert np.array_equal(got, want_bfv), (np_, no_split, "bfv")
                plans = ctx.baseconv_plans()
                assert any(ns == np_ and split for ns, _, split in plans) == (no_split is None), plans
                assert all(not split for ns, _, split in plans if ns > np_), plans
            finally:
                ctx.close()


def test_one_prime_above_2_58_decides_the_split():
    """every Q and P prime at 57.99 bits except the last Q prime, the smallest above 2^58: at the level below it every
    conversion runs split, at its own level it is a source or a destination of every conversion and none does -- the one
    prime decides the predicate (moving the cut from 58 to 59 bits changes the set read back here)"""
    need_gpu()
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    n = 1 << 14
    pr = params.ntt_primes_below(58, n, 7)
    q, p = pr[2:] + primes_above(58, n, 1), pr[:2]
    assert q[-1].bit_length() == 59 and q[-1] < (1 << 58) + (1 << 40) and all(m >> 58 == 0 for m in q[:-1] + p)
    top = len(q) - 1
    o = Oracle(n, q, p, 0)
    rng = np.random.default_rng(58)
    key = _key("max", q, p, top, n, rng)
    g = int(pow(5, 77, 2 * n))
    for lvl, want_split in ((top - 1, True), (top, False)):   # a context per level: its plans are that level's conversions
        ctx = DeviceContext(ALGO_CKKS, n, q, p)
        try:
            k = ctx.upload_key(key, top)
            mods = q[: lvl + 1]
            A = pattern_ct(("max", "half", "top"), mods, 2, n, rng)
            B = pattern_ct(("max", "alt", "uniform"), mods, 2, n, rng)
            da, db = ctx.upload(A), ctx.upload(B)
            got = ctx.download(ctx.ckks_mult_relin_rescale(lvl, da, db, k, 3), (3, 2, lvl, n))
            rot = ctx.download(ctx.ckks_rotate(lvl, da, g, k, 3), (3, 2, lvl + 1, n))
            for b in range(3):
                assert np.array_equal(got[b], o.ckks_mult_relin_rescale(lvl, A[b], B[b], key, top)), (lvl, b, "hmult")
                assert np.array_equal(rot[b], o.ckks_rotate(lvl, A[b], g, key, top)), (lvl, b, "rotate")
            plans = ctx.baseconv_plans()
            assert len(plans) >= 3 and all(split == want_split for _, _, split in plans), (lvl, want_split, plans)
        finally:
            ctx.close()
