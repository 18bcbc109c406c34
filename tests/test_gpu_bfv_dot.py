"""BFV encrypted inner product on the device (lsa_bfv_mult_sum / lsa_bfv_dot; ops.hip bfv_mult_sum / bfv_dot over k_tensor_sum)
against its CPU restatement tests/bfv_dot_model.py (oracle primitives only; held to exact integers by tests/test_bfv_dot_api.py)
on one batch item, against lsa_bfv_relin of its own d3, and at one term against lsa_bfv_mult / lsa_bfv_mult_relin.  Every
comparison is word for word.  The sum is NOT the lazy composition of lsa_bfv_mult per pair (that rounds once per pair), so the
model is the reference for n > 1.  The last test encrypts real messages and decrypts sum_i x_i y_i mod t exactly."""
import ctypes
import os
import re

import numpy as np
import pytest

from lattisense_amd import params
from tests import bfv_dot_model as model
from tests.gpu_util import env, need_gpu, rand_ct

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSA_ERR_ARG = 1


def _max_terms():
    text = open(os.path.join(ROOT, "lattisense_amd", "csrc", "tensor_sum.h")).read()
    return int(re.search(r"#define LSA_DOT_MAX_TERMS (\d+)", text).group(1))


MAX_TERMS = _max_terms()


class Rig:
    def __init__(self, n, q, p, t, klvl, seed, fp64=True):
        from lattisense_amd.device import ALGO_BFV, DeviceContext
        self.n, self.q, self.p, self.t, self.klvl = n, list(q), list(p), t, klvl
        self.rng = np.random.default_rng(seed)
        self.ctx = DeviceContext(ALGO_BFV, n, q, p, t)
        if not fp64:
            self.ctx.set_fp64_ntt(0)
        beta = (klvl + 1 + len(p) - 1) // len(p)
        self.key = rand_ct(self.rng, self.q[: klvl + 1] + self.p, 2, n, beta)
        self.k = self.ctx.upload_key(self.key, klvl)
        self._o = None

    @property
    def o(self):
        if self._o is None:
            from oracle.pyoracle import Oracle
            self._o = Oracle(self.n, self.q, self.p, self.t)
            assert self._o.mod == self.ctx.moduli   # the same auxiliary primes on both sides
        return self._o

    def ct(self, lvl, batch):
        return rand_ct(self.rng, self.q[: lvl + 1], 2, self.n, batch)

    def close(self):
        self.ctx.close()


def _arr(ctype, values):
    return (ctype * max(len(values), 1))(*values)


def dot(rig, lvl, dA, dB, batch, addend=None, **kw):
    return rig.ctx.download(rig.ctx.bfv_dot(lvl, dA, dB, rig.k, batch, addend=addend, **kw), (batch, 2, lvl + 1, rig.n))


def mult_sum(rig, lvl, dA, dB, batch, addend=None, **kw):
    return rig.ctx.download(rig.ctx.bfv_mult_sum(lvl, dA, dB, batch, addend=addend, **kw), (batch, 3, lvl + 1, rig.n))


def check_against_model(rig, lvl, hA, hB, dA, dB, batch, item, hE=None, dE=None, what=""):
    """device d3 and dot against the model on `item`, and dot == relin(mult_sum) on the whole batch; returns the dot"""
    ctx = rig.ctx
    d3 = ctx.bfv_mult_sum(lvl, dA, dB, batch, addend=dE)
    got3 = ctx.download(d3, (batch, 3, lvl + 1, rig.n))
    got = dot(rig, lvl, dA, dB, batch, dE)
    views = {}   # one view per batch array, so that the model extends a repeated operand once

    def pick(x):
        return views.setdefault(id(x), x[item])

    want3 = model.mult_sum(rig.o, lvl, [pick(x) for x in hA], [pick(x) for x in hB], hE[item] if hE is not None else None)
    assert np.array_equal(got3[item], want3), ("mult_sum against the model", what)
    assert np.array_equal(got[item], rig.o.bfv_relin(lvl, want3, rig.key, rig.klvl)), ("dot against the model", what)
    assert np.array_equal(got, ctx.download(ctx.bfv_relin(lvl, d3, rig.k, batch), (batch, 2, lvl + 1, rig.n))), ("dot == relin(mult_sum)", what)
    return got


def test_small_ring_levels_terms_tiles_and_streams():
    """N = 2^12 on the N = 2^13 primes: levels 0..2, batch 3 with items 0 and 2 equal, n in {1, 2, 3, LSA_DOT_MAX_TERMS + 1}, with
    and without an addend; level 1 with n >= 3 is the case M(n) = M(1) + 1.  Then tile batch 0 / 1 / 2, single and dual stream"""
    need_gpu()
    from lattisense_amd._native import check, lib
    P = params.BFV_DEFAULT[8192]
    rig = Rig(1 << 12, P["q"], P["p"], P["t"], 2, 1201)
    ctx, batch = rig.ctx, 3
    assert [model.aux_limbs(rig.n, rig.q, 1, m) for m in (1, 2, 3)] == [2, 2, 3]
    try:
        for lvl in range(3):
            pool = 4   # term i is a[i % 4] x b[(3 i + 1) % 4]: 16 distinct pairs from 4 + 4 ciphertexts
            hA, hB, hE = [rig.ct(lvl, batch) for _ in range(pool)], [rig.ct(lvl, batch) for _ in range(pool)], rig.ct(lvl, batch)
            for x in hA + hB + [hE]:
                x[2] = x[0]
            pA, pB, dE = [ctx.upload(x) for x in hA], [ctx.upload(x) for x in hB], ctx.upload(hE)
            ref = {}
            for n in (1, 2, 3, MAX_TERMS + 1):
                ia, ib = [i % pool for i in range(n)], [(3 * i + 1) % pool for i in range(n)]
                for addend in (False, True):
                    got = check_against_model(rig, lvl, [hA[i] for i in ia], [hB[i] for i in ib], [pA[i] for i in ia], [pB[i] for i in ib],
                                              batch, 1, hE if addend else None, dE if addend else None, (lvl, n, addend))
                    assert np.array_equal(got[2], got[0]) and not np.array_equal(got[1], got[0])
                    ref[(n, addend)] = got
            one = ctx.download(ctx.bfv_mult_relin(lvl, pA[0], pB[1], rig.k, batch), (batch, 2, lvl + 1, rig.n))
            assert np.array_equal(ref[(1, False)], one), ("n == 1 is bfv_mult_relin", lvl)
            d3 = ctx.download(ctx.bfv_mult(lvl, pA[0], pB[1], batch), (batch, 3, lvl + 1, rig.n))
            assert np.array_equal(mult_sum(rig, lvl, [pA[0]], [pB[1]], batch), d3), ("n == 1 is bfv_mult", lvl)
            for dual in (0, 1):
                check(lib().lsa_set_dual_stream(ctx.h, dual))
                for tile in (0, 1, 2):
                    ctx.set_tile_batch(tile)
                    for (n, addend), want in ref.items():
                        ia, ib = [i % pool for i in range(n)], [(3 * i + 1) % pool for i in range(n)]
                        got = dot(rig, lvl, [pA[i] for i in ia], [pB[i] for i in ib], batch, dE if addend else None)
                        assert np.array_equal(got, want), (lvl, dual, tile, n, addend)
            check(lib().lsa_set_dual_stream(ctx.h, 0))
            ctx.set_tile_batch(0)
    finally:
        rig.close()


def test_one_context_runs_a_level_over_two_auxiliary_bases():
    """bfv_mult and bfv_mult_sum share one basis builder whose cached constants and conversion plans are keyed by (L, M).  N = 2^12,
    level 1, batch 3 (items 0 and 2 equal), ONE context: n = 3 builds the M(3) = 3 basis first, then bfv_mult and n = 1 run the same
    level over M(1) = 2, then n = 3 again -- folded, then with LSA_BFV_FOLD=0 (read per call: both sets of constants sit in the
    cache).  The three pairs are a plain one, one whose b is shared by the batch (stride 0) and a square: bfv_mult on each is the
    oracle's on item 1 and mult_sum(n = 1) on the whole batch, and both sums of the three are the model's.
    A second context takes the other order -- unfolded before folded, bfv_mult and n = 1 (M = 2) before n = 3 (M = 3), then M = 2
    again: the M = 3 vector of Q^-1 begins with the M = 2 one, so only the short vector cached first shows a name without M"""
    need_gpu()
    from lattisense_amd._native import check, lib
    P = params.BFV_DEFAULT[8192]
    n, lvl, batch = 1 << 12, 1, 3
    w2, w3 = 2 * (lvl + 1) * n, 3 * (lvl + 1) * n
    assert [model.aux_limbs(n, P["q"], lvl, m) for m in (1, 3)] == [2, 3]
    want3 = want1 = None
    for sum_first, folds, seed in ((True, (None, "0"), 1207), (False, ("0", None), 1208)):
        rig = Rig(n, P["q"], P["p"], P["t"], 2, seed)
        ctx = rig.ctx

        def mult(a, b, sb):
            out = ctx.alloc(batch * w3)
            check(lib().lsa_bfv_mult(ctx.h, lvl, a.ptr, b.ptr, out.ptr, batch, w2, sb, w3, ctx.stream))
            return ctx.download(out, (batch, 3, lvl + 1, n))

        try:
            if want3 is None:   # the operands and their references, once
                hA, hB, hW = [rig.ct(lvl, batch) for _ in range(3)], rig.ct(lvl, batch), rig.ct(lvl, 1)
                for x in hA + [hB]:
                    x[2] = x[0]

                def host(i):   # item i of the three pairs
                    return [hA[0][i], hA[1][i], hA[2][i]], [hB[i], hW[0], hA[2][i]]

                want3 = {i: model.mult_sum(rig.o, lvl, *host(i)) for i in (0, 1)}
                want1 = [rig.o.bfv_mult(lvl, a, b) for a, b in zip(*host(1))]
            dA, dB, dW = [ctx.upload(x) for x in hA], ctx.upload(hB), ctx.upload(hW)
            pairs = [("plain", dA[0], dB, w2), ("b shared by the batch", dA[1], dW, 0), ("square", dA[2], dA[2], w2)]

            def three(tag):
                got = mult_sum(rig, lvl, dA, [dB, dW, dA[2]], batch, sbs=[w2, 0, w2])
                assert np.array_equal(got[0], want3[0]) and np.array_equal(got[1], want3[1]), ("n = 3 against the model", tag)
                assert np.array_equal(got[2], got[0]) and not np.array_equal(got[1], got[0]), tag

            def ones(tag):
                for k, (what, a, b, sb) in enumerate(pairs):
                    got = mult(a, b, sb)
                    assert np.array_equal(got[1], want1[k]), ("bfv_mult against the oracle", what, tag)
                    assert np.array_equal(got, mult_sum(rig, lvl, [a], [b], batch, sbs=[sb])), ("n == 1 is bfv_mult", what, tag)
                    assert np.array_equal(got[2], got[0]) and not np.array_equal(got[1], got[0]), (what, tag)

            for fold in folds:
                with env(LSA_BFV_FOLD=fold):
                    tag = (sum_first, fold)
                    for step in (three, ones, three) if sum_first else (ones, three, ones):
                        step(tag)
        finally:
            rig.close()


def test_tight_chain_three_groups():
    """a chain whose top level leaves G = 1 spare bit: max_terms = 2, so n = 5 runs as groups of 2, 2 and 1, each scaled down on
    its own and added in Q"""
    need_gpu()
    from lattisense_amd.device import bfv_dot_plan
    n = 1 << 12
    q = params.ntt_primes_below(57, n, 2) + params.ntt_primes_below(56, n, 1)
    p = params.ntt_primes_below(58, n, 1)
    assert model.plan(n, q, 2, 5) == {"G": 1, "max_terms": 2, "groups": 3, "aux_limbs": 3}
    assert bfv_dot_plan(n, q, 2, 5) == {"max_terms": 2, "groups": 3, "aux_limbs": 3}
    rig = Rig(n, q, p, 65537, 2, 1202)
    try:
        batch, lvl = 2, 2
        hA, hB, hE = [rig.ct(lvl, batch) for _ in range(5)], [rig.ct(lvl, batch) for _ in range(5)], rig.ct(lvl, batch)
        dA, dB, dE = [rig.ctx.upload(x) for x in hA], [rig.ctx.upload(x) for x in hB], rig.ctx.upload(hE)
        check_against_model(rig, lvl, hA, hB, dA, dB, batch, 1, None, None, "no addend")
        check_against_model(rig, lvl, hA, hB, dA, dB, batch, 0, hE, dE, "addend")
    finally:
        rig.close()


def test_split_at_the_shipped_n13_set():
    """the N = 2^13 set at its top level has G = 7: 257 terms (one pair, repeated pointers) run as groups of 128, 128 and 1"""
    need_gpu()
    P = params.BFV_DEFAULT[8192]
    rig = Rig(1 << 13, P["q"], P["p"], P["t"], 2, 1301)
    try:
        lvl, batch, n = 2, 2, 257
        assert model.plan(rig.n, rig.q, lvl, n)["groups"] == 3 and model.plan(rig.n, rig.q, lvl, n)["max_terms"] == 128
        hA, hB = rig.ct(lvl, batch), rig.ct(lvl, batch)
        dA, dB = rig.ctx.upload(hA), rig.ctx.upload(hB)
        check_against_model(rig, lvl, [hA] * n, [hB] * n, [dA] * n, [dB] * n, batch, 1, what="257 terms")
    finally:
        rig.close()


@pytest.mark.parametrize("shape", ["n14_level3", "n15_12q_3p"])
def test_bench_shapes(shape):
    """N = 2^14 level 3 (the reference bench shape) and N = 2^15 with 12 Q + 3 P at the top level (two-pass rings, the 24-row
    tensor), batch 2, n = 3, against the model"""
    need_gpu()
    if shape == "n14_level3":
        P, n, lvl = params.BFV_DEFAULT[16384], 1 << 14, 3
    else:
        P, n, lvl = params.BFV_DEFAULT[32768], 1 << 15, 11
    rig = Rig(n, P["q"], P["p"], P["t"], lvl, 1400 + lvl)
    try:
        batch = 2
        hA, hB, hE = [rig.ct(lvl, batch) for _ in range(3)], [rig.ct(lvl, batch) for _ in range(3)], rig.ct(lvl, batch)
        dA, dB, dE = [rig.ctx.upload(x) for x in hA], [rig.ctx.upload(x) for x in hB], rig.ctx.upload(hE)
        check_against_model(rig, lvl, hA, hB, dA, dB, batch, 1, hE, dE, shape)
    finally:
        rig.close()


def test_near_worst_residues_across_the_launch_bound():
    """every coefficient of every operand at +-(Q/2 - Q/2^20): the extended residues at the 61-bit auxiliary primes and the 128-bit
    sums are as large as they get; n = 33 repeated pointers = 2 LSA_DOT_MAX_TERMS + 1, at the default chunk and at 16 pairs per
    launch (16 + 16 + 1)"""
    need_gpu()
    P = params.BFV_DEFAULT[8192]
    rig = Rig(1 << 12, P["q"], P["p"], P["t"], 2, 1203)
    try:
        lvl, batch, n = 2, 2, 33
        assert model.plan(rig.n, rig.q, lvl, n)["groups"] == 1
        Q = model.product(rig.q)
        c = Q // 2 - (Q >> 20)
        pos, neg = model.constant_ct(rig.o, lvl, c, c), model.constant_ct(rig.o, lvl, -c, -c)
        hP, hN = np.stack([pos, pos]), np.stack([neg, pos])
        dP, dN = rig.ctx.upload(hP), rig.ctx.upload(hN)
        for name, hB, dB in (("++", hP, dP), ("+-", hN, dN)):
            got = check_against_model(rig, lvl, [hP] * n, [hB] * n, [dP] * n, [dB] * n, batch, 0, what=name)
            rig.ctx.set_bfv_dot_chunk(MAX_TERMS)
            try:
                assert np.array_equal(dot(rig, lvl, [dP] * n, [dB] * n, batch), got), ("16 pairs per launch", name)
            finally:
                rig.ctx.set_bfv_dot_chunk(0)
    finally:
        rig.close()


def test_shared_operands_squares_and_chunk_sizes():
    """stride 0 on the b side (one ciphertext for the whole batch, extended once) against the same call on widened copies and the
    model; as[i] == bs[i]; every chunk size gives the same words"""
    need_gpu()
    P = params.BFV_DEFAULT[8192]
    rig = Rig(1 << 12, P["q"], P["p"], P["t"], 2, 1204)
    ctx = rig.ctx
    try:
        lvl, batch, n = 2, 3, 4
        hA, hW = [rig.ct(lvl, batch) for _ in range(n)], [rig.ct(lvl, 1) for _ in range(n)]
        dA, dW = [ctx.upload(x) for x in hA], [ctx.upload(x) for x in hW]
        hWide = [np.repeat(x, batch, axis=0) for x in hW]
        dWide = [ctx.upload(x) for x in hWide]
        want = check_against_model(rig, lvl, hA, hWide, dA, dWide, batch, 2, what="widened")
        for tile in (0, 2):
            ctx.set_tile_batch(tile)
            assert np.array_equal(dot(rig, lvl, dA, dW, batch, sbs=[0] * n), want), ("stride 0 on b", tile)
            assert np.array_equal(dot(rig, lvl, dW, dA, batch, sas=[0] * n), dot(rig, lvl, dWide, dA, batch)), ("stride 0 on a", tile)
        ctx.set_tile_batch(0)
        sq = check_against_model(rig, lvl, hA, hA, dA, dA, batch, 0, what="squares")
        copies = [ctx.upload(x) for x in hA]                          # the same words from other pointers: extended twice
        assert np.array_equal(dot(rig, lvl, dA, copies, batch), sq)
        for g in (1, 2, 3, MAX_TERMS, MAX_TERMS + 5):
            ctx.set_bfv_dot_chunk(g)
            assert np.array_equal(dot(rig, lvl, dA, dWide, batch), want), ("chunk", g)
        ctx.set_bfv_dot_chunk(0)
    finally:
        rig.close()


@pytest.mark.parametrize("mode", ["LSA_BFV_FOLD=0", "fp64_off"])
def test_switches(mode):
    """the unfolded extension and tail (LSA_BFV_FOLD=0, read per call) and a context with lsa_set_fp64_ntt(0) give the same
    words.  This chain (54 / 55-bit Q, 55-bit P, 61-bit auxiliary primes) has no FP64-engine limb, so fp64_off runs the integer
    engine on every row as the default does: it shows that the setting itself changes nothing.  The comparison of the two engines
    lives in tests/test_gpu_bfv_operator_chains.py (test_dot_variants on the fp and mixed chains)."""
    need_gpu()
    P = params.BFV_DEFAULT[8192]
    n, lvl, batch, terms = 1 << 12, 1, 2, 5    # level 1, five terms: M(5) = M(1) + 1
    base = Rig(n, P["q"], P["p"], P["t"], 2, 77)
    hA, hB, hE = [base.ct(lvl, batch) for _ in range(terms)], [base.ct(lvl, batch) for _ in range(terms)], base.ct(lvl, batch)
    try:
        dA, dB, dE = [base.ctx.upload(x) for x in hA], [base.ctx.upload(x) for x in hB], base.ctx.upload(hE)
        ref = check_against_model(base, lvl, hA, hB, dA, dB, batch, 1, hE, dE, "default")
        ref3 = mult_sum(base, lvl, dA, dB, batch, dE)
    finally:
        base.close()
    rig = Rig(n, P["q"], P["p"], P["t"], 2, 77, fp64=mode != "fp64_off")   # the same seed: the same key
    try:
        assert np.array_equal(rig.key, base.key)
        dA, dB, dE = [rig.ctx.upload(x) for x in hA], [rig.ctx.upload(x) for x in hB], rig.ctx.upload(hE)
        with env(LSA_BFV_FOLD="0" if mode == "LSA_BFV_FOLD=0" else None):
            assert np.array_equal(dot(rig, lvl, dA, dB, batch, dE), ref), mode
            assert np.array_equal(mult_sum(rig, lvl, dA, dB, batch, dE), ref3), mode
    finally:
        rig.close()


def test_unfolded_groups_on_the_tight_chain():
    """LSA_BFV_FOLD=0 where later groups are scaled down into the workspace and added: the same words as the folded form"""
    need_gpu()
    n = 1 << 12
    q = params.ntt_primes_below(57, n, 2) + params.ntt_primes_below(56, n, 1)
    rig = Rig(n, q, params.ntt_primes_below(58, n, 1), 65537, 2, 1205)
    try:
        lvl, batch = 2, 2
        hA, hB = [rig.ct(lvl, batch) for _ in range(3)], [rig.ct(lvl, batch) for _ in range(3)]
        dA, dB = [rig.ctx.upload(x) for x in hA], [rig.ctx.upload(x) for x in hB]
        ref = check_against_model(rig, lvl, hA, hB, dA, dB, batch, 0, what="folded")
        with env(LSA_BFV_FOLD="0"):
            assert np.array_equal(dot(rig, lvl, dA, dB, batch), ref)
    finally:
        rig.close()


def test_argument_errors():
    """every argument error returns LSA_ERR_ARG with a message that begins "bfv_dot", queues nothing (the output keeps its
    sentinel), and leaves the context usable"""
    need_gpu()
    from lattisense_amd._native import lib
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    P = params.BFV_DEFAULT[8192]
    rig = Rig(1 << 12, P["q"], P["p"], P["t"], 2, 1206)
    ctx, N = rig.ctx, rig.n
    try:
        lvl, batch, n = 2, 2, 2
        L = lvl + 1
        w, w3 = 2 * L * N, 3 * L * N
        hA, hB = [rig.ct(lvl, batch) for _ in range(n)], [rig.ct(lvl, batch) for _ in range(n)]
        dA, dB, dE = [ctx.upload(x) for x in hA], [ctx.upload(x) for x in hB], ctx.upload(rig.ct(lvl, batch))
        ref = dot(rig, lvl, dA, dB, batch, dE)
        out = ctx.upload(np.full(batch * w3 + 2, 7, dtype=np.uint64))   # large enough for either entry point
        pa, pb = [x.ptr for x in dA], [x.ptr for x in dB]
        low_key = ctx.upload_key(rand_ct(rig.rng, rig.q[:2] + rig.p, 2, N, 2), 1)

        def call(which, c=ctx, level=lvl, a=pa, sa=(w, w), b=pb, sb=(w, w), e=dE.ptr, se=w, o=out.ptr, bt=batch, so=None, key=rig.k,
                 drop_arrays=()):
            nn = len(a)
            A = None if "as" in drop_arrays else _arr(ctypes.c_void_p, list(a))
            SA = None if "sas" in drop_arrays else _arr(ctypes.c_longlong, list(sa))
            B = None if "bs" in drop_arrays else _arr(ctypes.c_void_p, list(b))
            SB = None if "sbs" in drop_arrays else _arr(ctypes.c_longlong, list(sb))
            if which == "dot":
                rc = lib().lsa_bfv_dot(c.h, level, nn, A, SA, B, SB, e, se, key, o, bt, so if so is not None else 2 * (level + 1) * N, ctx.stream)
            else:
                rc = lib().lsa_bfv_mult_sum(c.h, level, nn, A, SA, B, SB, e, se, o, bt, so if so is not None else 3 * (level + 1) * N, ctx.stream)
            return rc, lib().lsa_last_error().decode()

        def fails(needle="", only=None, **kw):
            for which in ("dot", "sum"):
                if only and which != only:
                    continue
                rc, msg = call(which, **kw)
                assert rc == LSA_ERR_ARG, (which, kw, rc, msg)
                assert msg.startswith("bfv_dot") and needle in msg, (which, kw, msg)

        C = params.CKKS_DEFAULT[16384]
        ckks = DeviceContext(ALGO_CKKS, 4096, C["q"][:3], C["p"])
        fails("BFV", c=ckks, level=0)
        ckks.close()
        fails("term", a=[], b=[], sa=[], sb=[])                        # n < 1
        fails("level", level=3)
        fails("level", level=-1)
        fails("null", a=(pa[0], None))
        fails("null", b=(None, pb[1]))
        fails("null", drop_arrays=("as",))
        fails("null", drop_arrays=("sbs",))
        fails("null", o=None)
        fails("stride", sa=(w - 2, w))                                  # short
        fails("stride", sb=(w, -w))                                     # negative
        fails("stride", se=w - 2)
        fails("stride", so=2)                                           # short output stride
        fails("stride", so=0)                                           # an output is never shared
        fails("even", sa=(w + 1, w))                                    # odd
        fails("even", se=w + 1)
        fails("aligned", o=out.ptr + 8)                                 # off the 16-byte grid
        fails("aligned", a=(pa[0] + 8, pa[1]))
        fails("key", only="dot", key=None)                              # missing
        fails("key", only="dot", key=low_key)                           # exported below the level
        fails("overlap", o=pa[1])
        fails("overlap", o=pb[0] + 8 * N)
        fails("overlap", o=dE.ptr)
        fails("overlap", o=pb[0], sb=(0, w))                            # a shared operand is still an input
        assert np.all(ctx.download(out, (batch * w3 + 2,)) == 7)         # nothing was queued
        for which in ("dot", "sum"):                                    # batch <= 0: a no-op
            for bt in (0, -1):
                rc, msg = call(which, bt=bt)
                assert rc == 0, msg
        assert np.all(ctx.download(out, (batch * w3 + 2,)) == 7)
        assert np.array_equal(dot(rig, lvl, dA, dB, batch, dE), ref)     # the context stays usable
    finally:
        rig.close()


def test_semantics_six_encrypted_pairs():
    """N = 2^12, 6 pairs of encrypted slot vectors: the device words are the model's, they decrypt to exactly sum_i x_i y_i mod
    t, and they are not the words of the eager sum of bfv_mult_relin (six roundings, six key switches): a new operator"""
    need_gpu()
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    P = params.BFV_DEFAULT[8192]
    N, q, p, t = 1 << 12, P["q"], P["p"], P["t"]
    lvl, terms = 2, 6
    o = Oracle(N, q, p, t)
    c = Client(o, seed=12)
    rlk = c.gen_relin_key(lvl)
    rng = np.random.default_rng(12)
    xs = [rng.integers(0, t, N, dtype=np.uint64) for _ in range(terms)]
    ys = [rng.integers(0, t, N, dtype=np.uint64) for _ in range(terms)]
    A, B = [c.bfv_encrypt(x, lvl) for x in xs], [c.bfv_encrypt(y, lvl) for y in ys]
    ctx = DeviceContext(ALGO_BFV, N, q, p, t)
    try:
        k = ctx.upload_key(rlk, lvl)
        out = ctx.bfv_dot(lvl, [ctx.upload(a[None]) for a in A], [ctx.upload(b[None]) for b in B], k, 1)
        got = ctx.download(out, (1, 2, lvl + 1, N))[0]
    finally:
        ctx.close()
    assert np.array_equal(got, model.dot(o, lvl, A, B, rlk, lvl))
    eager = o.bfv_mult_relin(lvl, A[0], B[0], rlk, lvl)
    for a, b in zip(A[1:], B[1:]):
        term = o.bfv_mult_relin(lvl, a, b, rlk, lvl)
        for h in range(2):
            for j in range(lvl + 1):
                eager[h, j] = o.vec("add", j, eager[h, j], term[h, j])
    assert not np.array_equal(got, eager)
    want = sum(x.astype(object) * y.astype(object) for x, y in zip(xs, ys)) % t
    assert np.array_equal(np.asarray(c.bfv_decrypt(got)).astype(object), want)
    assert np.array_equal(np.asarray(c.bfv_decrypt(eager)).astype(object), want)
