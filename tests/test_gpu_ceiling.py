"""GPU parity at the 61-bit modulus ceiling: every ciphertext limb a prime with 8 (q - 1)^2 < q 2^64 < 9 (q - 1)^2
(tests/boundary.py ceiling_chain), the long sums on operands at the top of the range.

A  lsa_ckks_mac_plain (k_mac_plain) and B  lsa_ckks_mult_sum / lsa_ckks_dot (k_tensor_sum) against exact Python integers per
coefficient -- sum of products (+ addend) mod q, not a composition of oracle calls -- at term counts on both sides of every fold
and of the launch bound; the operands are the arrays tests/test_ceiling_inputs.py shows to discriminate.  C  the key switch
(k_ks_mac: eight register-resident digits at L = 8, the streaming loop and its fold at L = 9, 10, a short last digit at np = 2)
with a top-of-range key.  D  the rescale head and the three steps on a chain that alternates ceiling primes with small ones.
E  the transforms on 16 ceiling primes.  F  BFV with ceiling Q and P.  C to F compare with the CPU oracle.  Every comparison
is word for word.

What these cases can and cannot see (tests/test_ceiling_inputs.py has the arithmetic): k_mac_plain and k_tensor_sum finish with
a Montgomery multiply by 2^128 mod q that canonicalises any 64-bit word, and k_ks_mac joins its segments with add_mod onto a
zero accumulator -- a second conditional subtraction.  A fold moved from every 8th to every 16th term leaves non-canonical
intermediates that those tails absorb at every shape here (16 terms per launch, at most 10 digits): by that model the stored
words stay right and these tests pass with the fold moved; they pin the results at the ceiling, not the position of the folds.

All Q limbs here are integer-engine limbs, so by default no key switch takes the fused second pass + key MAC kernel
(LSA_KS_FUSED_ENGINES = 2: FP64-engine limbs only); that is read back and asserted, and a child process with
LSA_KS_FUSED_ENGINES=3 runs the fused kernel on them and asserts that the two paths differ."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from lattisense_amd import params
from tests.boundary import (CEILING_LOGN, CEILING_SLOTS, DOT_TERMS, MAC_TERMS, PATTERNS, ceiling_chain, ceiling_dot_operands,
                            ceiling_mac_operands, dot_term, is_ceiling, mac_term, pattern_ct, pattern_key)
from tests.gpu_util import env, need_gpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = len(CEILING_SLOTS)
PAD = 6                          # words behind every output item (even: 16-byte alignment holds)
SENT = 0xABCDEF0123456789        # no residue: every modulus is below 2^61


def obj(a):
    return np.asarray(a).astype(object)


def _mod(total, q):
    """[...][L][N] Python integers -> canonical residues per limb"""
    qv = np.array([int(m) for m in q[: total.shape[-2]]], dtype=object)[:, None]
    return (total % qv).astype(np.uint64)


def _padded(ctx, batch, words):
    so = words + PAD
    return ctx.upload(np.full(batch * so, SENT, dtype=np.uint64)), so


def _fetch(ctx, buf, so, shape):
    a = ctx.download(buf, (shape[0], so))
    w = int(np.prod(shape[1:]))
    assert np.all(a[:, w:] == SENT), "the padding behind an output item was written"
    return a[:, :w].reshape(shape)


def _diff(got, want):
    return np.argwhere((got != want).any(axis=-1))[:8]


# ---------------------------------------------------------------- A: k_mac_plain

class MacRig:
    """per ring: context, oracle, the operands of tests/boundary.py at levels top and 1, and the integer products per
    (ciphertext, plaintext, shared) -- made once, never written"""

    def __init__(self, logn):
        from lattisense_amd.device import ALGO_CKKS, DeviceContext
        from oracle.pyoracle import Oracle
        self.N = 1 << logn
        C, self.cts, self.pts, self.addend = ceiling_mac_operands(logn)
        self.q, self.p = C["q"], C["p"]
        self.o = Oracle(self.N, self.q, self.p, 0)
        self.ctx = DeviceContext(ALGO_CKKS, self.N, self.q, self.p)
        self.dev = {}
        for lvl in (3, 1):
            cut = lambda x, ax: np.ascontiguousarray(np.take(x, range(lvl + 1), axis=ax))   # noqa: E731
            self.dev[lvl] = ([self.ctx.upload(cut(x, 2)) for x in self.cts], [self.ctx.upload(cut(x, 1)) for x in self.pts],
                             self.ctx.upload(cut(self.addend, 2)))
        self.prod = {}

    def product(self, key):
        if key not in self.prod:
            ci, pi, shared = key
            pt = self.pts[pi][:1] if shared else self.pts[pi]
            self.prod[key] = obj(self.cts[ci]) * obj(pt)[:, None]
        return self.prod[key]

    def want(self, n, lvl, addend):
        total = sum(self.product(mac_term(i)) for i in range(n))
        if addend:
            total = total + obj(self.addend)
        return _mod(total[:, :, : lvl + 1], self.q)


_MAC = {}


def _mac_rig(logn):
    if logn not in _MAC:
        _MAC[logn] = MacRig(logn)
    return _MAC[logn]


@pytest.mark.parametrize("n", MAC_TERMS)
def test_a_mac_plain_long_sums(n):
    need_gpu()
    from lattisense_amd._native import check, lib
    rig = _mac_rig(CEILING_LOGN[n])
    ctx, N = rig.ctx, rig.N
    for lvl in (3, 1):
        L = lvl + 1
        dct, dpt, dadd = rig.dev[lvl]
        terms = [mac_term(i) for i in range(n)]
        pc = (ctypes.c_void_p * n)(*[dct[ci].ptr for ci, _, _ in terms])
        sc = (ctypes.c_longlong * n)(*([2 * L * N] * n))
        pp = (ctypes.c_void_p * n)(*[dpt[pi].ptr for _, pi, _ in terms])
        sp = (ctypes.c_longlong * n)(*[0 if shared else L * N for _, _, shared in terms])
        for addend, rescale in ((True, 0), (True, 1), (False, 0), (False, 1)):
            rows = lvl if rescale else L
            out, so = _padded(ctx, BATCH, 2 * rows * N)
            check(lib().lsa_ckks_mac_plain(ctx.h, lvl, n, pc, sc, pp, sp, dadd.ptr if addend else None, 2 * L * N, out.ptr, so, BATCH,
                                           rescale, ctx.stream))
            got = _fetch(ctx, out, so, (BATCH, 2, rows, N))
            want = rig.want(n, lvl, addend)
            if rescale:
                want = np.stack([rig.o.ckks_rescale(lvl, want[b]) for b in range(BATCH)])
            assert np.array_equal(got, want), (n, lvl, addend, rescale, _diff(got, want))


def test_a_mult_plain_and_addsub_plain_on_max_and_half():
    need_gpu()
    rig = _mac_rig(13)
    ctx, N, q = rig.ctx, rig.N, rig.q
    rng = np.random.default_rng(61)
    names_ct, names_pt = ("max", "half", "half"), ("max", "max", "half")
    for lvl in (3, 1):
        L = lvl + 1
        ct, pt = pattern_ct(names_ct, q[:L], 2, N, rng), pattern_ct(names_pt, q[:L], 1, N, rng)[:, 0]
        dct, dpt = ctx.upload(ct), ctx.upload(pt)
        want = _mod(obj(ct) * obj(pt)[:, None], q)
        for rescale in (False, True):
            rows = lvl if rescale else L
            got = ctx.download(ctx.ckks_mult_plain(lvl, dct, dpt, BATCH, rescale=rescale), (BATCH, 2, rows, N))
            w = np.stack([rig.o.ckks_rescale(lvl, want[b]) for b in range(BATCH)]) if rescale else want
            assert np.array_equal(got, w), ("mult_plain", lvl, rescale, _diff(got, w))
        for op in (0, 1):
            want = obj(ct).copy()
            want[:, 0] = want[:, 0] + obj(pt) if op == 0 else want[:, 0] - obj(pt)
            want = _mod(want, q)
            got = ctx.download(ctx.ckks_addsub_plain(op, lvl, dct, dpt, BATCH), (BATCH, 2, L, N))
            assert np.array_equal(got, want), ("addsub_plain", op, lvl, _diff(got, want))


# ---------------------------------------------------------------- B: k_tensor_sum

class DotRig:
    def __init__(self, logn):
        from lattisense_amd.device import ALGO_CKKS, DeviceContext
        from oracle.pyoracle import Oracle
        self.N = 1 << logn
        C, self.As, self.Bs, self.addend = ceiling_dot_operands(logn)
        self.q, self.p = C["q"], C["p"]
        self.o = Oracle(self.N, self.q, self.p, 0)
        self.ctx = DeviceContext(ALGO_CKKS, self.N, self.q, self.p)
        self.key = pattern_key("top", self.q + self.p, 4, self.N, np.random.default_rng(6300 + logn))
        self.k = self.ctx.upload_key(self.key, 3)
        self.dA, self.dB = [self.ctx.upload(x) for x in self.As], [self.ctx.upload(x) for x in self.Bs]
        self.dB2 = [self.ctx.upload(np.ascontiguousarray(x[:, :, :3])) for x in self.Bs]      # the b side at level 2
        self.dadd, self.dadd2 = self.ctx.upload(self.addend), self.ctx.upload(np.ascontiguousarray(self.addend[:, :, :3]))
        self.tensor = {}

    def pair(self, key):
        if key not in self.tensor:
            a, b = obj(self.As[key[0]]), obj(self.Bs[key[1]])
            self.tensor[key] = np.stack([a[:, 0] * b[:, 0], a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0], a[:, 1] * b[:, 1]], axis=1)
        return self.tensor[key]

    def want(self, n, lvl, addend):
        total = sum(self.pair(dot_term(i)) for i in range(n))
        if addend:
            total = total.copy()
            total[:, :2] = total[:, :2] + obj(self.addend)
        return _mod(total[:, :, : lvl + 1], self.q)


_DOT = {}


def _dot_rig(logn):
    if logn not in _DOT:
        _DOT[logn] = DotRig(logn)
    return _DOT[logn]


def _arr(ctype, values):
    return (ctype * len(values))(*values)


@pytest.mark.parametrize("n", DOT_TERMS)
def test_b_mult_sum_and_dot_long_sums(n):
    need_gpu()
    from lattisense_amd._native import check, lib
    rig = _dot_rig(CEILING_LOGN[n])
    ctx, N, o = rig.ctx, rig.N, rig.o
    terms = [dot_term(i) for i in range(n)]
    # lvl 3: every operand at its own level; lvl 2: the a side stays at level 3 and is read through its four rows per polynomial
    for lvl, dB, dadd, a_rpp in ((3, rig.dB, rig.dadd, None), (2, rig.dB2, rig.dadd2, [4] * n)):
        L = lvl + 1
        pa, pb = _arr(ctypes.c_void_p, [rig.dA[ai].ptr for ai, _ in terms]), _arr(ctypes.c_void_p, [dB[bi].ptr for _, bi in terms])
        sa, sb = _arr(ctypes.c_longlong, [2 * 4 * N] * n), _arr(ctypes.c_longlong, [2 * L * N] * n)
        ra = _arr(ctypes.c_int, a_rpp) if a_rpp else None
        for addend in (True, False):
            want = rig.want(n, lvl, addend)
            out, so = _padded(ctx, BATCH, 3 * L * N)
            check(lib().lsa_ckks_mult_sum(ctx.h, lvl, n, pa, sa, ra, pb, sb, None, dadd.ptr if addend else None, 2 * L * N, out.ptr, BATCH,
                                          so, ctx.stream))
            got = _fetch(ctx, out, so, (BATCH, 3, L, N))
            assert np.array_equal(got, want), ("mult_sum", n, lvl, addend, _diff(got, want))
            if n in (9, 17):
                relin = [o.ckks_relin(lvl, want[b], rig.key, 3) for b in range(BATCH)]
                for rescale in (0, 1):
                    rows = lvl if rescale else L
                    w = np.stack([o.ckks_rescale(lvl, r) if rescale else r for r in relin])
                    out, so = _padded(ctx, BATCH, 2 * rows * N)
                    check(lib().lsa_ckks_dot(ctx.h, lvl, n, pa, sa, ra, pb, sb, None, dadd.ptr if addend else None, 2 * L * N, rig.k,
                                             out.ptr, BATCH, so, rescale, ctx.stream))
                    got = _fetch(ctx, out, so, (BATCH, 2, rows, N))
                    assert np.array_equal(got, w), ("dot", n, lvl, addend, rescale, _diff(got, w))


# ---------------------------------------------------------------- C: the key switch on 61-bit Q

KS_SLOTS_A = ("max", "half", "top", "uniform")
KS_SLOTS_B = ("max", "top", "uniform", "half")
KS_CASES = ((1, (8, 9, 10)), (2, (9,)))


def _key_switch_cases(logn, cases, want_fused):
    """HMult+relin+rescale (LSA_HMULT_FOLD 1 / 0), mult -> relin -> rescale, rotate and rotate_many at level L - 1 with the
    top-of-range key of that level, under the default switches and LSA_KS_FUSED=0, each against the oracle.  want_fused: what
    key_switch_fused must read by default (under LSA_KS_FUSED=0 it must read false)"""
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    n = 1 << logn
    nb = len(KS_SLOTS_A)
    rng = np.random.default_rng(6400 + logn)
    for np_, Ls in cases:
        C = ceiling_chain(n, max(Ls), np_)
        q, p = C["q"], C["p"]
        o = Oracle(n, q, p, 0)
        ctx = DeviceContext(ALGO_CKKS, n, q, p)
        try:
            for L in Ls:
                lvl = klvl = L - 1
                mods, beta = q[:L], (L + np_ - 1) // np_
                gs = [5, int(pow(5, 77, 2 * n))]
                keys = [pattern_key("top", mods + p, beta, n, rng) for _ in range(3)]
                hk = [ctx.upload_key(x, klvl) for x in keys]
                A, B = pattern_ct(KS_SLOTS_A, mods, 2, n, rng), pattern_ct(KS_SLOTS_B, mods, 2, n, rng)
                da, db = ctx.upload(A), ctx.upload(B)
                want_mul = np.stack([o.ckks_mult_relin_rescale(lvl, A[b], B[b], keys[0], klvl) for b in range(nb)])
                want_rot = [np.stack([o.ckks_rotate(lvl, A[b], g, keys[1 + i], klvl) for b in range(nb)]) for i, g in enumerate(gs)]
                assert ctx.key_switch_fused(lvl, hk[0]) == want_fused, (np_, L, "the path a 61-bit chain takes by default")
                for fused in (None, "0"):
                    with env(LSA_KS_FUSED=fused):
                        tag = (logn, np_, L, "LSA_KS_FUSED=%s" % fused)
                        if fused == "0":
                            assert not ctx.key_switch_fused(lvl, hk[0]), tag
                        for fold in (None, "0"):
                            with env(LSA_HMULT_FOLD=fold):
                                got = ctx.download(ctx.ckks_mult_relin_rescale(lvl, da, db, hk[0], nb), want_mul.shape)
                            assert np.array_equal(got, want_mul), tag + ("hmult, fold=%s" % fold, _diff(got, want_mul))
                        d3 = ctx.ckks_mult(lvl, da, db, nb)
                        got = ctx.download(ctx.ckks_rescale(lvl, 2, ctx.ckks_relin(lvl, d3, hk[0], nb), nb), want_mul.shape)
                        assert np.array_equal(got, want_mul), tag + ("three steps", _diff(got, want_mul))
                        outs = ctx.ckks_rotate_many(lvl, da, {g: hk[1 + i] for i, g in enumerate(gs)}, nb)
                        for i, g in enumerate(gs):
                            got = ctx.download(ctx.ckks_rotate(lvl, da, g, hk[1 + i], nb), want_rot[i].shape)
                            assert np.array_equal(got, want_rot[i]), tag + ("rotate", g, _diff(got, want_rot[i]))
                            got = ctx.download(outs[g], want_rot[i].shape)
                            assert np.array_equal(got, want_rot[i]), tag + ("rotate_many", g, _diff(got, want_rot[i]))
                for k in hk:
                    ctx.destroy_key(k)
        finally:
            ctx.close()


@pytest.mark.parametrize("logn", [12, 13])
def test_c_key_switch_on_ceiling_limbs(logn):
    """every target limb is an integer-engine limb: the unfused k_ks_mac runs under both settings (asserted)"""
    need_gpu()
    _key_switch_cases(logn, KS_CASES, False)


def test_c_key_switch_fused_on_ceiling_limbs_in_a_child():
    """LSA_KS_FUSED_ENGINES=3 (read once per process) at N = 2^13: the fused kernel takes the 61-bit limbs by default and
    LSA_KS_FUSED=0 does not, so the two runs compared with the oracle are two paths"""
    need_gpu()
    code = "from tests.test_gpu_ceiling import _key_switch_cases, KS_CASES; _key_switch_cases(13, KS_CASES, True)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, LSA_KS_FUSED_ENGINES="3"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------- D: rescale head and three steps on the mixed chain

def test_d_rescale_and_three_steps_on_the_mixed_chain():
    """every level >= 1 of ceiling_mixed_chain at N = 2^13: ckks_rescale on pattern coefficients, mult -> relin -> rescale and
    the fused operator, fused tails 0 / 1, both engines (tests/test_gpu_boundary.py _ckks_levels)"""
    need_gpu()
    from tests.boundary import ceiling_mixed_chain
    from tests.test_gpu_boundary import _ckks_levels
    C = ceiling_mixed_chain(1 << 13, 2)
    _ckks_levels(1 << 13, "interleaved", range(1, len(C["q"])), 6113, tiles=(1,), chain=C)


# ---------------------------------------------------------------- E: transforms

@pytest.mark.parametrize("logn", [12, 13, 16])
def test_e_transforms_on_ceiling_primes(logn):
    """forward, inverse and round trip of all nine patterns on 16 ceiling primes as Q rows"""
    need_gpu()
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    n = 1 << logn
    C = ceiling_chain(n, 16, 1)
    q, p = C["q"], C["p"]
    o = Oracle(n, q, p, 0)
    rng = np.random.default_rng(6500 + logn)
    data = pattern_ct(PATTERNS, q, 1, n, rng)                              # [9][1][16][N]
    want_f = np.stack([np.stack([o.ntt(i, data[b, 0, i]) for i in range(16)]) for b in range(len(PATTERNS))])[:, None]
    want_i = np.stack([np.stack([o.intt(i, data[b, 0, i]) for i in range(16)]) for b in range(len(PATTERNS))])[:, None]
    mod_of = list(range(16))
    ctx = DeviceContext(ALGO_CKKS, n, q, p)
    try:
        for b0 in range(0, len(PATTERNS), 3):
            sl = slice(b0, b0 + 3)
            buf = ctx.upload(data[sl])
            ctx.ntt(buf, 3, 16, mod_of, inverse=False)
            got = ctx.download(buf, data[sl].shape)
            assert np.array_equal(got, want_f[sl]), (PATTERNS[sl], _diff(got, want_f[sl]))
            ctx.ntt(buf, 3, 16, mod_of, inverse=True)
            assert np.array_equal(ctx.download(buf, data[sl].shape), data[sl]), (PATTERNS[sl], "round trip")
            buf = ctx.upload(data[sl])
            ctx.ntt(buf, 3, 16, mod_of, inverse=True)
            got = ctx.download(buf, data[sl].shape)
            assert np.array_equal(got, want_i[sl]), ("inverse", PATTERNS[sl], _diff(got, want_i[sl]))
    finally:
        ctx.close()


# ---------------------------------------------------------------- F: BFV

def test_f_bfv_on_ceiling_limbs():
    """five ceiling Q primes and two P primes at N = 2^13; the auxiliary base of the multiply is the next 61-bit primes, also
    at the ceiling; no conversion runs the 29-bit split"""
    need_gpu()
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    from oracle.pyoracle import Oracle
    from tests.test_gpu_bfv_ptmul import _want_mac
    n, t = 1 << 13, 65537
    C = ceiling_chain(n, 5, 2)
    q, p = C["q"], C["p"]
    o = Oracle(n, q, p, t)
    assert not set(o.aux) & set(q + p) and o.aux == params.ntt_primes_below(61, n, len(o.aux), avoid=q + p)
    assert all(is_ceiling(m) for m in o.aux)
    rng = np.random.default_rng(6600)
    L = len(q)
    lvl = klvl = L - 1
    names = ("top", "max", "uniform")
    beta = (L + len(p) - 1) // len(p)
    key, gkey = pattern_key("top", q + p, beta, n, rng), pattern_key("max", q + p, beta, n, rng)
    g = 5
    A, B = pattern_ct(names, q, 2, n, rng), pattern_ct(("max", "uniform", "top"), q, 2, n, rng)
    pts = [pattern_ct(names, q, 1, n, rng)[:, 0], pattern_ct(("max", "top", "uniform"), q, 1, n, rng)[:, 0]]
    want_mul = np.stack([o.bfv_mult_relin(lvl, A[b], B[b], key, klvl) for b in range(3)])
    want_rot = np.stack([o.bfv_rotate(lvl, A[b], g, gkey, klvl) for b in range(3)])
    want_mac = np.stack([_want_mac(o, L, [A[b], B[b]], [pts[0][b], pts[1][b]]) for b in range(3)])
    ctx = DeviceContext(ALGO_BFV, n, q, p, t)
    try:
        assert ctx.moduli == o.mod
        k, hg = ctx.upload_key(key, klvl), ctx.upload_key(gkey, klvl)
        da, db = ctx.upload(A), ctx.upload(B)
        got = ctx.download(ctx.bfv_mult_relin(lvl, da, db, k, 3), want_mul.shape)
        assert np.array_equal(got, want_mul), ("mult_relin", _diff(got, want_mul))
        got = ctx.download(ctx.bfv_rotate(lvl, da, g, hg, 3), want_rot.shape)
        assert np.array_equal(got, want_rot), ("rotate", _diff(got, want_rot))
        got = ctx.download(ctx.bfv_mac_plain_mul(lvl, [da, db], [ctx.upload(x) for x in pts], 3), want_mac.shape)
        assert np.array_equal(got, want_mac), ("pt_mul MAC", _diff(got, want_mac))
        plans = ctx.baseconv_plans()
        assert len(plans) >= 3 and not any(split for _, _, split in plans), plans
    finally:
        ctx.close()
