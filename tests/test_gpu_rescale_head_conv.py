"""The merged ModDown + rescale with its head formed inside ModDown's base conversion (key_switch.hip ks_head_in_conv,
k_baseconv<.., HEAD>; lsa_set_rescale_head_in_conv: 0 never, 1 rings with N >= 2^16, 2 every ring).  The conversion reads INTT(acc_l)
(and INTT(base_l)), keeps t = (INTT(acc_l) - conv_l) * P^-1 (+ base_l) in registers and stores in_j = conv_j * P^-1 + lift_j(t); the
element-wise kernel that wrote t is gone and the forward transform of in_j has no load-side prologue.  The path changes which kernel
forms in_j, never a residue: every output is compared word for word with the same call under mode 0 and with the CPU oracle, at the
smallest shapes at which each branch exists, batch 3 in tiles of 2.

Which path ran is read from the profiler (lsa_profile_begin(ctx, 1)), per merged rescale and tile of nb items:
  element-wise kind: one launch fewer, and the bytes of that launch fewer (k_sub_mul on two rows: reads acc_l and conv_l, and base_l
    with a base, writes t): 8 N * 2 nb * (3 + base)
  base-conversion kind: the same launches; per polynomial the head form reads the k source rows, acc_l (and base_l) and writes L - 1
    rows where the plain form reads k and writes L: the bytes move by 8 N * 2 nb * base
  NTT kind: the same launches (the prologue pass becomes the plain pass; the inverse transform of base_l only moves ahead)
A gate that silently falls back shows none of this and fails; a shape that must fall back has to show none of it."""
import ctypes

import numpy as np
import pytest

from lattisense_amd import params
from tests.gpu_util import need_gpu
from tests.test_gpu_ckks_dot import oracle_dot
from tests.test_gpu_ks_tail_in_mac import CHAINS, Rig as TailRig

pytestmark = pytest.mark.gpu

PROF_NTT, PROF_BASECONV, PROF_ELEMWISE = 0, 1, 4
C16 = params.CKKS_DEFAULT[65536]
Q, P = C16["q"], C16["p"]
B16 = params.CKKS_BOOTSTRAP_65536
WIDE = {   # 60/61-bit primes (1 mod 2^17): the conversion's 128-bit accumulate
    "w": (B16["q"][:3], B16["p"][:2]),          # q_l (40 / 41 bits) <= 2 q_j for every j: one conditional subtraction
    "x": (B16["q"][:3][::-1], B16["p"][:2]),    # the same primes, the 61-bit one last: q_l > 2 q_j, the general reduction
}
DEEP = (Q[:15], P[:2])   # 14 stored targets: split over blockIdx.z


def _ct(x, i, limbs):
    """batch item i of a ciphertext array at its leading `limbs` limbs, contiguous for the oracle"""
    return np.ascontiguousarray(x[i, :, :limbs])


def tiles_of(batch, tile):
    return [min(tile, batch - b0) for b0 in range(0, batch, tile)]


def want_delta(n, batch, tile, base, rescales=1):
    """(element-wise launches, element-wise bytes, base-conversion launches, base-conversion bytes, NTT launches) of mode 2 minus mode 0"""
    nbs = tiles_of(batch, tile)
    return (-rescales * len(nbs), -rescales * sum(8 * n * 2 * nb * (3 + base) for nb in nbs), 0,
            rescales * sum(8 * n * 2 * nb * base for nb in nbs), 0)


class Rig(TailRig):
    def profiled(self, call, mode, shape, tail=None):
        """(words, profile) of call() under lsa_set_rescale_head_in_conv(mode) (None: the context's default) and, where given,
        lsa_set_ks_tail_in_mac(tail)"""
        from lattisense_amd._native import lib
        L, ctx = lib(), self.ctx
        if mode is not None:
            ctx.set_rescale_head_in_conv(mode)
        if tail is not None:
            ctx.set_ks_tail_in_mac(tail)
        assert L.lsa_profile_begin(ctx.h, 1) == 0
        try:
            out = call()
            ctx.sync()
        finally:
            assert L.lsa_profile_end(ctx.h) == 0
            ctx.set_rescale_head_in_conv(1)
            ctx.set_ks_tail_in_mac(1)
        prof = []
        for kind in (PROF_ELEMWISE, PROF_BASECONV, PROF_NTT):
            by, n = ctypes.c_double(), ctypes.c_longlong()
            assert L.lsa_profile_read(ctx.h, kind, None, ctypes.byref(by), None, ctypes.byref(n)) == 0
            prof.append((n.value, by.value))
        (en, eb), (bn, bb), (nn, _) = prof
        return ctx.download(out, shape), (en, eb, bn, bb, nn)

    def compare(self, call, shape, want, on, base, tag, mode=2, tail=None, batch=None, rescales=1, count_ntt=True):
        """mode == mode 0 == want (None: no model), and the profiler shows the head inside the conversion exactly when `on`"""
        batch = self.batch if batch is None else batch
        got, p2 = self.profiled(call, mode, shape, tail)
        old, p0 = self.profiled(call, 0, shape, tail)
        assert np.array_equal(got, old), ("differs from mode 0", tag)
        if want is not None:
            assert np.array_equal(got, want), ("differs from the oracle", tag)
        delta = tuple(a - b for a, b in zip(p2, p0))
        expect = want_delta(self.n, batch, self.tile, base, rescales) if on else (0, 0, 0, 0, 0)
        print("rescale head in conversion", tag, "mode 2" if mode == 2 else mode, p2, "mode 0", p0, "delta", delta, "expected", expect)
        if not count_ntt:   # (chunks split the transform launches by their fused operands: not counted)
            delta, expect = delta[:4], expect[:4]
        assert delta == expect, ("which path ran", tag, delta, expect)

    def hmult(self, level, on, tag, mode=2, tail=None, batch=None, count_ntt=True):
        batch = self.batch if batch is None else batch
        da, db = self.operands(level)
        self.compare(lambda: self.ctx.ckks_mult_relin_rescale(level, da, db, self.key, batch), (batch, 2, level, self.n),
                     self.oracle(level)[:batch], on, 0, tag, mode, tail, batch, count_ntt=count_ntt)


_RIGS = {}


def _rig(n, chain, seed, **kw):
    need_gpu()
    if (n, chain) not in _RIGS:
        _RIGS[(n, chain)] = Rig(n, {**CHAINS, **WIDE, "deep": DEEP}[chain], seed, **kw)
    return _RIGS[(n, chain)]


def teardown_module(module):
    for r in _RIGS.values():
        r.close()
    _RIGS.clear()


# ------------------------------------------------------------------------------------------------ N = 2^14, mode 2
@pytest.mark.parametrize("tail", [2, 0])
@pytest.mark.parametrize("chain,level", [("a", 4), ("b", 3), ("c", 4), ("a", 1)])
def test_n14_mode2(chain, level, tail):
    """(a) every limb on the FP64 engine, l a lifted digit, (b) l inside a digit, (c) integer-engine q_0 and P limbs, (a, 1) a single
    target besides l; under the tail in the key MAC (the mac_rescale sequence) and without it (the whole-transform sequence)"""
    r = _rig(1 << 14, chain, 2400 + ord(chain))
    r.hmult(level, True, (chain, level, tail), tail=tail)


@pytest.mark.parametrize("chain,level", [("w", 2), ("w", 1), ("x", 2), ("x", 1)])
def test_n14_wide_primes_generic_accumulate(chain, level):
    """60/61-bit special primes: the 128-bit accumulate; q_l <= 2 q_j everywhere (w) and q_l > 2 q_j (x at level 2: q_l has 61 bits)"""
    r = _rig(1 << 14, chain, 2400 + ord(chain))
    ql, qs = r.q[level], r.q[:level]
    assert any(ql > 2 * qj for qj in qs) == (chain == "x" and level == 2)
    assert all(p >= (1 << 58) for p in r.p)   # the 29-bit split accumulate is not taken
    r.hmult(level, True, (chain, level))


def test_n12_targets_split_over_blocks_one_pass_ring():
    """L = 15: 14 stored targets go to two blocks of seven, each converting l for itself; a one-pass ring: no fused key MAC"""
    r = _rig(1 << 12, "deep", 2412)
    r.hmult(14, True, "deep")


# ------------------------------------------------------------------------------------------------ with a base
@pytest.mark.parametrize("chain", ["a", "c"])
def test_n14_dot_with_rescale(chain):
    """ckks_dot with rescale (base_polys == 2: the summed tensor's d0, d1 are the base; INTT(base_l) runs ahead of the conversion):
    two terms, and one term whose first operand is held one level higher (rows per polynomial above the limb count)"""
    from lattisense_amd._native import check, lib
    r = _rig(1 << 14, chain, 2400 + ord(chain))
    ctx, lvl = r.ctx, r.klvl - 1
    L = lvl + 1
    hi_a, hi_b = r.operands(r.klvl)
    da, db = r.operands(lvl)
    want = np.stack([oracle_dot(r.o, lvl, [_ct(r.A, i, L), _ct(r.B, i, L)], [_ct(r.B, i, L), _ct(r.A, i, L)], r.raw, r.klvl, True)
                     for i in range(r.batch)])
    shape = (r.batch, 2, lvl, r.n)
    r.compare(lambda: ctx.ckks_dot(lvl, [da, db], [db, da], r.key, r.batch, rescale=True), shape, want, True, 1, (chain, "dot, two terms"))

    want1 = np.stack([oracle_dot(r.o, lvl, [_ct(r.A, i, L)], [_ct(r.B, i, L)], r.raw, r.klvl, True) for i in range(r.batch)])
    w_hi, w = 2 * (r.klvl + 1) * r.n, 2 * L * r.n

    def one_term_rpp():
        out = ctx.alloc(r.batch * 2 * lvl * r.n)
        arr = lambda t, v: (t * 1)(v)   # noqa: E731
        check(lib().lsa_ckks_dot(ctx.h, lvl, 1, arr(ctypes.c_void_p, hi_a.ptr), arr(ctypes.c_longlong, w_hi), arr(ctypes.c_int, r.klvl + 1),
                                 arr(ctypes.c_void_p, db.ptr), arr(ctypes.c_longlong, w), None, None, 0, r.key, out.ptr, r.batch,
                                 2 * lvl * r.n, 1, ctx.stream))
        return out
    r.compare(one_term_rpp, shape, want1, True, 1, (chain, "dot, operand at a higher level"))


@pytest.mark.parametrize("chain", ["a", "c"])
def test_n14_evaluator_product_with_an_operand_at_a_higher_level(chain):
    """a cubic in the monomial basis with four baby steps: x^2 = x * x at level l and x^3 = x^2 * x at level l - 1 with x read through
    the leading rows of the input (ckks_mult_relin_rescale_rpp, rows per polynomial above the limb count) -- two merged rescales,
    both with the head inside the conversion.  (The operator's own words are held to the CPU model by tests/test_gpu_ckks_poly.py.)"""
    from lattisense_amd.device import PolynomialPlan
    r = _rig(1 << 14, chain, 2400 + ord(chain))
    plan = PolynomialPlan(r.ctx, [0.25, 0.5, -0.125, 0.375], r.klvl, float(2 ** 45), basis="monomial", log_baby=2)
    try:
        assert plan.mults == 2 and plan.log_baby == 2, (plan.mults, plan.log_baby, plan.depth)
        dx = r.operands(r.klvl)[0]
        r.compare(lambda: plan.run(dx, r.batch, r.key), (r.batch, 2, plan.level_out + 1, r.n), None, True, 0, (chain, "evaluator"), rescales=2)
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------ variants
@pytest.mark.parametrize("variant", ["dual_stream", "chunk_1mib", "modup_lift_0", "batch_1"])
def test_n14_mode2_variants(variant):
    from lattisense_amd._native import check, lib
    r = _rig(1 << 14, "c", 2400 + ord("c"))
    ctx = r.ctx
    try:
        if variant == "dual_stream":
            check(lib().lsa_set_dual_stream(ctx.h, 1))
        elif variant == "chunk_1mib":
            ctx.set_ntt_chunk_mib(1)
        elif variant == "modup_lift_0":
            ctx.set_modup_lift(0)
        r.hmult(4, True, ("c", variant), tail=2, batch=1 if variant == "batch_1" else None, count_ntt=variant != "chunk_1mib")
    finally:
        check(lib().lsa_set_dual_stream(ctx.h, 0))
        ctx.set_ntt_chunk_mib(0)
        ctx.set_modup_lift(1)


# ------------------------------------------------------------------------------------------------ defaults and fallbacks
def test_n14_default_mode_keeps_the_parent_sequence():
    """mode 1 stops below N = 2^16 (the pinned rigs of tests/test_gpu_ks_callers.py run at N <= 2^14 under default settings)"""
    r = _rig(1 << 14, "a", 2400 + ord("a"))
    r.hmult(4, False, "default at 2^14", mode=None)


def test_n16_on_by_default_off_under_mode_0():
    need_gpu()
    r = Rig(1 << 16, (Q[0:5], P[:2]), 2416, batch=2, tile=2)
    try:
        r.hmult(4, True, "2^16 default", mode=None)
        r.hmult(4, True, "2^16 mode 2")
    finally:
        r.close()


def test_n14_fuse_tails_0_and_level_0_take_the_earlier_path():
    from lattisense_amd._native import check, lib
    r = _rig(1 << 14, "a", 2400 + ord("a"))
    try:
        check(lib().lsa_set_fuse_tails(r.ctx.h, 0))
        r.hmult(4, False, "fuse_tails=0")
    finally:
        check(lib().lsa_set_fuse_tails(r.ctx.h, 1))
    # level 0 has no rescale: the key switch of a level-0 dot (no rescale) under mode 2
    da, db = r.operands(0)
    want = np.stack([oracle_dot(r.o, 0, [_ct(r.A, i, 1)], [_ct(r.B, i, 1)], r.raw, r.klvl, False) for i in range(r.batch)])
    r.compare(lambda: r.ctx.ckks_dot(0, [da], [db], r.key, r.batch, rescale=False), (r.batch, 2, 1, r.n), want, False, 1, "level 0")


def test_mode_is_0_1_or_2():
    r = _rig(1 << 14, "a", 2400 + ord("a"))
    from lattisense_amd._native import lib
    assert lib().lsa_set_rescale_head_in_conv(r.ctx.h, 3) != 0 and lib().lsa_set_rescale_head_in_conv(r.ctx.h, -1) != 0
    r.hmult(4, False, "the refused values left the default", mode=None)
