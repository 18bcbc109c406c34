"""CKKS HMult+relin+rescale with the merged rescale tail finished inside the fused key MAC (key_switch.hip KsTile::mac_rescale,
k_ntt_r16_ksmac<MU, true, true>; lsa_set_ks_tail_in_mac: 0 never, 1 where the second pass has eight stages, 2 wherever the shape
allows).  The path changes which kernel stores the rescaled FP64-engine limbs, never a residue: every output is compared bit for bit
with the CPU oracle and with the same call under mode 0, at the smallest shapes at which each branch exists, on one ciphertext
operation of a few limbs, batch 3 in tiles of 2.

Which path ran is read from the profiler (lsa_profile_begin(ctx, 1)): the sequence hands limb l = level to the stand-alone key MAC,
so that kind's algorithmic bytes grow by exactly one Q target per tile, and the NTT kind's launch count moves by the launches the
sequence changes (ntt_launch_delta below restates the rule).  A gate that silently falls back shows neither and fails; a shape that
must fall back has to show neither."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from lattisense_amd import params
from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROF_NTT, PROF_KSMAC = 0, 2
BATCH, TILE = 3, 2
C16 = params.CKKS_DEFAULT[65536]
Q, P = C16["q"], C16["p"]
CHAINS = {   # name: (q, p)
    "a": (Q[1:6], Q[6:8]),    # every limb on the FP64 engine, digits of 2, 2 and 1 limbs: l is the single-limb lifted digit
    "b": (Q[1:5], Q[6:8]),    # l sits inside a two-limb digit
    "c": (Q[0:5], P[:2]),     # an integer-engine limb 0 (the passes = 2 epilogue) and integer-engine P limbs
    "e": (Q[0:2], P[:2]),     # the only FP64-engine Q limb is l: falls back
}


def fp_engine(m):
    return m < (1 << 47)


def _rand(rng, mods, shape, n):
    out = np.empty((*shape, len(mods), n), dtype=np.uint64)
    for i, m in enumerate(mods):
        out[..., i, :] = rng.integers(0, m, size=(*shape, n), dtype=np.uint64)
    return out


def ntt_launch_delta(q, p, level):
    """NTT-kind launches of one tile under the tail sequence minus those of the parent's sequence (no chunking):
    +1 where limb l brings the stand-alone second pass of the extension transform into being: that launch covers the extension rows
       of the targets outside the fused kernel -- integer-engine limbs, and now l; a Q limb has such rows only with two digits or more
    +1 where some P limb is on the FP64 engine: the fused kernel runs once for them ahead of ModDown and once for the Q limbs
    -1 where no Q limb below l is on the integer engine: the epilogue's second pass has no row left (its first pass stays)"""
    L = level + 1
    beta = -(-L // len(p))
    targets = q[:L] + p

    def second_pass(extra):
        return any((not fp_engine(m) or tl == extra) and (tl >= L or beta > 1) for tl, m in enumerate(targets))
    return (int(second_pass(level)) - int(second_pass(None)) + int(any(fp_engine(m) for m in p)) -
            int(all(fp_engine(m) for m in q[:level])))


def ksmac_bytes_delta(n, q, p, level, batch, tile):
    """limb l as one more Q target of the stand-alone key MAC (launch_ks_mac's count with the tensor fold), per tile"""
    beta = -(-(level + 1) // len(p))
    return sum(8 * n * (nb * (beta + 2 + 3) + 2 * beta) for nb in (min(tile, batch - b0) for b0 in range(0, batch, tile)))


class Rig:
    def __init__(self, n, chain, seed, batch=BATCH, tile=TILE):
        from lattisense_amd.device import ALGO_CKKS, DeviceContext
        from oracle.pyoracle import Oracle
        self.n, (self.q, self.p) = n, CHAINS[chain] if isinstance(chain, str) else chain
        self.batch, self.tile = batch, tile
        self.klvl = len(self.q) - 1
        rng = np.random.default_rng(seed)
        beta = -(-(self.klvl + 1) // len(self.p))
        self.o = Oracle(n, self.q, self.p, 0)
        self.ctx = DeviceContext(ALGO_CKKS, n, self.q, self.p)
        self.ctx.set_tile_batch(tile)
        self.raw = _rand(rng, self.q + self.p, (beta, 2), n)
        self.key = self.ctx.upload_key(self.raw, self.klvl)
        self.A = _rand(rng, self.q, (batch, 2), n)
        self.B = _rand(rng, self.q, (batch, 2), n)
        self.dev, self.want = {}, {}

    def close(self):
        self.ctx.close()

    def operands(self, level):
        if level not in self.dev:
            L = level + 1
            self.dev[level] = (self.ctx.upload(self.A[:, :, :L]), self.ctx.upload(self.B[:, :, :L]))
        return self.dev[level]

    def oracle(self, level):
        """computed once per level and shared by every variant"""
        if level not in self.want:
            L = level + 1
            self.want[level] = np.stack([self.o.ckks_mult_relin_rescale(level, np.ascontiguousarray(self.A[i, :, :L]),
                                                                        np.ascontiguousarray(self.B[i, :, :L]), self.raw, self.klvl)
                                         for i in range(self.batch)])
            self.want[level].setflags(write=False)
        return self.want[level]

    def run(self, level, mode, batch=None):
        """(words, NTT launches, key-MAC bytes) of one call under lsa_set_ks_tail_in_mac(mode); None: the context's default"""
        from lattisense_amd._native import lib
        L, ctx = lib(), self.ctx
        batch = self.batch if batch is None else batch
        da, db = self.operands(level)
        if mode is not None:
            ctx.set_ks_tail_in_mac(mode)
        assert L.lsa_profile_begin(ctx.h, 1) == 0
        try:
            out = ctx.ckks_mult_relin_rescale(level, da, db, self.key, batch)
            ctx.sync()
        finally:
            assert L.lsa_profile_end(ctx.h) == 0
            if mode is not None:
                ctx.set_ks_tail_in_mac(1)
        by, n = ctypes.c_double(), ctypes.c_longlong()
        assert L.lsa_profile_read(ctx.h, PROF_NTT, None, None, None, ctypes.byref(n)) == 0
        assert L.lsa_profile_read(ctx.h, PROF_KSMAC, None, ctypes.byref(by), None, None) == 0
        return ctx.download(out, (batch, 2, level, self.n)), n.value, by.value

    def check(self, level, mode, on, tag, batch=None, count_launches=True):
        """mode == mode 0 == oracle, and the profiler shows the tail sequence exactly when `on`"""
        batch = self.batch if batch is None else batch
        got, launches, mac_bytes = self.run(level, mode, batch)
        old, launches0, mac_bytes0 = self.run(level, 0, batch)
        assert np.array_equal(got, old), ("differs from mode 0", tag)
        assert np.array_equal(got, self.oracle(level)[:batch]), ("differs from the oracle", tag)
        tiles = -(-batch // self.tile)
        want_bytes = ksmac_bytes_delta(self.n, self.q, self.p, level, batch, self.tile) if on else 0
        assert mac_bytes - mac_bytes0 == want_bytes, ("which path ran: key-MAC bytes", mac_bytes, mac_bytes0, want_bytes, tag)
        if count_launches:
            want_launches = tiles * ntt_launch_delta(self.q, self.p, level) if on else 0
            assert launches - launches0 == want_launches, ("which path ran: NTT launches", launches, launches0, want_launches, tag)


_RIGS = {}


def _rig(n, chain, seed):
    need_gpu()
    if (n, chain) not in _RIGS:
        _RIGS[(n, chain)] = Rig(n, chain, seed)
    return _RIGS[(n, chain)]


def teardown_module(module):
    for r in _RIGS.values():
        r.close()
    _RIGS.clear()


def test_launch_delta_rule_at_the_headline_shape():
    """the headline chain (q_0 and the four P limbs on the integer engine, twelve FP64-engine Q limbs): no launch is added"""
    assert ntt_launch_delta(Q[:13], P[:4], 12) == 0
    assert [ntt_launch_delta(*CHAINS[c], len(CHAINS[c][0]) - 1) for c in "abc"] == [1, 1, 0]
    assert ntt_launch_delta(*CHAINS["a"], 1) == 0   # one digit: l has no extension row


# ------------------------------------------------------------------------------------------------ N = 2^14, mode 2
@pytest.mark.parametrize("chain,level", [("a", 4), ("b", 3), ("c", 4), ("a", 1)])
def test_n14_mode2(chain, level):
    """(a) l the single-limb lifted digit, (b) l inside a two-limb digit, (c) integer-engine limb 0 and P limbs, (d) level 1 of (a)"""
    r = _rig(1 << 14, chain, 1400 + ord(chain))
    r.check(level, 2, True, (chain, level))


def test_n14_default_mode_keeps_the_parent_sequence():
    """mode 1: seven-stage second passes stay on the parent's sequence (the pinned rigs of tests/test_gpu_ks_callers.py)"""
    r = _rig(1 << 14, "a", 1400 + ord("a"))
    r.check(4, None, False, "default at 2^14")


def test_n14_only_fp64_q_limb_is_l_falls_back():
    """(e) q_0 on the integer engine, l = 1 the only FP64-engine Q limb"""
    r = _rig(1 << 14, "e", 1405)
    r.check(1, 2, False, "e")


@pytest.mark.parametrize("chain", ["a", "c"])
@pytest.mark.parametrize("variant", ["dual_stream", "chunk_1mib", "modup_lift_0", "batch_1"])
def test_n14_mode2_variants(chain, variant):
    from lattisense_amd._native import check, lib
    r = _rig(1 << 14, chain, 1400 + ord(chain))
    ctx, level = r.ctx, 4
    try:
        if variant == "dual_stream":
            check(lib().lsa_set_dual_stream(ctx.h, 1))
        elif variant == "chunk_1mib":
            ctx.set_ntt_chunk_mib(1)
        elif variant == "modup_lift_0":
            ctx.set_modup_lift(0)
        # (chunks split the transform launches: the launch count is checked without them)
        r.check(level, 2, True, (chain, variant), batch=1 if variant == "batch_1" else None, count_launches=variant != "chunk_1mib")
    finally:
        check(lib().lsa_set_dual_stream(ctx.h, 0))
        ctx.set_ntt_chunk_mib(0)
        ctx.set_modup_lift(1)


@pytest.mark.parametrize("chain", ["a", "c"])
def test_n14_mode2_operands_held_at_a_higher_level(chain):
    """polynomial evaluation multiplies powers kept at different levels (ckks_mult_relin_rescale_rpp: rows per polynomial above
    the limb count).  A cubic in the monomial basis with four baby steps is one leaf over the powers x, x^2 = x * x (level l) and
    x^3 = x^2 * x (level l - 1: x^2 sits there, x is read through the leading rows of the input at level l, rpp = l + 1 > L) --
    two multiplications, no other.  Mode 2 == mode 0 word for word, and the key MAC's bytes grow by exactly limb l of BOTH
    multiplications: the one with the operand at the higher level took the tail sequence too.  (The operator's own words are
    held to the CPU model by tests/test_gpu_ckks_poly.py.)"""
    from lattisense_amd._native import lib
    from lattisense_amd.device import PolynomialPlan
    r = _rig(1 << 14, chain, 1400 + ord(chain))
    L, ctx = lib(), r.ctx
    plan = PolynomialPlan(ctx, [0.25, 0.5, -0.125, 0.375], r.klvl, float(2 ** 45), basis="monomial", log_baby=2)
    try:
        assert plan.mults == 2 and plan.log_baby == 2, (plan.mults, plan.log_baby, plan.depth)
        dx = r.operands(r.klvl)[0]

        def run(mode):
            ctx.set_ks_tail_in_mac(mode)
            assert L.lsa_profile_begin(ctx.h, 1) == 0
            try:
                out = plan.run(dx, r.batch, r.key)
                ctx.sync()
            finally:
                assert L.lsa_profile_end(ctx.h) == 0
                ctx.set_ks_tail_in_mac(1)
            by = ctypes.c_double()
            assert L.lsa_profile_read(ctx.h, PROF_KSMAC, None, ctypes.byref(by), None, None) == 0
            return ctx.download(out, (r.batch, 2, plan.level_out + 1, r.n)), by.value
        got, by2 = run(2)
        old, by0 = run(0)
        assert np.array_equal(got, old)
        want = sum(ksmac_bytes_delta(r.n, r.q, r.p, lvl, r.batch, r.tile) for lvl in (r.klvl, r.klvl - 1))
        assert by2 - by0 == want, ("which path ran", by2, by0, want)
    finally:
        plan.close()


def test_n14_fuse_tails_0_falls_back():
    from lattisense_amd._native import check, lib
    r = _rig(1 << 14, "a", 1400 + ord("a"))
    try:
        check(lib().lsa_set_fuse_tails(r.ctx.h, 0))
        r.check(4, 2, False, "fuse_tails=0")
    finally:
        check(lib().lsa_set_fuse_tails(r.ctx.h, 1))


def _child_fold_off():
    """LSA_HMULT_FOLD=0 (set by the parent test for this process): the key switch has a base, the tail sequence must not run"""
    r = Rig(1 << 14, "a", 1400 + ord("a"))
    try:
        r.check(4, 2, False, "LSA_HMULT_FOLD=0")
    finally:
        r.close()


def test_n14_hmult_fold_0_falls_back_in_a_child():
    need_gpu()
    out = subprocess.run([sys.executable, "-c", "from tests.test_gpu_ks_tail_in_mac import _child_fold_off; _child_fold_off()"], cwd=ROOT,
                         env=dict(os.environ, LSA_HMULT_FOLD="0"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ N = 2^16, default mode
def test_n16_on_by_default_off_under_mode_0():
    need_gpu()
    r = Rig(1 << 16, (Q[0:5], P[:2]), 1600, batch=2, tile=2)
    try:
        r.check(4, None, True, "2^16 default")
        r.check(4, 2, True, "2^16 mode 2")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ N = 2^17
def test_n17_nine_stage_second_pass_keeps_the_parent_words():
    """the nine-stage second pass has no tail variant: mode 2 falls back"""
    need_gpu()
    C = params.ckks_n17_chain()
    r = Rig(C["n"], (C["q"][:3], C["p"]), 1700, batch=1, tile=1)
    try:
        r.check(2, 2, False, "2^17")
    finally:
        r.close()
