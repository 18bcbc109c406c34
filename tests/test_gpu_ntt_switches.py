"""Parity of the transform paths that only a PROCESS or CONTEXT switch selects (lattisense_amd/csrc/switches.h: LSA_NTT_R16,
LSA_NTT_R8X3, LSA_R16_PRO; LSA_NTT_MU_A, LSA_NTT_FP_RAW), each against the CPU oracle, never against the default path.

A PROCESS switch is read once per process, so each of its values runs in a fresh child process (the form of
tests/test_gpu_hmult_fold.py::test_fused_key_mac_on_both_engines_in_a_child); the child imports the helpers of this module and
of the modules whose shapes it reuses.  If a child ends by a signal or its time limit, the remaining child tests of this file
skip: nothing more is started on a device that may have faulted.  A CONTEXT switch is read when a context is made, so those
run in this process, each in a context of its own.

What the switches reach:
  LSA_NTT_R16=0   every pass on the staged kernel k_ntt_pass, at two-pass shapes with every fused variant: plain transforms,
                  CKKS HMult+relin+rescale folded and unfolded (the fused tensor / rescale epilogues and the product prologue),
                  rotate with and without LSA_ROT_SCATTER, BFV multiply+relin, BFV ct x pt_mul (the product taken by the
                  forward transform's last store) and rotate-and-MAC
  LSA_R16_PRO=0   the eight-stage first pass with a fused prologue (N = 2^16 only) on the staged kernel
  LSA_NTT_R8X3=0  the nine-stage second pass of N = 2^17 on the staged kernel
  LSA_NTT_MU_A    every first-pass length make_ntt_plan accepts; most of them fail ntt_r16_shape_ok / ks_fused_enabled and fall
                  to the staged kernel and the stand-alone key MAC
  LSA_NTT_FP_RAW=0  FP64-engine limbs canonical between the passes; it also turns the fused key MAC off
Keys cross contexts of the two LSA_NTT_FP_RAW settings only as host arrays: a key handle belongs to the context that uploaded
it (lsa_key_upload / lsa_key_destroy take the context), so "a key uploaded under one setting, used under the other" is not an
operation the interface has; what is checked instead is that the same host key gives the oracle's result under both."""
import os
import subprocess
import sys

import numpy as np
import pytest

from lattisense_amd import params
from tests.gpu_util import env, need_gpu, rand_ct

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CHILD_DIED = []          # a child that ended by a signal or its time limit: no further child is started


def _rand(rng, mods, shape, n):
    out = np.empty((*shape, len(mods), n), dtype=np.uint64)
    for i, m in enumerate(mods):
        out[..., i, :] = rng.integers(0, m, size=(*shape, n), dtype=np.uint64)
    return out


# ------------------------------------------------------------------------------------------------ the operators, against the oracle
def ntt_parity(logn):
    """forward transform of every row against o.ntt, and the round trip: the 60/40/40/61-bit set of tests/test_gpu_ntt.py"""
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    n = 1 << logn
    B = params.CKKS_BOOTSTRAP_65536
    q, p = B["q"][:3], B["p"][:1]
    mods = q + p
    ctx = DeviceContext(ALGO_CKKS, n, q, p)
    try:
        o = Oracle(n, q, p, 0)
        rng = np.random.default_rng(logn)
        batch, polys = 3, 2
        data = rand_ct(rng, mods, polys, n, batch)
        data[0, 0, 0, :4] = [0, mods[0] - 1, 1, mods[0] - 2]
        data[1, 1] = np.array([m - 1 for m in mods], dtype=np.uint64)[:, None]      # all-max limbs: worst-case growth
        buf = ctx.upload(data)
        mod_of = list(range(len(mods)))
        ctx.ntt(buf, batch, polys * len(mods), mod_of, inverse=False)
        got = ctx.download(buf, data.shape)
        for b in range(batch):
            for pl in range(polys):
                for i in range(len(mods)):
                    assert np.array_equal(got[b, pl, i], o.ntt(i, data[b, pl, i])), ("ntt", logn, b, pl, i)
        fwd = rand_ct(rng, mods, polys, n, batch)                                    # and the inverse on its own
        buf2 = ctx.upload(fwd)
        ctx.ntt(buf2, batch, polys * len(mods), mod_of, inverse=True)
        inv = ctx.download(buf2, data.shape)
        for b, pl, i in [(0, 0, 0), (1, 1, 1), (2, 0, 2), (2, 1, 3)]:
            assert np.array_equal(inv[b, pl, i], o.intt(i, fwd[b, pl, i])), ("intt", logn, b, pl, i)
        ctx.ntt(buf, batch, polys * len(mods), mod_of, inverse=True)
        assert np.array_equal(ctx.download(buf, data.shape), data), ("round trip", logn)
    finally:
        ctx.close()


def ckks_ops(n, q, p, lvl, klvl, batch, seed, fused=None, oracle_items=None):
    """HMult+relin+rescale with the tensor product folded into the key switch and with LSA_HMULT_FOLD=0, and a rotation with
    and without LSA_ROT_SCATTER: every form against the oracle.  fused: what ctx.key_switch_fused must say (None: not asked)"""
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    rng = np.random.default_rng(seed)
    o = Oracle(n, q, p, 0)
    A = _rand(rng, q[: lvl + 1], (batch, 2), n)
    B = _rand(rng, q[: lvl + 1], (batch, 2), n)
    beta = (klvl + 1 + len(p) - 1) // len(p)
    key = _rand(rng, q[: klvl + 1] + p, (beta, 2), n)
    g = int(pow(5, 77, 2 * n))
    items = range(batch) if oracle_items is None else oracle_items
    want_mul = {b: o.ckks_mult_relin_rescale(lvl, A[b], B[b], key, klvl) for b in items}
    want_rot = {b: o.ckks_rotate(lvl, A[b], g, key, klvl) for b in items}
    ctx = DeviceContext(ALGO_CKKS, n, q, p)
    try:
        k = ctx.upload_key(key, klvl)
        if fused is not None:
            assert ctx.key_switch_fused(lvl, k) == fused, ("fused key MAC", n, lvl)
        da, db = ctx.upload(A), ctx.upload(B)
        for fold in (None, "0"):
            with env(LSA_HMULT_FOLD=fold):
                got = ctx.download(ctx.ckks_mult_relin_rescale(lvl, da, db, k, batch), (batch, 2, lvl, n))
            for b in items:
                assert np.array_equal(got[b], want_mul[b]), ("hmult", n, lvl, "fold" if fold is None else "unfolded", b)
        for scatter in (None, "0"):
            with env(LSA_ROT_SCATTER=scatter):
                got = ctx.download(ctx.ckks_rotate(lvl, da, g, k, batch), (batch, 2, lvl + 1, n))
            for b in items:
                assert np.array_equal(got[b], want_rot[b]), ("rotate", n, lvl, "scatter" if scatter is None else "permute", b)
    finally:
        ctx.close()


def ckks_small(logn, seed=0, fused=None):
    """the shape of tests/test_gpu_ab_switches.py: six 46/47-bit Q limbs, two special primes, level 4 with a level-5 key"""
    C = params.CKKS_DEFAULT[65536]
    ckks_ops(1 << logn, C["q"][:6], C["p"][:2], 4, 5, 2, 100 * logn + seed, fused=fused)


def ckks_mixed_engines(logn, seed=0):
    """the bootstrap chain's first limbs and one special prime: a 60-bit integer-engine limb, FP64-engine limbs, a 61-bit P"""
    B = params.CKKS_BOOTSTRAP_65536
    ckks_ops(1 << logn, B["q"][:4], B["p"][:2], 3, 3, 2, 200 * logn + seed)


def bfv_mult_relin(n, q, p, t, batch, seed):
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    from oracle.pyoracle import Oracle
    rng = np.random.default_rng(seed)
    o = Oracle(n, q, p, t)
    lvl = klvl = len(q) - 1
    A = _rand(rng, q, (batch, 2), n)
    B = _rand(rng, q, (batch, 2), n)
    beta = (klvl + 1 + len(p) - 1) // len(p)
    key = _rand(rng, q + p, (beta, 2), n)
    ctx = DeviceContext(ALGO_BFV, n, q, p, t)
    try:
        k = ctx.upload_key(key, klvl)
        got = ctx.download(ctx.bfv_mult_relin(lvl, ctx.upload(A), ctx.upload(B), k, batch), (batch, 2, lvl + 1, n))
        for b in range(batch):
            assert np.array_equal(got[b], o.bfv_mult_relin(lvl, A[b], B[b], key, klvl)), ("bfv mult+relin", n, b)
    finally:
        ctx.close()


def bfv_ops(n, q, p, t, seed):
    """BFV multiply+relin, ct x pt_mul (fused: the product in the forward transform's last store) and one rotate-and-MAC"""
    from tests.test_gpu_bfv_ptmul import _check_level, _ctx
    from tests.test_gpu_bfv_rotmac import _Ring, _els
    bfv_mult_relin(n, q, p, t, 2 if len(q) <= 8 else 1, seed)
    top = len(q) - 1
    ctx, o = _ctx(n, q, p, t)
    try:
        _check_level(ctx, o, top, 2 if len(q) <= 8 else 1, np.random.default_rng(seed + 1), terms=(2,))
    finally:
        ctx.close()
    els = _els(n, [1, 7], row=True)
    r = _Ring(n, q, p, t, els, seed + 2)
    try:
        r.check(top, els + [1], batch=1, tag=(n,))
    finally:
        r.close()


def r16_off():
    """the body of the LSA_NTT_R16=0 child"""
    for logn in (15, 16):
        ntt_parity(logn)
    F = params.BFV_DEFAULT[16384]
    with env(LSA_NTT_WIDE="0"):
        ckks_small(14)
        ckks_mixed_engines(14)
        bfv_ops(1 << 14, F["q"], F["p"], F["t"], 1400)
    ckks_small(16)
    ckks_mixed_engines(16)
    C = params.bfv_n16_chain()
    bfv_ops(C["n"], C["q"], C["p"], C["t"], 1600)


def r16_pro_off():
    """the body of the LSA_R16_PRO=0 child: N = 2^16 is the only ring whose first pass has eight stages and takes the prologue"""
    ntt_parity(16)
    ckks_small(16, seed=1)
    ckks_mixed_engines(16, seed=1)


def r8x3_off():
    """the body of the LSA_NTT_R8X3=0 child: N = 2^17 on params.ckks_n17_chain(), one HMult sized like
    tests/test_gpu_ckks.py::test_n17_deep_chain_hmult_bit_exact plus a rotation, and the plain transforms on its limbs"""
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    C = params.ckks_n17_chain()
    n, q, p = C["n"], C["q"], C["p"]
    mods = [q[0], q[1], q[len(q) - 1], p[0]]
    idx = [0, 1, len(q) - 1, len(q)]
    ctx = DeviceContext(ALGO_CKKS, n, q, p)
    try:
        o = Oracle(n, q, p, 0)
        rng = np.random.default_rng(17)
        data = rand_ct(rng, mods, 1, n, 2)
        buf = ctx.upload(data)
        ctx.ntt(buf, 2, len(mods), idx, inverse=False)
        got = ctx.download(buf, data.shape)
        for b in range(2):
            for i, j in enumerate(idx):
                assert np.array_equal(got[b, 0, i], o.ntt(j, data[b, 0, i])), ("ntt", b, j)
        ctx.ntt(buf, 2, len(mods), idx, inverse=True)
        assert np.array_equal(ctx.download(buf, data.shape), data)
    finally:
        ctx.close()
    ckks_ops(n, q, p, len(q) - 1, len(q) - 1, 1, 1717)


# ------------------------------------------------------------------------------------------------ PROCESS switches: one child each
def _child(body, timeout, **switches):
    if _CHILD_DIED:
        pytest.skip("an earlier child of this file ended by %s: no more GPU work is started" % _CHILD_DIED[0])
    code = "from tests import test_gpu_ntt_switches as t; t.%s()" % body
    try:
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, **switches), capture_output=True, text=True,
                           timeout=timeout)
    except subprocess.TimeoutExpired as e:
        _CHILD_DIED.append("its time limit")
        pytest.fail("%s under %s did not end in %d s\n%s" % (body, switches, timeout, str(e.stderr or "")[-4000:]))
    if r.returncode < 0:
        _CHILD_DIED.append("signal %d" % -r.returncode)
    assert r.returncode == 0, "%s under %s: exit %d\n%s%s" % (body, switches, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_staged_kernel_on_every_pass_in_a_child():
    need_gpu()
    _child("r16_off", 1500, LSA_NTT_R16="0")


def test_fused_prologue_on_the_staged_kernel_in_a_child():
    need_gpu()
    _child("r16_pro_off", 900, LSA_R16_PRO="0")


def test_nine_stage_second_pass_on_the_staged_kernel_in_a_child():
    need_gpu()
    _child("r8x3_off", 900, LSA_NTT_R8X3="0")


# ------------------------------------------------------------------------------------------------ CONTEXT switches: in this process
TAU = 12          # LSA_NTT_TAU (build_flags.h): a pass works on 2^12 elements


def accepted_mu_a(logn):
    """the documented rule of make_ntt_plan (ntt_plan.h): an override counts when 1 <= mu_a <= TAU - 4 and the second pass still
    fits, log N - mu_a <= TAU; tests/test_switches_host.py holds this rule to the header"""
    return [m for m in range(1, 17) if m <= TAU - 4 and logn - m <= TAU]


@pytest.mark.parametrize("logn", [14, 15, 16])
def test_every_first_pass_length(logn):
    """LSA_NTT_MU_A over every accepted value (the default is min(log N / 2, 8)): transforms of every limb, HMult+relin+rescale
    and a rotation.  The fused second pass + key MAC exists for MU = 7, 8 (and 9) second passes on a radix-16-squared shape:
    ctx.key_switch_fused must say so, which also shows that the override reached the plan (an ignored one would leave the
    default plan, fused at every value)."""
    need_gpu()
    accepted = accepted_mu_a(logn)
    assert accepted == {14: [2, 3, 4, 5, 6, 7, 8], 15: [3, 4, 5, 6, 7, 8], 16: [4, 5, 6, 7, 8]}[logn]
    default = min(logn // 2, TAU - 4)
    unfused = 0
    for mu_a in accepted:
        with env(LSA_NTT_MU_A=str(mu_a), LSA_NTT_WIDE="0" if logn == 14 else None):
            ntt_parity(logn)
            if mu_a == default:
                ckks_small(logn, seed=mu_a, fused=True)
            else:
                unfused += _mu_a_case(logn, mu_a)
    assert unfused > 0          # some plan left the fused kernel: the override is not ignored


def _mu_a_case(logn, mu_a):
    """the operators under a non-default first-pass length; returns 1 if the plan no longer takes the fused key MAC"""
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    C = params.CKKS_DEFAULT[65536]
    n, q, p = 1 << logn, C["q"][:6], C["p"][:2]
    ctx = DeviceContext(ALGO_CKKS, n, q, p)
    try:
        rng = np.random.default_rng(mu_a)
        k = ctx.upload_key(_rand(rng, q + p, (3, 2), n), 5)
        fused = ctx.key_switch_fused(4, k)
    finally:
        ctx.close()
    mu_b = logn - mu_a
    if mu_b not in (7, 8, 9):
        assert not fused, (logn, mu_a)
    ckks_small(logn, seed=mu_a, fused=fused)
    return 0 if fused else 1


@pytest.mark.parametrize("logn", [14, 16])
def test_canonical_words_between_the_passes(logn):
    """LSA_NTT_FP_RAW=0: ks_fused_enabled is false (`!c.fp_raw`), so the stand-alone key MAC runs; the same host key under the
    default afterwards (see the module docstring on keys and contexts)"""
    need_gpu()
    wide = "0" if logn == 14 else None
    for raw in ("0", None):
        with env(LSA_NTT_FP_RAW=raw, LSA_NTT_WIDE=wide):
            ntt_parity(logn)
            ckks_small(logn, seed=7, fused=raw is None)          # the same seed: the same key and operands under both settings
            ckks_mixed_engines(logn, seed=7)
