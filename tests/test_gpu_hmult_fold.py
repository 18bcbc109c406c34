"""CKKS HMult+relin+rescale with the tensor product folded into the key switch (ops.hip ckks_mult_relin_rescale_rpp, the
default with fused tails; LSA_HMULT_FOLD=0 runs k_tensor, key switch and rescale as before).  The fold changes which kernels
compute the residues, never the residues: every output is compared bit for bit with the older path in the same process
and with the CPU oracle, under the shapes and switches that select different kernels (fused / stand-alone key MAC, FP64 /
integer engine target limbs, MU = 7 / 8 / 9 second passes, tiles and streams)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from lattisense_amd import params
from tests.gpu_util import env, need_gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand(rng, mods, shape, n):
    out = np.empty((*shape, len(mods), n), dtype=np.uint64)
    for i, m in enumerate(mods):
        out[..., i, :] = rng.integers(0, m, size=(*shape, n), dtype=np.uint64)
    return out


def _hmult(ctx, lvl, da, db, k, batch, fold):
    with env(LSA_HMULT_FOLD=None if fold else "0"):
        out = ctx.ckks_mult_relin_rescale(lvl, da, db, k, batch)
        return ctx.download(out, (batch, 2, lvl, ctx.n))


def _fold_vs_old(n, q, p, levels, klvl, batch, seed, square=False, oracle_levels=(), fp64=True):
    """fold == LSA_HMULT_FOLD=0 at every level; == the oracle at `oracle_levels` (first batch item)"""
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    rng = np.random.default_rng(seed)
    ctx = DeviceContext(ALGO_CKKS, n, q, p)
    if not fp64:
        ctx.set_fp64_ntt(0)
    beta = (klvl + 1 + len(p) - 1) // len(p)
    key = _rand(rng, q[: klvl + 1] + p, (beta, 2), n)
    k = ctx.upload_key(key, klvl)
    o = None
    try:
        for lvl in levels:
            A = _rand(rng, q[: lvl + 1], (batch, 2), n)
            B = A if square else _rand(rng, q[: lvl + 1], (batch, 2), n)
            da = ctx.upload(A)
            db = da if square else ctx.upload(B)
            got = _hmult(ctx, lvl, da, db, k, batch, True)
            want = _hmult(ctx, lvl, da, db, k, batch, False)
            assert np.array_equal(got, want), ("fold differs from the older path", n, lvl)
            if lvl in oracle_levels:
                if o is None:
                    from oracle.pyoracle import Oracle
                    o = Oracle(n, q, p, 0)
                assert np.array_equal(got[0], o.ckks_mult_relin_rescale(lvl, A[0], B[0], key, klvl)), ("oracle", n, lvl)
    finally:
        ctx.close()


def test_headline_shape_tiles_streams_and_batch_positions():
    """N = 2^16, L = 13, k = 4: fold and older path under tiles 1, 5 and the default, single and dual stream; the same
    ciphertext pair at batch positions 0 and 5 gives the same output; item 0 against the oracle"""
    need_gpu()
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    C = params.CKKS_DEFAULT[65536]
    n, q, p = 1 << 16, C["q"][:13], C["p"][:4]
    lvl = klvl = 12
    batch = 7
    rng = np.random.default_rng(2016)
    A = _rand(rng, q, (batch, 2), n)
    B = _rand(rng, q, (batch, 2), n)
    A[5], B[5] = A[0], B[0]
    key = _rand(rng, q + p, (4, 2), n)
    ctx = DeviceContext(ALGO_CKKS, n, q, p)
    try:
        k = ctx.upload_key(key, klvl)
        da, db = ctx.upload(A), ctx.upload(B)
        ref = _hmult(ctx, lvl, da, db, k, batch, False)
        assert np.array_equal(ref[0], Oracle(n, q, p, 0).ckks_mult_relin_rescale(lvl, A[0], B[0], key, klvl))
        for dual in (0, 1):
            check(lib().lsa_set_dual_stream(ctx.h, dual))
            for tile in (0, 1, 5):
                ctx.set_tile_batch(tile)
                for fold in (True, False):
                    got = _hmult(ctx, lvl, da, db, k, batch, fold)
                    assert np.array_equal(got, ref), (dual, tile, fold)
                    assert np.array_equal(got[5], got[0]), (dual, tile, fold)
    finally:
        ctx.close()


def test_every_level_and_a_square_small_ring():
    need_gpu()
    C = params.CKKS_DEFAULT[65536]
    q, p = C["q"][:13], C["p"][:4]
    _fold_vs_old(1 << 13, q, p, range(1, 13), 12, 3, 13, oracle_levels=(1, 4, 12))
    _fold_vs_old(1 << 13, q, p, (6, 12), 12, 2, 14, square=True, oracle_levels=(12,))


def test_n14_mu7_second_pass():
    need_gpu()
    C = params.CKKS_DEFAULT[65536]
    _fold_vs_old(1 << 14, C["q"][:13], C["p"][:4], (3, 12), 12, 3, 1414, oracle_levels=(12,))


def test_n17_chain_mu9():
    """the 25Q+5P chain at N = 2^17: the nine-stage second pass (MU = 9) of the fused key MAC, six digits"""
    need_gpu()
    C = params.ckks_n17_chain()
    q, p = C["q"], C["p"]
    _fold_vs_old(C["n"], q, p, (len(q) - 1,), len(q) - 1, 1, 1717)


def test_integer_engine_q_limbs():
    """the bootstrap chain: its 60-bit Q limbs are integer-engine targets (the stand-alone key MAC) next to FP64 ones"""
    need_gpu()
    P = params.CKKS_BOOTSTRAP_65536
    q, p = P["q"], P["p"]
    _fold_vs_old(1 << 14, q, p, (24, 13), 24, 2, 2424, oracle_levels=(24,))


@pytest.mark.parametrize("mode", ["fp64_off", "LSA_KS_FUSED=0", "fuse_tails_off"])
def test_switches(mode, monkeypatch):
    need_gpu()
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    C = params.CKKS_DEFAULT[65536]
    n, q, p = 1 << 16, C["q"][:6], C["p"][:2]
    if mode == "LSA_KS_FUSED=0":
        monkeypatch.setenv("LSA_KS_FUSED", "0")
    lvl, klvl, batch = 5, 5, 2
    rng = np.random.default_rng(len(mode))
    A = _rand(rng, q, (batch, 2), n)
    B = _rand(rng, q, (batch, 2), n)
    key = _rand(rng, q + p, (3, 2), n)
    ctx = DeviceContext(ALGO_CKKS, n, q, p)
    try:
        if mode == "fp64_off":
            ctx.set_fp64_ntt(0)
        if mode == "fuse_tails_off":
            check(lib().lsa_set_fuse_tails(ctx.h, 0))
        k = ctx.upload_key(key, klvl)
        da, db = ctx.upload(A), ctx.upload(B)
        got = _hmult(ctx, lvl, da, db, k, batch, True)
        assert np.array_equal(got, _hmult(ctx, lvl, da, db, k, batch, False)), mode
        assert np.array_equal(got[1], Oracle(n, q, p, 0).ckks_mult_relin_rescale(lvl, A[1], B[1], key, klvl)), mode
    finally:
        ctx.close()


def test_fused_key_mac_on_both_engines_in_a_child():
    """LSA_KS_FUSED_ENGINES is read once per process: integer-engine target limbs through the fused kernel too
    (k_ntt_r16_ksmac<MU, false>), in a fresh child process"""
    need_gpu()
    code = ("from lattisense_amd import params; from tests.test_gpu_hmult_fold import _fold_vs_old; "
            "P = params.CKKS_BOOTSTRAP_65536; _fold_vs_old(1 << 16, P['q'], P['p'], (24, 7), 24, 2, 33, oracle_levels=(7,)); "
            "C = params.CKKS_DEFAULT[65536]; _fold_vs_old(1 << 16, C['q'][:13], C['p'][:4], (12,), 12, 2, 34)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, LSA_KS_FUSED_ENGINES="3"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
