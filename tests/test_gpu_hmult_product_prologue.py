"""CKKS HMult+relin+rescale with d2 = a1 b1 formed by the load of the key switch's inverse transform (the product prologue,
NttPassArgs::fz_pro == 3) instead of a stand-alone kernel.  The inverse transform's first pass is the MU = 7 second pass at
N = 2^14, MU = 8 at 2^16 and the nine-stage pass at 2^17.  Outputs are compared bit for bit with the CPU oracle and with
LSA_HMULT_FOLD=0 (k_tensor, key switch, merged tail) in the same process, under tiles that split the batch unevenly."""
import numpy as np
import pytest

from lattisense_amd import params
from tests.gpu_util import need_gpu
from tests.test_gpu_hmult_fold import _hmult, _rand

pytestmark = pytest.mark.gpu


def _check(n, q, p, lvl, klvl, batch, tiles, seed, oracle_items=(0,)):
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.pyoracle import Oracle
    rng = np.random.default_rng(seed)
    L = lvl + 1
    beta = (klvl + 1 + len(p) - 1) // len(p)
    key = _rand(rng, q[: klvl + 1] + p, (beta, 2), n)
    A = _rand(rng, q[:L], (batch, 2), n)
    B = _rand(rng, q[:L], (batch, 2), n)
    A[batch - 1], B[batch - 1] = A[0], B[0]   # the same pair in the first and the last (short) tile
    ctx = DeviceContext(ALGO_CKKS, n, q, p)
    try:
        k = ctx.upload_key(key, klvl)
        da, db = ctx.upload(A), ctx.upload(B)
        ref = _hmult(ctx, lvl, da, db, k, batch, False)
        o = Oracle(n, q, p, 0)
        for i in oracle_items:
            assert np.array_equal(ref[i], o.ckks_mult_relin_rescale(lvl, A[i], B[i], key, klvl)), ("oracle", n, lvl, i)
        for tile in tiles:
            ctx.set_tile_batch(tile)
            for fold in (True, False, True):
                got = _hmult(ctx, lvl, da, db, k, batch, fold)
                assert np.array_equal(got, ref), (n, lvl, tile, fold)
                assert np.array_equal(got[batch - 1], got[0]), (n, lvl, tile, fold)
    finally:
        ctx.close()


def test_n14_uneven_tiles():
    need_gpu()
    C = params.CKKS_DEFAULT[65536]
    _check(1 << 14, C["q"][:13], C["p"][:4], 12, 12, 5, (0, 2, 3), 8014)


def test_n16_headline_chain_uneven_tiles():
    need_gpu()
    C = params.CKKS_DEFAULT[65536]
    _check(1 << 16, C["q"][:13], C["p"][:4], 12, 12, 5, (0, 2), 8016)


def test_n16_integer_engine_limbs():
    """the bootstrap chain's 60-bit Q limbs take the integer-engine product (two Montgomery products) next to FP64 limbs"""
    need_gpu()
    P = params.CKKS_BOOTSTRAP_65536
    _check(1 << 16, P["q"], P["p"], 9, 24, 3, (0, 2), 8116)


def test_n17_nine_stage_pass():
    need_gpu()
    C = params.ckks_n17_chain()
    q, p = C["q"], C["p"]
    _check(C["n"], q, p, 4, len(q) - 1, 3, (0, 2), 8017)
