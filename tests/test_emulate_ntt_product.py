"""CPU replay of the inverse transform with the product prologue (NttPassArgs::fz_pro == 3): the first executed pass of the
inverse NTT forms a * b mod q as it loads, for the tensor-fold HMult's ModUp input d2 = a1 b1.  Both butterfly engines, the
radix-16-squared / nine-stage second passes (N = 2^14 .. 2^17) and the staged kernel, compared bit for bit with the oracle's
inverse transform of the product.  The same kernels are checked on the GPU in tests/test_gpu_hmult_product_prologue.py."""
import ctypes

import numpy as np
import pytest

from lattisense_amd import params
from oracle.pyoracle import Oracle
from tests.boundary import pattern, primes_above
from tests.test_emulate_ntt import emu  # noqa: F401  (the replay library fixture)


def _mods(logn):
    if logn >= 17:
        P = params.ckks_n17_chain()
        return [m for m in (P["q"][0], P["q"][1], P["p"][0]) if (m - 1) % (2 << logn) == 0]
    D = params.CKKS_DEFAULT[65536]
    B = params.CKKS_BOOTSTRAP_65536
    return [D["q"][1], B["q"][10], B["q"][0], B["p"][0]]   # 46- and 39-bit (FP64 engine), 60- and 61-bit (integer engine)


def _run(emu, n, mods, A, B, flags, tau=12):
    batch, rows = A.shape[0], A.shape[1]
    out = np.zeros_like(A)
    arr = (ctypes.c_uint64 * len(mods))(*mods)
    mo = (ctypes.c_ubyte * rows)(*range(rows))
    P = ctypes.POINTER(ctypes.c_uint64)
    emu.lsa_emu_intt_prod.restype = ctypes.c_int
    r = emu.lsa_emu_intt_prod(ctypes.c_int(n), arr, len(mods), A.ctypes.data_as(P), B.ctypes.data_as(P), out.ctypes.data_as(P),
                              batch, ctypes.c_longlong(rows * n), rows, mo, rows, tau, int(flags))
    assert r == 0
    return out


def _check(emu, logn, flags, tau=12):
    n = 1 << logn
    mods = _mods(logn)
    if len(mods) < 2:
        pytest.skip("the generated chain has no two primes = 1 mod 2^%d" % (logn + 1))
    o = Oracle(n, mods, [], 0)
    rng = np.random.default_rng(1000 + logn)
    batch, rows = 2, len(mods)
    A = np.stack([np.stack([rng.integers(0, m, size=n, dtype=np.uint64) for m in mods]) for _ in range(batch)])
    B = np.stack([np.stack([rng.integers(0, m, size=n, dtype=np.uint64) for m in mods]) for _ in range(batch)])
    qm = np.array([m - 1 for m in mods], dtype=np.uint64)[:, None]
    A[1], B[1] = qm, qm                                      # (q-1)^2: every product = 1, the worst case of the lift
    A[0, :, :2], B[0, :, :2] = qm, np.array([[0, 1]], dtype=np.uint64) * np.ones((rows, 1), dtype=np.uint64)
    got = _run(emu, n, mods, A, B, flags, tau)
    for b in range(batch):
        for r, m in enumerate(mods):
            d2 = np.array([(int(x) * int(y)) % m for x, y in zip(A[b, r], B[b, r])], dtype=np.uint64)
            assert np.array_equal(got[b, r], o.intt(r, d2)), (logn, flags, b, r)


@pytest.mark.parametrize("logn", [14, 15, 16, 17])
def test_product_prologue_second_passes(emu, logn):
    """the inverse transform's first pass is the radix-16-squared second pass (MU = 7 / 8) or the nine-stage one (2^17)"""
    _check(emu, logn, 4 | 1)   # FP64 engine where the prime allows it
    _check(emu, logn, 4)       # integer engine for every limb
    _check(emu, logn, 4 | 3)   # interleaved workgroup order of mixed-engine launches


@pytest.mark.parametrize("logn,tau", [(12, 12), (13, 12), (14, 12), (16, 12), (13, 10)])
def test_product_prologue_staged_kernel(emu, logn, tau):
    """the staged k_ntt_pass takes the prologue where no register-image kernel runs the first pass (single-pass plans,
    small tiles, LSA_NTT_R16=0)"""
    _check(emu, logn, 1, tau)
    _check(emu, logn, 0, tau)


def _edge_mods(n):
    """47-bit FP64-engine primes on both ends of their range (just above 2^46, just below 2^47) and the integer-engine primes on
    either side of the lazy-butterfly limit 2^57"""
    return primes_above(46, n, 1) + params.ntt_primes_below(47, n, 1) + params.ntt_primes_below(57, n, 1) + primes_above(57, n, 1)


@pytest.mark.parametrize("logn", [12, 13, 14, 15, 16, 17])
def test_product_prologue_threshold_primes_and_extreme_pairs(emu, logn):
    """(q-1)^2, half . half and max . one operand pairs (and the half points against the maximum) on the edge primes"""
    n = 1 << logn
    mods = _edge_mods(n)
    assert [m.bit_length() for m in mods] == [47, 47, 57, 58]
    o = Oracle(n, mods, [], 0)
    rng = np.random.default_rng(logn)
    pairs = (("max", "max"), ("half", "half"), ("max", "one"), ("half", "max"), ("top", "top"), ("alt", "alt1"))
    A = np.stack([np.stack([pattern(a, m, n, rng) for m in mods]) for a, _ in pairs])
    B = np.stack([np.stack([pattern(b, m, n, rng) for m in mods]) for _, b in pairs])
    want = np.empty_like(A)
    for b in range(len(pairs)):
        for r, m in enumerate(mods):
            d2 = np.array([(int(x) * int(y)) % m for x, y in zip(A[b, r], B[b, r])], dtype=np.uint64)
            want[b, r] = o.intt(r, d2)
    for flags in (1, 0) + ((4 | 1, 4, 4 | 3) if logn >= 14 else ()):
        got = _run(emu, n, mods, A, B, flags)
        assert np.array_equal(got, want), (logn, flags, np.argwhere((got != want).any(axis=-1)))
