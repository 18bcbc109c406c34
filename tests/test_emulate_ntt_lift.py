"""CPU replay of the forward transform with the lift prologue (NttPassArgs::fz_pro == 4): the first executed pass reads one
source row x over q_s per polynomial and takes x mod p_t as the input of every target row -- the ModUp of a key-switch digit
with one source limb, where the exact base conversion is the identity.  Both butterfly engines and each kernel family (the
staged kernel in its single-pass and two-pass forms, the 7- and 8-stage radix-16-squared first passes, the nine-stage second
pass behind a lifted first pass), compared bit for bit with the oracle's transform of x mod p_t computed here.  The replay
aborts on any violated range invariant (LSA_EMU_CHECK).  The same kernels run on the GPU in tests/test_gpu_modup_lift.py."""
import ctypes

import numpy as np
import pytest

from lattisense_amd import params
from oracle.pyoracle import Oracle
from tests.boundary import primes_above
from tests.test_emulate_ntt import emu  # noqa: F401  (the replay library fixture)

SKIP = 0xFF


def _mods(n):
    """every modulus is a source once and a target of all the others, so each relation occurs on each engine:
    source below the target, slightly above it (q_s <= 2 p_t: one conditional subtraction), far above an FP64-engine target
    from below 2^52 (one exact FP64 reduction) and from above it (integer reduction, then converted), far above an
    integer-engine target (general reduction)"""
    mods = [params.ntt_primes_below(61, n, 1)[0],    # integer engine; the far source of every other target
            params.ntt_primes_below(57, n, 1)[0],    # integer-engine target far below the 61-bit source
            params.ntt_primes_below(50, n, 1)[0],    # far above the FP64-engine targets, below 2^52
            params.ntt_primes_below(47, n, 1)[0],    # FP64 engine, the largest size it takes
            primes_above(46, n, 1)[0],               # FP64 engine, slightly below the previous one
            params.ntt_primes_below(39, n, 1)[0]]    # FP64 engine, small
    assert [m.bit_length() for m in mods] == [61, 57, 50, 47, 47, 39]
    assert mods[4] < mods[3] <= 2 * mods[4]
    return mods


def _sources(mods, n, rng):
    """[2][len(mods)][n]: slot 0 uniform below q_s with the worst-case residues 0, q_s - 1 and p_t - 1, p_t, p_t + 1 of every
    target below q_s in front, slot 1 all q_s - 1 (the largest input of every butterfly at once)"""
    src = np.empty((2, len(mods), n), dtype=np.uint64)
    for p, qs in enumerate(mods):
        src[0, p] = rng.integers(0, qs, size=n, dtype=np.uint64)
        edge = [0, qs - 1] + [v for pt in mods for v in (pt - 1, pt, pt + 1) if v < qs]
        src[0, p, :len(edge)] = np.array(edge, dtype=np.uint64)
        src[1, p] = qs - 1
    return src


def _lift(emu, n, mods, src, flags, tau=12):
    k = len(mods)
    rows = k * k
    mod_of = [SKIP if j == p else j for p in range(k) for j in range(k)]   # the own row is skipped, as in the key switch
    out = np.zeros((src.shape[0], rows, n), dtype=np.uint64)
    arr = (ctypes.c_uint64 * k)(*mods)
    mo = (ctypes.c_ubyte * rows)(*mod_of)
    P = ctypes.POINTER(ctypes.c_uint64)
    emu.lsa_emu_ntt_lift.restype = ctypes.c_int
    r = emu.lsa_emu_ntt_lift(ctypes.c_int(n), arr, k, src.ctypes.data_as(P), 0, k, out.ctypes.data_as(P), src.shape[0],
                             ctypes.c_longlong(rows * n), rows, mo, rows, tau, int(flags))
    assert r == 0
    return out.reshape(src.shape[0], k, k, n)


def _check(emu, logn, flag_sets, tau=12):
    n = 1 << logn
    mods = _mods(n)
    k = len(mods)
    o = Oracle(n, mods, [], 0)
    src = _sources(mods, n, np.random.default_rng(90 + logn))
    want = np.zeros((2, k, k, n), dtype=np.uint64)
    for b in range(2):
        for p in range(k):
            for j, pt in enumerate(mods):
                if j != p:
                    want[b, p, j] = o.ntt(j, src[b, p] % np.uint64(pt))
    for flags in flag_sets:
        got = _lift(emu, n, mods, src, flags, tau)
        assert np.array_equal(got, want), (logn, flags, np.argwhere((got != want).any(axis=-1)))


@pytest.mark.parametrize("logn,tau", [(12, 12), (13, 12), (14, 12), (16, 12), (13, 10), (13, 13), (11, 12)])
def test_lift_prologue_staged_kernel(emu, logn, tau):
    """k_ntt_pass: the single-pass form (N <= 2^12, the whole-limb 2^13 tile, a partial tile at 2^11) and the first pass of the
    two-pass plans; FP64 engine where the prime allows it, the integer engine for every limb, the interleaved order"""
    _check(emu, logn, (1, 0, 3), tau)


@pytest.mark.parametrize("logn", [14, 15, 16, 17])
def test_lift_prologue_radix16_first_passes(emu, logn):
    """k_ntt_r16 first passes of seven (2^14) and eight stages, the second pass k_ntt_r16 / k_ntt_r8x3 (2^17) reading what the
    lifted first pass handed over (raw FP64 hand-off)"""
    _check(emu, logn, (4 | 1, 4, 4 | 3))
