"""CPU-only: the batch chunking of launch_ntt (lsa_set_ntt_chunk_mib; lattisense_amd/csrc/ntt_chunk.h).

  test_ntt_chunk_functions   tests/cpp/test_ntt_chunk.cpp (g++ -fsanitize=address,undefined): ntt_chunk_items against exact integer
                             arithmetic and the tiling of the batch, ntt_chunk_rebase on every fusion shape the operators build
  test_chunked_*_replay      the CPU replay (emu_ntt.cpp) of the product prologue and of the lift prologue run chunk by chunk
                             through ntt_chunk_rebase, operands with batch strides of their own: word for word the unchunked
                             replay and the oracle's transform of the multiplied / lifted input

The GPU runs the same launcher arithmetic in tests/test_gpu_ntt_chunk.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from lattisense_amd import params
from oracle.pyoracle import Oracle
from tests.test_emulate_ntt import emu  # noqa: F401  (the replay library fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P64 = ctypes.POINTER(ctypes.c_uint64)
SKIP = 0xFF
BATCH = 5
SENT = np.uint64(0xABCDEF0123456789)


def test_ntt_chunk_functions(tmp_path):
    exe = str(tmp_path / "test_ntt_chunk")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-attributes", "-DLSA_EMULATE",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_ntt_chunk.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK ntt_chunk" in out.stdout


def _mods():
    D = params.CKKS_DEFAULT[65536]
    B = params.CKKS_BOOTSTRAP_65536
    return [D["q"][1], B["q"][10], B["q"][0], B["p"][0]]   # 46- and 39-bit (FP64 engine), 60- and 61-bit (integer engine)


def _padded(items, pad):
    """[batch][...] -> a flat sentinel-filled buffer with `pad` words between the items, and the stride in words"""
    w = items[0].size
    buf = np.full(len(items) * (w + pad), SENT, dtype=np.uint64)
    for b, it in enumerate(items):
        buf[b * (w + pad): b * (w + pad) + w] = it.ravel()
    return buf, w + pad


def _unpad(buf, batch, stride, shape):
    w = int(np.prod(shape))
    out = np.stack([buf[b * stride: b * stride + w].reshape(shape) for b in range(batch)])
    gaps = np.concatenate([buf[b * stride + w: (b + 1) * stride] for b in range(batch)])
    assert (gaps == SENT).all(), "the replay wrote between the items"
    return out


# ------------------------------------------------------------------------------------------------ product prologue
def _prod(emu, n, mods, A, sa, Bv, sb, flags, chunk):
    rows = len(mods)
    out, so = _padded(np.zeros((BATCH, rows, n), dtype=np.uint64), 34)
    arr = (ctypes.c_uint64 * len(mods))(*mods)
    mo = (ctypes.c_ubyte * rows)(*range(rows))
    emu.lsa_emu_intt_prod_chunked.restype = ctypes.c_int
    r = emu.lsa_emu_intt_prod_chunked(ctypes.c_int(n), arr, len(mods), A.ctypes.data_as(P64), ctypes.c_longlong(sa),
                                      Bv.ctypes.data_as(P64), ctypes.c_longlong(sb), out.ctypes.data_as(P64), BATCH,
                                      ctypes.c_longlong(so), rows, mo, rows, 12, int(flags), int(chunk))
    assert r == 0
    return _unpad(out, BATCH, so, (rows, n))


@pytest.mark.parametrize("logn", [13, 15])
def test_chunked_product_prologue_replay(emu, logn):
    """inverse transform of a * b formed in the first executed pass; a, b and the output each with a stride of its own (b shared
    by the whole batch in a second run), chunks of 1 and of 2 items (2, 2, 1)"""
    n = 1 << logn
    mods = _mods()
    o = Oracle(n, mods, [], 0)
    rng = np.random.default_rng(2000 + logn)
    A = np.stack([np.stack([rng.integers(0, m, size=n, dtype=np.uint64) for m in mods]) for _ in range(BATCH)])
    Bv = np.stack([np.stack([rng.integers(0, m, size=n, dtype=np.uint64) for m in mods]) for _ in range(BATCH)])
    qm = np.array([m - 1 for m in mods], dtype=np.uint64)[:, None]
    A[BATCH - 1], Bv[BATCH - 1] = qm, qm                    # (q-1)^2 in the ragged last chunk

    def want_of(bsel):
        w = np.empty_like(A)
        for b in range(BATCH):
            for r, m in enumerate(mods):
                d2 = np.array([(int(x) * int(y)) % m for x, y in zip(A[b, r], Bv[bsel(b), r])], dtype=np.uint64)
                w[b, r] = o.intt(r, d2)
        return w

    pa, sa = _padded(A, 10)
    pb, sb = _padded(Bv, 18)
    assert len({sa, sb, len(mods) * n + 34}) == 3
    flag_sets = (1, 0) + ((4 | 1, 4, 4 | 3) if logn >= 14 else ())
    for (bbuf, bstride, bsel) in ((pb, sb, lambda b: b), (pb[2 * sb:], 0, lambda b: 2)):
        want = want_of(bsel)
        for flags in flag_sets:
            whole = _prod(emu, n, mods, pa, sa, bbuf, bstride, flags, 0)
            assert np.array_equal(whole, want), (logn, flags, "unchunked")
            for chunk in (1, 2):
                got = _prod(emu, n, mods, pa, sa, bbuf, bstride, flags, chunk)
                assert np.array_equal(got, want), (logn, flags, chunk, np.argwhere((got != want).any(axis=-1)))
                assert np.array_equal(got, whole)


# ------------------------------------------------------------------------------------------------ lift prologue
def _lift(emu, n, mods, src, ssrc, flags, chunk):
    k = len(mods)
    rows = k * k
    mod_of = [SKIP if j == p else j for p in range(k) for j in range(k)]   # the own row is skipped, as in the key switch
    out, so = _padded(np.zeros((BATCH, rows, n), dtype=np.uint64), 34)
    arr = (ctypes.c_uint64 * k)(*mods)
    mo = (ctypes.c_ubyte * rows)(*mod_of)
    emu.lsa_emu_ntt_lift_chunked.restype = ctypes.c_int
    r = emu.lsa_emu_ntt_lift_chunked(ctypes.c_int(n), arr, k, src.ctypes.data_as(P64), ctypes.c_longlong(ssrc), 0, k,
                                     out.ctypes.data_as(P64), BATCH, ctypes.c_longlong(so), rows, mo, rows, 12, int(flags), int(chunk))
    assert r == 0
    return _unpad(out, BATCH, so, (k, k, n))


@pytest.mark.parametrize("logn", [13, 15])
def test_chunked_lift_prologue_replay(emu, logn):
    """forward transform of x mod p_t lifted by the load; the source rows with a stride of their own, chunks of 1 and of 2 items"""
    n = 1 << logn
    mods = _mods()
    k = len(mods)
    o = Oracle(n, mods, [], 0)
    rng = np.random.default_rng(3000 + logn)
    src = np.stack([np.stack([rng.integers(0, m, size=n, dtype=np.uint64) for m in mods]) for _ in range(BATCH)])
    src[BATCH - 1] = np.array([m - 1 for m in mods], dtype=np.uint64)[:, None]
    want = np.zeros((BATCH, k, k, n), dtype=np.uint64)
    for b in range(BATCH):
        for p in range(k):
            for j, pt in enumerate(mods):
                if j != p:
                    want[b, p, j] = o.ntt(j, src[b, p] % np.uint64(pt))
    ps, ssrc = _padded(src, 22)
    assert ssrc != k * k * n + 34 and ssrc != k * n
    for flags in (1, 0, 3) + ((4 | 1, 4, 4 | 3) if logn >= 14 else ()):
        whole = _lift(emu, n, mods, ps, ssrc, flags, 0)
        assert np.array_equal(whole, want), (logn, flags, "unchunked")
        for chunk in (1, 2):
            got = _lift(emu, n, mods, ps, ssrc, flags, chunk)
            assert np.array_equal(got, want), (logn, flags, chunk, np.argwhere((got != want).any(axis=-1)))
            assert np.array_equal(got, whole)
