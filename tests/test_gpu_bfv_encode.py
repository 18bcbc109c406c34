"""lsa_bfv_encode on the device (csrc/bfv_encode.hip, k_bfv_encode_t) against the CPU client, word for word.  Form 0 (ring-t
coefficients) equals Client.bfv_encode at N = 2^12 .. 2^15 -- 2^15 is the kernel's LDS limit -- and at N = 2^16, where the
transform runs on the host; on all zeros, all t-1, a single 1 in slot 0, N/2-1, N/2 and N-1, and random values; with a padded
batch stride.  Form 1 (pt_mul) equals the words of tests/test_gpu_bfv_ptmul.py's pt_mul helper and multiplies messages; form 2
(extended) equals a forward transform per row of Q_level u P.  Both butterfly engines give the same words.  Every refusal of the
header arrives before anything is written."""
import ctypes

import numpy as np
import pytest

from lattisense_amd import params
from tests.bfv_lt_model import encode_ext, encode_pt_mul
from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu


def _message(err):
    return str(err).split(": ", 1)[1]


def _chain(n):
    if n == 65536:                                  # two Q limbs and one special prime of the N = 2^16 chain, t = 786433
        B = params.bfv_n16_chain()
        return B["q"][:2], B["p"][:1], B["t"]
    B = params.BFV_DEFAULT[n]
    return B["q"], B["p"], B["t"]


def _rig(n):
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    q, p, t = _chain(n)
    o = Oracle(n, q, p, t)
    return DeviceContext(ALGO_BFV, n, q, p, t), o, Client(o, seed=n % 1000), t


def _inputs(n, t, rng):
    rows = [np.zeros(n, dtype=np.uint64), np.full(n, t - 1, dtype=np.uint64)]
    for slot in (0, n // 2 - 1, n // 2, n - 1):
        v = np.zeros(n, dtype=np.uint64)
        v[slot] = 1
        rows.append(v)
    rows.append(rng.integers(0, t, n).astype(np.uint64))
    return np.stack(rows)


@pytest.mark.parametrize("n", [4096, 8192, 16384, 32768, 65536])
def test_form0_against_the_client(n):
    need_gpu()
    ctx, o, c, t = _rig(n)
    try:
        rng = np.random.default_rng(n)
        vals = _inputs(n, t, rng)
        want = np.stack([c.bfv_encode(v) for v in vals])
        assert int(want.max()) < t
        got = ctx.download(ctx.bfv_encode(0, 0, vals), vals.shape)
        for i in range(len(vals)):
            assert np.array_equal(got[i], want[i]), "input %d of N = %d differs from Client.bfv_encode" % (i, n)
        sout = n + 64                               # batch 3, padded: the padding is nobody's
        out = ctx.upload(np.full(3 * sout, 7, dtype=np.uint64))
        ctx.bfv_encode(0, 0, vals[4:7], out=out, sout=sout)
        pad = ctx.download(out, (3, sout))
        assert np.array_equal(pad[:, :n], want[4:7]) and np.all(pad[:, n:] == 7)
        ctx.bfv_encode(0, 0, vals[:0].reshape(0, n), out=out, sout=sout)    # batch 0: a no-op
        assert np.array_equal(ctx.download(out, (3, sout)), pad)
    finally:
        ctx.close()


@pytest.mark.parametrize("n, levels", [(4096, (1,)), (16384, (0, 5))])
def test_form1_is_the_pt_mul_helper_and_multiplies_messages(n, levels):
    need_gpu()
    ctx, o, c, t = _rig(n)
    try:
        rng = np.random.default_rng(n + 1)
        m2 = rng.integers(0, t, (2, n)).astype(np.uint64)
        for lvl in levels:
            L = lvl + 1
            want = np.stack([encode_pt_mul(o, c, lvl, m) for m in m2])
            pt = ctx.bfv_encode(lvl, 1, m2)
            assert np.array_equal(ctx.download(pt, (2, L, n)), want), (n, lvl)
            ctx.set_fp64_ntt(0)
            try:
                assert np.array_equal(ctx.download(ctx.bfv_encode(lvl, 1, m2), (2, L, n)), want), ("integer engine", n, lvl)
            finally:
                ctx.set_fp64_ntt(1)
            sout = L * n + 2 * n                    # padded stride: the Montgomery step runs per item
            out = ctx.upload(np.full(2 * sout, 7, dtype=np.uint64))
            ctx.bfv_encode(lvl, 1, m2, out=out, sout=sout)
            pad = ctx.download(out, (2, sout))
            assert np.array_equal(pad[:, : L * n].reshape(2, L, n), want) and np.all(pad[:, L * n:] == 7)
        lvl = levels[-1]
        m1 = rng.integers(0, t, n).astype(np.uint64)
        ct = c.bfv_encrypt(m1, lvl)
        prod = ctx.bfv_mult_plain_mul(lvl, ctx.upload(ct[None]), ctx.bfv_encode(lvl, 1, m2[:1]), 1)
        got = ctx.download(prod, (1, 2, lvl + 1, n))[0]
        assert np.array_equal(c.bfv_decrypt(got), m1 * m2[0] % np.uint64(t))
    finally:
        ctx.close()


def test_form2_is_a_forward_transform_per_row():
    """N = 2^13 (54 / 55-bit Q, 55-bit P): no row of this chain is an FP64-engine limb, so the run after lsa_set_fp64_ntt(0)
    ("integer engine") uses the engine the first run used and shows that the setting itself changes nothing.  The comparison of
    the two engines on form 2 lives in tests/test_gpu_bfv_operator_chains.py (test_encode_variants on the fp and mixed chains)."""
    need_gpu()
    n, lvl = 8192, 2
    ctx, o, c, t = _rig(n)
    try:
        rng = np.random.default_rng(82)
        vals = np.stack([rng.integers(0, t, n).astype(np.uint64), np.full(n, t - 1, dtype=np.uint64), np.zeros(n, dtype=np.uint64)])
        T = lvl + 1 + len(o.p)
        want = np.stack([encode_ext(o, c, lvl, v) for v in vals])
        assert want.shape == (3, T, n)
        assert np.array_equal(ctx.download(ctx.bfv_encode(lvl, 2, vals), (3, T, n)), want)
        ctx.set_fp64_ntt(0)
        try:
            assert np.array_equal(ctx.download(ctx.bfv_encode(lvl, 2, vals), (3, T, n)), want), "integer engine"
        finally:
            ctx.set_fp64_ntt(1)
        low = np.stack([encode_ext(o, c, 0, v) for v in vals])          # level 0: q_0 and the special prime
        assert np.array_equal(ctx.download(ctx.bfv_encode(0, 2, vals), (3, 1 + len(o.p), n)), low)
    finally:
        ctx.close()


def test_refusals_arrive_before_anything_is_written():
    need_gpu()
    from lattisense_amd._native import LsaError, check, lib
    from lattisense_amd.device import ALGO_BFV, ALGO_CKKS, DeviceContext
    n = 4096
    ctx, o, c, t = _rig(n)
    try:
        vals = np.random.default_rng(3).integers(0, t, (2, n)).astype(np.uint64)
        out = ctx.upload(np.full(8 * n, 7, dtype=np.uint64))
        vp = vals.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))

        def fails(fn, needle):
            with pytest.raises(LsaError) as e:
                fn()
            assert e.value.code == 1 and _message(e.value).startswith("lsa_bfv_encode") and needle in _message(e.value), e.value
            assert np.all(ctx.download(out, (8 * n,)) == 7)
        call = lambda h, lvl, form, v, o_, so, b: check(lib().lsa_bfv_encode(h, lvl, form, v, o_, so, b, ctx.stream))
        fails(lambda: call(ctx.h, 2, 0, vp, out.ptr, n, 2), "level")
        fails(lambda: call(ctx.h, -1, 0, vp, out.ptr, n, 2), "level")
        fails(lambda: call(ctx.h, 1, 3, vp, out.ptr, 3 * n, 2), "form")
        fails(lambda: call(ctx.h, 1, -1, vp, out.ptr, 3 * n, 2), "form")
        fails(lambda: call(ctx.h, 1, 0, None, out.ptr, n, 2), "null")
        fails(lambda: call(ctx.h, 1, 0, vp, None, n, 2), "null")
        fails(lambda: call(ctx.h, 1, 0, vp, out.ptr + 8, n, 2), "16-byte")
        fails(lambda: call(ctx.h, 1, 0, vp, out.ptr, n + 1, 2), "even")
        fails(lambda: call(ctx.h, 1, 1, vp, out.ptr, n, 2), "stride")          # pt_mul at level 1 needs 2 N words
        fails(lambda: call(ctx.h, 1, 2, vp, out.ptr, 2 * n, 2), "stride")      # extended needs 3 N
        bad = vals.copy()
        bad[1, 17] = t
        fails(lambda: call(ctx.h, 1, 0, bad.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), out.ptr, n, 2), "below t")
        P = params.CKKS_DEFAULT[4096]
        ckks = DeviceContext(ALGO_CKKS, n, P["q"], P["p"])
        fails(lambda: call(ckks.h, 0, 0, vp, out.ptr, n, 2), "not BFV")
        ckks.close()
        B = params.BFV_DEFAULT[8192]                # t = 65537 has no slots at N = 2^16
        noslots = DeviceContext(ALGO_BFV, 65536, params.bfv_n16_chain()["q"][:2], params.bfv_n16_chain()["p"][:1], B["t"])
        big = np.zeros((1, 65536), dtype=np.uint64)
        fails(lambda: call(noslots.h, 0, 0, big.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), out.ptr, 65536, 1), "1 mod 2N")
        noslots.close()
        assert np.array_equal(ctx.download(ctx.bfv_encode(1, 0, vals), (2, n)), np.stack([c.bfv_encode(v) for v in vals]))
    finally:
        ctx.close()
