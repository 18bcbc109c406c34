"""BFV past 16 limbs: the multiply's two exact base conversions (Q -> QMul and back) with more than 16 source limbs run the wide
conversion (kernels.hip k_baseconv_wide).  Bit-exact against the CPU oracle on both sides of the 16-source boundary, on the
N = 2^16 chain (params.bfv_n16_chain, 24 Q + 4 P) at its full ring, on the reference's N = 2^15 set at its full ring, and
through the task runtime; plus the message-level check: decrypt == x*y mod t / the rotated vector."""
import json
import os

import numpy as np
import pytest

from lattisense_amd import params
from tests.gpu_util import env, need_gpu, rand_ct

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASKS = os.path.join(ROOT, "tests", "golden", "tasks")


def _rand_key(rng, q, p, klvl, n):
    beta = (klvl + 1 + len(p) - 1) // len(p)
    key = np.empty((beta, 2, klvl + 1 + len(p), n), dtype=np.uint64)
    for j, m in enumerate(q[: klvl + 1] + p):
        key[:, :, j, :] = rng.integers(0, m, size=(beta, 2, n), dtype=np.uint64)
    return key


def _boundary_run(q, p, t, levels, seed):
    """bfv_mult_relin at each level on the ring shrunk to 1024, LSA_BFV_FOLD on/off x tile batch default/1, vs the oracle"""
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    from oracle.pyoracle import Oracle
    n = 1024
    ctx = DeviceContext(ALGO_BFV, n, q, p, t)
    o = Oracle(n, q, p, t)
    assert ctx.moduli == o.mod
    rng = np.random.default_rng(seed)
    klvl = len(q) - 1
    key = _rand_key(rng, q, p, klvl, n)
    k = ctx.upload_key(key, klvl)
    for lvl in levels:
        A, Bc = rand_ct(rng, q[: lvl + 1], 2, n, 2), rand_ct(rng, q[: lvl + 1], 2, n, 2)
        want = np.stack([o.bfv_mult_relin(lvl, A[i], Bc[i], key, klvl) for i in range(2)])
        da, db = ctx.upload(A), ctx.upload(Bc)
        for fold in ("1", "0"):
            with env(LSA_BFV_FOLD=fold):
                for tb in (0, 1):
                    ctx.set_tile_batch(tb)
                    out = ctx.bfv_mult_relin(lvl, da, db, k, 2)
                    assert np.array_equal(ctx.download(out, want.shape), want), (lvl, fold, tb)
        ctx.set_tile_batch(0)
    ctx.destroy_key(k)
    ctx.close()


def test_wide_conversion_at_every_boundary():
    """levels 14, 15 (15 / 16 Q limbs: the narrow kernel) and 16, 17, 23 (17, 18, 24 Q limbs and as many auxiliary limbs:
    the wide kernel, partial and exact 24-source shapes) of the N = 2^16 chain"""
    need_gpu()
    C = params.bfv_n16_chain()
    _boundary_run(C["q"], C["p"], C["t"], [14, 15, 16, 17, 23], 16)


def test_wide_conversion_up_to_32_sources():
    """the 32-source shapes: a 32-prime chain of the same kind, at 25, 29 and 32 Q limbs"""
    need_gpu()
    C = params.bfv_n16_chain()
    q = params.ntt_primes_below(59, C["n"], 32, avoid=C["p"])
    _boundary_run(q, C["p"], C["t"], [24, 28, 31], 32)


@pytest.fixture(scope="module")
def n16():
    """the N = 2^16 chain at its full ring: device context, oracle, client, relinearisation key at the top level"""
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    C = params.bfv_n16_chain()
    n, q, p, t = C["n"], C["q"], C["p"], C["t"]
    ctx = DeviceContext(ALGO_BFV, n, q, p, t)
    o = Oracle(n, q, p, t)
    assert ctx.moduli == o.mod
    c = Client(o, seed=65536)
    lvl = len(q) - 1
    rlk = c.gen_relin_key(lvl)
    k = ctx.upload_key(rlk, lvl)
    yield ctx, o, c, rlk, k, lvl
    ctx.destroy_key(k)
    ctx.close()


def test_n16_full_ring_mult_relin_decrypts(n16):
    need_gpu()
    ctx, o, c, rlk, k, lvl = n16
    n, t = ctx.n, ctx.t
    rng = np.random.default_rng(1)
    x = rng.integers(0, t, size=n, dtype=np.uint64)
    y = rng.integers(0, t, size=n, dtype=np.uint64)
    A, Bc = c.bfv_encrypt(x, lvl)[None], c.bfv_encrypt(y, lvl)[None]
    da, db = ctx.upload(A), ctx.upload(Bc)
    d3 = ctx.bfv_mult(lvl, da, db, 1)
    want_d3 = o.bfv_mult(lvl, A[0], Bc[0])[None]
    assert np.array_equal(ctx.download(d3, want_d3.shape), want_d3)
    z = ctx.bfv_relin(lvl, d3, k, 1)
    want_z = o.bfv_relin(lvl, want_d3[0], rlk, lvl)[None]
    got = ctx.download(z, want_z.shape)
    assert np.array_equal(got, want_z)
    z2 = ctx.bfv_mult_relin(lvl, da, db, k, 1)
    assert np.array_equal(ctx.download(z2, want_z.shape), want_z)
    assert np.array_equal(c.bfv_decrypt(got[0]), x * y % np.uint64(t))


def test_n16_full_ring_rotate_and_rescale(n16):
    need_gpu()
    from oracle.client import galois_element_for_col_rotation, galois_element_for_row_rotation
    ctx, o, c, rlk, k, lvl = n16
    n, t = ctx.n, ctx.t
    x = (np.arange(n, dtype=np.uint64) * np.uint64(7)) % np.uint64(t)
    A = c.bfv_encrypt(x, lvl)[None]
    da = ctx.upload(A)
    h = n // 2
    for step, g in [(1, galois_element_for_col_rotation(1, n)), (None, galois_element_for_row_rotation(n))]:
        glk = c.gen_galois_key(g, lvl)
        gk = ctx.upload_key(glk, lvl)
        out = ctx.bfv_rotate(lvl, da, g, gk, 1)
        want = o.bfv_rotate(lvl, A[0], g, glk, lvl)[None]
        got = ctx.download(out, want.shape)
        assert np.array_equal(got, want), step
        exp = (np.concatenate([x[h:], x[:h]]) if step is None
               else np.concatenate([np.roll(x[:h], -step), np.roll(x[h:], -step)]))
        assert np.array_equal(c.bfv_decrypt(got[0]), exp), step
        ctx.destroy_key(gk)
    rs = ctx.bfv_rescale(lvl, 2, da, 1)
    want = o.bfv_rescale(lvl, A[0])[None]
    got = ctx.download(rs, want.shape)
    assert np.array_equal(got, want)
    assert np.array_equal(c.bfv_decrypt(got[0]), x)


def test_n16_batch_position_independence(n16):
    """the same ciphertext pair at positions 0 and 3 of a batch of 4 gives the same product"""
    need_gpu()
    ctx, o, c, rlk, k, lvl = n16
    n = ctx.n
    q = ctx.q[: lvl + 1]
    rng = np.random.default_rng(4)
    A, Bc = rand_ct(rng, q, 2, n, 4), rand_ct(rng, q, 2, n, 4)
    A[3], Bc[3] = A[0], Bc[0]
    out = ctx.download(ctx.bfv_mult_relin(lvl, ctx.upload(A), ctx.upload(Bc), k, 4), (4, 2, lvl + 1, n))
    assert np.array_equal(out[0], out[3])
    assert not np.array_equal(out[0], out[1])


def test_n15_reference_set_full_ring():
    """the reference's largest BFV set (12 Q + 3 P, N = 2^15) at its full ring and top level"""
    need_gpu()
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    from oracle.client import Client, galois_element_for_col_rotation
    from oracle.pyoracle import Oracle
    P = params.BFV_DEFAULT[32768]
    n, q, p, t = 32768, P["q"], P["p"], P["t"]
    ctx = DeviceContext(ALGO_BFV, n, q, p, t)
    o = Oracle(n, q, p, t)
    assert ctx.moduli == o.mod
    c = Client(o, seed=32768)
    lvl = len(q) - 1
    rng = np.random.default_rng(15)
    x = rng.integers(0, t, size=n, dtype=np.uint64)
    y = rng.integers(0, t, size=n, dtype=np.uint64)
    A, Bc = c.bfv_encrypt(x, lvl)[None], c.bfv_encrypt(y, lvl)[None]
    rlk = c.gen_relin_key(lvl)
    k = ctx.upload_key(rlk, lvl)
    da, db = ctx.upload(A), ctx.upload(Bc)
    want = o.bfv_mult_relin(lvl, A[0], Bc[0], rlk, lvl)[None]
    got = ctx.download(ctx.bfv_mult_relin(lvl, da, db, k, 1), want.shape)
    assert np.array_equal(got, want)
    assert np.array_equal(c.bfv_decrypt(got[0]), x * y % np.uint64(t))
    g = galois_element_for_col_rotation(1, n)
    glk = c.gen_galois_key(g, lvl)
    gk = ctx.upload_key(glk, lvl)
    want = o.bfv_rotate(lvl, A[0], g, glk, lvl)[None]
    got = ctx.download(ctx.bfv_rotate(lvl, da, g, gk, 1), want.shape)
    assert np.array_equal(got, want)
    h = n // 2
    assert np.array_equal(c.bfv_decrypt(got[0]), np.concatenate([np.roll(x[:h], -1), np.roll(x[h:], -1)]))
    ctx.destroy_key(gk)
    ctx.destroy_key(k)
    ctx.close()


def test_n16_cmc_relin_task():
    """BFV mult_relin x2 at level 23 of the N = 2^16 chain through the task runtime (fixture emitted by the reference's
    frontend, tools/gen_task_fixtures.py), vs the oracle and decrypted"""
    need_gpu()
    from lattisense_amd.task import Argument, Ciphertext, FheTaskGpu, KeySwitchKey
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    name = "bfv_n65536_l23_cmc_relin_x2"
    g = json.load(open(os.path.join(TASKS, name, "mega_ag.json")))
    P = g["parameter"]
    C = params.bfv_n16_chain()
    assert (P["n"], P["q"], P["p"], P["t"]) == (C["n"], C["q"], C["p"], C["t"])
    n, lvl, t = P["n"], P["max_level"], P["t"]
    o = Oracle(n, P["q"], P["p"], t)
    c = Client(o, seed=7)
    rng = np.random.default_rng(23)
    xm = [rng.integers(0, t, size=n, dtype=np.uint64) for _ in range(2)]
    ym = [rng.integers(0, t, size=n, dtype=np.uint64) for _ in range(2)]
    xs, ys = [c.bfv_encrypt(m, lvl) for m in xm], [c.bfv_encrypt(m, lvl) for m in ym]
    rlk = c.gen_relin_key(lvl)
    task = FheTaskGpu(os.path.join(TASKS, name))
    try:
        zs = [Ciphertext.empty(1, lvl, n) for _ in range(2)]
        task.run([Argument("xs", [Ciphertext(x) for x in xs]), Argument("ys", [Ciphertext(y) for y in ys]),
                  Argument("rlk_ntt", [KeySwitchKey(rlk, lvl, len(P["p"]))])], [Argument("zs", zs)])
    finally:
        task.close()
    for i in range(2):
        assert np.array_equal(zs[i].data, o.bfv_mult_relin(lvl, xs[i], ys[i], rlk, lvl))
        assert np.array_equal(c.bfv_decrypt(zs[i].data), xm[i] * ym[i] % np.uint64(t))
