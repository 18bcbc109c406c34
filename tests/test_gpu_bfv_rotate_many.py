"""Hoisted BFV rotations (lsa_bfv_rotate_many): one decomposition of the input for several Galois elements, the automorphism
applied by the ModDown tail's loads (kernels.hip k_sub_mul_perm).  Every output bit-identical to lsa_bfv_rotate and to the
CPU oracle, under every switch that changes the path (LSA_ROT_SCATTER, fused tails, tile batch), with an output aliasing the
input; at the full N = 2^16 ring; at message level (decrypt == the rotated vector, unittests/test_gpu_bfv.cpp:493-528); and
through the task runtime on the reference's BFV_4_advanced_rotate_col graphs, which now run as ONE hoisted batch."""
import ctypes

import numpy as np
import pytest

from lattisense_amd import params
from tests import ref_suite as rs
from tests.gpu_util import env, need_gpu, rand_ct

pytestmark = pytest.mark.gpu


def _rand_key(rng, q, p, klvl, n):
    beta = (klvl + 1 + len(p) - 1) // len(p)
    key = np.empty((beta, 2, klvl + 1 + len(p), n), dtype=np.uint64)
    for j, m in enumerate(q[: klvl + 1] + p):
        key[:, :, j, :] = rng.integers(0, m, size=(beta, 2, n), dtype=np.uint64)
    return key


def _rotate_many_raw(ctx, lvl, in_ptr, els, keys, outs, batch):
    from lattisense_amd._native import lib
    m = len(els)
    s = 2 * (lvl + 1) * ctx.n
    return lib().lsa_bfv_rotate_many(ctx.h, lvl, in_ptr, m, (ctypes.c_uint64 * max(m, 1))(*els),
                                     (ctypes.c_void_p * max(m, 1))(*[k.value if k is not None else None for k in keys]),
                                     (ctypes.c_void_p * max(m, 1))(*outs), batch, s, s, ctx.stream)


@pytest.fixture(scope="module")
def n14():
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    from oracle.pyoracle import Oracle
    P = params.BFV_DEFAULT[16384]
    n, q, p, t = 16384, P["q"], P["p"], P["t"]
    ctx = DeviceContext(ALGO_BFV, n, q, p, t)
    o = Oracle(n, q, p, t)
    yield ctx, o
    ctx.close()


def test_operator_parity_every_path(n14):
    need_gpu()
    from lattisense_amd._native import LsaError, check, lib
    from oracle.client import galois_element_for_col_rotation
    ctx, o = n14
    n, q, p = ctx.n, ctx.q, params.BFV_DEFAULT[16384]["p"]
    lvl, klvl, batch = 3, 5, 3
    L = lvl + 1
    shape = (batch, 2, L, n)
    rng = np.random.default_rng(1493)
    A = rand_ct(rng, q[:L], 2, n, batch)
    da = ctx.upload(A)
    els = [5, pow(5, 77, 2 * n), galois_element_for_col_rotation(-900, n), 2 * n - 1]
    raw = {g: _rand_key(rng, q, p, klvl, n) for g in els}
    keys = {g: ctx.upload_key(raw[g], klvl) for g in els}
    refs = {}
    for g in els:
        refs[g] = ctx.download(ctx.bfv_rotate(lvl, da, g, keys[g], batch), shape)
        assert np.array_equal(refs[g][1], o.bfv_rotate(lvl, A[1], g, raw[g], klvl)), g
    try:
        for scatter in ("1", "0"):
            with env(LSA_ROT_SCATTER=scatter):
                for fuse in (1, 0):
                    check(lib().lsa_set_fuse_tails(ctx.h, fuse))
                    for tile in (0, 1, 3):
                        ctx.set_tile_batch(tile)
                        outs = ctx.bfv_rotate_many(lvl, da, keys, batch)
                        for g in els:
                            assert np.array_equal(ctx.download(outs[g], shape), refs[g]), (scatter, fuse, tile, g)
                        # an output that IS the input (the first one: the others must still see the intact ciphertext)
                        alias = ctx.upload(A)
                        others = [ctx.alloc(batch * 2 * L * n) for _ in els[1:]]
                        check(_rotate_many_raw(ctx, lvl, alias.ptr, els, [keys[g] for g in els], [alias.ptr] + [b.ptr for b in others],
                                               batch))
                        assert np.array_equal(ctx.download(alias, shape), refs[els[0]]), (scatter, fuse, tile)
                        for g, b in zip(els[1:], others):
                            assert np.array_equal(ctx.download(b, shape), refs[g]), (scatter, fuse, tile, g)
    finally:
        check(lib().lsa_set_fuse_tails(ctx.h, 1))
        ctx.set_tile_batch(0)
    # one element: the same as bfv_rotate
    one = ctx.bfv_rotate_many(lvl, da, {els[2]: keys[els[2]]}, batch)
    assert np.array_equal(ctx.download(one[els[2]], shape), refs[els[2]])
    # nothing to do is not an error; a missing key is
    assert lib().lsa_bfv_rotate_many(ctx.h, lvl, da.ptr, 0, None, None, None, batch, 2 * L * n, 2 * L * n, ctx.stream) == 0
    spare = ctx.alloc(batch * 2 * L * n)
    with pytest.raises(LsaError, match="null key"):
        check(_rotate_many_raw(ctx, lvl, da.ptr, els[:2], [keys[els[0]], None], [spare.ptr, spare.ptr], batch))
    for k in keys.values():
        ctx.destroy_key(k)


def test_message_level_rotations(n14):
    """oracle client keys: decrypt(rotate_many(x)) == the rotated columns / swapped rows (test_gpu_bfv.cpp:520-524)"""
    need_gpu()
    from oracle.client import Client, galois_element_for_col_rotation, galois_element_for_row_rotation
    ctx, o = n14
    n, t = ctx.n, ctx.t
    lvl, klvl = 3, 5
    c = Client(o, seed=16384)
    rng = np.random.default_rng(5)
    x = rng.integers(0, t, size=n, dtype=np.uint64)
    A = c.bfv_encrypt(x, lvl)[None]
    steps = [-900, 20, 400, 2000, 3009]
    els = [galois_element_for_col_rotation(s, n) for s in steps] + [galois_element_for_row_rotation(n)]
    raw = {g: c.gen_galois_key(g, klvl) for g in els}
    keys = {g: ctx.upload_key(raw[g], klvl) for g in els}
    outs = ctx.bfv_rotate_many(lvl, ctx.upload(A), keys, 1)
    h = n // 2
    for s, g in zip(steps + [None], els):
        got = ctx.download(outs[g], (1, 2, lvl + 1, n))
        assert np.array_equal(got[0], o.bfv_rotate(lvl, A[0], g, raw[g], klvl)), s
        want = (np.concatenate([x[h:], x[:h]]) if s is None
                else np.concatenate([np.roll(x[:h], -s), np.roll(x[h:], -s)]))
        assert np.array_equal(c.bfv_decrypt(got[0]), want), s
    for k in keys.values():
        ctx.destroy_key(k)


def test_full_ring_n16():
    """N = 2^16 (params.bfv_n16_chain, 24 Q + 4 P) at the top level, two elements, against the oracle"""
    need_gpu()
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    from oracle.client import galois_element_for_col_rotation, galois_element_for_row_rotation
    from oracle.pyoracle import Oracle
    C = params.bfv_n16_chain()
    n, q, p, t = C["n"], C["q"], C["p"], C["t"]
    lvl = len(q) - 1
    ctx = DeviceContext(ALGO_BFV, n, q, p, t)
    o = Oracle(n, q, p, t)
    rng = np.random.default_rng(65536)
    A = rand_ct(rng, q, 2, n, 1)
    els = [galois_element_for_col_rotation(1, n), galois_element_for_row_rotation(n)]
    raw = {g: _rand_key(rng, q, p, lvl, n) for g in els}
    keys = {g: ctx.upload_key(raw[g], lvl) for g in els}
    outs = ctx.bfv_rotate_many(lvl, ctx.upload(A), keys, 1)
    for g in els:
        got = ctx.download(outs[g], (1, 2, lvl + 1, n))
        assert np.array_equal(got[0], o.bfv_rotate(lvl, A[0], g, raw[g], lvl)), g
    for k in keys.values():
        ctx.destroy_key(k)
    ctx.close()


@pytest.fixture(scope="module")
def suite(tmp_path_factory):
    return rs.unpack(str(tmp_path_factory.mktemp("ref_suite_rot")))


@pytest.mark.parametrize("tag", ["bfv_param_default_n16384_t10001", "bfv_param_default_n8192_t10001",
                                 "bfv_param_custom_n8192_t10001"])
def test_runtime_hoists_advanced_rotate_col(suite, tag):
    """the reference's BFV_4_advanced_rotate_col (4 ciphertexts x 5 steps) at every level: bit-exact against the oracle and
    ONE GPU batch (five separate rotation buckets without hoisting)"""
    need_gpu()
    ran = 0
    for _, name, lv, path in rs.tasks(suite, tag):
        if not name.startswith("BFV_4_advanced_rotate_col"):
            continue
        _, st = rs.run_and_compare(path, seed=lv)
        assert st["gpu_batches"] == 1, (path, st)
        ran += 1
    assert ran >= 2, tag
