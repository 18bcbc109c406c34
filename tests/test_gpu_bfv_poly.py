"""BFV polynomial evaluator and constant operands on the device (lsa_bfv_poly_* / lsa_bfv_poly_eval, lsa_bfv_affine_const;
csrc/bfv_poly.hip over k_bfv_poly_leaves) against their CPU restatement tests/bfv_poly_model.py (oracle primitives only; held to
the mathematics by tests/test_bfv_poly_api.py) on one batch item, and against the composition of the public entry points the
header names.  Every comparison is word for word.  The rig is that of tests/test_gpu_bfv_dot.py: N = 2^12 on the N = 2^13 primes,
random ciphertexts, a random key at level 2.  The last test encrypts real messages and decrypts p(values) mod t exactly."""
import ctypes
import os

import numpy as np
import pytest

from lattisense_amd import params
from tests import bfv_poly_model as model
from tests.gpu_util import need_gpu, rand_ct
from tests.test_gpu_bfv_dot import Rig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSA_ERR_ARG = 1
N = 1 << 12
T = params.BFV_DEFAULT[8192]["t"]


def _coeffs(seed, n):
    return [int(x) for x in np.random.default_rng(seed).integers(1, T, n)]


def _cases():
    """(id, coefficients, log_baby)"""
    out = [("dense%d" % n, _coeffs(n, n), 0) for n in (2, 3, 8, 16, 24)]
    out += [("dense16_b%d" % b, _coeffs(16, 16), b) for b in (1, 2, 3, 4)]   # b = 4: 15 sources, the ninth-term fold runs
    out.append(("dense24_b1", _coeffs(24, 24), 1))                           # 12 leaves: two launches, the second short
    out.append(("odd32", [c if k % 2 else 0 for k, c in enumerate(_coeffs(32, 32))], 0))
    out.append(("upper_zero32", _coeffs(33, 16) + [0] * 16, 0))
    out.append(("x12", [0] * 12 + [1], 0))
    out.append(("const_leaves16", [c if k % 4 == 0 else 0 for k, c in enumerate(_coeffs(34, 16))], 2))
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def rig():
    need_gpu()
    P = params.BFV_DEFAULT[8192]
    r = Rig(N, P["q"], P["p"], P["t"], 2, 4150)
    yield r
    r.close()


@pytest.fixture(scope="module")
def inputs(rig):
    """per level: host [3][2][level+1][N] with items 0 and 2 equal, and its device copy"""
    out = {}
    for lvl in range(3):
        h = rig.ct(lvl, 3)
        h[2] = h[0]
        out[lvl] = (h, rig.ctx.upload(h))
    return out


def run_plan(rig, coeffs, lvl, d_in, batch, log_baby=0, out=None):
    from lattisense_amd.device import BfvPolynomialPlan
    plan = BfvPolynomialPlan(rig.ctx, coeffs, lvl, log_baby)
    try:
        got = rig.ctx.download(plan.run(d_in, batch, rig.k, out=out), (batch, 2, lvl + 1, rig.n))
        return got, plan.info()
    finally:
        plan.close()


def test_leaf_kernel_through_affine_const(rig, inputs):
    """levels 0..2, batch 3, k and c at the values where the centring and the scale-up turn, against vec and bfv_scale_up; once in
    place; with k = 1 only word [0][j][0] of each limb differs from the input"""
    ctx, o, t = rig.ctx, rig.o, rig.t
    rng = np.random.default_rng(9)
    specials = [0, 1, t - 1, (t - 1) // 2, (t + 1) // 2]
    for lvl in range(3):
        h, d = inputs[lvl]
        shape = (3, 2, lvl + 1, N)
        for k in specials + [int(rng.integers(2, t - 1))]:
            for c in specials + [int(rng.integers(2, t - 1))]:
                got = ctx.download(ctx.bfv_affine_const(lvl, d, k, c, 3), shape)
                for b in (0, 1):
                    assert np.array_equal(got[b], model.affine_const(o, lvl, h[b], k, c)), (lvl, k, c, b)
                assert np.array_equal(got[2], got[0]), (lvl, k, c)
                if k == 1:
                    diff = np.argwhere(got != h)
                    want = [[b, 0, j, 0] for b in range(3) for j in range(lvl + 1)] if c else []
                    assert diff.tolist() == want, (lvl, c)
        k, c = (t + 1) // 2, 12345
        want = ctx.download(ctx.bfv_affine_const(lvl, d, k, c, 3), shape)
        work = ctx.upload(h)
        assert ctx.bfv_affine_const(lvl, work, k, c, 3, out=work) is work
        assert np.array_equal(ctx.download(work, shape), want), ("in place", lvl)


def test_affine_const_many_distinct_constants_on_a_callers_stream(rig, inputs):
    """the constants travel in the launch's arguments: 300 distinct (k, c) pairs, queued back to back on a non-blocking stream of
    the caller's into 300 outputs without a host wait in between, each the model's words -- and the entry point's own code neither
    allocates, nor copies to the device, nor caches anything per pair"""
    from lattisense_amd._native import check, lib
    ctx, o, t, lvl = rig.ctx, rig.o, rig.t, 2
    h, d = inputs[lvl]
    w = 2 * (lvl + 1) * N
    rng = np.random.default_rng(300)
    pairs = [(int(k), int(c)) for k, c in zip(rng.integers(0, t, 300), rng.integers(0, t, 300))]
    assert len(set(pairs)) == 300
    outs = ctx.alloc(300 * w)
    st = ctypes.c_void_p()
    check(lib().lsa_stream_create(ctx.h, ctypes.byref(st)))
    try:
        ctx.sync()
        for i, (k, c) in enumerate(pairs):
            check(lib().lsa_bfv_affine_const(ctx.h, lvl, d.ptr, w, k, c, outs.ptr + 8 * i * w, w, 1, st))
        check(lib().lsa_stream_synchronize(ctx.h, st))
    finally:
        check(lib().lsa_stream_destroy(ctx.h, st))
    got = ctx.download(outs, (300, 2, lvl + 1, N))
    for i, (k, c) in enumerate(pairs):
        assert np.array_equal(got[i], model.affine_const(o, lvl, h[0], k, c)), (i, k, c)
    src = open(os.path.join(ROOT, "lattisense_amd", "csrc", "bfv_poly.hip")).read()
    body = src[src.index("void bfv_affine_const("):]
    assert "raw_vec" not in body and "const_vec" not in body and "hipMalloc" not in body and "hipMemcpy" not in body


def test_batch_sizes_share_one_workspace(rig, inputs):
    """one plan run at batch 3, 1, 2 and 3 again: the same words per item every time (the workspace of another batch size is given
    back, not kept beside the new one)"""
    from lattisense_amd.device import BfvPolynomialPlan
    ctx, lvl = rig.ctx, 2
    h, d = inputs[lvl]
    plan = BfvPolynomialPlan(ctx, _coeffs(16, 16), lvl)
    try:
        ref = ctx.download(plan.run(d, 3, rig.k), (3, 2, lvl + 1, N))
        for batch in (1, 2, 3):
            got = ctx.download(plan.run(d, batch, rig.k), (batch, 2, lvl + 1, N))
            assert np.array_equal(got, ref[:batch]), batch
    finally:
        plan.close()


@pytest.mark.parametrize("lvl", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_evaluator_against_the_model(rig, inputs, case, lvl):
    """batch 3 with items 0 and 2 equal and item 1 different: item 1 is the model's, item 2 is item 0, item 1 is not"""
    from lattisense_amd.device import bfv_poly_plan
    name, coeffs, log_baby = case
    h, d = inputs[lvl]
    got, info = run_plan(rig, coeffs, lvl, d, 3, log_baby)
    counts = model.counts(coeffs, log_baby)
    assert {k: info[k] for k in model.COUNTS} == counts and bfv_poly_plan(rig.t, coeffs, log_baby) == counts
    assert info["level"] == lvl and info["n_coef"] == len(coeffs)
    if name == "dense24_b1":
        assert counts["n_leaves"] == 12 and counts["n_leaf_launches"] == 2
    if name == "dense16_b4":
        assert counts["n_pairs"] == 0 and counts["n_mult"] == 14      # 15 sources in one launch, out is leaf_0 itself
    assert np.array_equal(got[1], model.evaluate(rig.o, lvl, h[1], coeffs, rig.key, rig.klvl, log_baby)), (name, lvl)
    assert np.array_equal(got[2], got[0]) and not np.array_equal(got[1], got[0]), (name, lvl)


def test_composition_of_public_entry_points(rig, inputs):
    """c0 + c1 x + c2 x^2 + c4 x^4 + c5 x^5 + c6 x^6 at log_baby 2: x^2 and y = x^4 by lsa_bfv_mult_relin, the two two-term leaves
    by lsa_bfv_affine_const per term and lsa_poly_addsub, the sum by lsa_bfv_dot with leaf_0 as its addend -- the same words"""
    ctx, lvl, batch = rig.ctx, 2, 3
    h, d = inputs[lvl]
    cf = _coeffs(77, 7)
    cf[3] = 0
    got, info = run_plan(rig, cf, lvl, d, batch, 2)
    assert (info["n_mult"], info["n_leaves"], info["n_pairs"]) == (3, 2, 1)
    x2 = ctx.bfv_mult_relin(lvl, d, d, rig.k, batch)
    y = ctx.bfv_mult_relin(lvl, x2, x2, rig.k, batch)
    leaves = []
    for g in (0, 1):
        a = ctx.bfv_affine_const(lvl, d, cf[4 * g + 1], cf[4 * g], batch)
        b = ctx.bfv_affine_const(lvl, x2, cf[4 * g + 2], 0, batch)
        leaves.append(ctx.addsub(0, lvl, 2, a, b, batch))
    want = ctx.download(ctx.bfv_dot(lvl, [leaves[1]], [y], rig.k, batch, addend=leaves[0]), (batch, 2, lvl + 1, N))
    assert np.array_equal(got, want)


def test_switches(rig, inputs):
    """tile batch 0 / 1 / 2 and single / dual stream give the same words; so does a fresh context with lsa_set_fp64_ntt(0).  This
    chain (54 / 55-bit Q, 55-bit P, 61-bit auxiliary primes) has no FP64-engine limb, so both contexts run the integer engine on
    every row: the run shows that the setting itself changes nothing.  The comparison of the two engines lives in
    tests/test_gpu_bfv_operator_chains.py (test_poly_eval_variants on the fp and mixed chains)."""
    from lattisense_amd._native import check, lib
    ctx, lvl, batch = rig.ctx, 2, 3
    h, d = inputs[lvl]
    coeffs = _coeffs(16, 16)
    ref, _ = run_plan(rig, coeffs, lvl, d, batch)
    try:
        for dual in (0, 1):
            check(lib().lsa_set_dual_stream(ctx.h, dual))
            for tile in (0, 1, 2):
                ctx.set_tile_batch(tile)
                got, _ = run_plan(rig, coeffs, lvl, d, batch)
                assert np.array_equal(got, ref), (dual, tile)
    finally:
        check(lib().lsa_set_dual_stream(ctx.h, 0))
        ctx.set_tile_batch(0)
    P = params.BFV_DEFAULT[8192]
    other = Rig(N, P["q"], P["p"], P["t"], 2, 4150, fp64=False)   # the same seed: the same key
    try:
        assert np.array_equal(other.key, rig.key)
        got, _ = run_plan(other, coeffs, lvl, other.ctx.upload(h), batch)
        assert np.array_equal(got, ref), "fp64 off"
    finally:
        other.close()


def test_argument_errors(rig, inputs):
    """every argument error returns LSA_ERR_ARG with a message that begins "bfv_poly" (or "lsa_bfv_affine_const"), queues nothing
    (the output keeps its sentinel), and leaves the context and the plan usable"""
    from lattisense_amd._native import lib
    from lattisense_amd.device import ALGO_BFV, ALGO_CKKS, BfvPolynomialPlan, DeviceContext
    L = lib()
    ctx, lvl, batch = rig.ctx, 2, 2
    h, d = inputs[lvl]
    w = 2 * (lvl + 1) * N
    coeffs = _coeffs(8, 8)
    cf = (ctypes.c_uint64 * 8)(*coeffs)
    P = params.BFV_DEFAULT[8192]
    C = params.CKKS_DEFAULT[16384]
    ckks = DeviceContext(ALGO_CKKS, 4096, C["q"][:3], C["p"])
    bfv2 = DeviceContext(ALGO_BFV, N, P["q"], P["p"], P["t"])
    out = ctx.upload(np.full(batch * w + 2, 7, dtype=np.uint64))
    low_key = ctx.upload_key(rand_ct(rig.rng, rig.q[:2] + rig.p, 2, N, 2), 1)
    plan = BfvPolynomialPlan(ctx, coeffs, lvl)
    try:
        def create_fails(needle, c=ctx, level=lvl, n=8, coef=cf, b=0, handle=True):
            hd = ctypes.c_void_p()
            rc = L.lsa_bfv_poly_create(c.h, level, n, coef, b, None, ctypes.byref(hd) if handle else None)
            msg = L.lsa_last_error().decode()
            assert rc == LSA_ERR_ARG and msg.startswith("bfv_poly") and needle in msg, (needle, rc, msg)
            assert not hd.value

        create_fails("BFV", c=ckks, level=0)
        create_fails("level", level=3)
        create_fails("level", level=-1)
        create_fails("n_coef", n=0)
        create_fails("n_coef", n=257)
        create_fails("below t", coef=(ctypes.c_uint64 * 8)(*(coeffs[:7] + [rig.t])))
        create_fails("degree 0", coef=(ctypes.c_uint64 * 8)(5, 0, 0, 0, 0, 0, 0, 0))
        create_fails("log_baby", b=5)
        create_fails("log_baby", b=-1)
        create_fails("null", coef=None)
        create_fails("null", handle=False)

        def eval_fails(needle, c=ctx, p=plan.h, i=d.ptr, o=out.ptr, bt=batch, si=w, so=w, key=rig.k):
            rc = L.lsa_bfv_poly_eval(c.h, p, i, o, bt, si, so, key, ctx.stream)
            msg = L.lsa_last_error().decode()
            assert rc == LSA_ERR_ARG and msg.startswith("bfv_poly") and needle in msg, (needle, rc, msg)

        eval_fails("null", p=None)
        eval_fails("another context", c=bfv2)
        eval_fails("null", i=None)
        eval_fails("null", o=None)
        eval_fails("key", key=None)
        eval_fails("key", key=low_key)
        eval_fails("overlap", o=d.ptr)
        eval_fails("overlap", o=d.ptr + 8 * N)
        eval_fails("aligned", o=out.ptr + 8)
        eval_fails("aligned", i=d.ptr + 8)
        eval_fails("even", so=w + 1)
        eval_fails("even", si=w + 1)
        eval_fails("stride", so=w - 2)
        eval_fails("stride", si=0)

        def affine_fails(needle, c=ctx, level=lvl, i=d.ptr, si=w, k=3, cst=4, o=out.ptr, so=w, bt=batch):
            rc = L.lsa_bfv_affine_const(c.h, level, i, si, k, cst, o, so, bt, ctx.stream)
            msg = L.lsa_last_error().decode()
            assert rc == LSA_ERR_ARG and msg.startswith("lsa_bfv_affine_const") and needle in msg, (needle, rc, msg)

        affine_fails("BFV", c=ckks, level=0)
        affine_fails("level", level=3)
        affine_fails("below t", k=rig.t)
        affine_fails("below t", cst=rig.t)
        affine_fails("null", i=None)
        affine_fails("null", o=None)
        affine_fails("overlap", o=d.ptr + 8 * N)        # in place means the same pointer and the same stride
        affine_fails("overlap", o=d.ptr, so=w + 2)
        affine_fails("aligned", o=out.ptr + 8)
        affine_fails("even", si=w + 1)
        affine_fails("stride", so=w - 2)
        assert np.all(ctx.download(out, (batch * w + 2,)) == 7)         # nothing was queued
        for bt in (0, -1):                                               # batch <= 0: a no-op
            assert L.lsa_bfv_poly_eval(ctx.h, plan.h, d.ptr, out.ptr, bt, w, w, rig.k, ctx.stream) == 0
            assert L.lsa_bfv_affine_const(ctx.h, lvl, d.ptr, w, 3, 4, out.ptr, w, bt, ctx.stream) == 0
        assert np.all(ctx.download(out, (batch * w + 2,)) == 7)
        got = ctx.download(plan.run(d, batch, rig.k), (batch, 2, lvl + 1, N))   # the plan and the context stay usable
        assert np.array_equal(got[1], model.evaluate(rig.o, lvl, h[1], coeffs, rig.key, rig.klvl))
    finally:
        plan.close()
        ckks.close()
        bfv2.close()


def test_semantics_real_messages():
    """encrypted slot values, dense 8 at the planner's choice and dense 16 at log_baby 3: the device words are the model's and
    decrypt to exactly p(values) mod t in every slot"""
    need_gpu()
    from lattisense_amd.device import ALGO_BFV, BfvPolynomialPlan, DeviceContext
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    P = params.BFV_DEFAULT[8192]
    q, p, t = P["q"], P["p"], P["t"]
    lvl = 2
    o = Oracle(N, q, p, t)
    c = Client(o, seed=41)
    rlk = c.gen_relin_key(lvl)
    rng = np.random.default_rng(41)
    x = rng.integers(0, t, N, dtype=np.uint64)
    ct = c.bfv_encrypt(x, lvl)
    ctx = DeviceContext(ALGO_BFV, N, q, p, t)
    try:
        k = ctx.upload_key(rlk, lvl)
        d = ctx.upload(ct[None])
        for n_coef, log_baby in ((8, 0), (16, 3)):
            cf = [int(v) for v in rng.integers(0, t, n_coef)]
            plan = BfvPolynomialPlan(ctx, cf, lvl, log_baby)
            try:
                got = ctx.download(plan.run(d, 1, k), (1, 2, lvl + 1, N))[0]
            finally:
                plan.close()
            assert np.array_equal(got, model.evaluate(o, lvl, ct, cf, rlk, lvl, log_baby)), n_coef
            assert np.array_equal(np.asarray(c.bfv_decrypt(got)).astype(object), model.polynomial_mod_t(cf, x, t)), n_coef
    finally:
        ctx.close()
