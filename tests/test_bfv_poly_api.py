"""BFV polynomial evaluator without a GPU: the entry points are exported, bound and declared; the planner of lsa_bfv_poly_plan
(csrc/bfv_poly.h, through the library and compiled for the host by tests/cpp/test_bfv_poly_plan.cpp) against the planner stated in
plain Python in tests/bfv_poly_model.py; the refusals that need no device; the constants of the leaf kernel against the oracle's
scaleUp; and the model itself held to the mathematics: on the oracle alone, with real encryptions, it decrypts exactly to
p(values) mod t."""
import ctypes
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from lattisense_amd import params
from tests import bfv_poly_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lattisense_amd.h")
ENTRY_POINTS = {"lsa_bfv_poly_plan": 10, "lsa_bfv_poly_create": 7, "lsa_bfv_poly_destroy": 1, "lsa_bfv_poly_info": 9,
                "lsa_bfv_poly_eval": 9, "lsa_bfv_affine_const": 10}
T = 65537
LSA_ERR_ARG = 1


def polynomials():
    """(name, coefficients) over t = 65537: the shapes the planner treats differently"""
    rng = np.random.default_rng(4150)

    def dense(n):
        return [int(x) for x in rng.integers(1, T, n)]

    out = [("dense%d" % n, dense(n)) for n in (2, 3, 4, 8, 16, 24, 32, 41, 64, 256)]
    odd = dense(32)
    out.append(("odd32", [c if k % 2 else 0 for k, c in enumerate(odd)]))
    out.append(("upper_zero32", dense(16) + [0] * 16))
    out.append(("x12", [0] * 12 + [1]))
    out.append(("const_leaves16", [c if k % 4 == 0 else 0 for k, c in enumerate(dense(16))]))
    return out


@pytest.fixture(scope="module")
def native():
    from lattisense_amd import build, _native
    build.build_native()
    return _native


def test_header_signatures_and_wrappers(native):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    from lattisense_amd import device
    L = native.lib()
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\b(?:int|void)\s+%s\s*\(([^;]*?)\)\s*;" % name, txt, flags=re.S)
        assert m, name + " is not declared"
        assert len(m.group(1).split(",")) == nargs, name
        assert len(native.SIGNATURES[name][1]) == nargs, name
        assert hasattr(L, name), name + " is not exported"
    assert "typedef struct lsa_bfv_polynomial_st* lsa_bfv_polynomial;" in txt
    assert list(inspect.signature(device.bfv_poly_plan).parameters) == ["t", "coeffs", "log_baby"]
    assert list(inspect.signature(device.BfvPolynomialPlan.__init__).parameters) == ["self", "ctx", "coeffs", "level", "log_baby"]
    assert list(inspect.signature(device.BfvPolynomialPlan.run).parameters) == ["self", "in_buf", "batch", "rlk", "out"]
    assert list(inspect.signature(device.DeviceContext.bfv_affine_const).parameters) == ["self", "level", "ct", "k", "c", "batch", "out"]
    assert issubclass(device.BfvPolynomialPlan, device._Plan) and device.BfvPolynomialPlan._destroy == "lsa_bfv_poly_destroy"
    assert callable(device.BfvPolynomialPlan.info) and callable(device.BfvPolynomialPlan.close)


def test_python_planner_on_known_values():
    """the figures of the issue's table and a few counted by hand, from the Python planner alone"""
    d16, d8 = [1] * 16, [1] * 8
    assert [model.counts(d16, b)["depth"] for b in (1, 2, 3, 4)] == [5, 5, 4, 4]
    assert [model.counts(d8, b)["depth"] for b in (1, 2, 3, 4)] == [4, 3, 3, 3]
    assert model.counts(d16) == {"log_baby": 3, "depth": 4, "n_mult": 8, "n_leaves": 2, "n_leaf_launches": 1, "n_pairs": 1}
    assert model.counts(d8) == {"log_baby": 2, "depth": 3, "n_mult": 4, "n_leaves": 2, "n_leaf_launches": 1, "n_pairs": 1}
    # dense 24 at log_baby 1: 12 leaves in two launches; x, y .. y^11 (11 giants), one sum
    assert model.counts([1] * 24, 1) == {"log_baby": 1, "depth": 6, "n_mult": 12, "n_leaves": 12, "n_leaf_launches": 2, "n_pairs": 11}
    # x^12 at log_baby 2: leaf_3 = 1 (a constant), y, y^2, y^3, one sum; x^2 for y; no leaf_0
    assert model.counts([0] * 12 + [1], 2) == {"log_baby": 2, "depth": 5, "n_mult": 5, "n_leaves": 1, "n_leaf_launches": 1, "n_pairs": 1}
    # c0 + c1 x at log_baby 4: the leaf alone
    assert model.counts([3, 5], 4) == {"log_baby": 4, "depth": 0, "n_mult": 0, "n_leaves": 1, "n_leaf_launches": 1, "n_pairs": 0}


def test_plan_entry_point_against_the_python_planner(native):
    from lattisense_amd.device import bfv_poly_plan
    for name, cf in polynomials():
        for b in range(5):
            assert bfv_poly_plan(T, cf, b) == model.counts(cf, b), (name, b)
    cases = dict(polynomials())
    assert bfv_poly_plan(T, cases["dense8"])["log_baby"] == 2
    assert bfv_poly_plan(T, cases["dense16"])["log_baby"] == 3
    # trailing zeros change G but add no leaf
    assert bfv_poly_plan(T, cases["dense8"] + [0] * 9, 2) == model.counts(cases["dense8"] + [0] * 9, 2)
    assert native.lib().lsa_bfv_poly_plan(T, 2, (ctypes.c_uint64 * 2)(1, 1), 0, None, None, None, None, None, None) == 0   # outputs optional


def test_plan_host_function_against_the_python_planner(tmp_path):
    """csrc/bfv_poly.h compiles for the host alone (g++, no HIP) and gives the same counts under -fsanitize=undefined"""
    exe = str(tmp_path / "test_bfv_poly_plan")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-DLSA_EMULATE", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_bfv_poly_plan.cpp"), "-o", exe])
    cases = [(cf, b) for _, cf in polynomials() for b in range(5)]
    text = "".join("%d %d %d %s\n" % (T, b, len(cf), " ".join(map(str, cf))) for cf, b in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    got = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    assert len(got) == len(cases)
    for (cf, b), r in zip(cases, got):
        assert r == tuple(model.counts(cf, b)[k] for k in model.COUNTS), (len(cf), b)


def test_leaf_constants_against_the_oracle(tmp_path):
    """the words the plan uploads for the leaf kernel (csrc/bfv_poly.h, compiled for the host): K centred mod q_j, and word 0 of
    the oracle's scaleUp of the constant polynomial, at levels 0..2 of the N = 2^13 primes and at an even t"""
    from oracle.pyoracle import Oracle
    exe = str(tmp_path / "test_bfv_poly_plan")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-DLSA_EMULATE", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_bfv_poly_plan.cpp"), "-o", exe])
    P = params.BFV_DEFAULT[8192]
    rng = np.random.default_rng(3)
    for t in (P["t"], 1 << 16):
        o = Oracle(64, P["q"], P["p"], t)
        vals = [0, 1, t - 1, (t - 1) // 2, (t + 1) // 2, t // 2, t // 2 + 1] + [int(x) for x in rng.integers(0, t, 20)]
        cases = [(lvl, v, vals[(i * 7 + 3) % len(vals)]) for lvl in range(3) for i, v in enumerate(vals)]
        text = "".join("%d %d %d %d %s\n" % (t, k, c, lvl + 1, " ".join(map(str, o.q[: lvl + 1]))) for lvl, k, c in cases)
        out = subprocess.run([exe, "consts"], input=text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
        rows = [[int(x) for x in line.split()] for line in out.stdout.splitlines()]
        assert len(rows) == len(cases)
        for (lvl, k, c), r in zip(cases, rows):
            pt = np.zeros(o.n, dtype=np.uint64)
            pt[0] = c
            up = o.bfv_scale_up(lvl, pt)
            assert not up[:, 1:].any()
            assert r[0::2] == [model.centred(k, t) % o.q[j] for j in range(lvl + 1)], (t, lvl, k)
            assert r[1::2] == [int(up[j, 0]) for j in range(lvl + 1)], (t, lvl, c)


def test_refusals_without_a_device(native):
    L = native.lib()

    def refused(needle, t, cf, b, n=None):
        arr = (ctypes.c_uint64 * max(len(cf), 1))(*cf) if cf is not None else None
        rc = L.lsa_bfv_poly_plan(t, len(cf) if n is None else n, arr, b, None, None, None, None, None, None)
        msg = L.lsa_last_error().decode()
        assert rc == LSA_ERR_ARG and msg.startswith("bfv_poly") and needle in msg, (needle, rc, msg)

    refused("n_coef", T, [], 0)
    refused("n_coef", T, [1] * 257, 0)
    refused("below t", T, [1, T], 0)
    refused("below t", T, [T + 5, 1], 0)
    refused("degree 0", T, [7], 0)
    refused("degree 0", T, [7, 0, 0], 0)
    refused("degree 0", T, [0, 0, 0, 0], 0)
    refused("log_baby", T, [1, 1], -1)
    refused("log_baby", T, [1, 1], 5)
    refused("null", T, None, 0, n=2)
    # the entry points that take a context refuse a null one before they touch a device
    h = ctypes.c_void_p()
    cf = (ctypes.c_uint64 * 2)(1, 1)
    assert L.lsa_bfv_poly_create(None, 0, 2, cf, 0, None, ctypes.byref(h)) == LSA_ERR_ARG
    assert L.lsa_last_error().decode().startswith("bfv_poly")
    assert L.lsa_bfv_poly_eval(None, None, None, None, 1, 0, 0, None, None) == LSA_ERR_ARG
    assert L.lsa_last_error().decode().startswith("bfv_poly")
    assert L.lsa_bfv_poly_info(None, None, None, None, None, None, None, None, None) == LSA_ERR_ARG
    assert L.lsa_last_error().decode().startswith("bfv_poly")
    assert L.lsa_bfv_affine_const(None, 0, None, 0, 1, 1, None, 0, 1, None) == LSA_ERR_ARG
    assert L.lsa_last_error().decode().startswith("lsa_bfv_affine_const")
    L.lsa_bfv_poly_destroy(None)   # a null handle is nothing to destroy


@pytest.fixture(scope="module")
def rig():
    """N = 2^12, level 2 on the N = 2^13 primes; a secret key, its relinearisation key"""
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    P = params.BFV_DEFAULT[8192]
    o = Oracle(1 << 12, P["q"], P["p"], P["t"])
    c = Client(o, seed=415)
    return o, c, c.gen_relin_key(2)


def test_affine_const_model_decrypts(rig):
    """k * x + c slot-wise, at the constants where the centring and the scale-up turn: the kernel's semantics on the oracle"""
    o, c, _ = rig
    rng = np.random.default_rng(7)
    x = rng.integers(0, o.t, o.n, dtype=np.uint64)
    ct = c.bfv_encrypt(x, 2)
    t = o.t
    for k, cst in ((1, 0), (0, 5), (t - 1, 1), ((t - 1) // 2, t - 1), ((t + 1) // 2, (t + 1) // 2), (12345, 54321)):
        got = np.asarray(c.bfv_decrypt(model.affine_const(o, 2, ct, k, cst))).astype(object)
        assert np.array_equal(got, (x.astype(object) * k + cst) % t), (k, cst)


@pytest.mark.parametrize("n_coef,log_baby", [(8, 1), (8, 2), (16, 3)])
def test_model_decrypts_exactly(rig, n_coef, log_baby):
    """uniform values and coefficients: the model's ciphertext decrypts to p(values) mod t in every slot"""
    o, c, rlk = rig
    rng = np.random.default_rng(100 + n_coef + log_baby)
    x = rng.integers(0, o.t, o.n, dtype=np.uint64)
    cf = [int(v) for v in rng.integers(0, o.t, n_coef)]
    out = model.evaluate(o, 2, c.bfv_encrypt(x, 2), cf, rlk, 2, log_baby)
    assert np.array_equal(np.asarray(c.bfv_decrypt(out)).astype(object), model.polynomial_mod_t(cf, x, o.t))


def test_bench_tool_dry_run():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_bfv_poly.py"), "--dry-run"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert lines and all(r["tool"] == "bench_bfv_poly" and r["dry_run"] for r in lines)
    assert {(r["n"], r["degree"]) for r in lines} == {(1 << 14, 15), (1 << 14, 31)}
    for r in lines:
        assert r["plan"] == model.counts([1] * (r["degree"] + 1)), r
