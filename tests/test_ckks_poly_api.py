"""CKKS polynomial evaluator, the part that needs no GPU: the entry points exist and are bound, the host-side planner
(lsa_poly_plan) agrees with the pure-Python planner model of tests/poly_model.py, the planner's own choice needs fewer ciphertext
multiplications than binary splitting, and the benchmark tool's dry run reports the counts."""
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import poly_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = {"lsa_poly_plan": 11, "lsa_poly_create": 11, "lsa_poly_destroy": 1, "lsa_poly_info": 10, "lsa_poly_constants": 3,
                "lsa_ckks_poly_eval": 9}


@pytest.fixture(scope="module")
def native():
    from lattisense_amd import build, _native
    build.build_native()
    return _native


def test_entry_points_are_exported_bound_and_declared(native):
    L = native.lib()
    header = open(os.path.join(ROOT, "include", "lattisense_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, arity in ENTRY_POINTS.items():
        assert hasattr(L, name), name
        assert name in native.SIGNATURES and len(native.SIGNATURES[name][1]) == arity, name
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, "%s is not declared in the header" % name
        assert len(m.group(1).split(",")) == arity, name
    assert "lsa_polynomial_st" in header


def test_python_plan_class_exists():
    from lattisense_amd import device
    sig = inspect.signature(device.PolynomialPlan.__init__)
    assert list(sig.parameters)[1:] == ["ctx", "coeffs", "level", "scale_in", "basis", "interval", "scale_out", "log_baby"]
    assert sig.parameters["basis"].default == "chebyshev" and sig.parameters["interval"].default == (-1, 1)
    assert sig.parameters["scale_out"].default is None and sig.parameters["log_baby"].default == 0
    assert list(inspect.signature(device.PolynomialPlan.run).parameters)[1:] == ["in_buf", "batch", "rlk", "out"]
    for attr in ("run", "constants", "close"):
        assert callable(getattr(device.PolynomialPlan, attr))


def _polys():
    rng = np.random.default_rng(7)
    out = [("dense%d" % n, rng.uniform(-1, 1, n)) for n in (2, 3, 8, 16, 24, 32, 41, 64, 128, 256)]
    out.append(("odd31", np.where(np.arange(32) % 2 == 1, rng.uniform(-1, 1, 32), 0.0)))
    out.append(("upper_half_zero", np.concatenate([rng.uniform(-1, 1, 16), np.zeros(16)])))
    return out


POLYS = _polys()


@pytest.mark.parametrize("interval", [False, True])
@pytest.mark.parametrize("basis", ["chebyshev", "monomial"])
@pytest.mark.parametrize("log_baby", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("name,coeffs", POLYS, ids=[p[0] for p in POLYS])
def test_planner_against_the_python_model(native, name, coeffs, log_baby, basis, interval):
    from lattisense_amd.device import plan_polynomial
    got = plan_polynomial(coeffs, 12, basis, log_baby, interval)
    assert got == pm.plan(coeffs, basis, log_baby, interval)
    k = max(1, (len(coeffs) - 1).bit_length())
    assert got["depth"] == k + (1 if interval else 0)
    assert 1 <= got["log_baby"] <= min(4, k)
    if log_baby:
        assert got["log_baby"] == min(log_baby, k)


@pytest.mark.parametrize("basis", ["chebyshev", "monomial"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8])
def test_multiplication_counts(native, k, basis):
    """log_baby = 1 is the binary splitting of the oracle, 2^(k-1) + k - 2; the planner's own choice is strictly below it for
    every dense 2^k from k = 4, and never above it"""
    from lattisense_amd.device import plan_polynomial
    coeffs = np.random.default_rng(k).uniform(-1, 1, 1 << k)
    binary = pm.binary_splitting_mults(k)
    assert plan_polynomial(coeffs, 12, basis, 1)["mults"] == binary
    own = plan_polynomial(coeffs, 12, basis, 0)
    assert own["mults"] <= binary
    if k >= 4:
        assert own["mults"] < binary
    assert own["mults"] == min(plan_polynomial(coeffs, 12, basis, b)["mults"] for b in range(1, min(4, k) + 1))


def test_counts_named_in_the_design(native):
    from lattisense_amd.device import plan_polynomial
    rng = np.random.default_rng(1)
    assert plan_polynomial(rng.uniform(-1, 1, 64), 12, "chebyshev", 3)["mults"] == 18          # against 36
    assert plan_polynomial(rng.uniform(-1, 1, 32), 12, "chebyshev", 3)["mults"] == 13          # against 19
    assert plan_polynomial(rng.uniform(-1, 1, 64), 12)["log_baby"] == 3
    half = plan_polynomial(np.concatenate([rng.uniform(-1, 1, 16), np.zeros(16)]), 12, "monomial", 3)
    assert half["depth"] == 5 and half["mults"] <= plan_polynomial(rng.uniform(-1, 1, 16), 12, "monomial", 3)["mults"]   # a zero upper half costs nothing


def test_planner_errors(native):
    from lattisense_amd.device import plan_polynomial
    good = np.random.default_rng(2).uniform(-1, 1, 16)

    def fails(fn, needle):
        with pytest.raises(native.LsaError) as e:
            fn()
        assert e.value.code == 1 and "poly" in str(e.value) and needle in str(e.value), e.value
    fails(lambda: plan_polynomial(good, 3), "levels")                       # level_in < depth
    fails(lambda: plan_polynomial(good, 4, interval=True), "levels")
    assert plan_polynomial(good, 4)["depth"] == 4
    fails(lambda: plan_polynomial([1.5], 12), "degree 0")
    fails(lambda: plan_polynomial([1.5, 0.0, 0.0, 0.0], 12), "degree 0")
    fails(lambda: plan_polynomial(np.ones(257), 12), "256")
    fails(lambda: plan_polynomial(good, 12, log_baby=5), "log_baby")
    fails(lambda: plan_polynomial([1.0, float("nan")], 12), "finite")


@pytest.mark.parametrize("degree", [31, 63])
def test_bench_tool_dry_run(native, degree):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_ckks_poly.py"), "--degree", str(degree), "--dry-run"],
                         capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    k = (degree).bit_length()
    assert r["dry_run"] is True and r["degree"] == degree and r["depth"] == k
    assert r["plans"]["binary"]["mults"] == pm.binary_splitting_mults(k) and r["plans"]["binary"]["log_baby"] == 1
    assert r["plans"]["planner"]["mults"] == {31: 13, 63: 18}[degree]
    assert sum(r["plans"]["planner"]["mult_levels"].values()) == r["plans"]["planner"]["mults"]
