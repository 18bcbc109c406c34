"""CKKS encrypted inner product, the part that needs no GPU: the two entry points exist, are bound and declared with the arities
of the header, the DeviceContext methods have the documented parameter lists, and the benchmark tool's dry run prints a
limb-stream model in which lsa_ckks_dot moves strictly fewer rows than the lazy composition from the existing entry points, and
that fewer than the eager sum of HMults, for every n >= 2."""
import inspect
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = {"lsa_ckks_mult_sum": 15, "lsa_ckks_dot": 17}


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


def test_python_methods():
    from lattisense_amd import device
    sig = inspect.signature(device.DeviceContext.ckks_mult_sum)
    assert list(sig.parameters)[1:] == ["level", "a_list", "b_list", "batch", "addend", "out"]
    assert sig.parameters["addend"].default is None and sig.parameters["out"].default is None
    sig = inspect.signature(device.DeviceContext.ckks_dot)
    assert list(sig.parameters)[1:] == ["level", "a_list", "b_list", "rlk", "batch", "rescale", "addend", "out"]
    assert sig.parameters["rescale"].default is True
    assert sig.parameters["addend"].default is None and sig.parameters["out"].default is None


def test_launch_bound_of_the_tool_is_the_header_s():
    text = open(os.path.join(ROOT, "lattisense_amd", "csrc", "tensor_sum.h")).read()
    m = re.search(r"#define LSA_DOT_MAX_TERMS (\d+)", text)
    assert m
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import bench_ckks_dot
    finally:
        sys.path.pop(0)
    assert bench_ckks_dot.DOT_MAX_TERMS == int(m.group(1))


def _dry_run(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_ckks_dot.py"), "--dry-run", *args],
                         capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_bench_tool_dry_run():
    r = _dry_run()
    assert r["dry_run"] is True and r["n"] == 65536 and r["level"] == 12 and r["special_primes"] == 4
    assert r["terms"] == [2, 4, 8, 16, 32] and set(r["streams_per_ct"]) == {"2", "4", "8", "16", "32"}
    assert "ms_per_call" not in r


def test_stream_model_orders_the_legs():
    r = _dry_run("--terms", ",".join(str(n) for n in range(2, 70)))
    for n in range(2, 70):
        m = r["streams_per_ct"][str(n)]
        assert m["dot"] < m["lazy_composition"] < m["eager"], (n, m)
        assert m["predicted_lazy_over_dot"] > 1 and m["predicted_eager_over_dot"] > m["predicted_lazy_over_dot"]
    # the tensor part of the model: four operand rows per term and limb, three output rows, six more per accumulating launch
    a2, a3 = r["streams_per_ct"]["2"]["dot"], r["streams_per_ct"]["3"]["dot"]
    assert a3 - a2 == 4 * 13
    assert r["streams_per_ct"]["17"]["dot"] - r["streams_per_ct"]["16"]["dot"] == 4 * 13 + 6 * 13
