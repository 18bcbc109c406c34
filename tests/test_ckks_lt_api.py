"""CKKS linear-transform operator, the part that needs no GPU: the entry points exist and are bound, the host-side planner
(lsa_lt_plan_rotations) agrees with the oracle's restatement of the reference planner and with the planner's own recorded
output, and the benchmark tool's dry run reports the division and limb-stream counts the design claims."""
import inspect
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "bootstrap", "planner_rotations.json")))

ENTRY_POINTS = {"lsa_lt_create": 11, "lsa_lt_destroy": 1, "lsa_lt_info": 9, "lsa_lt_diagonals": 3, "lsa_lt_galois_elements": 3,
                "lsa_lt_plaintext": 4, "lsa_ckks_linear_transform": 12, "lsa_lt_plan_rotations": 8}


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
    assert "lsa_linear_transform_st" in header


def test_python_plan_class_exists():
    from lattisense_amd import device
    sig = inspect.signature(device.LinearTransformPlan.__init__)
    assert list(sig.parameters)[1:] == ["ctx", "level", "diags", "log_slots", "pt_scale", "ratio", "double_hoist"]
    assert sig.parameters["double_hoist"].default is True
    for attr in ("oracle_plains", "run", "close"):
        assert callable(getattr(device.LinearTransformPlan, attr))


INDEX_SETS = [
    ("two", [0, 1], 1 << 11),
    ("band", list(range(-3, 4)), 1 << 11),
    ("dense64", list(range(64)), 1 << 11),
    ("dense200", list(range(200)), 1 << 11),
    ("strided", list(range(0, 2017, 32)), 1 << 11),
    ("sparse_packing", list(range(-5, 40)), 1 << 9),     # period 2^9 inside N = 2^12
]


@pytest.mark.parametrize("ratio", [1.0, 2.0, 4.0])
@pytest.mark.parametrize("name,index,period", INDEX_SETS, ids=[s[0] for s in INDEX_SETS])
def test_planner_against_the_oracle(native, name, index, period, ratio):
    from lattisense_amd.device import plan_rotations
    from oracle.ckks_bootstrap import bsgs_split, rotations_of
    n1, rot = plan_rotations(period, index, ratio)
    ks = sorted(k % period for k in index)
    want_n1 = 0 if len(ks) < 3 else bsgs_split(ks, period, ratio)
    assert n1 == want_n1
    assert rot == rotations_of({k: None for k in ks}, period, ratio)


def test_planner_shapes_named_in_the_design(native):
    """64 dense diagonals are exactly one 8 x 8 block; 200 are 16 x 13 at ratio 2 and 8 x 25 at ratio 1"""
    from lattisense_amd.device import plan_rotations
    from oracle.ckks_bootstrap import bsgs_sets

    def shape(d, ratio):
        n1, _ = plan_rotations(1 << 11, list(range(d)), ratio)
        g, b = bsgs_sets(list(range(d)), 1 << 11, n1)
        return n1, len(b), len(g)
    assert shape(64, 2.0) == (8, 8, 8)
    assert shape(200, 2.0) == (16, 16, 13)
    assert shape(200, 1.0) == (8, 8, 25)


def test_planner_default_ratio_and_errors(native):
    from lattisense_amd.device import plan_rotations
    assert plan_rotations(1 << 11, list(range(200)), 0.0) == plan_rotations(1 << 11, list(range(200)), 2.0)
    with pytest.raises(native.LsaError) as e:
        plan_rotations(1 << 9, [3, 3 + 512], 2.0)          # equal modulo the period
    assert e.value.code == 1 and "515" in str(e.value)
    with pytest.raises(native.LsaError) as e:
        plan_rotations(1000, [0, 1, 2], 2.0)
    assert e.value.code == 1


@pytest.mark.parametrize("key", sorted(k for k in GOLD if "cts" in GOLD[k]))
def test_planner_against_the_reference_planners_recorded_output(native, key):
    """per configuration the union over its matrices equals the recorded rotation set; nothing is added outside the matrices of
    a dense plan's CoeffsToSlots / SlotsToCoeffs lists (the conjugation is a Galois element of its own, SubSum is sparse-only:
    tests/test_oracle_bootstrap.py)"""
    from lattisense_amd.device import plan_rotations
    log_n = int(key.split("_")[0][4:])
    period = 1 << (log_n - 1)
    for name in ("cts", "stc"):
        union = set()
        for diagonals in GOLD[key][name]["diagonals"]:
            union |= set(plan_rotations(period, diagonals, 2.0)[1])
        assert sorted(union) == GOLD[key][name]["rotations"], (key, name)


@pytest.mark.parametrize("shape", ["n14", "n16"])
@pytest.mark.parametrize("d", [8, 64, 200])
def test_bench_tool_dry_run(native, shape, d):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_ckks_lt.py"), "--shape", shape, "--diagonals", str(d),
                          "--batch", "4", "--dry-run"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    nb, ng = r["babies"], r["giants"]
    assert r["diagonals"] == d and r["dry_run"] is True
    assert r["divisions_by_p"]["operator"] == ng + 1
    assert r["divisions_by_p"]["operator"] < r["divisions_by_p"]["composition"]
    blocked, fallback = r["inner_sum_streams"]["blocked"], r["inner_sum_streams"]["fallback"]
    assert fallback == d * 3 + 2 * ng
    assert blocked == 2 * nb * -(-ng // 8) + d + 2 * ng * -(-nb // 8)
    assert blocked <= fallback
    if ng > 1 and (nb > 8 or ng > 8):
        assert blocked < fallback
