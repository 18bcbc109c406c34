"""CPU-side checks of the hoisted BFV rotation entry point: the library exports lsa_bfv_rotate_many, the Python layer has
DeviceContext.bfv_rotate_many, and tools/bench_bfv_rotate_many.py --dry-run prints a byte model in which the hoisted form
moves fewer bytes than the separate rotations.  No compute calls."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    from lattisense_amd import build, _native
    build.build_native()
    return _native


def test_entry_point_exported_and_bound(native):
    assert hasattr(native.lib(), "lsa_bfv_rotate_many")
    assert "lsa_bfv_rotate_many" in native.SIGNATURES
    assert native.SIGNATURES["lsa_bfv_rotate_many"] == native.SIGNATURES["lsa_ckks_rotate_many"]


def test_device_context_method():
    from lattisense_amd.device import DeviceContext
    assert callable(getattr(DeviceContext, "bfv_rotate_many", None))


@pytest.mark.parametrize("shape,m", [("n14", 2), ("n14", 5), ("n16", 2), ("n16", 5)])
def test_tool_dry_run_byte_model(shape, m):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_bfv_rotate_many.py"), "--dry-run", "--shape", shape,
                          "--m", str(m)], capture_output=True, text=True, check=True, timeout=120).stdout
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1, out
    d = json.loads(lines[0])
    assert d["config"]["m"] == m and len(d["config"]["galois_elements"]) == m
    assert d["config"]["ring_degree"] == {"n14": 16384, "n16": 65536}[shape]
    bm = d["byte_model"]
    assert 0 < bm["bytes_hoisted_per_ct"] < bm["bytes_separate_per_ct"]
