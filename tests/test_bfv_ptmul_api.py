"""CPU-side checks of BFV ct x pt_mul: the task runtime binds the frontend's pt_mul graphs (mult, cmp_sum, cmpac_sum) that it
refused before, still refuses a MAC that mixes pt_mul and ring-t plaintexts and BFV ct x Delta-scaled pt, the library exports
and binds lsa_bfv_mult_plain_mul / lsa_bfv_mac_plain_mul, and tools/bench_bfv_mult_plain_mul.py --dry-run prints a byte
model in which the fused form moves fewer bytes than the unfused one.  No compute calls."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASKS = os.path.join(ROOT, "tests", "golden", "tasks")
FIXTURES = ["bfv_n4096_cmp_mul", "bfv_n4096_cmpac_mul", "bfv_n16384_cmpac_mul20"]


@pytest.fixture(scope="module")
def native():
    from lattisense_amd import build, _native
    build.build_native()
    return _native


@pytest.mark.parametrize("fusion", ["0", "1"])
@pytest.mark.parametrize("name", FIXTURES)
def test_ptmul_graphs_bind(native, name, fusion, monkeypatch):
    from lattisense_amd.task import FheTaskGpu
    if fusion == "0":
        monkeypatch.setenv("LSA_NO_GRAPH_FUSION", "1")
    g = json.load(open(os.path.join(TASKS, name, "mega_ag.json")))
    assert any(d["type"] == "pt_mul" for d in g["data"].values())
    t = FheTaskGpu(os.path.join(TASKS, name))
    t.close()


def test_mixed_plaintext_mac_is_refused(native):
    from lattisense_amd.task import FheTaskGpu
    with pytest.raises(RuntimeError, match="pt_mul and other plaintext flavours"):
        FheTaskGpu(os.path.join(TASKS, "bfv_n4096_cmpac_mixed_unsupported"))


def test_delta_scaled_plaintext_still_refused(native):
    from lattisense_amd.task import FheTaskGpu
    with pytest.raises(RuntimeError, match="Multiply with plaintext only supported for CKKS scheme"):
        FheTaskGpu(os.path.join(TASKS, "bfv_n4096_cmp_unsupported"))


def test_entry_points_exported_and_bound(native):
    for sym in ("lsa_bfv_mult_plain_mul", "lsa_bfv_mac_plain_mul"):
        assert hasattr(native.lib(), sym)
        assert sym in native.SIGNATURES
    assert native.SIGNATURES["lsa_bfv_mult_plain_mul"] == native.SIGNATURES["lsa_bfv_mult"]


def test_device_context_methods():
    from lattisense_amd.device import DeviceContext
    assert callable(getattr(DeviceContext, "bfv_mult_plain_mul", None))
    assert callable(getattr(DeviceContext, "bfv_mac_plain_mul", None))


@pytest.mark.parametrize("shape,op", [("n14", "mult"), ("n14", "mac"), ("n16", "mult"), ("n16", "mac")])
def test_tool_dry_run_byte_model(shape, op):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_bfv_mult_plain_mul.py"), "--dry-run", "--shape", shape,
                          "--op", op, "--terms", "16"], capture_output=True, text=True, check=True, timeout=120).stdout
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1, out
    d = json.loads(lines[0])
    assert d["config"]["ring_degree"] == {"n14": 16384, "n16": 65536}[shape]
    assert d["config"]["terms"] == (1 if op == "mult" else 16)
    bm = d["byte_model"]
    assert 0 < bm["bytes_fused_per_ct"] < bm["bytes_unfused_per_ct"]
