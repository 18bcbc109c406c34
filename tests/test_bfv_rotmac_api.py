"""CPU-side checks of the hoisted BFV rotate-and-MAC entry point: the library exports lsa_bfv_rotate_mac_plain_mul and
_native binds it, the Python layer has DeviceContext.bfv_rotate_mac_plain_mul, and tools/bench_bfv_rotate_mac.py --dry-run
prints the transform counts of the issue's table and a byte model in which the fused form moves fewer bytes than the
composition lsa_bfv_rotate_many + lsa_bfv_mac_plain_mul.  No compute calls."""
import ctypes
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
    assert hasattr(native.lib(), "lsa_bfv_rotate_mac_plain_mul")
    res, argtypes = native.SIGNATURES["lsa_bfv_rotate_mac_plain_mul"]
    assert res is ctypes.c_int
    # ctx, level, in, n, galois_elements, glk, pts, spts, partial, spartial, out, batch, sin, sout, stream
    assert len(argtypes) == 15
    assert argtypes[3] is ctypes.c_int and argtypes[11] is ctypes.c_int


def test_header_declares_entry_point():
    src = open(os.path.join(ROOT, "include", "lattisense_amd.h")).read()
    assert "int lsa_bfv_rotate_mac_plain_mul(" in src


def test_device_context_method():
    from lattisense_amd.device import DeviceContext
    assert callable(getattr(DeviceContext, "bfv_rotate_mac_plain_mul", None))


@pytest.mark.parametrize("shape,m", [("n14", 4), ("n14", 8), ("n14", 16), ("n16", 4), ("n16", 8), ("n16", 16)])
def test_tool_dry_run_models(shape, m):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_bfv_rotate_mac.py"), "--dry-run", "--shape", shape,
                          "--m", str(m)], capture_output=True, text=True, check=True, timeout=120).stdout
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1, out
    d = json.loads(lines[0])
    cfg = d["config"]
    assert cfg["rotations"] == m and len(cfg["galois_elements"]) == m + 1 and cfg["galois_elements"][0] == 1
    assert cfg["ring_degree"] == {"n14": 16384, "n16": 65536}[shape]
    tr = d["transforms"]
    # per rotation term: 2(L+k) INTT + 2L NTT now, 2k INTT + 2L NTT fused (28 / 16 and 104 / 56)
    want = {"n14": (28, 16), "n16": (104, 56)}[shape]
    assert (tr["per_rotation_term_composition"], tr["per_rotation_term_fused"]) == want
    assert tr["per_ct_fused"] < tr["per_ct_composition"]
    bm = d["byte_model"]
    assert 0 < bm["bytes_fused_per_ct"] < bm["bytes_composition_per_ct"]


# the load-time peephole TaskGraph::fuse_rotate_mac on the frontend's rotate-then-accumulate graphs (data / compute counts
# include the ABI bridge nodes).  Without it: the rotations, the pt_mul product and the MAC nodes as the frontend wrote them.
#   rotmac4: mult(X, p_0) + 2-term cmpac_sum + 1-term cmpac_sum (the frontend's slicing): 3 rotations, the product and both
#            MACs become 2 fused nodes (the first absorbs the product, the second keeps the first's output as its partial)
#   rotmac_row_partial: row + column rotation and an input partial sum: 2 rotations + 1 MAC -> 1 node
#   rotmac_shared: a rotation that is also a task output is not private: unchanged
#   rotmac20: 19 rotations, a 16-term cmp_sum and a 4-term cmpac_sum -> 2 nodes
PEEPHOLE = {
    "bfv_n4096_rotmac4": ({"data": 32, "compute": 24}, {"data": 28, "compute": 20}),
    "bfv_n4096_rotmac_row_partial": ({"data": 23, "compute": 17}, {"data": 21, "compute": 15}),
    "bfv_n4096_rotmac_shared": ({"data": 22, "compute": 17}, {"data": 22, "compute": 17}),
    "bfv_n16384_rotmac20": ({"data": 143, "compute": 103}, {"data": 124, "compute": 84}),
}


@pytest.mark.parametrize("name", sorted(PEEPHOLE))
def test_rotate_mac_peephole_counts(native, name, monkeypatch):
    from lattisense_amd.task import FheTaskGpu
    plain, fused = PEEPHOLE[name]
    path = os.path.join(ROOT, "tests", "golden", "tasks", name)
    monkeypatch.delenv("LSA_NO_GRAPH_FUSION", raising=False)
    c = FheTaskGpu(path).counts()
    assert {k: c[k] for k in ("data", "compute")} == fused, c
    monkeypatch.setenv("LSA_NO_GRAPH_FUSION", "1")
    c = FheTaskGpu(path).counts()
    assert {k: c[k] for k in ("data", "compute")} == plain, c
