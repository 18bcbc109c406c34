"""CPU-only: the scalar load / store conversions of the NTT kernels (lattisense_amd/csrc/ntt_core.h: ntt_load_fix, ntt_store_fix,
ntt_prod_fix, fp_modmul, fp_reduce) against unsigned __int128 arithmetic, for every (target prime, dropped prime) pair of the
threshold-straddling chain of tests/boundary.py and its 61-bit special prime, with the range bounds their comments claim
asserted inside the FP64 paths (tests/cpp/test_ntt_fix.cpp, built with g++ -fsanitize=undefined).  The device build runs the
same functions."""
import os
import subprocess

from tests.boundary import straddle_chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ntt_fix_functions(tmp_path):
    exe = str(tmp_path / "test_ntt_fix")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-attributes", "-DLSA_EMULATE",
                           "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_ntt_fix.cpp"), "-o", exe])
    C = straddle_chain(1 << 16, 1)
    out = subprocess.run([exe] + [str(m) for m in C["q"] + C["p"]], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK ntt_fix" in out.stdout


def test_straddle_chain_classes():
    """the helper's own assertions hold at every ring degree the GPU module uses, and over the three orders every combination
    of (near, fp_lift, target engine) that can occur does"""
    from tests.boundary import ORDERS, fp_engine, head_flags
    for logn in (12, 13, 14, 16, 17):
        seen = set()
        for order in ORDERS:
            q = straddle_chain(1 << logn, 3, order)["q"]
            seen |= {head_flags(q[l], q[i]) + (fp_engine(q[i]),) for l in range(1, len(q)) for i in range(l)}
        # (near without fp_lift cannot occur on an FP64-engine target: q_l >= 2^48 > 2 q_i)
        assert seen == {(True, True, True), (False, True, True), (False, False, True), (True, False, False),
                        (False, False, False)}, (logn, seen)
