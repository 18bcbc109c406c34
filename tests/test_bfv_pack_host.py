"""CPU-only: the plan and the tail's point arithmetic of the BFV coefficient packing (lattisense_amd/csrc/bfv_pack.h), compiled for the
host by tests/cpp/test_bfv_pack.cpp with g++ -fsanitize=address,undefined: the plan against a brute-force walk for every count <= 64
with and without the trace, every input consumed exactly once and input i landing on coefficient i * N / 2^k, and the shifted-source
rule against a schoolbook multiplication by X^s for s in {1, 2, N/2} at x = 0, s-1, s, N-1."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bfv_pack_host_program(tmp_path):
    exe = str(tmp_path / "test_bfv_pack")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_bfv_pack.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert out.stdout.split() == ["ok", "plan", "ok", "refusals", "ok", "point"]
