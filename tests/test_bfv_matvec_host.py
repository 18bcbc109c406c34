"""CPU-only: the plan of the BFV plaintext matrix x ciphertext vector product (lattisense_amd/csrc/bfv_matvec.h), compiled for the host
by tests/cpp/test_bfv_matvec.cpp with g++ -fsanitize=address,undefined and run as its own process: every rows, cols <= 40 at several
batches, workspace sizes and forced blocks -- column blocks cover the columns exactly once, row blocks the rows, a tile fits the
workspace and is as large as it may be, launches = tiles x column blocks -- and the refusals."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bfv_matvec_host_program(tmp_path):
    exe = str(tmp_path / "test_bfv_matvec")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_bfv_matvec.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert out.stdout.split() == ["ok", "plan", "ok", "refusals"]
