"""CPU-only: the plan of the BFV select-by-index operator (lattisense_amd/csrc/bfv_select.h) and the fold rule of the pair key MAC
(ks_mac_pair.h), compiled for the host by tests/cpp/test_bfv_select.cpp with g++ -fsanitize=address,undefined: the plan against a
brute-force walk of the CMux tree for every count <= 64 -- every index below count reaches node 0, count - 1 products -- the refusals,
and no run of more than eight products between two folds."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bfv_select_host_program(tmp_path):
    exe = str(tmp_path / "test_bfv_select")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_bfv_select.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert out.stdout.split() == ["ok", "plan", "ok", "refusals", "ok", "fold"]
