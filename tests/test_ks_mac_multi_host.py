"""CPU-only: the per-point arithmetic of k_ks_mac_multi and k_ext_sum (lattisense_amd/csrc/ks_mac_multi.h, compiled for the host by
tests/cpp/test_ks_mac_multi.cpp with g++ -DLSA_EMULATE) against unsigned __int128 arithmetic: K = 1..4 keys, 1 / 2 / 8 / 9 / 17
digits (9 and 17 cross the fold-every-8 rule), moduli at the 61-bit ceiling, around 2^40 and at 2^30, worst-case residues q - 1,
zeros and random operands; K keys at once against K single-key evaluations.  The program is stand-alone (its own main, its own
cases): built once plain and once with -fsanitize=address,undefined (the sanitizer runtimes linked statically, so the binary does not
depend on what else the process loads), each binary run directly in the inherited environment."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_ks_mac_multi.cpp")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]], ids=["plain", "asan-ubsan"])
def test_ks_mac_multi_points_against_int128(tmp_path, flags):
    exe = str(tmp_path / "test_ks_mac_multi")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-DLSA_EMULATE"] + flags + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    word, n = out.stdout.split()
    # 6 primes x 5 digit counts x (1 + 1 + 50 fills) x (1 + 2 + 3 + 4 keys) + 6 x 4 x 3 sums
    assert word == "ok" and int(n) == 6 * 5 * 52 * 10 + 6 * 4 * 3
