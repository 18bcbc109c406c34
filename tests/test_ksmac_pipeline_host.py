"""CPU-only: the cached twiddles of the fused key MAC (lattisense_amd/csrc/ntt_r16.h: the cache's layout, fill and get, the radix
groups that take their twiddles from the caller) against the functions the loop had before (tests/cpp/test_ksmac_pipeline.cpp,
a stand-alone program built with -fsanitize=address,undefined)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ksmac_pipeline_helpers(tmp_path):
    exe = str(tmp_path / "test_ksmac_pipeline")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-attributes", "-DLSA_EMULATE",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_ksmac_pipeline.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK ksmac_pipeline" in out.stdout
