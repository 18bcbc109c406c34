"""CPU-only: the Galois key set every plan operator looks its keys up in (lattisense_amd/csrc/galois_keys.h), compiled for the
host by tests/cpp/test_galois_keys.cpp with g++ -fsanitize=address,undefined: a missing element (the message; the first one in the
order of the plan's list), a null key and a key without data, a repeated element (the later key wins), an empty list against an
empty set, and the order of the keys that resolve returns."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_key_set_host_program(tmp_path):
    exe = str(tmp_path / "test_galois_keys")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_galois_keys.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert out.stdout.split() == ["ok", "missing", "ok", "null", "ok", "duplicate", "ok", "empty", "ok", "order"]
