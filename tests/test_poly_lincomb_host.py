"""CPU-only: the per-element arithmetic of k_poly_lincomb (lattisense_amd/csrc/poly_lincomb.h, compiled for the host by
tests/cpp/test_poly_lincomb.cpp with g++ -fsanitize=undefined) against Python integers: 1 to 15 terms, primes of 30 to 61 bits,
worst-case residues (every value and every constant equal to q - 1, where the 128-bit sum of eight products is largest), zeros
and random operands."""
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# NTT-friendly primes of the chains in lattisense_amd/params.py plus the extremes the library admits
PRIMES = [(1 << 30) - 35, 1099511922689, 35184372121601, 0x7fffffffe90001, 0xffffffffffc0001, 0x1fffffffffe00001]


def test_lincomb_elements_against_python_integers(tmp_path):
    exe = str(tmp_path / "test_poly_lincomb")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-DLSA_EMULATE", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_poly_lincomb.cpp"), "-o", exe])
    rnd = random.Random(5)
    cases = []
    for q in PRIMES:
        assert 30 <= q.bit_length() <= 61
        for n in range(1, 16):
            cases.append((q, [q - 1] * n, [q - 1] * n))                      # worst case
            cases.append((q, [q - 1] * n, [1] * n))
            cases.append((q, [0] * n, [q - 1] * n))
            cases.append((q, [q - 1] * n, [(q - 1) * (i % 2) for i in range(n)]))   # unused powers: zero constants
            for _ in range(20):
                cases.append((q, [rnd.randrange(q) for _ in range(n)], [rnd.randrange(q) for _ in range(n)]))
    text = "".join("%d %d %s %s\n" % (q, len(v), " ".join(map(str, v)), " ".join(map(str, k))) for q, v, k in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    got = [int(x) for x in out.stdout.split()]
    assert len(got) == len(cases)
    for (q, v, k), r in zip(cases, got):
        assert r == sum(a * b for a, b in zip(v, k)) % q, (q, len(v))
