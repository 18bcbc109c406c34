"""CPU-only: the per-coefficient arithmetic of k_tensor_sum (lattisense_amd/csrc/tensor_sum.h, compiled for the host by
tests/cpp/test_tensor_sum.cpp with g++ -DLSA_EMULATE -fsanitize=undefined) against Python integers: 1 to 40 terms (every fold
boundary -- d1 folds before term 4, 8, ..., d0 and d2 before term 8, 16, ... -- and LSA_DOT_MAX_TERMS, past which the operator
continues in accumulating launches), primes of 30 to 61 bits, worst-case residues (every operand, the addend and the carried
partial sum at q - 1, where the 128-bit sums are largest), zeros and random operands."""
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the primes of tests/test_poly_lincomb_host.py: the chains of lattisense_amd/params.py plus the extremes the library admits
PRIMES = [(1 << 30) - 35, 1099511922689, 35184372121601, 0x7fffffffe90001, 0xffffffffffc0001, 0x1fffffffffe00001]
MAX_N = 40


def test_tensor_sum_elements_against_python_integers(tmp_path):
    exe = str(tmp_path / "test_tensor_sum")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-DLSA_EMULATE", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_tensor_sum.cpp"), "-o", exe])
    max_terms = int(subprocess.run([exe, "--max-terms"], capture_output=True, text=True, check=True).stdout)
    assert 1 <= max_terms < MAX_N, "the sweep below must cross LSA_DOT_MAX_TERMS"
    rnd = random.Random(9)
    cases = []
    for q in PRIMES:
        assert 30 <= q.bit_length() <= 61
        for n in range(1, MAX_N + 1):
            for mode in (0, 1):
                top, zero = [q - 1] * n, [0] * n
                cases.append((mode, q, top, top, top, top, (q - 1, q - 1)))                # the largest sums
                cases.append((mode, q, top, top, top, top, (0, 0)))
                cases.append((mode, q, zero, top, top, zero, (q - 1, 0)))                  # d1 alone
                cases.append((mode, q, zero, zero, zero, zero, (0, q - 1)))
                cases.append((mode, q, top, zero, [1] * n, top, (1, 1)))
                for _ in range(6):
                    v = [[rnd.randrange(q) for _ in range(n)] for _ in range(4)]
                    cases.append((mode, q, v[0], v[1], v[2], v[3], (rnd.randrange(q), rnd.randrange(q))))
    text = "".join("%d %d %d %s %d %d\n" % (mode, q, len(a0), " ".join(" ".join(map(str, v)) for v in (a0, a1, b0, b1)), e[0], e[1])
                   for mode, q, a0, a1, b0, b1, e in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    got = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    assert len(got) == len(cases)
    for (mode, q, a0, a1, b0, b1, e), r in zip(cases, got):
        want = ((e[0] + sum(x * y for x, y in zip(a0, b0))) % q,
                (e[1] + sum(x * y + z * w for x, y, z, w in zip(a0, b1, a1, b0))) % q,
                sum(x * y for x, y in zip(a1, b1)) % q)
        assert r == want, (mode, q, len(a0))
