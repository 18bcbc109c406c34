"""CPU-only: the per-word arithmetic of k_lift_i64 and k_cconst (lattisense_amd/csrc/plain_ops.h, compiled for the host by
tests/cpp/test_plain_ops.cpp with g++ -DLSA_EMULATE -fsanitize=undefined) against Python integers.

lift_i64: the signed coefficients an encoder can hand over (|v| < 4.6e18, the bound round_even enforces), at the values where
the reduction can go wrong -- 0, +-1, the modulus and its neighbours, 2^62 and the largest admitted magnitude -- and random ones.
cconst_pair and the per-word multiply-add: rounded constants at 0, +-1, +-(q - 1) and random 62-bit values, words at 0, 1, q - 1
and random, I a true square root of -1 modulo each prime (all primes are 1 mod 4)."""
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the primes of tests/test_tensor_sum_host.py: 30 to 61 bits
PRIMES = [(1 << 30) - 35, 1099511922689, 35184372121601, 0x7fffffffe90001, 0xffffffffffc0001, 0x1fffffffffe00001]
MAX_MAG = 4599999999999999999


def _exe(tmp_path):
    exe = str(tmp_path / "test_plain_ops")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-DLSA_EMULATE", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_plain_ops.cpp"), "-o", exe])
    return exe


def _run(exe, lines):
    out = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    got = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    assert len(got) == len(lines)
    return got


def _sqrt_minus_one(q, rnd):
    assert q % 4 == 1
    while True:
        g = rnd.randrange(2, q - 1)
        r = pow(g, (q - 1) // 4, q)
        if r * r % q == q - 1:
            return r


def test_lift_i64_against_python_integers(tmp_path):
    exe = _exe(tmp_path)
    rnd = random.Random(13)
    cases = []
    for q in PRIMES:
        assert 30 <= q.bit_length() <= 61
        mags = [0, 1, q - 1, q, q + 1, 1 << 62, MAX_MAG] + [rnd.randrange(MAX_MAG + 1) for _ in range(200)]
        mags += [rnd.randrange(q) for _ in range(50)] + [k * q + d for k in (2, 3, 1000) for d in (-1, 0, 1)]
        for a in mags:
            if a > MAX_MAG:
                continue
            cases += [(q, a), (q, -a)]
    got = _run(exe, ["L %d %d\n" % c for c in cases])
    for (q, v), (r,) in zip(cases, got):
        assert r == v % q, (q, v, r)


def test_cconst_pair_and_word_against_python_integers(tmp_path):
    exe = _exe(tmp_path)
    rnd = random.Random(14)
    cases = []
    for q in PRIMES:
        I = _sqrt_minus_one(q, rnd)
        ks = [0, 1, -1, q - 1, -(q - 1), rnd.randrange(1 << 61, 1 << 62), -rnd.randrange(1 << 61, 1 << 62)]
        words = [0, 1, q - 1, rnd.randrange(q), rnd.randrange(q)]
        for root in (I, q - I):
            for kre in ks:
                for kim in ks:
                    for w in words:
                        cases.append((q, root, kre, kim, rnd.choice(ks), rnd.choice(ks), w))
        for _ in range(300):
            k = [rnd.randrange(-MAX_MAG, MAX_MAG + 1) for _ in range(4)]
            cases.append((q, I, k[0], k[1], k[2], k[3], rnd.randrange(q)))
    got = _run(exe, ["C %d %d %d %d %d %d %d\n" % c for c in cases])
    for (q, I, kre, kim, bre, bim, w), r in zip(cases, got):
        kp, km = (kre + kim * I) % q, (kre - kim * I) % q
        bp, bm = (bre + bim * I) % q, (bre - bim * I) % q
        want = (kp, km, bp, bm, w * kp % q, w * km % q, (w + bp) % q, (w + bm) % q, (w * kp + bp) % q, (w * km + bm) % q)
        assert r == want, (q, I, kre, kim, bre, bim, w)
