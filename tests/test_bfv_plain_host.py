"""CPU-only: the per-word arithmetic of k_bfv_addsub_plain (lattisense_amd/csrc/bfv_plain.h, compiled for the host by
tests/cpp/test_bfv_plain.cpp with g++ -DLSA_EMULATE -fsanitize=undefined) against Python integers and against
bfv_poly_scale_up_word (bfv_poly.h), the host formula of the same scale-up.

The reduction mod t goes through the reciprocal floor(2^64 / t) and ONE conditional subtraction: it is held against `%` on the
words where the quotient estimate is one short or the input is at the edge of the 64-bit range.  t: 65537, 786433 and 4294828033,
the largest prime below 2^32 that is 1 mod 8192 (checked below).  q: a 39-bit, a 47-bit prime and one just below 2^61.  m: 0, 1,
t - 1, t, floor(t/2) and floor(t/2) + 1, 2^32 - 1, 2^32, 2^63, 2^64 - 1 and 1000 random words.  Both signs of
u - floor(t/2) occur for every (t, q)."""
import os
import random
import subprocess

from lattisense_amd import params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T_EDGE = 4294828033
TS = [65537, 786433, T_EDGE]


def _primes():
    qs = [params.ntt_primes_below(39, 2048, 1)[0], params.ntt_primes_below(47, 2048, 1)[0], params.ntt_primes_below(61, 2048, 1)[0]]
    assert [q.bit_length() for q in qs] == [39, 47, 61] and all(params._is_prime(q) for q in qs)
    assert (1 << 61) - qs[2] < (1 << 40)
    return qs


def _exe(tmp_path):
    exe = str(tmp_path / "test_bfv_plain")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-DLSA_EMULATE", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_bfv_plain.cpp"), "-o", exe])
    return exe


def _run(exe, lines):
    out = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    got = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    assert len(got) == len(lines)
    return got


def _words(t, rnd):
    return [0, 1, t - 1, t, t // 2, t // 2 + 1, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1] + [rnd.randrange(1 << 64) for _ in range(1000)]


def test_the_edge_modulus_is_the_largest_prime_below_2_32_that_is_1_mod_8192():
    assert params._is_prime(T_EDGE) and T_EDGE % 8192 == 1 and T_EDGE < (1 << 32)
    assert not any(params._is_prime(c) for c in range(T_EDGE + 8192, 1 << 32, 8192))
    assert params._is_prime(65537) and params._is_prime(786433)


def test_reduction_mod_t_against_python_integers(tmp_path):
    exe = _exe(tmp_path)
    rnd = random.Random(31)
    cases = []
    for t in TS + [2, 3, 4, (1 << 32) - 1, (1 << 31) + 11]:
        xs = _words(t, rnd)
        xs += [k * t + d for k in (1, 2, (1 << 64) // t - 1, (1 << 64) // t) for d in (-1, 0, 1)]           # around multiples of t
        xs += [(t - 1) * (t - 1) + t // 2, (t - 1) * (t - 1), rnd.randrange(t) * rnd.randrange(t) + t // 2]    # what the kernel feeds it
        cases += [(t, x) for x in xs if 0 <= x < (1 << 64)]
    got = _run(exe, ["R %d %d\n" % c for c in cases])
    for (t, x), (r,) in zip(cases, got):
        assert r == x % t, (t, x, r)


def test_scale_up_and_the_three_ops_against_python_integers(tmp_path):
    exe = _exe(tmp_path)
    rnd = random.Random(32)
    cases = []
    for t in TS:
        for q in _primes():
            for qmt in (q % t, 1, t - 1):
                ms = _words(t, rnd) if qmt == q % t else _words(t, rnd)[:60]
                for m in ms:
                    cases.append((t, q, qmt, m, rnd.choice([0, 1, q - 1, rnd.randrange(q)])))
    got = _run(exe, ["S %d %d %d %d %d\n" % c for c in cases])
    signs = {}
    for (t, q, qmt, m, c0), (r, u, p, ref, w0, w1, w2) in zip(cases, got):
        th = t // 2
        u_want = ((m % t) * qmt + th) % t
        p_want = (u_want - th) * (-pow(t, -1, q)) % q
        assert (r, u, p) == (m % t, u_want, p_want), (t, q, qmt, m)
        assert ref == p_want, ("bfv_poly_scale_up_word", t, q, qmt, m)
        assert (w0, w1, w2) == ((c0 + p_want) % q, (c0 - p_want) % q, (p_want - c0) % q), (t, q, qmt, m, c0)
        signs.setdefault((t, q), set()).add(u_want < th)
    assert len(signs) == 9 and all(s == {True, False} for s in signs.values()), signs
