"""CPU-only: the merged ModDown + rescale tail of an FP64-engine limb (lattisense_amd/csrc/ntt_core.h, fp_merged_tail), the one
function the epilogue pass and the tail variant of the fused key MAC both store through, against 128-bit integer arithmetic over
the edges of its stated ranges (tests/cpp/test_ks_tail.cpp, built with -fsanitize=address,undefined): the FP64-engine primes of the
default N = 2^16 chain, the smallest modulus the ring allows and the largest prime below 2^47 that a ring of 2^16 points can use."""
import os
import subprocess

from lattisense_amd import params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _is_prime(n):
    """deterministic Miller-Rabin for n < 2^64"""
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def _ntt_prime_below(bound, n):
    q = (bound - 1) // (2 * n) * (2 * n) + 1
    while not _is_prime(q):
        q -= 2 * n
    return q


def test_ks_tail_function(tmp_path):
    exe = str(tmp_path / "test_ks_tail")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-attributes", "-DLSA_EMULATE",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_ks_tail.cpp"), "-o", exe])
    n = 1 << 16
    P = params.CKKS_DEFAULT[n]
    fp = sorted({m for m in P["q"] + P["p"] if m < (1 << 47)})
    top = _ntt_prime_below(1 << 47, n)
    assert (1 << 47) - top < (1 << 24), top   # "just below 2^47"
    mods = [fp[0], fp[len(fp) // 2], fp[-1], _ntt_prime_below(1 << 30, n), top]
    out = subprocess.run([exe] + [str(m) for m in mods], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK ks_tail %d moduli" % len(mods) in out.stdout
