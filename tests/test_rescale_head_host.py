"""CPU-only: the merged ModDown + rescale head per coefficient (lattisense_amd/csrc/ntt_core.h, rescale_head_*), the functions the
forward transform's load-side prologue and the rescale-head form of the base conversion (k_baseconv<.., HEAD>) both call, against
128-bit integer arithmetic (tests/cpp/test_rescale_head.cpp, built with -fsanitize=address,undefined): q_l at 45, 46, 56 and 61 bits,
q_j on either side of q_l / 2 -- just above (one conditional subtraction, at its limit), just below (the general reduction, at its
smallest quotient) -- of q_l's own size, larger than q_l, and a 30-bit one (the general reduction with a large quotient)."""
import os
import subprocess

from lattisense_amd import params
from tests.test_ks_tail_host import _is_prime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 14


def _prime(bound, step):
    """the NTT prime (1 mod 2N) next to `bound`: the first at or above it (step > 0) or below it (step < 0)"""
    q = bound // (2 * N) * (2 * N) + 1
    if step > 0 and q < bound:
        q += 2 * N
    while not _is_prime(q) or (step < 0 and q >= bound):
        q += step * 2 * N
    return q


def test_rescale_head_functions(tmp_path):
    exe = str(tmp_path / "test_rescale_head")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-attributes", "-DLSA_EMULATE",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_rescale_head.cpp"), "-o", exe])
    Q = params.CKKS_DEFAULT[65536]["q"]
    B = params.CKKS_BOOTSTRAP_65536
    qls = [_prime(1 << 45, -1), Q[1], _prime(1 << 56, -1), max(B["q"] + B["p"])]
    assert [q.bit_length() for q in qls] == [45, 46, 56, 61], qls
    pairs = []
    for ql in qls:
        above, below = _prime(ql // 2 + 1, +1), _prime(ql // 2, -1)
        assert 2 * above >= ql > 2 * below and above - below < (1 << 30)
        same = _prime(ql, -1)
        larger = _prime(min(2 * ql, (1 << 61) - 1), -1) if ql.bit_length() < 61 else _prime(ql + 1, +1)
        assert larger > ql and larger.bit_length() <= 61
        for qj in (above, below, same, larger, _prime(1 << 30, -1)):
            pairs += [ql, qj]
    # the chain's own neighbours too: the integer-engine q_0 under an FP64-engine q_l and the reverse
    pairs += [Q[1], Q[0], Q[0], Q[1]]
    out = subprocess.run([exe] + [str(m) for m in pairs], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK rescale_head %d pairs" % (len(pairs) // 2) in out.stdout, out.stdout
    near, general = (int(out.stdout.split("(")[1].split()[i]) for i in (0, 2))
    assert near >= 12 and general >= 8, out.stdout   # both reductions ran
