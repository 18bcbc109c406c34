"""The cases of the BFV operator-chain tests, shared by the CPU file (tests/test_bfv_operator_chains.py: chain properties, the
host-only planners accept every case) and the GPU file (tests/test_gpu_bfv_operator_chains.py: every case word for word against
the CPU models).  The chains themselves are tests/boundary.py bfv_operator_chain."""
import re
import os

import numpy as np

from tests.boundary import BFV_OPERATOR_CHAINS, BFV_OPERATOR_T, bfv_operator_chain, digit_sizes, lift_level

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS = BFV_OPERATOR_CHAINS
T = BFV_OPERATOR_T
RINGS = (11, 13, 14)          # single pass, and the two two-pass plans (6 + 7 and 7 + 7 stages; whole-limb capable)
RINGS_MULT = (12, 13, 14)     # the multiply's elementwise kernels and the dot / polynomial rigs start at N = 2^12
TWO_PASS = (13, 14)


def max_terms():
    text = open(os.path.join(ROOT, "lattisense_amd", "csrc", "tensor_sum.h")).read()
    return int(re.search(r"#define LSA_DOT_MAX_TERMS (\d+)", text).group(1))


DOT_TERMS = (1, 2, 3, max_terms() + 1)
SLOT_CASES = ((1, 5, 4, 1), (1, 7, 2, 0), (1, 21, 4, 1), (-1, 7, 2, 0))     # (step, count, radix, rows)
LT_SPARSE = [-5, 0, 3, 64, 70, 1000]
LT_CASES = (("D7", list(range(7))), ("D20", list(range(20))), ("sparse", LT_SPARSE))
AFFINE_VALUES = (0, 1, T - 1, (T - 1) // 2, (T + 1) // 2)


def _coeffs(seed, n):
    return [int(x) for x in np.random.default_rng(seed).integers(1, T, n)]


def poly_cases():
    """(id, coefficients, log_baby): dense 8 at the planner's choice; dense 16 at log_baby 2 and 4 (b = 4: 15 sources in one leaf
    launch, the ninth-term fold runs); and 16 coefficients at log_baby 4 without x^9 (source index 8): the fold without a term"""
    no9 = _coeffs(169, 16)
    no9[9] = 0
    return (("dense8", _coeffs(8, 8), 0), ("dense16_b2", _coeffs(16, 16), 2), ("dense16_b4", _coeffs(16, 16), 4), ("no_x9_b4", no9, 4))


POLY_CASES = poly_cases()
DENSE4 = _coeffs(4, 4)


def levels(kind, n):
    """(top, lift): the top level of the chain, and the highest level below it whose last key-switch digit is one limb"""
    q, p = bfv_operator_chain(kind, n)
    lift = lift_level(q, p)
    assert digit_sizes(lift, len(p))[-1] == 1 and lift < len(q) - 1
    return len(q) - 1, lift


def lt_diags(index, period, seed):
    """{k: [2][period]} uniform below t, the second diagonal all t - 1 and the third all 0"""
    rng = np.random.default_rng(seed)
    d = {k: rng.integers(0, T, (2, period)).astype(np.uint64) for k in index}
    d[index[1]][:] = T - 1
    d[index[2]][:] = 0
    return d
