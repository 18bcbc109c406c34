"""The three chains of tests/test_gpu_bfv_operator_chains.py without a GPU: their stated properties (engine of every limb, the
level whose last key-switch digit is one limb and on which side of 2^53 that limb lies), the oracle's auxiliary primes, and the
host-only planners on every (level, term count, coefficient count, slot-sum shape, diagonal set) the GPU file runs -- a refusal
shows here and not as a GPU failure."""
import numpy as np
import pytest

from lattisense_amd import params
from tests import bfv_dot_model, bfv_poly_model
from tests.bfv_chain_cases import (AFFINE_VALUES, CHAINS, DENSE4, DOT_TERMS, LT_CASES, POLY_CASES, SLOT_CASES, T, levels, lt_diags,
                                   max_terms)
from tests.bfv_lt_model import plan_of
from tests.bfv_slot_sum_model import galois_elements_of, steps_of
from tests.boundary import bfv_fp_chain, bfv_mixed_chain, bfv_operator_chain, digit_sizes, fp_engine, is_ceiling

RINGS = (11, 13)
FP_ROWS = {"fp": lambda k: k == 6, "mixed": lambda k: 2 <= k < 8, "ceiling": lambda k: k == 0}


@pytest.fixture(scope="module")
def native():
    from lattisense_amd import build, _native
    build.build_native()
    return _native


@pytest.mark.parametrize("logn", RINGS)
@pytest.mark.parametrize("kind", CHAINS)
def test_chain_properties(kind, logn):
    n = 1 << logn
    q, p = bfv_operator_chain(kind, n)
    mods = q + p
    assert len(set(mods)) == len(mods) and len(p) == 2
    assert all(params._is_prime(m) and (m - 1) % (2 * n) == 0 and m >> 61 == 0 for m in mods)
    assert (T - 1) % (2 * n) == 0                                       # t = 65537 has slots on every ring used
    assert FP_ROWS[kind](sum(fp_engine(m) for m in mods)), [m.bit_length() for m in mods]
    top, lift = levels(kind, n)
    assert top == len(q) - 1 and digit_sizes(top, 2)[-1] == 2 and digit_sizes(lift, 2)[-1] == 1
    last = q[lift]                                                       # the one limb of the last digit at the lift level
    if kind == "ceiling":
        assert last >> 53 and all(is_ceiling(m) for m in mods)           # the conversion is kept
    else:
        assert last >> 53 == 0                                           # the ModUp lift is taken
    if kind == "fp":
        assert (q, p) == bfv_fp_chain(n)
        below47 = params.ntt_primes_below(47, n, 4)
        assert q[:2] == below47[:2] and p == below47[2:] and q[2] == params.ntt_primes_below(46, n, 1)[0]
        assert q[3] >> 45 == 1 and not any(params._is_prime(x) for x in range((1 << 45) + 1 + 2 * n, q[3], 2 * n))
    if kind == "mixed":
        assert q == bfv_mixed_chain(n)[0][:6] and p == bfv_mixed_chain(n)[1]
        bits = [m.bit_length() for m in q]
        assert bits == [46, 59, 47, 58, 48, 58] and [m.bit_length() for m in p] == [61, 61]
        assert fp_engine(q[0]) and fp_engine(q[2]) and not fp_engine(q[4])


@pytest.mark.parametrize("logn", RINGS)
@pytest.mark.parametrize("kind", CHAINS)
def test_oracle_auxiliary_primes_are_disjoint_from_the_chain(kind, logn):
    from oracle.pyoracle import Oracle
    n = 1 << logn
    q, p = bfv_operator_chain(kind, n)
    o = Oracle(n, q, p, T)
    assert o.mod == q + p + o.aux and o.aux and not set(o.aux) & set(q + p)
    assert len(set(o.aux)) == len(o.aux) and all(m.bit_length() == 61 and (m - 1) % (2 * n) == 0 and params._is_prime(m) for m in o.aux)
    assert len(o.aux) == bfv_dot_model.aux_limbs(n, q, len(q) - 1, 1)
    if kind == "ceiling":   # the chain holds the six largest primes below 2^61: the auxiliary base starts below them
        assert max(o.aux) < min(q + p)


@pytest.mark.parametrize("logn", RINGS)
@pytest.mark.parametrize("kind", CHAINS)
def test_host_planners_accept_every_case_of_the_gpu_file(native, kind, logn):
    from lattisense_amd.device import bfv_dot_plan, bfv_lt_plan, bfv_poly_plan, bfv_slot_sum_plan
    n = 1 << logn
    q, p = bfv_operator_chain(kind, n)
    nmul = bfv_dot_model.aux_limbs(n, q, len(q) - 1, 1)                  # what the context holds
    assert DOT_TERMS == (1, 2, 3, max_terms() + 1)
    for lvl in sorted(set(levels(kind, n)) | {0}):
        for terms in DOT_TERMS:
            want = bfv_dot_model.plan(n, q, lvl, terms)
            got = bfv_dot_plan(n, q, lvl, terms)
            assert got == {k: want[k] for k in ("max_terms", "groups", "aux_limbs")}, (lvl, terms)
            assert got["groups"] == 1 and got["aux_limbs"] <= nmul, (lvl, terms, got)   # no level is refused: none is lowered
        for name, cf, log_baby in POLY_CASES + (("dense4", DENSE4, 0),):
            counts = bfv_poly_model.counts(cf, log_baby)
            assert bfv_poly_plan(T, cf, log_baby) == counts, (name, lvl)
            # lsa_bfv_poly_create's own condition: the auxiliary basis of one product and of the final sum
            assert bfv_dot_model.aux_limbs(n, q, lvl, max(counts["n_pairs"], 1)) <= nmul, (name, lvl)
    assert bfv_poly_model.counts(POLY_CASES[2][1], 4)["n_pairs"] == 0 and POLY_CASES[3][1][9] == 0
    assert all(0 <= v < T for v in AFFINE_VALUES)
    for step, count, radix, rows in SLOT_CASES:
        got = bfv_slot_sum_plan(n, step, count, radix, rows)
        want = steps_of(n, step, count, radix, rows)
        assert got["galois_elements"] == galois_elements_of(n, step, count, radix, rows), (step, count, radix, rows)
        assert got["steps"] == len(want) and got["keyswitches"] == sum(len(k) for k in want)
    period = n // 2
    for name, index in LT_CASES:
        want = plan_of(period, index)
        got = bfv_lt_plan(n, period, index)
        assert (got["n1"], got["rotations"], got["babies"], got["giants"], got["moddowns"]) == \
            (want["n1"], want["rotations"], want["babies"], want["giants"], want["moddowns"]), name
        d = lt_diags(index, period, 1)
        assert np.all(d[index[1]] == T - 1) and not d[index[2]].any() and all(int(v.max()) < T for v in d.values())
