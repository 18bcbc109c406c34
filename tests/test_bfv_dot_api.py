"""BFV encrypted inner product without a GPU: the headroom rule of lsa_bfv_dot_plan (tables.cpp bfv_dot_plan, compiled for the
host by tests/cpp/test_bfv_dot_plan.cpp, and the library's own entry point) against the rule stated on Python integers in
tests/bfv_dot_model.py; the model against exact integer arithmetic at N = 64, on random operands and on near-worst operands at a
full group; and the same near-worst sum pushed through M(1) auxiliary primes where the rule asks for M(m), which must differ
from exact -- the check that holds the rule to the mathematics, and the proof that it can fail."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from lattisense_amd import params
from tests import bfv_dot_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lattisense_amd.h")
ENTRY_POINTS = {"lsa_bfv_mult_sum": 13, "lsa_bfv_dot": 14, "lsa_bfv_dot_plan": 8, "lsa_set_bfv_dot_chunk": 2}


def tight_chain(n):
    """three Q primes whose top level leaves one spare bit at ring degree n: bitlen(Q) + log n = 61 * 3 - 1"""
    logn = n.bit_length() - 1
    base, rem = divmod(182 - logn, 3)   # primes just below 2^b multiply to bit lengths that add up
    q = params.ntt_primes_below(base + 1, n, rem) + params.ntt_primes_below(base, n, 3 - rem)
    assert model.product(q).bit_length() + logn == 182
    return q


def shipped_sets():
    out = [(n, P["q"]) for n, P in sorted(params.BFV_DEFAULT.items())]
    out.append((1 << 16, params.bfv_n16_chain()["q"]))
    return out


def plan_cases():
    cases = []
    for n, q in shipped_sets() + [(1 << 12, tight_chain(1 << 12)), (64, tight_chain(64)), (1 << 12, params.BFV_DEFAULT[8192]["q"])]:
        for level in range(len(q)):
            mt = model.plan(n, q, level, 1)["max_terms"]
            for terms in sorted({1, 2, 3, 4, 5, 16, 17, 33, 128, 129, 256, 257, mt - 1, mt, mt + 1, 2 * mt, 2 * mt + 1, 3 * mt + 2} - {0}):
                if 1 <= terms < (1 << 31) - (1 << 30):
                    cases.append((n, q, level, terms))
    return cases


def test_header_signatures_and_wrappers():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    from lattisense_amd import _native, device
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, txt, flags=re.S)
        assert m, name + " is not declared"
        assert len(m.group(1).split(",")) == nargs, name
        assert len(_native.SIGNATURES[name][1]) == nargs, name
    assert list(inspect.signature(device.DeviceContext.bfv_mult_sum).parameters)[:5] == ["self", "level", "a_list", "b_list", "batch"]
    assert list(inspect.signature(device.DeviceContext.bfv_dot).parameters)[:6] == ["self", "level", "a_list", "b_list", "rlk", "batch"]
    assert list(inspect.signature(device.bfv_dot_plan).parameters) == ["n", "q", "level", "terms"]


def test_rule_values_at_the_shipped_sets():
    """the figures the documents quote, from the rule on Python integers"""
    B = params.BFV_DEFAULT
    assert model.plan(1 << 14, B[16384]["q"], 5, 1)["G"] == 24
    assert model.plan(1 << 15, B[32768]["q"], 11, 1)["G"] == 17
    assert model.plan(1 << 13, B[8192]["q"], 2, 1)["G"] == 7
    assert model.plan(1 << 12, tight_chain(1 << 12), 2, 5) == {"G": 1, "max_terms": 2, "groups": 3, "aux_limbs": 3}
    # level 1 of the N = 2^13 primes at N = 2^12: the third term takes a third auxiliary prime
    q = B[8192]["q"]
    assert [model.aux_limbs(1 << 12, q, 1, m) for m in (1, 2, 3)] == [2, 2, 3]
    for n, q in shipped_sets():
        for level in range(len(q)):
            p = model.plan(n, q, level, 1)
            nmul = (model.product(q).bit_length() + n.bit_length() - 1 + 60) // 61
            assert p["aux_limbs"] == model.aux_limbs(n, q, level, 1)
            assert model.aux_limbs(n, q, level, p["max_terms"]) <= nmul


def test_plan_host_function_against_the_rule(tmp_path):
    exe = str(tmp_path / "test_bfv_dot_plan")
    csrc = os.path.join(ROOT, "lattisense_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-DLSA_EMULATE", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_bfv_dot_plan.cpp"), os.path.join(csrc, "tables.cpp"), "-o", exe])
    cases = plan_cases()
    text = "".join("%d %d %d %d %s\n" % (n.bit_length() - 1, level, terms, len(q), " ".join(map(str, q))) for n, q, level, terms in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    got = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    assert len(got) == len(cases)
    for (n, q, level, terms), r in zip(cases, got):
        p = model.plan(n, q, level, terms)
        last = terms - (p["groups"] - 1) * p["max_terms"]
        want = (p["G"], p["max_terms"], p["groups"], p["aux_limbs"], model.aux_limbs(n, q, level, 1), model.aux_limbs(n, q, level, last))
        assert r == want, (n, level, terms)


def test_plan_entry_point_against_the_rule():
    from lattisense_amd import build, _native
    from lattisense_amd.device import bfv_dot_plan
    build.build_native()
    for n, q, level, terms in plan_cases():
        p = model.plan(n, q, level, terms)
        assert bfv_dot_plan(n, q, level, terms) == {"max_terms": p["max_terms"], "groups": p["groups"], "aux_limbs": p["aux_limbs"]}, (n, level, terms)
    L = _native.lib()
    q = params.BFV_DEFAULT[8192]["q"]
    qa = (ctypes.c_uint64 * 3)(*q)
    for args in ((8191, qa, 3, 0, 1), (8192, None, 3, 0, 1), (8192, qa, 3, 3, 1), (8192, qa, 3, -1, 1), (8192, qa, 3, 0, 0), (8192, qa, 0, 0, 1)):
        assert L.lsa_bfv_dot_plan(*args, None, None, None) == 1, args      # LSA_ERR_ARG
        assert L.lsa_last_error().decode().startswith("bfv_dot"), args
    assert L.lsa_bfv_dot_plan(8192, qa, 3, 2, 257, None, None, None) == 0   # every output is optional


def _rand_ct(rng, o, lvl):
    ct = np.empty((2, lvl + 1, o.n), dtype=np.uint64)
    for i in range(lvl + 1):
        ct[:, i, :] = rng.integers(0, o.mod[i], size=(2, o.n), dtype=np.uint64)
    return ct


@pytest.fixture(scope="module")
def small():
    """N = 64 on the primes of the N = 2^13 set (== 1 mod 2^14, so NTT primes here too)"""
    from oracle.pyoracle import Oracle
    P = params.BFV_DEFAULT[8192]
    return Oracle(64, P["q"], P["p"], P["t"])


def test_model_is_bfv_mult_at_one_term_and_exact_on_random_operands(small):
    o = small
    rng = np.random.default_rng(64)
    for lvl in range(o.nq):
        A, B = [_rand_ct(rng, o, lvl) for _ in range(5)], [_rand_ct(rng, o, lvl) for _ in range(5)]
        one = model.mult_sum(o, lvl, A[:1], B[:1])
        assert np.array_equal(one, o.bfv_mult(lvl, A[0], B[0])), lvl
        assert np.array_equal(one, model.exact_d3(o, lvl, A[:1], B[:1])), lvl
        assert np.array_equal(model.mult_sum(o, lvl, A, B), model.exact_d3(o, lvl, A, B)), lvl
        sq = model.mult_sum(o, lvl, A[:2], A[:2])
        assert np.array_equal(sq, model.exact_d3(o, lvl, A[:2], A[:2])), ("squares", lvl)


def test_near_worst_operands_at_a_full_group():
    """three 58-bit primes at N = 64: bitlen(Q) = 174, G = 183 - 174 - 6 = 3, so a full group is 8 terms over M(8) = 3 auxiliary
    primes.  Every coefficient of every operand is +-(Q/2 - Q/2^20) (exactly +-(Q-1)/2 is the edge of the oracle's float-corrected
    conversion, not of this operator); equal signs make every product add up.  9 terms: a full group and one more"""
    from oracle.pyoracle import Oracle
    n = 64
    q = params.ntt_primes_below(58, n, 3)
    o = Oracle(n, q, params.ntt_primes_below(59, n, 1), 65537)
    lvl = 2
    pl = model.plan(n, q, lvl, 8)
    assert pl == {"G": 3, "max_terms": 8, "groups": 1, "aux_limbs": 3} and len(o.aux) == 3
    Q = model.product(q)
    c = Q // 2 - (Q >> 20)
    pos, neg = model.constant_ct(o, lvl, c, c), model.constant_ct(o, lvl, -c, -c)
    mixed = model.constant_ct(o, lvl, c, -c)
    for name, As, Bs in (("++", [pos] * 8, [pos] * 8), ("+-", [pos] * 8, [neg] * 8), ("--", [neg] * 8, [neg] * 8),
                         ("mixed", [mixed] * 8, [pos] * 8)):
        assert np.array_equal(model.mult_sum(o, lvl, As, Bs), model.exact_d3(o, lvl, As, Bs)), name
    # a full group and one more term: two scale-downs, each exact, added in Q (two roundings: not the rounding of the whole sum)
    two = model.mult_sum(o, lvl, [pos] * 9, [neg] * 9)
    assert np.array_equal(two, model.exact_mult_sum(o, lvl, [pos] * 9, [neg] * 9))
    assert not np.array_equal(two, model.exact_d3(o, lvl, [pos] * 9, [neg] * 9))
    # the sum of a full group is as large as the basis can hold: within a bit of Q * QMul / 2
    top = max(abs(v) for dk in model.exact_tensor_sum(o, lvl, [pos] * 8, [pos] * 8) for v in dk)
    room = Q * model.product(o.aux[:3]) // 2
    assert top < room < 2 * top


def test_m1_limbs_differ_from_exact_where_the_rule_asks_for_more(small):
    """level 1 of the N = 2^13 primes at N = 64: bitlen(Q_1) + log N = 115, M(1) = 2 (122 bits of QMul), M(m) = 3 from m = 129.
    Near-worst operands, one pair repeated: the term count is the first at which the exact sum passes Q * QMul_2 / 2, taken from
    the actual product sizes.  There the rule's M(m) limbs are exact and M(1) limbs are not; one term fewer still fits both"""
    o, lvl = small, 1
    Q = model.product(o.q[:2])
    c = Q // 2 - (Q >> 20)
    a, b = model.constant_ct(o, lvl, c, c), model.constant_ct(o, lvl, -c, -c)
    one = max(abs(v) for dk in model.exact_tensor_sum(o, lvl, [a], [a]) for v in dk)
    room = Q * model.product(o.aux[:2]) // 2
    count = room // one + 1
    assert model.aux_limbs(o.n, o.q, lvl, 1) == 2
    assert 2 <= count <= model.plan(o.n, o.q, lvl, count)["max_terms"], count
    print("terms: %d, M(terms) = %d" % (count, model.aux_limbs(o.n, o.q, lvl, count)))
    assert model.aux_limbs(o.n, o.q, lvl, count) == 3       # the bitlen formula's slack ends before the basis does
    for As, Bs in (([a] * count, [a] * count), ([a] * count, [b] * count)):
        exact = model.exact_d3(o, lvl, As, Bs)
        assert np.array_equal(model.mult_sum(o, lvl, As, Bs), exact)
        assert not np.array_equal(model.mult_sum(o, lvl, As, Bs, force_aux=2), exact)
    fewer = count - 1
    assert np.array_equal(model.mult_sum(o, lvl, [a] * fewer, [a] * fewer, force_aux=2), model.exact_d3(o, lvl, [a] * fewer, [a] * fewer))


def test_bench_tool_dry_run():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_bfv_dot.py"), "--dry-run"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    import json
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert lines and all(r["tool"] == "bench_bfv_dot" and r["dry_run"] for r in lines)
    assert {(r["n"], r["level"], r["batch"]) for r in lines} == {(1 << 14, 3, 256), (1 << 15, 11, 32)}
