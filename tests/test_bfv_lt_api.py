"""CPU-only: the BFV slot encoder and linear transform (lsa_bfv_encode, lsa_bfv_lt_*, lsa_bfv_linear_transform) as far as they go
without a device.  The symbols and their argument types; the refusals that are decided before a device is needed; the encoder's
host tables (the routine that feeds k_bfv_encode_t and runs above N = 2^15) against Client.bfv_encode; the plan counts of
lsa_lt_plan_rotations against tests/bfv_lt_model.py's own restatement; and the model against the oracle's double-hoisted
linear transform and against the plaintext matrix product mod t at N = 4096, BFV_DEFAULT[4096], level 1 -- the (level, D) pairs
the GPU decrypt checks of tests/test_gpu_bfv_lt.py rely on."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

N = 4096
LEVEL = 1
ENTRY_POINTS = {"lsa_bfv_encode": 8, "lsa_bfv_lt_create": 9, "lsa_bfv_lt_destroy": 1, "lsa_bfv_lt_info": 10, "lsa_bfv_lt_diagonals": 3,
                "lsa_bfv_lt_galois_elements": 3, "lsa_bfv_lt_plaintext": 4, "lsa_bfv_linear_transform": 11}
SPARSE = [-5, 0, 3, 64, 70, 1000]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    from lattisense_amd import build, _native
    build.build_native()
    return _native


@pytest.fixture(scope="module")
def bfv():
    from lattisense_amd import params
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    from tests.bfv_slot_sum_model import make_evaluator
    B = params.BFV_DEFAULT[N]
    o = Oracle(N, B["q"], B["p"], B["t"])
    c = Client(o, seed=23)
    rng = np.random.default_rng(23)
    vals = rng.integers(0, B["t"], N)
    return types.SimpleNamespace(o=o, c=c, ev=make_evaluator(o, c, LEVEL), t=B["t"], rng=rng, vals=vals, ct=c.bfv_encrypt(vals, LEVEL))


def random_diags(rng, index, period, t):
    return {k: rng.integers(0, t, (2, period)).astype(np.uint64) for k in index}


def test_binding_table_has_the_entry_points(native):
    for name, nargs in ENTRY_POINTS.items():
        assert len(native.SIGNATURES[name][1]) == nargs, name
        assert hasattr(native.lib(), name)
    assert native.SIGNATURES["lsa_bfv_encode"][1][3] == ctypes.POINTER(ctypes.c_uint64)
    assert native.SIGNATURES["lsa_bfv_lt_create"][1][6] == ctypes.c_double
    assert native.SIGNATURES["lsa_bfv_lt_destroy"][0] is None


def test_refusals_without_a_device(native):
    L = native.lib()
    h = ctypes.c_void_p()
    one = (ctypes.c_uint64 * 2)(0, 0)
    idx = (ctypes.c_int * 1)(0)

    def refused(rc, prefix):
        msg = L.lsa_last_error().decode()
        assert rc == 1 and msg.startswith(prefix), (rc, msg)

    refused(L.lsa_bfv_encode(None, 0, 0, one, None, 0, 1, None), "lsa_bfv_encode")
    refused(L.lsa_bfv_lt_create(None, 0, 2, 1, idx, one, 0.0, None, ctypes.byref(h)), "lsa_bfv_lt_create")
    refused(L.lsa_bfv_lt_create(None, 0, 2, 1, idx, one, 0.0, None, None), "lsa_bfv_lt_create")
    refused(L.lsa_bfv_lt_info(None, *([None] * 9)), "lsa_bfv_lt_info")
    refused(L.lsa_bfv_lt_diagonals(None, idx, 1), "lsa_bfv_lt_diagonals")
    refused(L.lsa_bfv_lt_galois_elements(None, one, 1), "lsa_bfv_lt_galois_elements")
    refused(L.lsa_bfv_lt_plaintext(None, 0, one, 2), "lsa_bfv_lt_plaintext")
    refused(L.lsa_bfv_linear_transform(None, None, None, None, 1, 0, 0, 0, None, None, None), "lsa_bfv_linear_transform")
    L.lsa_bfv_lt_destroy(None)                                  # a null handle is ignored


def test_encoder_host_tables_against_the_client():
    """BfvEncodeTables (csrc/tables.cpp), compiled alone: the index matrix and the inverse transform mod t give
    Client.bfv_encode's coefficients at N = 1024 and 4096 (t = 65537) and at t = 786433; a t without slots is refused by name"""
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    import tempfile
    csrc = os.path.join(ROOT, "lattisense_amd", "csrc")
    src = r'''
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include "tables.h"
int main(int argc, char** argv) {
    const int n = atoi(argv[1]);
    const unsigned long long t = strtoull(argv[2], nullptr, 10);
    lsa::BfvEncodeTables T;
    try { T.build(n, t); } catch (const std::invalid_argument& e) { printf("refused: %s\n", e.what()); return 0; }
    std::vector<uint64_t> v(n), c(n);
    for (int i = 0; i < n; i++) if (scanf("%llu", (unsigned long long*)&v[i]) != 1) return 2;
    T.encode(v.data(), c.data());
    for (int i = 0; i < n; i++) printf("%llu\n", (unsigned long long)c[i]);
    return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "enc.cpp"), "w").write(src)
        exe = os.path.join(d, "enc")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DLSA_EMULATE", "-I" + csrc, "-o", exe, os.path.join(d, "enc.cpp"), os.path.join(csrc, "tables.cpp")])
        rng = np.random.default_rng(5)
        for n, t in ((1024, 65537), (4096, 65537), (4096, 786433)):
            q = [549755731969, 549755904001]
            c = Client(Oracle(n, q, [1073750017], t), seed=1)
            for vals in (rng.integers(0, t, n), np.full(n, t - 1), np.eye(1, n, n // 2, dtype=np.int64)[0]):
                out = subprocess.run([exe, str(n), str(t)], input="\n".join(str(int(v)) for v in vals), capture_output=True, text=True, check=True)
                got = np.array([int(x) for x in out.stdout.split()], dtype=np.uint64)
                assert np.array_equal(got, c.bfv_encode(vals)), (n, t)
        for n, t, needle in ((4096, 65539, "1 mod 2N"), (4096, (1 << 32) + 15, "2^32"), (65536, 65537, "1 mod 2N"), (8, 273, "prime")):
            out = subprocess.run([exe, str(n), str(t)], capture_output=True, text=True, check=True).stdout
            assert out.startswith("refused:") and needle in out, (n, t, out)


def test_plan_counts_against_the_restated_rule(native):
    from lattisense_amd.device import BfvLinearTransformPlan, bfv_lt_plan, plan_rotations
    from tests.bfv_lt_model import plan_of
    cases = [(N // 2, list(range(d))) for d in (1, 2, 3, 7, 64, 160)] + [(N // 2, SPARSE), (64, list(range(7))), (64, [-1, 0, 5, 17, 40, 62])]
    for period, index in cases:
        want = plan_of(period, index)
        n1, rot = plan_rotations(period, index)
        assert (n1, rot) == (want["n1"], want["rotations"]), (period, index)
        info = bfv_lt_plan(N, period, index)
        assert (info["n1"], info["babies"], info["giants"], info["moddowns"]) == (want["n1"], want["babies"], want["giants"], want["moddowns"])
        assert info["galois_elements"] == sorted(pow(5, r, 2 * N) for r in want["rotations"])
    assert plan_of(N // 2, list(range(160)))["n1"] == 16 and len(plan_of(N // 2, list(range(160)))["giants"]) == 10
    assert plan_of(N // 2, [0, 1])["n1"] == 0 and plan_of(N // 2, [0, 1])["giants"] == [0] and plan_of(N // 2, [0, 1])["moddowns"] == 1
    ctx = types.SimpleNamespace(n=N, h=None, stream=None)       # what a context is without a device: no handle
    plan = BfvLinearTransformPlan(ctx, LEVEL, {k: np.zeros(64, dtype=np.uint64) for k in (-1, 0, 5, 17, 40, 62)})
    assert plan.period == 64 and plan.diagonals == [0, 5, 17, 40, 62, 63]
    assert plan.galois_elements == sorted(pow(5, r, 2 * N) for r in plan_of(64, [-1, 0, 5, 17, 40, 62])["rotations"])
    with pytest.raises(native.LsaError) as e:
        plan.run(types.SimpleNamespace(ptr=None), 1, {})
    assert e.value.code == 1 and "lsa_bfv_lt_create: null" in str(e.value)
    with pytest.raises(Exception):
        plan_rotations(N // 2, [1, 1 + N // 2])                 # equal mod period


@pytest.mark.parametrize("D", [3, 7])
def test_model_equals_the_oracle_double_hoisted_transform(bfv, D):
    from oracle.ckks_bootstrap import Ct, linear_transform as oracle_lt
    from tests.bfv_lt_model import linear_transform, model_plains
    period = N // 2
    diags = random_diags(bfv.rng, range(D), period, bfv.t)
    plains = model_plains(bfv.o, bfv.c, LEVEL, period, diags)
    got = linear_transform(bfv.ev, bfv.ct, LEVEL, period, list(diags), plains)
    x = Ct(np.stack([np.stack([bfv.o.ntt(j, bfv.ct[pl, j]) for j in range(LEVEL + 1)]) for pl in range(2)]), LEVEL, 1.0)
    want = oracle_lt(bfv.ev, x, {k: None for k in diags}, plains=plains, rescale=False, n_slots=period, double_hoist=True)
    want = np.stack([np.stack([bfv.o.intt(j, want.data[pl, j]) for j in range(LEVEL + 1)]) for pl in range(2)])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("index, period", [([0], N // 2), ([0, 1], N // 2), (list(range(7)), N // 2), (SPARSE, N // 2), (list(range(7)), 64)])
def test_model_decrypts_to_the_plain_product(bfv, index, period):
    """level 1 of BFV_DEFAULT[4096] (Q = 2^78) carries these products: the noise of a term is about N t = 2^28 times that of a
    key-switched ciphertext, far below Q / 2t = 2^61"""
    from tests.bfv_lt_model import linear_transform, model_plains, plain_lt
    diags = random_diags(bfv.rng, index, period, bfv.t)
    plains = model_plains(bfv.o, bfv.c, LEVEL, period, diags)
    out = linear_transform(bfv.ev, bfv.ct, LEVEL, period, list(diags), plains)
    assert np.array_equal(bfv.c.bfv_decrypt(out).astype(np.int64), plain_lt(bfv.vals, diags, period, N, bfv.t))


def test_bench_tool_dry_run(native):
    import json
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_bfv_lt.py"), "--dry-run"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    lt = [r for r in lines if r["kind"] == "lt"]
    assert {(r["n"], r["D"]) for r in lt} == {(n, d) for n in (16384, 32768) for d in (8, 64, 256)}
    assert all(r["tool"] == "bench_bfv_lt" and r["dry_run"] for r in lines)
    d64 = [r for r in lt if r["n"] == 16384 and r["D"] == 64][0]
    assert d64["plan"]["moddowns"] < 64 and d64["composition"]["moddowns"] == 63
