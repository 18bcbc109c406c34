"""CPU-only: the plan of the BFV oblivious expansion (lsa_bfv_expand_plan, lattisense_amd/csrc/bfv_expand.h) through ctypes against
its restatement in tests/bfv_expand_model.py for every count in 1..33 and for N itself at N = 2^10 and 2^14; the refusals that need
no device; the model (the composition of Oracle.bfv_rotate, Oracle.vec and the numpy shift) decrypting to exactly the stated
coefficients on the BFV_DEFAULT[8192] chain with the message pre-scaled by 2^-k mod t; device.py planning without a GPU; the bench
tool's dry run."""
import ctypes
import types

import numpy as np
import pytest

from tests.bfv_expand_model import (decrypt_coeffs, encrypt_coeffs, expand, expected_plain, galois_elements_of, keyswitches_of,
                                    levels_of, nodes_of, prescale)

ENTRY_POINTS = {"lsa_bfv_expand_plan": 7, "lsa_bfv_expand_create": 4, "lsa_bfv_expand_destroy": 1, "lsa_bfv_expand_info": 7,
                "lsa_bfv_expand_galois_elements": 3, "lsa_bfv_expand_set_gather": 2, "lsa_bfv_expand": 12, "lsa_bfv_mul_monomial": 10}


@pytest.fixture(scope="module")
def native():
    from lattisense_amd import build, _native
    build.build_native()
    return _native


def call_plan(native, n, count, capacity=32):
    nl, nk, cnt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    g = (ctypes.c_uint64 * max(capacity, 1))()
    rc = native.lib().lsa_bfv_expand_plan(n, count, ctypes.byref(nl), ctypes.byref(nk), g, capacity, ctypes.byref(cnt))
    if rc:
        return rc, native.lib().lsa_last_error().decode()
    return 0, (nl.value, nk.value, [int(e) for e in g[: cnt.value]])


def test_binding_table_has_the_entry_points(native):
    for name, nargs in ENTRY_POINTS.items():
        assert len(native.SIGNATURES[name][1]) == nargs, name
        assert hasattr(native.lib(), name)


@pytest.mark.parametrize("n", [1 << 10, 1 << 14])
def test_plan_against_the_restated_rule(native, n):
    for count in list(range(1, 34)) + [n]:
        rc, got = call_plan(native, n, count)
        assert rc == 0, got
        k = levels_of(count)
        assert (1 << k) >= count and (k == 0 or (1 << (k - 1)) < count)
        assert got == (k, keyswitches_of(n, count), galois_elements_of(n, count)), count
        assert got[1] == sum(min(1 << j, count) for j in range(k))
        assert got[2] == sorted(n // (1 << j) + 1 for j in range(k))
        # the children are exactly the outputs 0 .. count-1, once each
        live = [0]
        for _, s, nodes, n_odd in nodes_of(n, count):
            assert nodes == len(live) and sorted(live) == list(range(nodes))
            live += [a + s for a in range(nodes) if a + s < count]
            assert len(live) == nodes + n_odd
        assert sorted(live) == list(range(count))
    assert call_plan(native, n, 1) == (0, (0, 0, []))
    assert call_plan(native, n, n)[1][:2] == (n.bit_length() - 1, n - 1)


def test_refusals_that_need_no_device(native):
    n = 1 << 10
    for args, needle in (((n, 0), "count"), ((n, -2), "count"), ((n, n + 1), "count"), ((1000, 4), "n_ring"), ((2, 1), "n_ring")):
        rc, msg = call_plan(native, *args)
        assert rc == 1 and msg.startswith("lsa_bfv_expand") and needle in msg, (args, rc, msg)
    rc, msg = call_plan(native, n, 9, capacity=3)
    assert rc == 1 and msg.startswith("lsa_bfv_expand_plan") and "capacity" in msg
    nl = ctypes.c_int()
    assert native.lib().lsa_bfv_expand_plan(n, 9, ctypes.byref(nl), None, None, 0, None) == 0 and nl.value == 4
    L = native.lib()
    h = ctypes.c_void_p()
    assert L.lsa_bfv_expand_create(None, 0, 4, ctypes.byref(h)) == 1 and "null context" in L.lsa_last_error().decode()
    assert L.lsa_bfv_expand_set_gather(None, 1) == 1 and L.lsa_last_error().decode().startswith("lsa_bfv_expand_set_gather")
    assert L.lsa_bfv_expand_info(None, *([None] * 6)) == 1 and L.lsa_last_error().decode().startswith("lsa_bfv_expand_info")
    assert L.lsa_bfv_expand_galois_elements(None, None, 0) == 1 and L.lsa_last_error().decode().startswith("lsa_bfv_expand_galois_elements")
    assert L.lsa_bfv_expand(None, None, None, 0, None, 0, 0, 1, 0, None, None, None) == 1
    assert L.lsa_last_error().decode().startswith("lsa_bfv_expand: null plan handle")
    assert L.lsa_bfv_mul_monomial(None, 0, 1, 1, None, None, 1, 0, 0, None) == 1 and "null context" in L.lsa_last_error().decode()
    L.lsa_bfv_expand_destroy(None)                                                                  # a null handle is ignored


@pytest.mark.parametrize("log_n,level,count", [(10, 2, 5), (11, 2, 16), (10, 1, 1024)])
def test_model_decrypts_to_the_stated_coefficients(log_n, level, count):
    """the BFV_DEFAULT[8192] chain (3 Q + 1 P, t = 65537): with m * 2^-k mod t encrypted, output i decrypts to
    sum_u m_(i + 2^k u) X^(2^k u) exactly; the full expansion leaves m_i in the constant coefficient and zero elsewhere"""
    from lattisense_amd import params
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    B = params.BFV_DEFAULT[8192]
    assert len(B["q"]) == 3 and len(B["p"]) == 1 and B["t"] == 65537
    n, t = 1 << log_n, B["t"]
    o = Oracle(n, B["q"], B["p"], t)
    c = Client(o, seed=31 + log_n)
    rng = np.random.default_rng(31 + count)
    m = rng.integers(0, t, n)
    ct = encrypt_coeffs(c, prescale(m, count, t), level)
    keys = {}

    def key_of(g):
        if g not in keys:
            keys[g] = c.gen_galois_key(g, 2)
        return keys[g]
    outs = expand(o, key_of, 2, ct, level, count)
    assert outs.shape == (count, 2, level + 1, n)
    assert sorted(keys) == galois_elements_of(n, count)
    check = range(count) if count <= 16 else (0, 1, 2, 3, 4, 5, 6, 7, 511, 512, 1023)
    for i in check:
        got = decrypt_coeffs(c, outs[i])
        assert np.array_equal(got, expected_plain(m, i, count, n, t)), i
        if count == n:
            assert got[0] == m[i] and not got[1:].any()


def test_device_py_plans_without_a_gpu_and_refuses_to_run(native):
    from lattisense_amd.device import BfvExpandPlan, bfv_expand_plan
    n = 1 << 12
    info = bfv_expand_plan(n, 11)
    assert (info["levels"], info["keyswitches"]) == (4, 1 + 2 + 4 + 8)
    assert info["galois_elements"] == [n // 8 + 1, n // 4 + 1, n // 2 + 1, n + 1]
    ctx = types.SimpleNamespace(n=n, h=None, stream=None)       # what a context is without a device: no handle
    plan = BfvExpandPlan(ctx, 2, 6)
    assert (plan.levels, plan.keyswitches, plan.galois_elements) == (3, 1 + 2 + 4, [n // 4 + 1, n // 2 + 1, n + 1])
    with pytest.raises(native.LsaError) as e:
        plan.run(types.SimpleNamespace(ptr=None), 1, {})
    assert e.value.code == 1 and "null context" in str(e.value)
    with pytest.raises(native.LsaError) as e:
        BfvExpandPlan(ctx, 2, n + 1)
    assert e.value.code == 1 and "count" in str(e.value)


def test_bench_tool_dry_run_prints_the_plan_counts(native):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "bench_bfv_expand.py"), "--dry-run", "--shapes", "4096", "--counts", "64,256"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2 and all(r["tool"] == "bench_bfv_expand" and r["dry_run"] for r in lines)
    by_count = {r["count"]: r["plan"] for r in lines}
    assert by_count[64] == {"levels": 6, "keyswitches": 63, "galois_elements": [4096 // (1 << j) + 1 for j in range(5, -1, -1)]}
    assert by_count[256]["keyswitches"] == 255 and by_count[256]["levels"] == 8
