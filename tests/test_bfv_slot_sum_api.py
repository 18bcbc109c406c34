"""CPU-only: the plan of the BFV slot sum (lsa_bfv_slot_sum_plan, lattisense_amd/csrc/slot_sum.h) through ctypes, and its two CPU
models.  For every count in 1..130, step in {1, 3, -1, -64}, radix in {2, 4} and rows in {0, 1} at N = 2^10 the returned counts and
Galois elements equal an independent restatement of the rule (below): powers of 5 for the column rotations plus 2N-1 for the row
step; a replay of the steps on index multisets over the 2 x N/2 slot matrix gives the slot sum.  Every bad argument is refused with
a message that begins "lsa_bfv_slot_sum" and names it.  At N = 2^10 on the BFV_DEFAULT[8192] primes the NTT-domain statement of the
words and the coefficient-domain (gathering) statement agree word for word and decrypt to exactly the plaintext sum mod t.
device.py plans without a GPU and refuses to run without one."""
import ctypes
import types
from collections import Counter

import numpy as np
import pytest

N = 1 << 10
H = N // 2
ROW = 2 * N - 1
ENTRY_POINTS = {"lsa_bfv_slot_sum_plan": 11, "lsa_bfv_slot_sum_create": 7, "lsa_bfv_slot_sum_destroy": 1, "lsa_bfv_slot_sum_info": 10,
                "lsa_bfv_slot_sum_galois_elements": 3, "lsa_bfv_slot_sum_set_gather": 2, "lsa_bfv_slot_sum": 11}
MODEL_CASES = [(1, 5, 4, 0), (1, 21, 4, 1), (1, 7, 2, 1), (-1, 8, 4, 0), (1, 512, 4, 1), (1, 512, 2, 1), (3, 12, 4, 0)]


@pytest.fixture(scope="module")
def native():
    from lattisense_amd import build, _native
    build.build_native()
    return _native


def restated_steps(h, step, count, radix, rows):
    """the rule, written again: [(("row",) | ("col", rotation mod h), "tail" | "next"), ...] per step; None where a column
    rotation is 0 mod h"""
    s, n = step, count
    steps = [[(("row",), "next")]] if rows else []
    while n > 1:
        keys = []
        if n % 2:
            keys.append((("col", (n - 1) * s % h), "tail"))
            n -= 1
        if radix == 4 and n % 4 == 0:
            keys += [(("col", i * s % h), "next") for i in (1, 2, 3)]
            s, n = 4 * s, n // 4
        else:
            keys.append((("col", s % h), "next"))
            s, n = 2 * s, n // 2
        if any(k[1] == 0 for k, _ in keys):
            return None
        steps.append(keys)
    return steps


def element(key):
    return ROW if key[0] == "row" else pow(5, key[1], 2 * N)


def replay(h, steps):
    """x as a multiset of (row, column) offsets of the input over the 2 x h slot matrix"""
    x, tail = Counter({(0, 0): 1}), Counter()
    for keys in steps:
        nxt = Counter(x)
        for key, dest in keys:
            if key[0] == "row":
                moved = Counter({(1 - r, i): c for (r, i), c in x.items()})
            else:
                moved = Counter({(r, (i + key[1]) % h): c for (r, i), c in x.items()})
            if dest == "tail":
                tail += moved
            else:
                nxt += moved
        x = nxt
    return x + tail


def call_plan(native, n, step, count, radix, rows, capacity=64):
    ns, nk, nm, cnt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    g = (ctypes.c_uint64 * capacity)()
    rc = native.lib().lsa_bfv_slot_sum_plan(n, step, count, radix, rows, ctypes.byref(ns), ctypes.byref(nk), ctypes.byref(nm), g, capacity,
                                            ctypes.byref(cnt))
    if rc:
        return rc, native.lib().lsa_last_error().decode()
    return 0, (ns.value, nk.value, nm.value, [int(e) for e in g[: cnt.value]])


def test_binding_table_has_the_entry_points(native):
    for name, nargs in ENTRY_POINTS.items():
        assert len(native.SIGNATURES[name][1]) == nargs, name
        assert hasattr(native.lib(), name)


def test_plan_against_the_restated_rule_and_a_replay(native):
    refused = 0
    for step in (1, 3, -1, -64):
        for radix in (2, 4):
            for rows in (0, 1):
                for count in range(1, 131):
                    want = restated_steps(H, step, count, radix, rows)
                    rc, got = call_plan(native, N, step, count, radix, rows)
                    if want is None:
                        assert rc == 1 and got.startswith("lsa_bfv_slot_sum") and "step" in got and "N/2" in got, (step, radix, count, got)
                        refused += 1
                        continue
                    assert rc == 0, got
                    ns, nk, nm, elts = got
                    has_tail = any(d == "tail" for keys in want for _, d in keys)
                    assert all(len(keys) <= 4 for keys in want)
                    assert ns == len(want) and nk == sum(len(keys) for keys in want) and nm == len(want) + (1 if has_tail else 0)
                    assert elts == sorted({element(k) for keys in want for k, _ in keys}), (step, radix, rows, count)
                    assert (ROW in elts) == bool(rows)
                    cols = {pow(5, r, 2 * N) for r in range(1, H)}
                    assert all(e == ROW or e in cols for e in elts)
                    sums = replay(H, want)
                    expect = Counter((r, i * step % H) for i in range(count) for r in ((0, 1) if rows else (0,)))
                    assert sums == expect, (step, radix, rows, count)
    # step -64 has order 8 in Z/512: every count above 8 meets a rotation that is a multiple of N/2, and nothing else is refused
    assert refused == 2 * 2 * (130 - 8)


def test_worked_examples(native):
    assert call_plan(native, N, 1, 1, 2, 0) == (0, (0, 0, 0, []))                                   # a copy: no keys
    assert call_plan(native, N, 1, 1, 4, 1) == (0, (1, 1, 1, [ROW]))                                # the row step alone
    assert call_plan(native, N, 1, 5, 4, 0) == (0, (1, 4, 2, sorted(pow(5, r, 2 * N) for r in (1, 2, 3, 4))))
    assert call_plan(native, N, 1, 5, 4, 1) == (0, (2, 5, 3, sorted([ROW] + [pow(5, r, 2 * N) for r in (1, 2, 3, 4)])))
    assert call_plan(native, N, 1, 100, 0, 1) == call_plan(native, N, 1, 100, 4, 1)                 # the default radix
    assert call_plan(native, N, 1, H, 2, 1)[1][:3] == (10, 10, 10)                                  # every slot holds the total
    assert call_plan(native, N, 1, 100, 2, 7) == call_plan(native, N, 1, 100, 2, 1)                 # rows is a flag


def test_refusals_name_the_argument(native):
    for args, needle in (((N, 1, 0, 2, 0), "count"), ((N, 1, -3, 2, 1), "count"), ((N, 1, H + 1, 2, 0), "count"), ((N, 1, 8, 3, 0), "radix"),
                         ((N, 1, 8, -2, 1), "radix"), ((N, 0, 2, 2, 0), "step"), ((N, H, 2, 4, 1), "step"), ((N, H // 2, 3, 2, 0), "step"),
                         ((N, H // 2, 4, 4, 0), "step"), ((1000, 1, 2, 2, 0), "n_ring")):
        rc, msg = call_plan(native, *args)
        assert rc == 1 and msg.startswith("lsa_bfv_slot_sum") and needle in msg, (args, rc, msg)
    assert call_plan(native, N, 1, H, 2, 1)[0] == 0                                                 # count == N/2 is a whole row
    rc, msg = call_plan(native, N, 1, 100, 2, 1, capacity=2)
    assert rc == 1 and msg.startswith("lsa_bfv_slot_sum") and "capacity" in msg
    ns = ctypes.c_int()
    assert native.lib().lsa_bfv_slot_sum_plan(N, 1, 100, 2, 1, ctypes.byref(ns), None, None, None, 0, None) == 0 and ns.value == 7
    L = native.lib()
    h = ctypes.c_void_p()
    assert L.lsa_bfv_slot_sum_create(None, 0, 1, 4, 0, 0, ctypes.byref(h)) == 1 and "null context" in L.lsa_last_error().decode()
    assert L.lsa_bfv_slot_sum_set_gather(None, 1) == 1 and L.lsa_last_error().decode().startswith("lsa_bfv_slot_sum_set_gather")
    assert L.lsa_bfv_slot_sum_info(None, *([None] * 9)) == 1 and L.lsa_last_error().decode().startswith("lsa_bfv_slot_sum_info")
    L.lsa_bfv_slot_sum_destroy(None)                                                                # a null handle is ignored


def test_models_agree_and_decrypt_to_the_exact_sum():
    """N = 2^10, the 3 Q + 1 P primes of BFV_DEFAULT[8192], t = 65537, top level: the header's words (NTT-domain steps on the
    oracle's rotate_ext / add_ext / moddown / add) equal the gathering form's (coefficient-domain x, no P * c0 in the products),
    and decrypt to the slot sum mod t exactly"""
    from lattisense_amd import params
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    from tests.bfv_slot_sum_model import galois_elements_of, make_evaluator, plain_slot_sum, slot_sum, slot_sum_coeff
    B = params.BFV_DEFAULT[8192]
    assert len(B["q"]) == 3 and len(B["p"]) == 1 and B["t"] == 65537
    o = Oracle(N, B["q"], B["p"], B["t"])
    c = Client(o, seed=17)
    ev = make_evaluator(o, c, 2)
    rng = np.random.default_rng(17)
    vals = rng.integers(0, B["t"], N)
    ct = c.bfv_encrypt(vals, 2)
    assert np.array_equal(c.bfv_decrypt(ct).astype(np.int64), vals)
    for step, count, radix, rows in MODEL_CASES:
        a = slot_sum(ev, ct, 2, step, count, radix, rows)
        assert set(galois_elements_of(N, step, count, radix, rows)) <= set(ev.glk)
        b = slot_sum_coeff(ev, ct, 2, step, count, radix, rows)
        assert np.array_equal(a, b), (step, count, radix, rows)
        want = plain_slot_sum(vals, N, step, count, rows, B["t"])
        assert np.array_equal(c.bfv_decrypt(a).astype(np.int64), want), (step, count, radix, rows)


def test_device_py_plans_without_a_gpu_and_refuses_to_run(native):
    import torch
    from lattisense_amd.device import BfvSlotSumPlan, bfv_slot_sum_plan
    info = bfv_slot_sum_plan(N, 3, 21, radix=4, rows=1)
    assert (info["steps"], info["keyswitches"], info["moddowns"]) == (3, 9, 4)
    assert info["galois_elements"] == sorted([ROW] + [pow(5, r, 2 * N) for r in (3, 6, 9, 12, 24, 36, 48, 60)])
    ctx = types.SimpleNamespace(n=N, h=None, stream=None)       # what a context is without a device: no handle
    plan = BfvSlotSumPlan(ctx, 2, -1, 8)
    assert plan.galois_elements == sorted(pow(5, r, 2 * N) for r in (H - 4, H - 3, H - 2, H - 1))
    assert (plan.steps, plan.keyswitches, plan.moddowns) == (2, 4, 2)   # radix 4
    plan2 = BfvSlotSumPlan(ctx, 2, -1, 8, radix=2, rows=1)
    assert plan2.galois_elements == sorted([ROW] + [pow(5, r, 2 * N) for r in (H - 4, H - 2, H - 1)])
    assert (plan2.steps, plan2.keyswitches, plan2.moddowns) == (4, 4, 4)
    with pytest.raises(native.LsaError) as e:
        plan.run(types.SimpleNamespace(ptr=None), 1, {})
    assert e.value.code == 1 and "null context" in str(e.value)
    if not torch.cuda.is_available():
        from lattisense_amd import params
        from lattisense_amd.device import ALGO_BFV, DeviceContext
        P = params.BFV_DEFAULT[8192]
        with pytest.raises(native.LsaError) as e:
            DeviceContext(ALGO_BFV, 8192, P["q"], P["p"], P["t"])
        assert e.value.code == 2                                 # LSA_ERR_NO_DEVICE: no CPU fallback exists


def test_bench_tool_dry_run_prints_the_plan_counts(native):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "bench_bfv_slot_sum.py"), "--dry-run", "--shapes", "16384", "--counts", "0,100"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 4 and all(r["tool"] == "bench_bfv_slot_sum" and r["dry_run"] for r in lines)
    full = [r for r in lines if r["count"] == 8192 and r["rows"] == 1][0]["plan"]
    assert full["chain"]["key_macs"] == 14 and full["radix2"]["decompositions"] == 14 and full["radix4"]["decompositions"] == 8
