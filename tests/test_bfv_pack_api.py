"""CPU-only: the plan of the BFV coefficient packing (lsa_bfv_pack_plan, lattisense_amd/csrc/bfv_pack.h) through ctypes against its
restatement in tests/bfv_pack_model.py for every count in 1..33 and for N itself at N = 2^10 and 2^14, with and without the trace;
the refusals that need no device; the model (the composition of the numpy shift, Oracle.vec and Oracle.bfv_rotate) decrypting to
exactly the stated coefficients on the BFV_DEFAULT[8192] chain; the full expansion followed by the full pack; device.py planning
without a GPU; the bench tool's dry run."""
import ctypes
import types

import numpy as np
import pytest

from tests.bfv_expand_model import decrypt_coeffs, encrypt_coeffs, expand, levels_of
from tests.bfv_pack_model import (encrypt_constant_terms, expected_positions, factor_of, galois_elements_of, keyswitches_of, nodes_of,
                                  pack, trace_elements_of)

ENTRY_POINTS = {"lsa_bfv_pack_plan": 9, "lsa_bfv_pack_create": 5, "lsa_bfv_pack_destroy": 1, "lsa_bfv_pack_info": 9,
                "lsa_bfv_pack_galois_elements": 3, "lsa_bfv_pack_set_gather": 2, "lsa_bfv_pack": 12}


@pytest.fixture(scope="module")
def native():
    from lattisense_amd import build, _native
    build.build_native()
    return _native


def call_plan(native, n, count, trace, capacity=32):
    nl, nt, nk, cnt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    g = (ctypes.c_uint64 * max(capacity, 1))()
    rc = native.lib().lsa_bfv_pack_plan(n, count, trace, ctypes.byref(nl), ctypes.byref(nt), ctypes.byref(nk), g, capacity, ctypes.byref(cnt))
    if rc:
        return rc, native.lib().lsa_last_error().decode()
    return 0, (nl.value, nt.value, nk.value, [int(e) for e in g[: cnt.value]])


def test_binding_table_has_the_entry_points(native):
    for name, nargs in ENTRY_POINTS.items():
        assert len(native.SIGNATURES[name][1]) == nargs, name
        assert hasattr(native.lib(), name)


@pytest.mark.parametrize("trace", [0, 1])
@pytest.mark.parametrize("n", [1 << 10, 1 << 14])
def test_plan_against_the_restated_rule(native, n, trace):
    logn = n.bit_length() - 1
    for count in list(range(1, 34)) + [n]:
        rc, got = call_plan(native, n, count, trace)
        assert rc == 0, got
        k = levels_of(count)
        assert (1 << k) >= count and (k == 0 or (1 << (k - 1)) < count)
        assert got == (k, len(trace_elements_of(n, count, trace)), keyswitches_of(n, count, trace), galois_elements_of(n, count, trace)), count
        assert got[1] == (logn - k if trace else 0)
        assert got[2] == (1 << k) - 1 + got[1]
        assert got[3] == [(1 << l) + 1 for l in range(1, (logn if trace else k) + 1)]
        # every input is consumed exactly once, and input i lands on coefficient i * N / 2^k
        pos = {i: 0 for i in range(count)}
        live = set(range(count))
        for lvl, (g, s, nodes, n_pair) in enumerate(nodes_of(n, count)):
            assert (g, s, nodes) == ((2 << lvl) + 1, n >> (lvl + 1), 1 << (k - 1 - lvl))
            assert n_pair == sum(1 for a in range(nodes) if a + nodes < count) and (lvl == 0 or n_pair == nodes)
            for a in range(n_pair):
                assert a + nodes in live
                live.remove(a + nodes)
            for i in pos:
                if (i >> (k - 1 - lvl)) & 1:
                    pos[i] += s
        assert live == {0}
        assert all(pos[i] == i * (n >> k) for i in pos)
    assert call_plan(native, n, 1, 0) == (0, (0, 0, 0, []))
    assert call_plan(native, n, n, trace)[1][:3] == (logn, 0, n - 1)


def test_refusals_that_need_no_device(native):
    n = 1 << 10
    for args, needle in (((n, 0), "count"), ((n, -2), "count"), ((n, n + 1), "count"), ((1000, 4), "n_ring"), ((2, 1), "n_ring")):
        for trace in (0, 1):
            rc, msg = call_plan(native, *args, trace)
            assert rc == 1 and msg.startswith("lsa_bfv_pack") and needle in msg, (args, rc, msg)
    rc, msg = call_plan(native, n, 9, 0, capacity=3)
    assert rc == 1 and msg.startswith("lsa_bfv_pack_plan") and "capacity" in msg
    rc, msg = call_plan(native, n, 2, 1, capacity=9)
    assert rc == 1 and msg.startswith("lsa_bfv_pack_plan") and "capacity" in msg
    nl = ctypes.c_int()
    assert native.lib().lsa_bfv_pack_plan(n, 9, 0, ctypes.byref(nl), None, None, None, 0, None) == 0 and nl.value == 4
    L = native.lib()
    h = ctypes.c_void_p()
    assert L.lsa_bfv_pack_create(None, 0, 4, 0, ctypes.byref(h)) == 1 and "null context" in L.lsa_last_error().decode()
    assert L.lsa_bfv_pack_set_gather(None, 1) == 1 and L.lsa_last_error().decode().startswith("lsa_bfv_pack_set_gather")
    assert L.lsa_bfv_pack_info(None, *([None] * 8)) == 1 and L.lsa_last_error().decode().startswith("lsa_bfv_pack_info")
    assert L.lsa_bfv_pack_galois_elements(None, None, 0) == 1 and L.lsa_last_error().decode().startswith("lsa_bfv_pack_galois_elements")
    assert L.lsa_bfv_pack(None, None, None, 0, 0, None, 0, 1, 0, None, None, None) == 1
    assert L.lsa_last_error().decode().startswith("lsa_bfv_pack: null plan handle")
    L.lsa_bfv_pack_destroy(None)                                                                    # a null handle is ignored


def _rig(log_n, seed):
    from lattisense_amd import params
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    B = params.BFV_DEFAULT[8192]
    assert len(B["q"]) == 3 and len(B["p"]) == 1 and B["t"] == 65537
    o = Oracle(1 << log_n, B["q"], B["p"], B["t"])
    c = Client(o, seed=seed)
    keys = {}

    def key_of(g):
        if g not in keys:
            keys[g] = c.gen_galois_key(g, 2)
        return keys[g]
    return o, c, keys, key_of


@pytest.mark.parametrize("log_n,level,count,trace", [(10, 1, 5, 1), (10, 1, 32, 0), (11, 2, 16, 1)])
def test_model_decrypts_to_the_stated_coefficients(log_n, level, count, trace):
    """the BFV_DEFAULT[8192] chain (3 Q + 1 P, t = 65537), inputs with random coefficients everywhere: coefficient i * N/2^k of the
    result is F * (coefficient 0 of input i), F = 2^k or N; with the trace every other coefficient is 0"""
    o, c, keys, key_of = _rig(log_n, 41 + log_n)
    n, t = 1 << log_n, o.t
    rng = np.random.default_rng(41 + count)
    values = rng.integers(0, t, count)
    items = encrypt_constant_terms(c, values, level, rng)
    res, left = pack(o, key_of, 2, [ct for _, ct in items], level, trace)
    assert res.shape == (2, level + 1, n) and len(left) == count
    assert sorted(keys) == galois_elements_of(n, count, trace)
    assert factor_of(n, count, trace) == (n if trace else 1 << levels_of(count))
    got = decrypt_coeffs(c, res)
    pos, want = expected_positions(values, n, count, trace, t)
    assert np.array_equal(got[pos], want)
    if trace:
        rest = np.ones(n, dtype=bool)
        rest[pos] = False
        assert not got[rest].any()
    for i in range(max(1, 1 << max(levels_of(count) - 1, 0)), count):                               # only ever read
        assert np.array_equal(left[i], items[i][1]), i


def test_full_expansion_then_full_pack():
    """N = 2^10, level 1, count 1024: lsa_bfv_expand's model, then this one on its outputs, decrypts to 2^20 m_i at coefficient i"""
    o, c, keys, key_of = _rig(10, 77)
    n, t = 1 << 10, o.t
    rng = np.random.default_rng(77)
    m = rng.integers(0, t, n)
    outs = expand(o, key_of, 2, encrypt_coeffs(c, m, 1), 1, n)
    res, _ = pack(o, key_of, 2, outs, 1, 0)
    assert np.array_equal(decrypt_coeffs(c, res), m * pow(2, 20, t) % t)


def test_device_py_plans_without_a_gpu_and_refuses_to_run(native):
    from lattisense_amd.device import BfvPackPlan, bfv_pack_plan
    n = 1 << 12
    info = bfv_pack_plan(n, 11)
    assert (info["levels"], info["trace_levels"], info["keyswitches"]) == (4, 0, 15) and info["galois_elements"] == [3, 5, 9, 17]
    info = bfv_pack_plan(n, 11, trace=True)
    assert (info["levels"], info["trace_levels"], info["keyswitches"]) == (4, 8, 23)
    assert info["galois_elements"] == [(1 << l) + 1 for l in range(1, 13)]
    ctx = types.SimpleNamespace(n=n, h=None, stream=None)       # what a context is without a device: no handle
    plan = BfvPackPlan(ctx, 2, 6, trace=True)
    assert (plan.levels, plan.trace_levels, plan.keyswitches) == (3, 9, 7 + 9)
    with pytest.raises(native.LsaError) as e:
        plan.run(types.SimpleNamespace(ptr=None), 1, {})
    assert e.value.code == 1 and "null context" in str(e.value)
    with pytest.raises(native.LsaError) as e:
        BfvPackPlan(ctx, 2, n + 1)
    assert e.value.code == 1 and "count" in str(e.value)


def test_bench_tool_dry_run_prints_the_plan_counts(native):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "bench_bfv_pack.py"), "--dry-run", "--shapes", "4096", "--counts", "64,256"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2 and all(r["tool"] == "bench_bfv_pack" and r["dry_run"] for r in lines)
    by_count = {r["count"]: r["plan"] for r in lines}
    assert by_count[64] == {"levels": 6, "trace_levels": 0, "keyswitches": 63, "galois_elements": [(1 << l) + 1 for l in range(1, 7)]}
    assert by_count[256]["keyswitches"] == 255 and by_count[256]["levels"] == 8
