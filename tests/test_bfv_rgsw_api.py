"""CPU-only: the plan of the BFV select-by-index operator (lsa_bfv_select_plan, lattisense_amd/csrc/bfv_select.h) through ctypes
against its restatement in tests/rgsw_model.py for every count in 1..33; the refusals that need no device; the model (Oracle.gadget_product
twice, Oracle.vec add, one Oracle.moddown) decrypting exactly: RGSW(X^5) [.] ct against the monomial shift, the CMux with R(0) and R(1),
select trees of depth 4 and of a count that is no power of two for every index, depth 2 on the BFV_DEFAULT[16384] chain; device.py
planning without a GPU; the bench tool's dry run."""
import ctypes
import types

import numpy as np
import pytest

from tests.bfv_expand_model import decrypt_coeffs, encrypt_coeffs, mul_monomial
from tests.rgsw_model import (cmux, constant, external_product, first_unchanged, levels_of, monomial, pairs_of, products_of, rgsw_encrypt,
                              select)

ENTRY_POINTS = {"lsa_set_rgsw_pair_mac": 2, "lsa_bfv_external_product": 12, "lsa_bfv_cmux": 12, "lsa_bfv_select_plan": 3,
                "lsa_bfv_select_create": 4, "lsa_bfv_select_destroy": 1, "lsa_bfv_select_info": 5, "lsa_bfv_select": 12}


@pytest.fixture(scope="module")
def native():
    from lattisense_amd import build, _native
    build.build_native()
    return _native


def call_plan(native, count):
    nl, npr = ctypes.c_int(), ctypes.c_int()
    rc = native.lib().lsa_bfv_select_plan(count, ctypes.byref(nl), ctypes.byref(npr))
    if rc:
        return rc, native.lib().lsa_last_error().decode()
    return 0, (nl.value, npr.value)


def test_binding_table_has_the_entry_points(native):
    for name, nargs in ENTRY_POINTS.items():
        assert len(native.SIGNATURES[name][1]) == nargs, name
        assert hasattr(native.lib(), name)


def test_plan_for_count_1_to_33(native):
    for count in range(1, 34):
        rc, got = call_plan(native, count)
        assert rc == 0, got
        k = levels_of(count)
        assert (1 << k) >= count and (k == 0 or (1 << (k - 1)) < count)
        assert got == (k, count - 1) and products_of(count) == count - 1, count
        # every index below count reaches node 0: bit j set takes the partner, which exists because idx < count
        for idx in range(count):
            node = idx
            for j, half, n_pair in pairs_of(count):
                assert node < 2 * half
                if node >= half:
                    assert node - half < n_pair, (count, idx, j)
                    node -= half
            assert node == 0
        for j, half, n_pair in pairs_of(count):
            assert n_pair == sum(1 for a in range(half) if a + half < count) and (j == k - 1 or n_pair == half)
    assert call_plan(native, 1) == (0, (0, 0))


def test_refusals_that_need_no_device(native):
    for count in (0, -3, (1 << 20) + 1):
        rc, msg = call_plan(native, count)
        assert rc == 1 and msg.startswith("lsa_bfv_select") and "count" in msg, (count, rc, msg)
    L = native.lib()
    assert L.lsa_bfv_select_plan(9, None, None) == 0
    h = ctypes.c_void_p()
    assert L.lsa_bfv_select_create(None, 0, 4, ctypes.byref(h)) == 1 and "null context" in L.lsa_last_error().decode()
    assert L.lsa_bfv_select_info(None, None, None, None, None) == 1 and L.lsa_last_error().decode().startswith("lsa_bfv_select_info")
    assert L.lsa_bfv_select(None, None, None, 0, 0, None, 0, 1, 0, None, None, None) == 1
    assert L.lsa_last_error().decode().startswith("lsa_bfv_select: null plan handle")
    assert L.lsa_bfv_external_product(None, 0, None, 0, None, None, None, 0, None, 0, 1, None) == 1
    assert L.lsa_bfv_cmux(None, 0, None, 0, None, 0, None, None, None, 0, 1, None) == 1
    assert L.lsa_set_rgsw_pair_mac(None, 0) == 1
    L.lsa_bfv_select_destroy(None)                                                                  # a null handle is ignored


def _rig(log_n, chain, seed):
    from lattisense_amd import params
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    B = params.BFV_DEFAULT[chain]
    o = Oracle(1 << log_n, B["q"], B["p"], B["t"])
    return o, Client(o, seed=seed)


def _noise_bits(client, ct, want):
    """log2 of the largest |phase - Delta * want| of a ciphertext that should hold `want` (coefficients mod t), and log2(Delta / 2)"""
    ph, Q = client._phase_bigint(np.asarray(ct), ntt_domain=False)
    t = client.o.t
    delta = Q // t
    err = 0
    for v, m in zip(ph, want):
        d = (v - delta * int(m)) % Q
        d = min(d, Q - d)
        # the message may sit at m or m - t: Delta * t = Q - (Q mod t)
        e = (v - delta * (int(m) - t)) % Q
        err = max(err, min(d, min(e, Q - e)))
    return max(err, 1).bit_length(), (delta // 2).bit_length()


def test_external_product_by_a_monomial_is_the_shift():
    """N = 2^11, BFV_DEFAULT[8192], level 2: RGSW(X^5) [.] ct decrypts to the coefficients of mul_monomial(ct, 5), with the error far
    below Delta / 2; a base is added on top"""
    o, c = _rig(11, 8192, 5)
    n, t, lvl = 1 << 11, o.t, 2
    rng = np.random.default_rng(5)
    m = rng.integers(0, t, n)
    ct = encrypt_coeffs(c, m, lvl)
    R = rgsw_encrypt(c, monomial(n, 5), lvl)
    res = external_product(o, lvl, ct, R, lvl)
    want = decrypt_coeffs(c, mul_monomial(o, ct, 5))
    assert np.array_equal(decrypt_coeffs(c, res), want)
    shifted = np.roll(m, 5)
    shifted[:5] = (-shifted[:5]) % t
    assert np.array_equal(want, shifted)
    err, room = _noise_bits(c, res, want)
    assert err <= 12 and room > 90, (err, room)                             # the error below 2^12, Delta / 2 above 2^90
    m2 = rng.integers(0, t, n)
    res2 = external_product(o, lvl, ct, R, lvl, base=encrypt_coeffs(c, m2, lvl))
    assert np.array_equal(decrypt_coeffs(c, res2), (want + m2) % t)


def test_cmux_takes_c1_under_one_and_c0_under_zero():
    o, c = _rig(11, 8192, 6)
    n, t, lvl = 1 << 11, o.t, 2
    rng = np.random.default_rng(6)
    m0, m1 = rng.integers(0, t, n), rng.integers(0, t, n)
    c0, c1 = encrypt_coeffs(c, m0, lvl), encrypt_coeffs(c, m1, lvl)
    for bit, want in ((0, m0), (1, m1)):
        res = cmux(o, lvl, c0, c1, rgsw_encrypt(c, constant(n, bit), lvl), lvl)
        assert np.array_equal(decrypt_coeffs(c, res), want), bit


@pytest.mark.parametrize("log_n,chain,level,count,indices", [(11, 8192, 2, 16, (0, 7, 15)), (11, 8192, 2, 5, (0, 1, 2, 3, 4)),
                                                             (12, 16384, 3, 4, (2,))])
def test_select_decrypts_to_the_indexed_input(log_n, chain, level, count, indices):
    """a depth-4 tree, a count that is no power of two with every valid index, depth 2 on the 6 Q + 2 P chain at level 3"""
    o, c = _rig(log_n, chain, 40 + count)
    n, t = 1 << log_n, o.t
    klvl = level
    rng = np.random.default_rng(40 + count)
    ms = [rng.integers(0, t, n) for _ in range(count)]
    cts = np.stack([encrypt_coeffs(c, m, level) for m in ms])
    k = levels_of(count)
    bits = {b: rgsw_encrypt(c, constant(n, b), klvl) for b in (0, 1)}
    for idx in indices:
        res, left = select(o, level, cts, [bits[(idx >> j) & 1] for j in range(k)], klvl)
        assert np.array_equal(decrypt_coeffs(c, res), ms[idx]), (count, idx)
        err, room = _noise_bits(c, res, ms[idx])
        assert err + 20 < room, (err, room)
        lo = first_unchanged(count)
        assert np.array_equal(left[lo:], cts[lo:])


def test_device_py_plans_without_a_gpu_and_refuses_to_run(native):
    from lattisense_amd.device import BfvSelectPlan, bfv_select_plan
    assert bfv_select_plan(11) == {"levels": 4, "products": 10}
    assert bfv_select_plan(1) == {"levels": 0, "products": 0}
    ctx = types.SimpleNamespace(n=1 << 12, h=None, stream=None)       # what a context is without a device: no handle
    plan = BfvSelectPlan(ctx, 2, 6)
    assert (plan.levels, plan.products) == (3, 5)
    with pytest.raises(native.LsaError) as e:
        plan.run(types.SimpleNamespace(ptr=None), 1, [])
    assert e.value.code == 1 and "null context" in str(e.value)
    with pytest.raises(native.LsaError) as e:
        BfvSelectPlan(ctx, 2, 0)
    assert e.value.code == 1 and "count" in str(e.value)


def test_bench_tool_dry_run_prints_the_plan_counts(native):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "bench_bfv_rgsw.py"), "--dry-run", "--shapes", "4096", "--counts", "64"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and all(r["tool"] == "bench_bfv_rgsw" and r["dry_run"] for r in lines)
    assert lines[0]["count"] == 64 and lines[0]["plan"] == {"levels": 6, "products": 63}
