"""CPU-only: the BFV plaintext matrix x ciphertext vector product's public surface -- the three entry points exported, bound and declared,
DeviceContext.bfv_matvec_plain_mul, the bench tool's dry run -- lsa_bfv_matvec_plan through ctypes against its restatement in
tests/bfv_matvec_model.py over a grid of (rows, cols, batch, workspace), the refusals that need no device, and the model decrypting: at
N = 2^11 on the BFV_DEFAULT[8192] chain a query for column `col` is expanded (tests/bfv_expand_model.py), multiplied with a 4 x 8
database of polynomials and the row picked by an encrypted index (tests/rgsw_model.py): the result decrypts to entry [row][col]."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.bfv_expand_model import decrypt_coeffs, encrypt_coeffs, expand, prescale
from tests.bfv_matvec_model import descale, matvec_ntt, plan_of, pt_mul_of, transform
from tests.rgsw_model import constant, levels_of, rgsw_encrypt, select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"lsa_bfv_matvec_plain_mul": 19, "lsa_bfv_matvec_plan": 10, "lsa_set_bfv_matvec_block": 3}
PAIRS = ((0, 0), (3, 7), (2, 5))     # (row, col) of the decryption tests, CPU and GPU


@pytest.fixture(scope="module")
def native():
    from lattisense_amd import build, _native
    build.build_native()
    return _native


def call_plan(native, n, limbs, rows, cols, batch, space):
    rb, cb, nl, wr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    rc = native.lib().lsa_bfv_matvec_plan(n, limbs, rows, cols, batch, space, ctypes.byref(rb), ctypes.byref(cb), ctypes.byref(nl),
                                          ctypes.byref(wr))
    if rc:
        return rc, native.lib().lsa_last_error().decode()
    return 0, (rb.value, cb.value, nl.value, wr.value)


def test_entry_points_exported_bound_and_declared(native):
    header = open(os.path.join(ROOT, "include", "lattisense_amd.h")).read()
    for name, nargs in ENTRY_POINTS.items():
        assert len(native.SIGNATURES[name][1]) == nargs, name
        assert hasattr(native.lib(), name)
        decl = re.search(r"\bint %s\(([^;]*?)\);" % name, header, re.S)
        assert decl is not None, name
        assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == nargs, name
    from lattisense_amd.device import DeviceContext
    assert callable(DeviceContext.bfv_matvec_plain_mul) and callable(DeviceContext.set_bfv_matvec_block)


def test_plan_over_a_grid(native):
    n, limbs = 2048, 3
    col = 2 * limbs * n * 8
    for rows in (1, 2, 3, 4, 5, 8, 9, 40):
        for cols in (1, 3, 8, 9, 17, 64):
            for batch in (1, 3, 16):
                for space in (col, 4 * col, 17 * col + 8, 100 * col, 8 << 30):
                    rc, got = call_plan(native, n, limbs, rows, cols, batch, space)
                    assert rc == 0, got
                    rb, cb, nl, wr = got
                    assert got == plan_of(n, limbs, rows, cols, batch, space), (rows, cols, batch, space)
                    # the column blocks cover the columns exactly once; a tile's columns fit; the row blocks cover the rows
                    blocks = [(j * cb, min(cb, cols - j * cb)) for j in range(-(-cols // cb))]
                    assert sum(c for _, c in blocks) == cols and all(c >= 1 for _, c in blocks) and blocks[-1][0] + blocks[-1][1] == cols
                    assert cb * col <= space and wr == cb * 2 * limbs
                    assert rb in (1, 2) and (rb == 1 or rows >= 2) and -(-rows // rb) * rb >= rows
                    tile = min(batch, (space // col) // cb)
                    assert nl == -(-batch // tile) * len(blocks)
    assert call_plan(native, 16384, 6, 1024, 256, 16, 8 << 30) == (0, (2, 256, 1, 256 * 12))
    assert native.lib().lsa_bfv_matvec_plan(2048, 3, 4, 4, 1, 8 << 30, None, None, None, None) == 0


def test_refusals_that_need_no_device(native):
    col = 2 * 3 * 2048 * 8
    for args, needle in (((2048, 3, 4, 4, 1, col - 8), "workspace"), ((2048, 3, 4, 4, 1, 0), "workspace"), ((2048, 3, 0, 4, 1, col), "rows"),
                         ((2048, 3, 4, 0, 1, col), "cols"), ((2048, 3, 4, 4, 0, col), "batch"), ((256, 3, 4, 4, 1, col), "n_ring"),
                         ((2048, 0, 4, 4, 1, col), "level_limbs")):
        rc, msg = call_plan(native, *args)
        assert rc == 1 and msg.startswith("lsa_bfv_matvec") and needle in msg, (args, rc, msg)
    L = native.lib()
    assert L.lsa_bfv_matvec_plain_mul(None, 0, 1, 1, None, 0, 0, None, 0, 0, 0, None, 0, 0, None, 0, 0, 1, None) == 1
    assert "null context" in L.lsa_last_error().decode()
    assert L.lsa_set_bfv_matvec_block(None, 0, 0) == 1


def test_device_py_plans_without_a_gpu(native):
    from lattisense_amd.device import bfv_matvec_plan
    assert bfv_matvec_plan(4096, 2, 64, 64, 16) == {"row_block": 2, "col_block": 64, "launches": 1, "workspace_rows": 256}
    assert bfv_matvec_plan(2048, 3, 9, 17, 1, workspace_bytes=4 * 2 * 3 * 2048 * 8)["launches"] == 5
    with pytest.raises(native.LsaError) as e:
        bfv_matvec_plan(2048, 3, 0, 4, 1)
    assert e.value.code == 1 and "rows" in str(e.value)


def test_bench_tool_dry_run_prints_shapes_and_accounting(native):
    import json
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_bfv_matvec.py"), "--dry-run", "--shapes", "4096", "--matrices",
                          "64x64,1024x256", "--batches", "16", "--max-db-gib", "8"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2 and all(r["tool"] == "bench_bfv_matvec" and r["dry_run"] for r in lines)
    assert lines[0]["plan"] == {"row_block": 2, "col_block": 64, "launches": 1, "workspace_rows": 256}
    assert lines[0]["database_bytes"] == 64 * 64 * 2 * 4096 * 8 and not lines[0]["dropped"] and lines[1]["dropped"]
    assert lines[0]["operator_rows"] < lines[0]["composition_rows"]


def _noise_bits(client, ct, want):
    """log2 of the largest |phase - Delta * want| of a ciphertext that should hold `want` (coefficients mod t), and log2(Delta / 2)"""
    ph, Q = client._phase_bigint(np.asarray(ct), ntt_domain=False)
    t = client.o.t
    delta = Q // t
    err = 0
    for v, m in zip(ph, want):
        d = (v - delta * int(m)) % Q
        d = min(d, Q - d)
        e = (v - delta * (int(m) - t)) % Q                                   # the message may sit at m or m - t
        err = max(err, min(d, min(e, Q - e)))
    return max(err, 1).bit_length(), (delta // 2).bit_length()


def pir_database(rng, t, n, rows, cols):
    """[rows][cols][N] polynomials with coefficients in [0, t)"""
    return rng.integers(0, t, size=(rows, cols, n))


def pir_query(client, n, t, level, cols, col):
    """a ciphertext of X^col * 2^-k: its expansion to `cols` outputs holds the constant 1 at output `col` and 0 elsewhere"""
    m = np.zeros(n, dtype=np.int64)
    m[col] = 1
    return encrypt_coeffs(client, prescale(m, cols, t), level)


def test_expand_matvec_select_decrypts_to_the_database_entry():
    """N = 2^11, BFV_DEFAULT[8192] (3 Q + 1 P), level 2, rows = 4, cols = 8: the models chained; the error is asserted against Delta / 2.
    A product with a database polynomial multiplies the error by at most N * t (2^11 * 2^17), summed over 8 columns: 2^31 on top of
    the expansion's, against Delta / 2 near 2^146."""
    from lattisense_amd import params
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    B = params.BFV_DEFAULT[8192]
    n, lvl, rows, cols = 1 << 11, 2, 4, 8
    o = Oracle(n, B["q"], B["p"], B["t"])
    c = Client(o, seed=29)
    t, L = o.t, lvl + 1
    rng = np.random.default_rng(29)
    db = pir_database(rng, t, n, rows, cols)
    ptd = descale(o, L, np.stack([np.stack([pt_mul_of(o, L, db[r, k]) for k in range(cols)]) for r in range(rows)]))
    keys = {}
    key_of = lambda g: keys.setdefault(g, c.gen_galois_key(g, lvl))
    bits = {b: rgsw_encrypt(c, constant(n, b), lvl) for b in (0, 1)}
    for row, col in PAIRS:
        query = expand(o, key_of, lvl, pir_query(c, n, t, lvl, cols, col), lvl, cols)
        scanned = matvec_ntt(o, L, transform(o, L, query), ptd)
        res, _ = select(o, lvl, scanned, [bits[(row >> j) & 1] for j in range(levels_of(rows))], lvl)
        assert np.array_equal(decrypt_coeffs(c, res), db[row, col]), (row, col)
        for r in range(rows):                                                # every scanned row holds its own entry of the column
            assert np.array_equal(decrypt_coeffs(c, scanned[r]), db[r, col]), (r, col)
        err, room = _noise_bits(c, res, db[row, col])
        assert err + 20 < room, (row, col, err, room)
