"""CPU-only: the BFV ring-t plaintext entry points are declared, exported and bound, the header's form-0 sentence names them, and
tools/bench_bfv_plain.py --dry-run prints the byte model its docstring and DESIGN.md 4.16 state."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("lsa_bfv_addsub_plain", "lsa_bfv_plain_lift", "lsa_bfv_mult_plain")


def test_entry_points_are_declared_exported_and_bound():
    from lattisense_amd import _native, build
    build.build_native()
    header = open(os.path.join(ROOT, "include", "lattisense_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(lsa_context ctx" % name, code), name
        assert name in _native.SIGNATURES and hasattr(_native.lib(), name), name
    # the same argument lists as the CKKS namesake, the plaintext stride next to the plaintext
    assert _native.SIGNATURES["lsa_bfv_addsub_plain"] == _native.SIGNATURES["lsa_ckks_addsub_plain"]
    assert len(_native.SIGNATURES["lsa_bfv_mult_plain"][1]) == 10 and len(_native.SIGNATURES["lsa_bfv_plain_lift"][1]) == 9


def test_the_form_0_sentence_of_the_encoder_names_real_entry_points():
    header = open(os.path.join(ROOT, "include", "lattisense_amd.h")).read()
    m = re.search(r"form: 0 = ring-t coefficients(.*?)\n \*\s+1 = pt_mul", header, re.S)
    assert m, "the form list of lsa_bfv_encode"
    named = re.findall(r"lsa_[a-z0-9_]+", m.group(1))
    assert set(named) == set(ENTRY_POINTS), named
    assert "entry points that lift" not in header


def test_bench_dry_run_prints_the_byte_model():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_bfv_plain.py"), "--dry-run"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    res = json.loads(out.stdout.strip().splitlines()[-1])
    from lattisense_amd import params
    L = len(params.BFV_DEFAULT[16384]["q"])
    assert (res["n"], res["q_limbs"], res["level"], res["batch"], res["dry_run"]) == (1 << 14, L, L - 1, 64, True)
    row = 8 * (1 << 14) * 64                                    # one row of N words for every item of the batch
    want = {"addsub": 4 * L + 1, "addsub_inplace": 2 * L + 1, "prescaled": 5 * L, "prescaled_inplace": 3 * L, "copy": 4 * L + 1}
    for leg, rows in want.items():
        assert res["model"][leg] == {"rows": rows, "bytes": rows * row}, leg
    assert res["model"]["addsub"]["bytes"] < res["model"]["prescaled"]["bytes"]
    assert res["model"]["addsub_inplace"]["bytes"] < res["model"]["prescaled_inplace"]["bytes"]
    assert {"mult_shared", "mult_per_item", "mult_prelifted"} <= set(res["model"])
