"""CKKS plaintext and constant operands, the part that needs no GPU: the seven entry points exist, are bound and declared with the
signatures of the header, the DeviceContext methods have the documented parameter lists, every entry point fails with
LSA_ERR_NO_DEVICE where there is no device (and with LSA_ERR_ARG for the null context where there is one), and the benchmark
tool's dry run prints the limb-stream model."""
import ctypes
import inspect
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the C parameter types of the header, in order
ENTRY_POINTS = {
    "lsa_ckks_encode": "lsa_context int int const double* double uint64_t* long long int void*",
    "lsa_ckks_mult_plain": "lsa_context int const uint64_t* long long const uint64_t* long long uint64_t* long long int int void*",
    "lsa_ckks_addsub_plain": "lsa_context int int const uint64_t* long long const uint64_t* long long uint64_t* long long int void*",
    "lsa_ckks_mac_plain": "lsa_context int int const uint64_t* const* const long long* const uint64_t* const* const long long* "
                          "const uint64_t* long long uint64_t* long long int int void*",
    "lsa_ckks_mult_const": "lsa_context int const uint64_t* long long double double double uint64_t* long long int int void*",
    "lsa_ckks_add_const": "lsa_context int const uint64_t* long long double double double uint64_t* long long int void*",
    "lsa_ckks_affine_const": "lsa_context int const uint64_t* long long double double double double double double uint64_t* long long "
                             "int int void*",
}
CTYPES_OF = {"lsa_context": ctypes.c_void_p, "int": ctypes.c_int, "double": ctypes.c_double, "long long": ctypes.c_longlong,
             "void*": ctypes.c_void_p, "uint64_t*": ctypes.c_void_p, "const uint64_t*": ctypes.c_void_p,
             "const double*": ctypes.POINTER(ctypes.c_double), "const uint64_t* const*": ctypes.POINTER(ctypes.c_void_p),
             "const long long*": ctypes.POINTER(ctypes.c_longlong)}
TYPE_RE = re.compile(r"const uint64_t\* const\*|const uint64_t\*|const long long\*|const double\*|uint64_t\*|void\*|long long|lsa_context|"
                     r"double|int")


@pytest.fixture(scope="module")
def native():
    from lattisense_amd import build, _native
    build.build_native()
    return _native


def _header_types(name):
    header = open(os.path.join(ROOT, "include", "lattisense_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, "%s is not declared in the header" % name
    out = []
    for param in m.group(1).split(","):
        param = " ".join(param.split())
        t = re.sub(r"\s*\b[A-Za-z_][A-Za-z_0-9]*$", "", param)           # drop the parameter's name
        out.append(t.replace(" *", "*"))
    return out


def test_entry_points_are_exported_bound_and_declared(native):
    L = native.lib()
    for name, spec in ENTRY_POINTS.items():
        want = TYPE_RE.findall(spec)
        assert " ".join(want) == spec, name
        assert hasattr(L, name), name
        assert _header_types(name) == want, (name, _header_types(name))
        res, args = native.SIGNATURES[name]
        assert res is ctypes.c_int and list(args) == [CTYPES_OF[t] for t in want], name


def test_python_methods():
    from lattisense_amd import device
    D = device.DeviceContext
    want = {"ckks_encode": ["level", "values", "scale", "batch", "out"],
            "ckks_mult_plain": ["level", "ct", "pt", "batch", "rescale", "out", "spt"],
            "ckks_addsub_plain": ["op", "level", "ct", "pt", "batch", "out", "spt"],
            "ckks_mac_plain": ["level", "cts", "pts", "batch", "rescale", "addend", "out", "spts"],
            "ckks_mult_const": ["level", "ct", "value", "const_scale", "batch", "rescale", "out"],
            "ckks_add_const": ["level", "ct", "value", "ct_scale", "batch", "out"],
            "ckks_affine_const": ["level", "ct", "alpha", "const_scale", "beta", "ct_scale", "batch", "rescale", "out"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(D, name))
        assert list(sig.parameters)[1:] == params, name
        assert sig.parameters["out"].default is None
        if "rescale" in params:
            assert sig.parameters["rescale"].default is False


def test_every_entry_point_reports_the_missing_device(native):
    """No context can exist without a device, so the call a program without one can make is the one with a null context: it must say
    LSA_ERR_NO_DEVICE (2), not compute and not crash.  On a box with a device the same call is the argument error it is (1)."""
    import torch
    L = native.lib()
    want = 1 if torch.cuda.is_available() else 2
    for name in ENTRY_POINTS:
        _, args = native.SIGNATURES[name]
        zero = [a() if a in (ctypes.c_int, ctypes.c_double, ctypes.c_longlong) else None for a in args]
        rc = getattr(L, name)(*zero)
        msg = L.lsa_last_error().decode()
        assert rc == want, (name, rc, msg)
        assert msg.startswith(name + ": "), (name, msg)
        if want == 2:
            assert "no HIP device" in msg, msg


def test_launch_bound_of_the_tool_is_the_header_s():
    text = open(os.path.join(ROOT, "lattisense_amd", "csrc", "lsa_internal.h")).read()
    m = re.search(r"#define LSA_MAC_MAX_TERMS (\d+)", text)
    assert m
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import bench_ckks_plain
    finally:
        sys.path.pop(0)
    assert bench_ckks_plain.MAC_MAX_TERMS == int(m.group(1))


def test_bench_tool_dry_run():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_ckks_plain.py"), "--dry-run"], capture_output=True,
                         text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["dry_run"] is True and r["n"] == 65536 and r["level"] == 12 and "ms_per_call" not in r
    m = r["streams_per_ct"]
    L = 13
    # one read and one write per row for a constant, two reads and one write through k_mac_plain
    assert m["mult_const"] == 4 * L and m["mult_plain"] == 6 * L and m["affine_const"] == 4 * L
    assert m["mult_const_then_add_const"] == 6 * L and m["add_const_in_place"] == 2 * L
    assert m["predicted_mult_plain_over_mult_const"] == 1.5 and m["predicted_two_calls_over_affine"] == 1.5
    assert m["encode_upload_words_per_n"] == 1 and m["rows_upload_words_per_n"] == L
    # a 17th term costs its own rows and one more accumulating launch (the sum so far read and written again)
    assert m["mac_plain"]["17"] - m["mac_plain"]["16"] == 4 * L + 4 * L
