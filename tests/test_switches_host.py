"""CPU-only: the run-time switch table (lattisense_amd/csrc/switches.h) is the only reader of the environment in csrc/, parses
every switch as specified below, and agrees with INTEGRATION.md section 6 and with how tests/ and tools/ set switches.
tests/cpp/test_switches.cpp prints the table and every accessor's value for the variable unset, empty, "0", "1", "2", "x"."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lattisense_amd", "csrc")
INPUTS = ["unset", "empty", "0", "1", "2", "x"]
ATOI = {"empty": 0, "0": 0, "1": 1, "2": 2, "x": 0}

# the specification: kind and parse of every switch (d: the caller's default, for the switches that take one)
OFF_IF_0 = ["LSA_NTT_R16", "LSA_NTT_R8X3", "LSA_R16_PRO", "LSA_KS_FUSED", "LSA_KSMAC_XCD", "LSA_ROT_SCATTER", "LSA_HMULT_FOLD",
            "LSA_BFV_FOLD", "LSA_PTMUL_FUSED", "LSA_ROTMAC_FUSED", "LSA_LT_BLOCKED_MAC"]
ON_IF_SET = ["LSA_BC_NO_SPLIT", "LSA_BT_NO_MULTI_MAC", "LSA_MACM_NO_XCD", "LSA_NO_KEY_CACHE", "LSA_NO_PIPELINE", "LSA_TASK_TRACE",
             "LSA_NO_GRAPH_FUSION"]
OVERRIDE_BOOL = {"LSA_NTT_FP_RAW": None, "LSA_BT_DOUBLE_HOIST": None, "LSA_LT_GIANT_SCATTER": 0}   # None: the caller's default
INT = {"LSA_NTT_MU_A": lambda v, d: 0 if v == "unset" else ATOI[v],
       "LSA_KS_FUSED_ENGINES": lambda v, d: 2 if v == "unset" else ATOI[v] & 3,
       "LSA_STAGE_THREADS": lambda v, d: d if v == "unset" else max(1, ATOI[v]),
       "LSA_BT_STOP": lambda v, d: -1 if v == "unset" else ATOI[v]}
DOUBLE = {"LSA_POOL_MAX_DEV_GIB": 48, "LSA_POOL_MAX_PIN_GIB": 16, "LSA_PIPELINE_MIN_MIB": 256}
TRISTATE = ["LSA_NTT_WIDE"]
CALLER_DEFAULT = {"LSA_NTT_FP_RAW", "LSA_BT_DOUBLE_HOIST", "LSA_STAGE_THREADS", "LSA_NTT_WIDE"}
PROCESS = {"LSA_NTT_R16", "LSA_NTT_R8X3", "LSA_R16_PRO", "LSA_KS_FUSED_ENGINES", "LSA_STAGE_THREADS"}
CONTEXT = {"LSA_NTT_MU_A", "LSA_NTT_FP_RAW", "LSA_NTT_WIDE"}
PLAN = {"LSA_BC_NO_SPLIT", "LSA_BT_DOUBLE_HOIST", "LSA_NO_PIPELINE", "LSA_NO_GRAPH_FUSION", "LSA_NO_KEY_CACHE", "LSA_PIPELINE_MIN_MIB",
        "LSA_POOL_MAX_DEV_GIB", "LSA_POOL_MAX_PIN_GIB"}
NOT_SWITCHES = {"LSA_NATIVE_LIB", "LSA_EXTRA_FLAGS", "LSA_TEST_TAG", "LSA_DRY_FAIL_RANK"}


def _expected(name, v, d):
    if name in OFF_IF_0:
        return 0 if v == "0" else 1
    if name in ON_IF_SET:
        return 0 if v == "unset" else 1
    if name in OVERRIDE_BOOL:
        dflt = OVERRIDE_BOOL[name] if OVERRIDE_BOOL[name] is not None else (1 if d else 0)
        return dflt if v == "unset" else 0 if v == "0" else 1
    if name in INT:
        return INT[name](v, d)
    if name in DOUBLE:
        return DOUBLE[name] if v == "unset" else ATOI[v]
    assert name in TRISTATE
    return d if v == "unset" else {"0": 0, "1": 1}.get(v, 2)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sw") / "test_switches")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_switches.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("LSA_")}
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    rows, vals, cached = {}, {}, {}
    for line in out.stdout.splitlines():
        f = line.split()
        if f[0] == "ROW":
            assert f[1] not in rows, "a switch is in the table twice: " + f[1]
            rows[f[1]] = (f[2], f[3])
        elif f[0] == "VAL":
            vals[(f[1], f[2], f[3])] = float(f[4])
        elif f[0] == "CACHED":
            cached.setdefault(f[1], []).append(int(f[2]))
    md = subprocess.run([exe, "--markdown"], capture_output=True, text=True, timeout=60, env=env).stdout
    return {"rows": rows, "vals": vals, "cached": cached, "markdown": md}


def test_every_switch_parses_as_specified(table):
    kinds = {"OFF_IF_0": set(OFF_IF_0), "ON_IF_SET": set(ON_IF_SET), "OVERRIDE_BOOL": set(OVERRIDE_BOOL), "INT": set(INT),
             "DOUBLE": set(DOUBLE), "TRISTATE": set(TRISTATE)}
    names = set().union(*kinds.values())
    assert set(table["rows"]) == names
    for name, (kind, life) in table["rows"].items():
        assert name in kinds[kind], (name, kind)
        assert life == ("PROCESS" if name in PROCESS else "CONTEXT" if name in CONTEXT else "PLAN" if name in PLAN else "CALL"), name
        for d in (("0", "5") if name in CALLER_DEFAULT else ("-",)):
            for v in INPUTS:
                assert table["vals"][(name, d, v)] == _expected(name, v, int(d) if d != "-" else None), (name, d, v)
    assert len(table["vals"]) == sum(12 if n in CALLER_DEFAULT else 6 for n in names)
    # a PROCESS accessor keeps its first value; every other row above was read through setenv + the accessor, so it is not cached
    assert set(table["cached"]) == PROCESS and all(all(v) for v in table["cached"].values())


def test_switches_h_is_the_only_reader():
    macros = set(re.findall(r"LSA_[A-Z0-9_]+", open(os.path.join(CSRC, "build_flags.h")).read()))
    names = set(OFF_IF_0) | set(ON_IF_SET) | set(OVERRIDE_BOOL) | set(INT) | set(DOUBLE) | set(TRISTATE)
    files = [f for f in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(f) and os.path.basename(f) != "switches.h"
             and not f.endswith(".so")]
    assert len(files) > 20
    for f in files:
        text = open(f, errors="replace").read()
        assert "getenv" not in text, f
        for lit in re.findall(r'"(LSA_[A-Z0-9_]+)"', text):
            assert lit in names or lit in macros, (f, lit)
    assert "getenv" in open(os.path.join(CSRC, "switches.h")).read()


def test_integration_md_shows_the_table(table):
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^## 6\. Runtime switches \(environment\)\n(.*?)(?=^## )", doc, re.S | re.M)
    assert m, "INTEGRATION.md section 6 not found"
    got = re.findall(r"^\| `(LSA_[A-Z0-9_]+)` \| (\w+) \|", m.group(1), re.M)
    assert got == [(n, life) for n, (_, life) in table["rows"].items()]      # the table's names, order and lifetimes, each once
    for line in table["markdown"].splitlines():                                # and its text
        assert line in m.group(1), line


def test_tests_and_tools_set_only_table_switches():
    names = set(OFF_IF_0) | set(ON_IF_SET) | set(OVERRIDE_BOOL) | set(INT) | set(DOUBLE) | set(TRISTATE)
    macros = set(re.findall(r"LSA_[A-Z0-9_]+", open(os.path.join(CSRC, "build_flags.h")).read()))   # -D names: compiler flags
    files = glob.glob(os.path.join(ROOT, "tests", "*.py")) + [f for f in glob.glob(os.path.join(ROOT, "tools", "*")) if os.path.isfile(f)]
    me = os.path.abspath(__file__)
    n = "(LSA_[A-Z0-9_]+)"
    puts = [r"environ\[\s*[\"']%s[\"']\s*\]\s*=(?!=)" % n, r"(?:setenv|setdefault)\(\s*[\"']%s[\"']" % n, r"(?<!-D)\b%s=(?!=)" % n,
            r"[\"']%s[\"']\s*:" % n]
    # in-process forms: os.environ[...] =, monkeypatch.setenv, gpu_util.env(...), a {"NAME": value} dict fed to one of them
    in_process = [puts[0], puts[1], r"\benv\([^)\n]*\b%s=" % n, puts[3]]
    seen = set()
    for f in files:
        if os.path.abspath(f) == me:
            continue
        text = open(f, errors="replace").read()
        for pat in puts:
            for name in re.findall(pat, text):
                assert name in names or name in NOT_SWITCHES or name in macros, (f, name)
                seen.add(name)
        if f.endswith(".py"):
            for pat in in_process:
                for name in re.findall(pat, text):
                    assert name not in PROCESS, "%s sets the per-process switch %s in process: it would test nothing" % (f, name)
    assert {"LSA_KS_FUSED", "LSA_KS_FUSED_ENGINES", "LSA_NTT_R16", "LSA_NO_GRAPH_FUSION"} <= seen   # the scan finds each form


# switches the rule below asks a GPU parity test for, and that have none: each with its reason
PARITY_EXEMPT = {
    "LSA_STAGE_THREADS": "host threads that stage task inputs and outputs: no device code path depends on it; its parse is held above",
}


def test_every_path_selecting_switch_is_named_by_a_gpu_parity_test(table):
    """A switch whose lifetime is PROCESS or CONTEXT, or whose text starts with "A/B", selects device code that the default never
    runs: it is named in at least one tests/test_gpu_*.py (which hold every form to the oracle), or exempt above with a reason.
    A new switch cannot arrive without one or the other.  (LSA_TASK_TRACE, the pool caps and LSA_PIPELINE_MIN_MIB fall outside
    the rule: CALL / PLAN lifetime, not A/B -- they print, or bound what is kept, and select no kernel.)"""
    text = {}
    for line in table["markdown"].splitlines():
        m = re.match(r"^\| `(LSA_[A-Z0-9_]+)` \| (\w+) \| (.*) \|$", line)
        if m:
            text[m.group(1)] = m.group(3)
    assert set(text) == set(table["rows"])
    gpu = {f: open(f).read() for f in glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py"))}
    assert len(gpu) > 15
    assert set(PARITY_EXEMPT) <= set(text) and all(len(r) > 10 for r in PARITY_EXEMPT.values())
    required = [n for n, (_, life) in table["rows"].items() if life in ("PROCESS", "CONTEXT") or text[n].startswith("A/B")]
    assert {"LSA_NTT_R16", "LSA_NTT_R8X3", "LSA_R16_PRO", "LSA_NTT_MU_A", "LSA_NTT_FP_RAW", "LSA_KS_FUSED", "LSA_MACM_NO_XCD"} <= set(required)
    for name in required:
        if name in PARITY_EXEMPT:
            continue
        users = [os.path.basename(f) for f, t in gpu.items() if re.search(r"\b%s\b" % name, t)]
        assert users, "%s selects a device path and no tests/test_gpu_*.py names it" % name
    assert set(PARITY_EXEMPT) <= set(required)          # no exemption for a switch the rule does not ask about


def test_first_pass_override_rule_of_make_ntt_plan(tmp_path):
    """the rule tests/test_gpu_ntt_switches.py::accepted_mu_a states, against ntt_plan.h itself: which LSA_NTT_MU_A values change
    the plan at N = 2^13 .. 2^17, and what the default is"""
    src = tmp_path / "plan.cpp"
    src.write_text('#include <cstdio>\n#define LSA_EMULATE 1\n#include "ntt_plan.h"\nint main() { for (int n = 13; n <= 17; n++) for (int m = 0; m <= 16; m++) {'
                   ' NttPlan p = make_ntt_plan(n, 12, m); std::printf("%d %d %d %d %d\\n", n, m, p.npass, p.pass[0].mu, p.pass[1].mu); } }\n')
    exe = str(tmp_path / "plan")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", CSRC, str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout
    from tests.test_gpu_ntt_switches import TAU, accepted_mu_a
    assert TAU == 12
    rows = [tuple(int(x) for x in line.split()) for line in out.splitlines()]
    assert len(rows) == 5 * 17
    for n, m, npass, mu_a, mu_b in rows:
        default = min(n // 2, TAU - 4)
        assert npass == 2 and mu_a + mu_b == n
        assert mu_a == (m if m in accepted_mu_a(n) else default), (n, m)
