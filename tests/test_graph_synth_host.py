"""CPU-side checks of the hand-built task graphs (tests/graph_synth.py, tests/graph_edge_cases.py); no device.

(a) the builder writes what the frontend writes: three committed fixtures are rebuilt call by call and compared field for
    field (the frontend's random node names aside);
(b) every case of the table loads with the load-time rewrites on and with LSA_NO_GRAPH_FUSION=1, and the difference of the
    data / compute counts is the delta the table derives by hand from the rewrite rules (zero where a rule must not fire).
"""
import json
import os

import pytest

from tests.graph_edge_cases import CASES
from tests.graph_synth import Graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASKS = os.path.join(ROOT, "tests", "golden", "tasks")


@pytest.fixture(scope="module")
def native():
    from lattisense_amd import build, _native
    build.build_native()
    return _native


# ---------------------------------------------------------------------------------------------------- (a) fixtures, rebuilt
def _ckks_n4096_cmc_relin_rescale():
    g = Graph("CKKS")
    for i in range(4):
        g.ct(4, id="x_%d" % i, index=i)
    for i in range(4):
        g.ct(4, id="y_%d" % i, index=4 + i)
    k = g.rlk(4, index=10)
    for i, (im, ir, iz) in enumerate(((9, 12, 14), (16, 18, 20), (22, 24, 26), (28, 30, 32))):
        m = g.mult(i, 4 + i, index=im)
        r = g.relin(m, k, index=ir)
        g.output(g.rescale(r, index=iz, id="z_%d" % i))
    return g


def _bfv_n4096_rotmac_row_partial():
    g = Graph("BFV")
    x, y = g.ct(2, id="x", index=0), g.ct(2, id="y", index=1)
    row, col = g.glk(8191, 2, index=2), g.glk(3125, 2, index=5)
    p0, p1 = g.pt_mul(2, id="p_0", index=8), g.pt_mul(2, id="p_1", index=9)
    g.set_inputs([x, y, p0, p1, row, col])
    r = g.rotate_row(x, row, index=4)
    c = g.rotate_col(x, col, index=7)
    assert g.compute[1]["step"] == 5   # 3125 = 5^5
    g.output(g.cmpac_sum([r, c], y, [p0, p1], index=11))
    return g


def _bfv_n4096_cmp_ringt():
    g = Graph("BFV")
    for i in range(4):
        g.ct(2, id="x_%d" % i, index=i)
    for i in range(4):
        g.pt_ringt(id="y_%d" % i, index=4 + i)
    for i in range(4):
        g.output(g.mult(i, 4 + i, index=9 + 2 * i, id="z_%d" % i))
    return g


REBUILT = {"ckks_n4096_cmc_relin_rescale": _ckks_n4096_cmc_relin_rescale,
           "bfv_n4096_rotmac_row_partial": _bfv_n4096_rotmac_row_partial,
           "bfv_n4096_cmp_ringt": _bfv_n4096_cmp_ringt}


def _without_random_names(g):
    """the graph with every compute node's name, and every datum's name that some compute node produces and the task does not
    return, blanked: those are the frontend's random 12-letter ids"""
    g = json.loads(json.dumps(g))
    made = {o for c in g["compute"].values() for o in c["outputs"]} - set(g["outputs"])
    for c in g["compute"].values():
        c["id"] = ""
    for k, d in g["data"].items():
        if int(k) in made:
            d["id"] = ""
    return g


@pytest.mark.parametrize("name", sorted(REBUILT))
def test_builder_reproduces_fixture(name, tmp_path):
    want = json.load(open(os.path.join(TASKS, name, "mega_ag.json")))
    path = REBUILT[name]().write(tmp_path / name)
    got = json.load(open(os.path.join(path, "mega_ag.json")))
    assert sorted(os.listdir(path)) == ["mega_ag.json"]
    want_n, got_n = _without_random_names(want), _without_random_names(got)
    if name == "bfv_n4096_rotmac_row_partial":   # its only output carries a random name too
        for gr in (want_n, got_n):
            gr["data"]["11"]["id"] = ""
    assert set(got_n) == set(want_n)
    for key in want_n:
        assert got_n[key] == want_n[key], key
    # the names that are blanked above are names all the same: 12 lower-case letters, no two alike
    names = [c["id"] for c in got["compute"].values()]
    assert all(len(s) == 12 and s.isalpha() and s.islower() for s in names) and len(set(names)) == len(names)


def test_builder_refuses_an_index_used_twice():
    g = Graph("CKKS")
    g.ct(2, index=3)
    with pytest.raises(AssertionError):
        g.ct(2, index=3)
    a = g.neg(3, at=5)
    with pytest.raises(AssertionError):
        g.neg(a, at=5)


def test_case_names_are_unique_and_sizes_bounded():
    assert len({c.name for c in CASES}) == len(CASES)
    for c in CASES:
        g = c.build()
        assert g.n == 4096 and max(d["level"] for d in g.data.values()) <= 4, c.name
        assert max([n.get("sum_cnt", 0) for n in g.compute.values()] + [sum(n["type"] == "mult" for n in g.compute.values())]) <= 33


# ---------------------------------------------------------------------------------------------------- (b) the rewrites' deltas
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_rewrite_delta(native, c, tmp_path, monkeypatch):
    from lattisense_amd.task import FheTaskGpu
    g = c.build()
    path = g.write(tmp_path / c.name)
    monkeypatch.setenv("LSA_NO_GRAPH_FUSION", "1")
    t = FheTaskGpu(path)
    plain = t.counts()
    t.close()
    monkeypatch.delenv("LSA_NO_GRAPH_FUSION")
    t = FheTaskGpu(path)
    fused = t.counts()
    t.close()
    assert plain["inputs"] == fused["inputs"] == len(g.inputs) and plain["outputs"] == fused["outputs"] == len(g.outputs)
    assert (fused["data"] - plain["data"], fused["compute"] - plain["compute"]) == c.delta, (plain, fused)
    # without the rewrites the loader adds only the bridges: per task input that a device node reads, two data and two nodes
    # (C struct, device copy; export, load), per task output the same (device copy, C struct; store, import)
    bridges = 2 * (len(g.inputs) + len(g.outputs))
    assert (plain["data"], plain["compute"]) == (len(g.data) + bridges, len(g.compute) + bridges)
    # what a run must count: the backend nodes are everything but the bridges
    assert c.plain[0] == len(g.compute) and c.fused[0] == len(g.compute) + c.delta[1]
