"""run_fhe_gpu_task on hand-built graphs at the edge of every load-time rewrite (tests/graph_edge_cases.py): each case runs
through FheTaskGpu.run with uniform random residues and keys, and every task output is compared word for word with the CPU
oracle walked over the JSON as written (tests/ref_suite.interpret), which knows nothing of the rewrites, the buckets, the
hoisting or the lifetimes.  Never a comparison of two runs of the runtime.

Modes: the default switches; LSA_NO_GRAPH_FUSION=1 (read when the task is made); a second run on the same handle (pooled
slabs are reused, the keys stay on the device); LSA_PIPELINE_MIN_MIB=0 for the cases of two or more independent components.
gpu_nodes / gpu_batches of the run are held to the case table's hand-derived values.  The oracle's values are computed once
per case and shared by the modes."""
import numpy as np
import pytest

from tests import ref_suite as rs
from tests.graph_edge_cases import CASES
from tests.gpu_util import env, need_gpu

pytestmark = pytest.mark.gpu

IDS = [c.name for c in CASES]
MULTI = [c for c in CASES if c.components >= 2]
# LSA_PIPELINE_MIN_MIB=0: a graph of four components is cut into 4 / 2 = 2 chunks of two components, in the order of their
# lowest compute index, and a chunk's nodes form buckets of their own; fewer than four components are not pipelined.
#   A4: each chunk holds one square written [x] and one written [x, x]: two buckets per chunk
#   B1_four_components: each chunk holds two MACs of one signature: one bucket per chunk
PIPELINED = {"A4_squares": (4, 4), "B1_four_components": (4, 2)}

_prepared = {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("graph_edges")


def _prepare(c, workdir):
    """(path, graph, input values, keys, oracle's value of every datum): once per case"""
    if c.name not in _prepared:
        path = c.build().write(workdir / c.name)
        g = rs.load(path)
        o = rs.oracle_for(g)
        vals, keys = rs.random_inputs(g, o, np.random.default_rng(CASES.index(c)))
        want = rs.interpret(g, o, vals, keys)
        for a in want.values():
            a.setflags(write=False)
        _prepared[c.name] = (path, g, vals, keys, want)
    return _prepared[c.name]


def _run(c, workdir, runs=1):
    """makes the task under the current environment, runs it `runs` times (fresh output buffers each time) and compares every
    output of the last run with the oracle; returns (last_run_stats, last_run_shards)"""
    from lattisense_amd.task import FheTaskGpu
    need_gpu()
    path, g, vals, keys, want = _prepare(c, workdir)
    t = FheTaskGpu(path)
    try:
        for _ in range(runs):
            ins, outs, out_cts = rs.arguments(g, vals, keys)
            t.run(ins, outs)
        st, sh = t.last_run_stats(), t.last_run_shards()
    finally:
        t.close()
    for k, (idx, ct) in enumerate(zip(g["outputs"], out_cts)):
        assert np.array_equal(ct.data, want[idx]), "%s: output %d (datum %d) differs from the oracle" % (c.name, k, idx)
    print("%s: gpu_nodes %d gpu_batches %d chunks %d" % (c.name, st["gpu_nodes"], st["gpu_batches"], sh["chunks"]))
    return st, sh


def _stats(st):
    return st["gpu_nodes"], st["gpu_batches"]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_default(c, workdir):
    with env(LSA_NO_GRAPH_FUSION=None, LSA_PIPELINE_MIN_MIB=None, LSA_NO_PIPELINE=None):
        st, sh = _run(c, workdir)
    assert _stats(st) == c.fused and sh["chunks"] == 0


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_no_graph_fusion(c, workdir):
    with env(LSA_NO_GRAPH_FUSION="1", LSA_PIPELINE_MIN_MIB=None, LSA_NO_PIPELINE=None):
        st, sh = _run(c, workdir)
    assert _stats(st) == c.plain and sh["chunks"] == 0


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_second_run_on_one_handle(c, workdir):
    with env(LSA_NO_GRAPH_FUSION=None, LSA_PIPELINE_MIN_MIB=None, LSA_NO_PIPELINE=None):
        st, sh = _run(c, workdir, runs=2)
    assert _stats(st) == c.fused and sh["chunks"] == 0


@pytest.mark.parametrize("c", MULTI, ids=[c.name for c in MULTI])
def test_pipelined(c, workdir):
    with env(LSA_NO_GRAPH_FUSION=None, LSA_PIPELINE_MIN_MIB="0", LSA_NO_PIPELINE=None):
        st, sh = _run(c, workdir)
    if c.components >= 4:
        assert sh["chunks"] == 2 and _stats(st) == PIPELINED[c.name]
    else:
        assert sh["chunks"] == 0 and _stats(st) == c.fused
