"""CPU-only: how the stand-alone key MACs cut a batch into grid.y groups (lattisense_amd/csrc/ks_mac_groups.h, the one function
behind launch_ks_mac and launch_ks_mac_multi), compiled for the host by tests/cpp/test_ks_mac_groups.cpp with
g++ -fsanitize=address,undefined and run directly.

  check: for every gx in [1, 4096] and batch in [1, 1100] the groups tile [0, batch) exactly and none is empty
  print: the triples of the shapes tests/test_gpu_batch_regimes.py launches, against tests/ks_groups.py, the pure-Python
         restatement those tests use to assert which regime a shape is in; and a grid of further shapes"""
import os
import subprocess

import pytest

from tests import ks_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ks_mac_groups") / "test_ks_mac_groups")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_ks_mac_groups.cpp"), "-o", path])
    return path


def _run(exe, *args):
    out = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout.splitlines()


def test_groups_tile_every_batch_exactly(exe):
    assert _run(exe, "check") == ["ok %d" % (4096 * 1100)]


def _triples(exe, shapes):
    flat = [x for s in shapes for x in s]
    rows = [tuple(int(x) for x in line.split()) for line in _run(exe, "print", *flat)]
    assert [r[:2] for r in rows] == [tuple(s) for s in shapes]
    return [r[2:] for r in rows]


def test_header_and_python_model_agree_on_the_gpu_tests_shapes(exe):
    got = _triples(exe, ks_groups.SHAPES)
    for (gx, batch), g in zip(ks_groups.SHAPES, got):
        assert g == ks_groups.ks_mac_groups(gx, batch), (gx, batch)
    by = dict(zip(ks_groups.SHAPES, got))
    # what the issue reads off the code for its cases: N = 2^12 with 7 targets and N = 2^16 with 8
    assert by[(56, 39)] == (37, 2, 20) and by[(56, 76)] == (37, 3, 26) and by[(1024, 5)] == (2, 3, 2)


def test_header_and_python_model_agree_on_a_grid(exe):
    shapes = [(gx, batch) for gx in (1, 7, 8, 40, 56, 136, 1024, 2047, 2048, 2049, 2176, 4096)
              for batch in (1, 2, 3, 5, 7, 17, 37, 39, 64, 76, 255, 256, 257, 512, 513, 1000, 1100)]
    for s, g in zip(shapes, _triples(exe, shapes)):
        assert g == ks_groups.ks_mac_groups(*s), s


def test_regime_predicate():
    assert ks_groups.short_last_group(56, 39) and ks_groups.short_last_group(56, 76) and ks_groups.short_last_group(1024, 5)
    assert not ks_groups.short_last_group(56, 7)           # bpt 1: the only regime of the small rings at batch <= 7
    assert not ks_groups.short_last_group(2176, 7)         # bpt = batch: N = 2^16, 17 targets
    assert not ks_groups.short_last_group(56, 74)          # full last group
    assert ks_groups.tile_cap(1 << 12) == 512 and ks_groups.tile_cap(1 << 14) == 256 and ks_groups.tile_cap(1 << 16) == 64
    assert ks_groups.auto_tile(1 << 12, 40, 513) == 512 and ks_groups.auto_tile(1 << 16, 1 << 20, 48) == 1
    # the headline shape, 13 Q + 4 P at level 12: the key switch, HMult with the tensor product folded in and as a kernel of its own
    assert (ks_groups.ks_tile_rows(12, 4), ks_groups.hmult_rows(12, 4, True), ks_groups.hmult_rows(12, 4, False)) == (141, 167, 206)


def test_spread_covers_every_source_and_differs_at_the_ends():
    import numpy as np
    rng = np.random.default_rng(1)
    src = np.arange(4 * 3, dtype=np.uint64).reshape(4, 3)
    for batch in (30, 37, 39, 76):
        items, pick = ks_groups.spread(rng, src, batch)
        assert items.shape == (batch, 3) and np.array_equal(items, src[pick])
        assert pick[0] != pick[-1] and set(pick.tolist()) == {0, 1, 2, 3}
    with pytest.raises(AssertionError):
        ks_groups.spread(rng, src, 29)
