"""Every entry point that reaches a key-switch tile (lattisense_amd/csrc/key_switch.h KsTile: ops.hip, slot_sum.hip and, through
them, linear_transform.hip) gives the words and queues the launches it gave when tests/golden/ks_callers.json was recorded
(tools/record_ks_callers.py, with the library of the commit before the key switch became a unit of its own).  Per case, exact
equality of
  (a) the SHA-256 of the output words,
  (b) for each of the five profiler kinds, the launches and the algorithmic bytes of the call (lsa_profile_begin(ctx, 1) /
      lsa_profile_read; the bytes are computed from shapes, integers in a double),
under the default settings, with unfused tails (lsa_set_fuse_tails 0) and on two streams (lsa_set_dual_stream 1), batch 3 in tiles of
2.  The cases and shapes are tests/ks_callers_cases.py's.  The settings are the context's setters; the one exception is the
giant-step form of the CKKS linear transform, which the library reads from LSA_LT_GIANT_SCATTER at every call and has no setter for.
A case the golden file does not hold fails."""
import json
import os

import pytest

from tests import ks_callers_cases as K
from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ks_callers.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def rigs():
    """rig by name, made on first use; contexts, keys and plans are released when the module is done"""
    need_gpu()
    made = {}

    def get(name):
        if name not in made:
            made[name] = K.make_rig(name)
        return made[name]
    yield get
    for r in made.values():
        r.close()


def test_shapes_take_the_paths_they_are_meant_to(rigs):
    """ckks14: a single-key switch runs the fused second pass + key MAC, and the last of its three digits has one limb; ckks12: one
    digit, never fused"""
    small, big = rigs("ckks12"), rigs("ckks14")
    assert not small.ctx.key_switch_fused(small.level, small.key("rlk")) and -(-small.L // len(small.p)) == 1
    assert big.ctx.key_switch_fused(big.level, big.key("rlk"))
    assert -(-big.L // len(big.p)) == 3 and big.L % len(big.p) == 1 and all(q < 1 << 53 for q in big.q)


@pytest.mark.parametrize("rig,case,setting", K.CASE_IDS, ids=["-".join(c) for c in K.CASE_IDS])
def test_words_and_launches_are_the_recorded_ones(golden, rigs, rig, case, setting):
    key = K.golden_key(rig, case, setting)
    assert key in golden, "tests/golden/ks_callers.json holds no record of " + key
    got = K.measure(rigs(rig), case, setting)
    print(key, got)
    assert got["launched"] == golden[key]["launched"]
    assert got["bytes"] == golden[key]["bytes"]
    assert got["sha256"] == golden[key]["sha256"]
