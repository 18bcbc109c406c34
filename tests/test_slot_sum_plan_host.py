"""CPU-only: the slot-sum planner and the element rule (lattisense_amd/csrc/slot_sum.h, galois_keys.h), compiled for the host by
tests/cpp/test_slot_sum_plan.cpp with g++ -fsanitize=address,undefined.

Plans: every plan of the grid at N = 2^10 -- count 1..40 and 63, 64, 65, 127, 128, 129, 130, 512; step 1, 3, -1, -64; radix 2, 4;
with and without the BFV row fold -- printed step by step, key by key (element:tail), refusals by their message, against
tests/golden/slot_sum_plans.txt.  That file was recorded with the two planners (one keyed by rotation, one by element) that the
single planner replaced: it pins what a plan is, for both schemes, across that change.

Elements: galois_of_rotation(r, N) for every r in [0, N/2) at N = 2^4 .. 2^12 and 64 spread r at N = 2^16 against pow(5, r, 2N)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "slot_sum_plans.txt")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("slot_sum_plan") / "test_slot_sum_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_slot_sum_plan.cpp"), "-o", path])
    return path


def _run(exe, mode):
    out = subprocess.run([exe, mode], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    return out.stdout.splitlines()


def test_plans_are_the_recorded_ones(exe):
    got, want = _run(exe, "plans"), open(GOLDEN).read().splitlines()
    assert len(want) == 48 * 4 * 2 * 2 and len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    refused = [w for w in want if " ! " in w]
    assert refused and all("a planned rotation a multiple of N/2" in w for w in refused)
    assert all(w.split(" ! ")[1].startswith("lsa_bfv_slot_sum: " if w.split(":")[0].endswith(" 1") else "slot sum: ") for w in refused)


def test_element_of_a_rotation_is_a_power_of_five(exe):
    rows = [tuple(int(x) for x in line.split()) for line in _run(exe, "elements")]
    assert len(rows) == sum((1 << logn) // 2 for logn in range(4, 13)) + 64
    assert {logn for logn, _, _ in rows} == set(range(4, 13)) | {16}
    spread = sorted(r for logn, r, _ in rows if logn == 16)
    assert spread[0] == 0 and spread[-1] == (1 << 15) - 1 and len(set(spread)) == 64
    for logn, r, e in rows:
        assert 0 <= r < (1 << logn) // 2
        assert e == pow(5, r, 2 << logn), (logn, r, e)
