"""CPU-only: the plan of the CKKS slot sum (lsa_slot_sum_plan, lattisense_amd/csrc/slot_sum.h) through ctypes.  For every count in
1..130, step in {1, 3, -1, -64} and radix in {2, 4} at N = 2^10 the returned counts and rotations equal an independent restatement
of the rule (below), a replay of the steps on index multisets gives {i*step mod N/2 : i < count}, and the radix-2 rotations are the
key set of Lattigo's InnerSumLog.  A plan whose rule meets a rotation that is a multiple of N/2 (step -64 from count 9 on) is
refused, as is every other bad argument, each with a message that names it.  device.py plans without a GPU and refuses to run
without one."""
import ctypes
import types
from collections import Counter

import pytest

N = 1 << 10
H = N // 2
ENTRY_POINTS = {"lsa_slot_sum_plan": 10, "lsa_slot_sum_create": 6, "lsa_slot_sum_destroy": 1, "lsa_slot_sum_info": 8,
                "lsa_slot_sum_galois_elements": 3, "lsa_slot_sum_set_multi_mac": 2, "lsa_ckks_slot_sum": 11}


@pytest.fixture(scope="module")
def native():
    from lattisense_amd import build, _native
    build.build_native()
    return _native


def restated_steps(h, step, count, radix):
    """the rule of the issue, written again: [(rotation mod h, "tail" | "next"), ...] per step; None where a rotation is 0 mod h"""
    s, n, steps = step, count, []
    while n > 1:
        keys = []
        if n % 2:
            keys.append(((n - 1) * s % h, "tail"))
            n -= 1
        if radix == 4 and n % 4 == 0:
            keys += [(i * s % h, "next") for i in (1, 2, 3)]
            s, n = 4 * s, n // 4
        else:
            keys.append((s % h, "next"))
            s, n = 2 * s, n // 2
        if any(r == 0 for r, _ in keys):
            return None
        steps.append(keys)
    return steps


def replay(h, steps):
    """x as a multiset of rotation amounts of the input: x <- x + sum of the NEXT rotations of x, the TAIL rotations aside"""
    x, tail = Counter({0: 1}), Counter()
    for keys in steps:
        nxt = Counter(x)
        for r, dest in keys:
            moved = Counter({(i + r) % h: c for i, c in x.items()})
            if dest == "tail":
                tail += moved
            else:
                nxt += moved
        x = nxt
    return x + tail


def call_plan(native, n, step, count, radix, capacity=64):
    ns, nk, nm, cnt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rot = (ctypes.c_int * capacity)()
    rc = native.lib().lsa_slot_sum_plan(n, step, count, radix, ctypes.byref(ns), ctypes.byref(nk), ctypes.byref(nm), rot, capacity,
                                        ctypes.byref(cnt))
    if rc:
        return rc, native.lib().lsa_last_error().decode()
    return 0, (ns.value, nk.value, nm.value, [int(r) for r in rot[: cnt.value]])


def test_binding_table_has_the_entry_points(native):
    for name, nargs in ENTRY_POINTS.items():
        assert len(native.SIGNATURES[name][1]) == nargs, name
        assert hasattr(native.lib(), name)


def test_plan_against_the_restated_rule_and_a_replay(native):
    refused = 0
    for step in (1, 3, -1, -64):
        for radix in (2, 4):
            for count in range(1, 131):
                want = restated_steps(H, step, count, radix)
                rc, got = call_plan(native, N, step, count, radix)
                if want is None:
                    assert rc == 1 and "step" in got and "N/2" in got, (step, radix, count, got)
                    refused += 1
                    continue
                assert rc == 0, got
                ns, nk, nm, rot = got
                has_tail = any(d == "tail" for keys in want for _, d in keys)
                assert all(len(keys) <= 4 for keys in want)
                assert ns == len(want) and nk == sum(len(keys) for keys in want) and nm == len(want) + (1 if has_tail else 0)
                assert rot == sorted({r for keys in want for r, _ in keys}), (step, radix, count)
                assert all(0 < r < H for r in rot)
                # the steps the library reports are the restated ones (counts and rotation set agree); their replay is the sum
                sums = replay(H, want)
                assert sums == Counter(i * step % H for i in range(count)), (step, radix, count)
                if len({i * step % H for i in range(count)}) == count:
                    assert set(sums.values()) == {1}                       # each element once
                if radix == 2:   # Lattigo InnerSumLog: 2^i * step for i < floor(log2 count), plus the set-bit offsets
                    top = count.bit_length() - 1
                    lattigo = {(1 << i) * step % H for i in range(top)}
                    lattigo |= {((count >> (k + 1)) << (k + 1)) * step % H for k in range(top) if count >> k & 1}
                    assert set(rot) == lattigo, (step, count)
    # step -64 has order 8 in Z/512: every count above 8 meets a rotation that is a multiple of N/2, and nothing else is refused
    assert refused == 2 * (130 - 8)


def test_worked_examples(native):
    assert call_plan(native, N, 1, 1, 2) == (0, (0, 0, 0, []))                       # a copy: no keys
    assert call_plan(native, N, 5, 3, 2) == (0, (1, 2, 2, [5, 10]))                  # tail 2s, next s
    assert call_plan(native, N, 1, 5, 4) == (0, (1, 4, 2, [1, 2, 3, 4]))             # one decomposition, four MACs, two divisions
    big = 1 << 16
    rc, (ns, nk, nm, rot) = call_plan(native, big, 1, 1 << 15, 4)
    assert (rc, ns, nk, nm) == (0, 8, 22, 8) and len(rot) == 22
    rc, (ns, nk, nm, rot) = call_plan(native, big, 1, 1 << 15, 2)
    assert (rc, ns, nk, nm) == (0, 15, 15, 15) and rot == [1 << i for i in range(15)]
    assert call_plan(native, N, 1, 100, 0) == call_plan(native, N, 1, 100, 4)         # the default radix
    assert call_plan(native, N, -8, 8, 2)[1][3] == [H - 32, H - 16, H - 8]            # Replicate: a negative step


def test_refusals_name_the_argument(native):
    for args, needle in (((N, 1, 0, 2), "count"), ((N, 1, -3, 2), "count"), ((N, 1, H + 1, 2), "count"), ((N, 1, 8, 3), "radix"),
                         ((N, 1, 8, -2), "radix"), ((N, 0, 2, 2), "step"), ((N, H, 2, 4), "step"), ((N, H // 2, 3, 2), "step"),
                         ((N, H // 2, 4, 4), "step"), ((1000, 1, 2, 2), "n_ring")):
        rc, msg = call_plan(native, *args)
        assert rc == 1 and needle in msg, (args, rc, msg)
    assert call_plan(native, N, 1, H, 2)[0] == 0                                      # count == N/2 is the whole vector
    rc, msg = call_plan(native, N, 1, 100, 2, capacity=2)
    assert rc == 1 and "buffer" in msg
    ns = ctypes.c_int()
    assert native.lib().lsa_slot_sum_plan(N, 1, 100, 2, ctypes.byref(ns), None, None, None, 0, None) == 0 and ns.value == 6


def test_device_py_plans_without_a_gpu_and_refuses_to_run(native):
    import torch
    from lattisense_amd.device import SlotSumPlan, plan_slot_sum
    info = plan_slot_sum(N, 3, 21, radix=4)
    assert info == {"steps": 2, "keyswitches": 8, "moddowns": 3, "rotations": [3, 6, 9, 12, 24, 36, 48, 60]}
    ctx = types.SimpleNamespace(n=N, h=None, stream=None)       # what a context is without a device: no handle
    plan = SlotSumPlan(ctx, 2, -1, 8)
    assert plan.rotations == [H - 4, H - 3, H - 2, H - 1] and (plan.steps, plan.keyswitches, plan.moddowns) == (2, 4, 2)   # radix 4
    plan2 = SlotSumPlan(ctx, 2, -1, 8, radix=2)
    assert plan2.rotations == [H - 4, H - 2, H - 1] and (plan2.steps, plan2.keyswitches, plan2.moddowns) == (3, 3, 3)
    assert plan.galois_elements == sorted(pow(5, r, 2 * N) for r in plan.rotations)
    with pytest.raises(native.LsaError) as e:
        plan.run(types.SimpleNamespace(ptr=None), 1, {})
    assert e.value.code == 1 and "null context" in str(e.value)
    if not torch.cuda.is_available():
        from lattisense_amd import params
        from lattisense_amd.device import ALGO_CKKS, DeviceContext
        P = params.CKKS_DEFAULT[65536]
        with pytest.raises(native.LsaError) as e:
            DeviceContext(ALGO_CKKS, 65536, P["q"], P["p"])
        assert e.value.code == 2                                 # LSA_ERR_NO_DEVICE: no CPU fallback exists
