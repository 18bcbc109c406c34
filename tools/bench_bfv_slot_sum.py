"""BFV slot sum (lsa_bfv_slot_sum) at two shapes: params.BFV_DEFAULT[16384] (N = 2^14, 6 Q + 2 P) at level 3, batch 256, and
params.BFV_DEFAULT[32768] (N = 2^15, 12 Q + 3 P) at the top level, batch 32; counts {8, 128, N/2, 100}, rows 0 and 1, step 1.  Legs
per (shape, count, rows), in one process:

(a) chain          the rotate + add chain over entry points that exist without the operator: the radix-2 plan (the row step first)
                   with one lsa_bfv_rotate (a full key switch) per rotation and lsa_poly_addsub for every sum -- the baseline;
(b) radix2_gather  the operator at radix 2 with the gathering tail (k_bfv_slot_tail; N <= 2^14 only);
(c) radix4_gather  the operator at radix 4 with the gathering tail (N <= 2^14 only);
(d) radix2_plain / radix4_plain   the operator with lsa_bfv_slot_sum_set_gather(plan, 0): c0 transformed too, the CKKS form.

Inputs and keys are uniform random residues (one key's words serve every Galois element); timing does not depend on them.
After `--warmup` calls of each, the legs are alternated `--rounds` times; HIP events on the launch stream; per leg the median, the
minimum and the maximum of the rounds.  Every timed call runs under `--leg-timeout` seconds: when a call does not come back the
process dumps its stack and exits.  Prints one JSON line per (shape, count, rows).

    python tools/bench_bfv_slot_sum.py [--shapes 16384,32768] [--counts 8,128,0,100] [--rows 0,1] [--steps 3] [--warmup 1]
                                       [--rounds 5] [--leg-timeout 120] [--dry-run]

A count of 0 stands for N/2.  --dry-run: needs no GPU; prints the plan counts of each leg (decompositions, key MACs, divisions by
P, Galois keys)."""
import argparse
import ctypes
import faulthandler
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lattisense_amd import params  # noqa: E402

SHAPES = {16384: {"level": 3, "batch": 256}, 32768: {"level": 11, "batch": 32}}
COUNTS = (8, 128, 0, 100)
GATHER_MAX_N = 1 << 14


def chain_steps(n_ring, count, rows, step=1):
    """the radix-2 plan as the chain runs it: [(Galois element, "tail" | "next"), ...] per step, the row step first"""
    h, m, s, n = n_ring // 2, 2 * n_ring, step, count
    steps = [[(m - 1, "next")]] if rows else []
    while n > 1:
        keys = []
        if n % 2:
            keys.append((pow(5, (n - 1) * s % h, m), "tail"))
            n -= 1
        keys.append((pow(5, s % h, m), "next"))
        s, n = 2 * s % h, n // 2
        steps.append(keys)
    return steps


def plan_counts(n_ring, count, rows):
    from lattisense_amd.device import bfv_slot_sum_plan
    out = {}
    for radix in (2, 4):
        p = bfv_slot_sum_plan(n_ring, 1, count, radix, rows)
        out["radix%d" % radix] = {"decompositions": p["steps"], "key_macs": p["keyswitches"], "moddowns": p["moddowns"],
                                  "galois_keys": len(p["galois_elements"])}
    rot = sum(len(k) for k in chain_steps(n_ring, count, rows))
    out["chain"] = {"decompositions": rot, "key_macs": rot, "moddowns": rot, "galois_keys": out["radix2"]["galois_keys"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(map(str, SHAPES)))
    ap.add_argument("--counts", default=",".join(map(str, COUNTS)))
    ap.add_argument("--rows", default="0,1")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--leg-timeout", type=float, default=120.0)
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    shapes = [int(t) for t in a.shapes.split(",")]
    rows_list = [int(t) for t in a.rows.split(",")]
    counts_of = lambda n: [int(t) or n // 2 for t in a.counts.split(",")]
    if a.dry_run:
        from lattisense_amd import build
        build.build_native()
        for n in shapes:
            for count in counts_of(n):
                for rows in rows_list:
                    print(json.dumps({"tool": "bench_bfv_slot_sum", "n": n, "level": SHAPES[n]["level"], "count": count, "rows": rows,
                                      "batch": SHAPES[n]["batch"], "dry_run": True, "plan": plan_counts(n, count, rows)}))
        return

    import numpy as np
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_BFV, BfvSlotSumPlan, DeviceContext
    for N in shapes:
        run_shape(a, N, counts_of(N), rows_list, np, check, lib, ALGO_BFV, BfvSlotSumPlan, DeviceContext)


def run_shape(a, N, counts, rows_list, np, check, lib, ALGO_BFV, BfvSlotSumPlan, DeviceContext):
    B = params.BFV_DEFAULT[N]
    q, p, level, batch = B["q"], B["p"], SHAPES[N]["level"], SHAPES[N]["batch"]
    rng = np.random.default_rng(1)
    ctx = DeviceContext(ALGO_BFV, N, q, p, B["t"])
    st = ctypes.c_void_p()
    check(lib().lsa_stream_create(ctx.h, ctypes.byref(st)))
    ctx.stream = st
    S = ctx.stream
    top, k = len(q) - 1, len(p)
    beta = -(-(top + 1) // k)
    mods = ctx.moduli[: top + 1] + ctx.moduli[len(q): len(q) + k]
    key = np.empty((beta, 2, top + 1 + k, N), dtype=np.uint64)
    for j, m in enumerate(mods):
        key[:, :, j, :] = rng.integers(0, m, size=(beta, 2, N), dtype=np.uint64)
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib().lsa_event_create(ctx.h, ctypes.byref(e0)))
    check(lib().lsa_event_create(ctx.h, ctypes.byref(e1)))

    def timed(fn, steps):
        faulthandler.dump_traceback_later(a.leg_timeout, exit=True)   # the leg's own time limit
        try:
            check(lib().lsa_event_record(ctx.h, e0, S))
            for _ in range(steps):
                fn()
            check(lib().lsa_event_record(ctx.h, e1, S))
            ctx.sync()
            ms = ctypes.c_float()
            check(lib().lsa_event_elapsed_ms(ctx.h, e0, e1, ctypes.byref(ms)))
        finally:
            faulthandler.cancel_dump_traceback_later()
        return ms.value / steps

    glk = {}   # Galois element -> key handle: the top-level key serves every level

    def keys_for(elements):
        for e in elements:
            if e not in glk:
                glk[e] = ctx.upload_key(key, top)
        return {e: glk[e] for e in elements}

    L = level + 1
    w = 2 * L * N
    x = np.empty((batch, 2, L, N), dtype=np.uint64)
    for j in range(L):
        x[:, :, j, :] = rng.integers(0, ctx.moduli[j], size=(batch, 2, N), dtype=np.uint64)
    xin = ctx.upload(x)
    del x
    out, cur, rot, tail = (ctx.alloc(batch * w) for _ in range(4))
    can_gather = N <= GATHER_MAX_N
    for count in counts:
        for rows in rows_list:
            plans = {r: BfvSlotSumPlan(ctx, level, 1, count, r, rows) for r in (2, 4)}
            keys = {r: keys_for(pl.galois_elements) for r, pl in plans.items()}
            csteps = chain_steps(N, count, rows)

            def leg_chain():
                src, have_tail = xin, False
                for ks in csteps:
                    for g, dest in ks:
                        dst = tail if dest == "tail" and not have_tail else rot   # the first tail rotation lands in `tail` itself
                        check(lib().lsa_bfv_rotate(ctx.h, level, src.ptr, g, glk[g], dst.ptr, batch, w, w, S))
                        if dest == "tail":
                            if have_tail:
                                check(lib().lsa_poly_addsub(ctx.h, 0, level, 2, tail.ptr, rot.ptr, tail.ptr, batch, w, w, w, S))
                            have_tail = True
                        else:
                            check(lib().lsa_poly_addsub(ctx.h, 0, level, 2, src.ptr, rot.ptr, cur.ptr, batch, w, w, w, S))
                    src = cur
                if have_tail:
                    check(lib().lsa_poly_addsub(ctx.h, 0, level, 2, src.ptr, tail.ptr, out.ptr, batch, w, w, w, S))

            def leg_op(radix, gather):
                def fn():
                    plans[radix].gather = gather
                    plans[radix].run(xin, batch, keys[radix], out=out)
                return fn

            legs = {"chain": leg_chain}
            if can_gather:
                legs.update({"radix2_gather": leg_op(2, True), "radix4_gather": leg_op(4, True)})
            legs.update({"radix2_plain": leg_op(2, False), "radix4_plain": leg_op(4, False)})
            for fn in legs.values():
                timed(fn, a.warmup)
            ms = {name: [] for name in legs}
            for _ in range(a.rounds):
                for name, fn in legs.items():
                    ms[name].append(timed(fn, a.steps))
            med = {name: statistics.median(v) for name, v in ms.items()}
            spread = {name: max(v) - min(v) for name, v in ms.items()}
            beats = lambda x, y: med[y] - med[x] > max(spread[x], spread[y])   # x faster than y by more than the legs' own spread
            res = {"tool": "bench_bfv_slot_sum", "n": N, "level": level, "special_primes": k, "count": count, "rows": rows, "batch": batch,
                   "dry_run": False, "plan": plan_counts(N, count, rows), "ms_rounds": ms,
                   "ms_per_call": {name: {"median": med[name], "min": min(v), "max": max(v)} for name, v in ms.items()},
                   "chain_over": {name: med["chain"] / med[name] for name in legs if name != "chain"},
                   "radix4_beats_radix2_by_more_than_spread": {f: beats("radix4_" + f, "radix2_" + f)
                                                               for f in (("gather", "plain") if can_gather else ("plain",))},
                   "radix2_beats_radix4_by_more_than_spread": {f: beats("radix2_" + f, "radix4_" + f)
                                                               for f in (("gather", "plain") if can_gather else ("plain",))},
                   "gather_beats_plain_by_more_than_spread": {"radix%d" % r: beats("radix%d_gather" % r, "radix%d_plain" % r)
                                                              for r in ((2, 4) if can_gather else ())},
                   "plain_beats_gather_by_more_than_spread": {"radix%d" % r: beats("radix%d_plain" % r, "radix%d_gather" % r)
                                                              for r in ((2, 4) if can_gather else ())},
                   "operator_not_slower_than_chain": {name: med[name] - med["chain"] <= max(spread[name], spread["chain"])
                                                      for name in legs if name != "chain"}}
            print(json.dumps(res), flush=True)
            for pl in plans.values():
                pl.close()
    ctx.close()


if __name__ == "__main__":
    main()
