"""BFV external product RLWE x RGSW (lsa_bfv_external_product) and select by an encrypted index (lsa_bfv_select) on
params.BFV_DEFAULT[N] at the top level, N = 2^12 / 2^13 / 2^14, batch 1 and 16, select with count 64.  Legs per (shape, batch), in one
process and on the same buffers:

(a) pair      the default form: both gadget products in ONE k_ks_mac_pair launch into one accumulator;
(b) two_step  lsa_set_rgsw_pair_mac(ctx, 0): launch_ks_mac twice, the second adding to the first's output;
(c) rotate    one lsa_bfv_rotate at the same shape (the external product alone): for orientation, no threshold.

The select consumes its inputs, so each call works on what the call before left: the residues stay canonical and timing does not
depend on them.  Inputs and keys are uniform random residues (one key's words serve every selector).  After `--warmup` calls of each,
the legs are alternated `--rounds` times; HIP events on the launch stream; per leg the median, the minimum and the maximum of the
rounds.  Every timed call runs under `--leg-timeout` seconds: when a call does not come back the process dumps its stack and exits.
Prints one JSON line per (shape, operator, batch).

    python tools/bench_bfv_rgsw.py [--shapes 4096,8192,16384] [--counts 64] [--batches 1,16] [--steps 3] [--warmup 1] [--rounds 5]
                                   [--leg-timeout 120] [--dry-run]

--dry-run: needs no GPU; prints the plan counts (levels, external products)."""
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

SHAPES = (4096, 8192, 16384)
COUNTS = (64,)
BATCHES = (1, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(map(str, SHAPES)))
    ap.add_argument("--counts", default=",".join(map(str, COUNTS)))
    ap.add_argument("--batches", default=",".join(map(str, BATCHES)))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--leg-timeout", type=float, default=120.0)
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    shapes = [int(t) for t in a.shapes.split(",")]
    counts = [int(t) for t in a.counts.split(",")]
    batches = [int(t) for t in a.batches.split(",")]
    if a.dry_run:
        from lattisense_amd import build
        from lattisense_amd.device import bfv_select_plan
        build.build_native()
        for n in shapes:
            for count in counts:
                print(json.dumps({"tool": "bench_bfv_rgsw", "n": n, "level": len(params.BFV_DEFAULT[n]["q"]) - 1, "count": count,
                                  "dry_run": True, "plan": bfv_select_plan(count)}))
        return

    import numpy as np
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_BFV, BfvSelectPlan, DeviceContext
    for N in shapes:
        run_shape(a, N, counts, batches, np, check, lib, ALGO_BFV, BfvSelectPlan, DeviceContext)


def run_shape(a, N, counts, batches, np, check, lib, ALGO_BFV, BfvSelectPlan, DeviceContext):
    B = params.BFV_DEFAULT[N]
    q, p = B["q"], B["p"]
    rng = np.random.default_rng(1)
    ctx = DeviceContext(ALGO_BFV, N, q, p, B["t"])
    st = ctypes.c_void_p()
    check(lib().lsa_stream_create(ctx.h, ctypes.byref(st)))
    ctx.stream = st
    S = ctx.stream
    level, k = len(q) - 1, len(p)
    L = level + 1
    beta = -(-L // k)
    mods = ctx.moduli[:L] + ctx.moduli[len(q): len(q) + k]
    key = np.empty((beta, 2, L + k, N), dtype=np.uint64)
    for j, m in enumerate(mods):
        key[:, :, j, :] = rng.integers(0, m, size=(beta, 2, N), dtype=np.uint64)
    r0, r1 = ctx.upload_key(key, level), ctx.upload_key(key, level)
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

    def measure(legs):
        for fn in legs.values():
            timed(fn, a.warmup)
        ms = {name: [] for name in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                ms[name].append(timed(fn, a.steps))
        ctx.set_rgsw_pair_mac(1)
        med = {name: statistics.median(t) for name, t in ms.items()}
        spread = {name: max(t) - min(t) for name, t in ms.items()}
        beats = lambda x, y: med[y] - med[x] > max(spread[x], spread[y])   # x faster than y by more than the legs' own spread
        return {"ms_rounds": ms, "ms_per_call": {name: {"median": med[name], "min": min(t), "max": max(t)} for name, t in ms.items()},
                "two_step_over_pair": med["two_step"] / med["pair"],
                "pair_beats_two_step_by_more_than_spread": beats("pair", "two_step"),
                "two_step_beats_pair_by_more_than_spread": beats("two_step", "pair")}, med

    w = 2 * L * N
    head = {"tool": "bench_bfv_rgsw", "n": N, "level": level, "special_primes": k, "beta": beta, "dry_run": False}
    for batch in batches:
        si = batch * w
        x = np.empty((batch, 2, L, N), dtype=np.uint64)
        for j in range(L):
            x[:, :, j, :] = rng.integers(0, ctx.moduli[j], size=(batch, 2, N), dtype=np.uint64)
        seed = ctx.upload(x)
        del x
        res = ctx.alloc(si)

        def leg_ep(pair):
            def fn():
                ctx.set_rgsw_pair_mac(pair)
                ctx.bfv_external_product(level, seed, (r0, r1), batch, out=res)
            return fn

        def leg_rotate():
            check(lib().lsa_bfv_rotate(ctx.h, level, seed.ptr, 3, r0, res.ptr, batch, w, w, S))

        out, med = measure({"pair": leg_ep(1), "two_step": leg_ep(0), "rotate": leg_rotate})
        out["external_product_over_rotate"] = med["pair"] / med["rotate"]
        print(json.dumps({**head, "op": "external_product", "batch": batch, **out}), flush=True)
        for count in counts:
            cin = ctx.alloc(count * si)
            for i in range(count):   # input i: the seed items shifted by X^i, filled on the device
                check(lib().lsa_bfv_mul_monomial(ctx.h, level, 2, i, seed.ptr, cin.ptr + 8 * i * si, batch, w, w, S))
            plan = BfvSelectPlan(ctx, level, count)
            sel = [(r0, r1)] * plan.levels

            def leg_sel(pair):
                def fn():
                    ctx.set_rgsw_pair_mac(pair)
                    plan.run(cin, batch, sel, out=res)
                return fn

            out, _ = measure({"pair": leg_sel(1), "two_step": leg_sel(0)})
            print(json.dumps({**head, "op": "select", "count": count, "batch": batch,
                              "plan": {"levels": plan.levels, "products": plan.products}, **out}), flush=True)
            plan.close()
            ctx.sync()
            cin.free()
    ctx.close()


if __name__ == "__main__":
    main()
