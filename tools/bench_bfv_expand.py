"""BFV oblivious expansion (lsa_bfv_expand) on params.BFV_DEFAULT[N] at the top level, N = 2^12 / 2^13 / 2^14, count 64 and 256,
batch 1 and 16.  Legs per (shape, count, batch), in one process and on the same buffers:

(a) composition  what a caller composes from the entry points: per node lsa_bfv_rotate, lsa_poly_addsub (sub), lsa_bfv_mul_monomial
                 into the odd child, lsa_poly_addsub (add) over the parent -- the baseline, the operator's words;
(b) gather       the operator with the gathering tail (k_bfv_expand_tail): a level is one batched key switch whose tail writes both
                 children;
(c) two_step     the operator with lsa_bfv_expand_set_gather(plan, 0): the key switch's tail into the workspace, then
                 k_bfv_expand_combine.

Inputs and keys are uniform random residues (one key's words serve every Galois element); timing does not depend on them.  After
`--warmup` calls of each, the legs are alternated `--rounds` times; HIP events on the launch stream; per leg the median, the minimum
and the maximum of the rounds.  Every timed call runs under `--leg-timeout` seconds: when a call does not come back the process
dumps its stack and exits.  Prints one JSON line per (shape, count, batch).

    python tools/bench_bfv_expand.py [--shapes 4096,8192,16384] [--counts 64,256] [--batches 1,16] [--steps 3] [--warmup 1]
                                     [--rounds 5] [--leg-timeout 120] [--dry-run]

--dry-run: needs no GPU; prints the plan counts (levels, key switches, Galois elements)."""
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
COUNTS = (64, 256)
BATCHES = (1, 16)


def nodes_of(n_ring, count):
    """[(Galois element, shift, nodes)] per level"""
    out, j = [], 0
    while (1 << j) < count:
        out.append((n_ring // (1 << j) + 1, 1 << j, min(1 << j, count)))
        j += 1
    return out


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
        from lattisense_amd.device import bfv_expand_plan
        build.build_native()
        for n in shapes:
            for count in counts:
                print(json.dumps({"tool": "bench_bfv_expand", "n": n, "level": len(params.BFV_DEFAULT[n]["q"]) - 1, "count": count,
                                  "dry_run": True, "plan": bfv_expand_plan(n, count)}))
        return

    import numpy as np
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_BFV, BfvExpandPlan, DeviceContext
    for N in shapes:
        run_shape(a, N, counts, batches, np, check, lib, ALGO_BFV, BfvExpandPlan, DeviceContext)


def run_shape(a, N, counts, batches, np, check, lib, ALGO_BFV, BfvExpandPlan, DeviceContext):
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

    glk = {}   # Galois element -> key handle

    def keys_for(elements):
        for e in elements:
            if e not in glk:
                glk[e] = ctx.upload_key(key, level)
        return {e: glk[e] for e in elements}

    w = 2 * L * N
    for batch in batches:
        x = np.empty((batch, 2, L, N), dtype=np.uint64)
        for j in range(L):
            x[:, :, j, :] = rng.integers(0, ctx.moduli[j], size=(batch, 2, N), dtype=np.uint64)
        xin = ctx.upload(x)
        del x
        rot, dif = ctx.alloc(batch * w), ctx.alloc(batch * w)
        for count in counts:
            plan = BfvExpandPlan(ctx, level, count)
            keys = keys_for(plan.galois_elements)
            si = batch * w
            out = ctx.alloc(count * si)
            levels = nodes_of(N, count)

            def leg_composition():
                for g, s, nodes in levels:
                    for n in range(nodes):
                        par = xin.ptr if s == 1 else out.ptr + 8 * n * si
                        even = out.ptr + 8 * n * si
                        check(lib().lsa_bfv_rotate(ctx.h, level, par, g, glk[g], rot.ptr, batch, w, w, S))
                        if n + s < count:
                            check(lib().lsa_poly_addsub(ctx.h, 1, level, 2, par, rot.ptr, dif.ptr, batch, w, w, w, S))
                            check(lib().lsa_bfv_mul_monomial(ctx.h, level, 2, -s, dif.ptr, out.ptr + 8 * (n + s) * si, batch, w, w, S))
                        check(lib().lsa_poly_addsub(ctx.h, 0, level, 2, par, rot.ptr, even, batch, w, w, w, S))

            def leg_op(gather):
                def fn():
                    plan.gather = gather
                    plan.run(xin, batch, keys, out=out)
                return fn

            legs = {"composition": leg_composition, "gather": leg_op(True), "two_step": leg_op(False)}
            for fn in legs.values():
                timed(fn, a.warmup)
            ms = {name: [] for name in legs}
            for _ in range(a.rounds):
                for name, fn in legs.items():
                    ms[name].append(timed(fn, a.steps))
            med = {name: statistics.median(v) for name, v in ms.items()}
            spread = {name: max(v) - min(v) for name, v in ms.items()}
            beats = lambda x, y: med[y] - med[x] > max(spread[x], spread[y])   # x faster than y by more than the legs' own spread
            res = {"tool": "bench_bfv_expand", "n": N, "level": level, "special_primes": k, "count": count, "batch": batch, "dry_run": False,
                   "plan": {"levels": plan.levels, "keyswitches": plan.keyswitches}, "ms_rounds": ms,
                   "ms_per_call": {name: {"median": med[name], "min": min(v), "max": max(v)} for name, v in ms.items()},
                   "composition_over": {name: med["composition"] / med[name] for name in legs if name != "composition"},
                   "gather_beats_two_step_by_more_than_spread": beats("gather", "two_step"),
                   "two_step_beats_gather_by_more_than_spread": beats("two_step", "gather")}
            print(json.dumps(res), flush=True)
            plan.close()
            ctx.sync()
            out.free()
    ctx.close()


if __name__ == "__main__":
    main()
