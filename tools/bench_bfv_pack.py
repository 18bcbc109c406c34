"""BFV coefficient packing (lsa_bfv_pack) on params.BFV_DEFAULT[N] at the top level, N = 2^12 / 2^13 / 2^14, count 64 and 256, batch 1
and 16, without the trace.  Legs per (shape, count, batch), in one process and on the same buffers:

(a) composition  what a caller composes from the entry points: per paired node lsa_bfv_mul_monomial of the partner, lsa_poly_addsub
                 (add) and (sub), lsa_bfv_rotate of the difference, lsa_poly_addsub (add) over the node -- the baseline, the
                 operator's words;
(b) gather       the operator with the gathering tail (k_bfv_pack_diff, then k_bfv_pack_tail inside the key switch): a level is one
                 batched key switch;
(c) two_step     the operator with lsa_bfv_pack_set_gather(plan, 0): the head writes the whole difference, the key switch's tail
                 goes into the workspace, then k_bfv_pack_combine.

Every leg consumes its inputs, so each call works on what the call before left: the residues stay canonical and timing does not
depend on them.  Inputs and keys are uniform random residues (one key's words serve every Galois element).  After `--warmup` calls of
each, the legs are alternated `--rounds` times; HIP events on the launch stream; per leg the median, the minimum and the maximum of
the rounds.  Every timed call runs under `--leg-timeout` seconds: when a call does not come back the process dumps its stack and
exits.  Prints one JSON line per (shape, count, batch).

    python tools/bench_bfv_pack.py [--shapes 4096,8192,16384] [--counts 64,256] [--batches 1,16] [--steps 3] [--warmup 1]
                                   [--rounds 5] [--leg-timeout 120] [--trace] [--dry-run]

--dry-run: needs no GPU; prints the plan counts (levels, trace levels, key switches, Galois elements)."""
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


def steps_of(n_ring, count, trace):
    """[(Galois element, shift, nodes, paired nodes)] per level, then the trace levels"""
    k = max(0, (count - 1).bit_length())
    out = []
    for j in range(k - 1, -1, -1):
        out.append(((1 << (k - j)) + 1, n_ring >> (k - j), 1 << j, min(1 << j, count - (1 << j))))
    if trace:
        out += [((1 << l) + 1, 0, 1, 0) for l in range(k + 1, n_ring.bit_length())]
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
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    shapes = [int(t) for t in a.shapes.split(",")]
    counts = [int(t) for t in a.counts.split(",")]
    batches = [int(t) for t in a.batches.split(",")]
    if a.dry_run:
        from lattisense_amd import build
        from lattisense_amd.device import bfv_pack_plan
        build.build_native()
        for n in shapes:
            for count in counts:
                print(json.dumps({"tool": "bench_bfv_pack", "n": n, "level": len(params.BFV_DEFAULT[n]["q"]) - 1, "count": count,
                                  "trace": bool(a.trace), "dry_run": True, "plan": bfv_pack_plan(n, count, a.trace)}))
        return

    import numpy as np
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_BFV, BfvPackPlan, DeviceContext
    for N in shapes:
        run_shape(a, N, counts, batches, np, check, lib, ALGO_BFV, BfvPackPlan, DeviceContext)


def run_shape(a, N, counts, batches, np, check, lib, ALGO_BFV, BfvPackPlan, DeviceContext):
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
        si = batch * w
        xb, u, v, rot, res = (ctx.alloc(si) for _ in range(5))
        x = np.empty((batch, 2, L, N), dtype=np.uint64)
        for j in range(L):
            x[:, :, j, :] = rng.integers(0, ctx.moduli[j], size=(batch, 2, N), dtype=np.uint64)
        seed = ctx.upload(x)
        del x
        for count in counts:
            cin = ctx.alloc(count * si)
            for i in range(count):   # input i: the seed items shifted by X^i, filled on the device
                check(lib().lsa_bfv_mul_monomial(ctx.h, level, 2, i, seed.ptr, cin.ptr + 8 * i * si, batch, w, w, S))
            plan = BfvPackPlan(ctx, level, count, a.trace)
            keys = keys_for(plan.galois_elements)
            steps = steps_of(N, count, a.trace)

            def leg_composition():
                for i, (g, s, nodes, n_pair) in enumerate(steps):
                    last = i + 1 == len(steps)
                    for n in range(nodes):
                        ca = cin.ptr + 8 * n * si
                        dst = res.ptr if last else ca
                        if n < n_pair:
                            check(lib().lsa_bfv_mul_monomial(ctx.h, level, 2, s, cin.ptr + 8 * (n + nodes) * si, xb.ptr, batch, w, w, S))
                            check(lib().lsa_poly_addsub(ctx.h, 0, level, 2, ca, xb.ptr, u.ptr, batch, w, w, w, S))
                            check(lib().lsa_poly_addsub(ctx.h, 1, level, 2, ca, xb.ptr, v.ptr, batch, w, w, w, S))
                            check(lib().lsa_bfv_rotate(ctx.h, level, v.ptr, g, glk[g], rot.ptr, batch, w, w, S))
                            check(lib().lsa_poly_addsub(ctx.h, 0, level, 2, u.ptr, rot.ptr, dst, batch, w, w, w, S))
                        else:
                            check(lib().lsa_bfv_rotate(ctx.h, level, ca, g, glk[g], rot.ptr, batch, w, w, S))
                            check(lib().lsa_poly_addsub(ctx.h, 0, level, 2, ca, rot.ptr, dst, batch, w, w, w, S))

            def leg_op(gather):
                def fn():
                    plan.gather = gather
                    plan.run(cin, batch, keys, out=res)
                return fn

            legs = {"composition": leg_composition, "gather": leg_op(True), "two_step": leg_op(False)}
            for fn in legs.values():
                timed(fn, a.warmup)
            ms = {name: [] for name in legs}
            for _ in range(a.rounds):
                for name, fn in legs.items():
                    ms[name].append(timed(fn, a.steps))
            med = {name: statistics.median(t) for name, t in ms.items()}
            spread = {name: max(t) - min(t) for name, t in ms.items()}
            beats = lambda x, y: med[y] - med[x] > max(spread[x], spread[y])   # x faster than y by more than the legs' own spread
            out = {"tool": "bench_bfv_pack", "n": N, "level": level, "special_primes": k, "count": count, "batch": batch,
                   "trace": bool(a.trace), "dry_run": False,
                   "plan": {"levels": plan.levels, "trace_levels": plan.trace_levels, "keyswitches": plan.keyswitches}, "ms_rounds": ms,
                   "ms_per_call": {name: {"median": med[name], "min": min(t), "max": max(t)} for name, t in ms.items()},
                   "composition_over": {name: med["composition"] / med[name] for name in legs if name != "composition"},
                   "composition_beats_gather_by_more_than_spread": beats("composition", "gather"),
                   "composition_beats_two_step_by_more_than_spread": beats("composition", "two_step"),
                   "gather_beats_two_step_by_more_than_spread": beats("gather", "two_step"),
                   "two_step_beats_gather_by_more_than_spread": beats("two_step", "gather")}
            print(json.dumps(out), flush=True)
            plan.close()
            ctx.sync()
            cin.free()
    ctx.close()


if __name__ == "__main__":
    main()
