"""CKKS slot sum (lsa_ckks_slot_sum) at N = 2^16 on the headline chain (params.CKKS_DEFAULT[65536] cut to 13 Q limbs + 4 P), at the
top level (12) and at level 3, counts {8, 128, 32768, 100}, batch 64, step 1.  Legs per (level, count), in one process:

(a) chain        the rotate + add chain over entry points that exist without the operator: the radix-2 plan with one
                 lsa_ckks_rotate (a full key switch) per rotation and lsa_poly_addsub for every sum -- the baseline;
(b) radix2       the operator at radix 2, multi-key MAC on (lsa_slot_sum_set_multi_mac(plan, 1): k_ks_mac_multi + k_ext_sum);
(c) radix4       the operator at radix 4, multi-key MAC on;
(d) radix2_seq / radix4_seq   (b) and (c) with the multi-key MAC off (one single-key MAC launch per key: the library's default).

Inputs and keys are uniform random residues (one key's words serve every Galois element); timing does not depend on them.
After `--warmup` calls of each, the legs are alternated `--rounds` times; HIP events on the launch stream; per leg the median, the
minimum and the maximum of the rounds.  Every timed call runs under `--leg-timeout` seconds: when a call does not come back the
process dumps its stack and exits.  Prints one JSON line per (level, count).

    python tools/bench_ckks_slot_sum.py [--levels 12,3] [--counts 8,128,32768,100] [--batch 64] [--steps 6] [--warmup 1]
                                        [--rounds 5] [--leg-timeout 120] [--dry-run]

--dry-run: needs no GPU; prints the plan counts of each leg (decompositions, key MACs, divisions by P, Galois keys)."""
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

N = 65536
LEVELS, COUNTS, BATCH = (12, 3), (8, 128, 32768, 100), 64


def chain_steps(count, step=1):
    """the radix-2 plan as the chain runs it: [(rotation, "tail" | "next"), ...] per step"""
    h, s, n, steps = N // 2, step, count, []
    while n > 1:
        keys = []
        if n % 2:
            keys.append(((n - 1) * s % h, "tail"))
            n -= 1
        keys.append((s % h, "next"))
        s, n = 2 * s % h, n // 2
        steps.append(keys)
    return steps


def plan_counts(count):
    from lattisense_amd.device import plan_slot_sum
    out = {}
    for radix in (2, 4):
        p = plan_slot_sum(N, 1, count, radix)
        out["radix%d" % radix] = {"decompositions": p["steps"], "key_macs": p["keyswitches"], "moddowns": p["moddowns"],
                                  "galois_keys": len(p["rotations"])}
    rot = sum(len(k) for k in chain_steps(count))
    out["chain"] = {"decompositions": rot, "key_macs": rot, "moddowns": rot, "galois_keys": out["radix2"]["galois_keys"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", default=",".join(map(str, LEVELS)))
    ap.add_argument("--counts", default=",".join(map(str, COUNTS)))
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--leg-timeout", type=float, default=120.0)
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    levels = [int(t) for t in a.levels.split(",")]
    counts = [int(t) for t in a.counts.split(",")]
    P = params.CKKS_DEFAULT[65536]
    q, p, batch = P["q"][:13], P["p"][:4], a.batch
    if a.dry_run:
        from lattisense_amd import build
        build.build_native()
        for count in counts:
            print(json.dumps({"tool": "bench_ckks_slot_sum", "n": N, "count": count, "batch": batch, "dry_run": True,
                              "plan": plan_counts(count)}))
        return

    import numpy as np
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_CKKS, DeviceContext, SlotSumPlan
    rng = np.random.default_rng(1)
    ctx = DeviceContext(ALGO_CKKS, N, q, p)
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

    for level in levels:
        L = level + 1
        w = 2 * L * N
        x = np.empty((batch, 2, L, N), dtype=np.uint64)
        for j in range(L):
            x[:, :, j, :] = rng.integers(0, ctx.moduli[j], size=(batch, 2, N), dtype=np.uint64)
        xin = ctx.upload(x)
        del x
        out, cur, rot, tail = (ctx.alloc(batch * w) for _ in range(4))
        for count in counts:
            plans = {r: SlotSumPlan(ctx, level, 1, count, r) for r in (2, 4)}
            keys = {r: keys_for(pl.galois_elements) for r, pl in plans.items()}
            csteps = chain_steps(count)

            def leg_chain():
                src, have_tail = xin, False
                for ks in csteps:
                    nxt = None
                    for r, dest in ks:
                        g = pow(5, r, 2 * N)
                        dst = tail if dest == "tail" and not have_tail else rot   # the first tail rotation lands in `tail` itself
                        check(lib().lsa_ckks_rotate(ctx.h, level, src.ptr, g, glk[g], dst.ptr, batch, w, w, S))
                        if dest == "tail":
                            if have_tail:
                                check(lib().lsa_poly_addsub(ctx.h, 0, level, 2, tail.ptr, rot.ptr, tail.ptr, batch, w, w, w, S))
                            have_tail = True
                        else:
                            nxt = rot
                            check(lib().lsa_poly_addsub(ctx.h, 0, level, 2, src.ptr, rot.ptr, cur.ptr, batch, w, w, w, S))
                    assert nxt is not None
                    src = cur
                if have_tail:
                    check(lib().lsa_poly_addsub(ctx.h, 0, level, 2, src.ptr, tail.ptr, out.ptr, batch, w, w, w, S))

            def leg_op(radix, multi):
                def fn():
                    plans[radix].multi_mac = multi
                    plans[radix].run(xin, batch, keys[radix], out=out)
                return fn

            legs = {"chain": leg_chain, "radix2": leg_op(2, True), "radix4": leg_op(4, True), "radix2_seq": leg_op(2, False),
                    "radix4_seq": leg_op(4, False)}
            for fn in legs.values():
                timed(fn, a.warmup)
            ms = {name: [] for name in legs}
            for _ in range(a.rounds):
                for name, fn in legs.items():
                    ms[name].append(timed(fn, a.steps))
            med = {name: statistics.median(v) for name, v in ms.items()}
            spread = {name: max(v) - min(v) for name, v in ms.items()}
            res = {"tool": "bench_ckks_slot_sum", "n": N, "level": level, "special_primes": k, "count": count, "batch": batch,
                   "dry_run": False, "plan": plan_counts(count), "ms_rounds": ms,
                   "ms_per_call": {name: {"median": med[name], "min": min(v), "max": max(v)} for name, v in ms.items()},
                   "chain_over": {name: med["chain"] / med[name] for name in legs if name != "chain"},
                   "radix4_beats_radix2_by_more_than_spread": med["radix2"] - med["radix4"] > max(spread["radix2"], spread["radix4"]),
                   "multi_mac_beats_seq_by_more_than_spread": {
                       "radix%d" % r: med["radix%d_seq" % r] - med["radix%d" % r] > max(spread["radix%d" % r], spread["radix%d_seq" % r])
                       for r in (2, 4)},
                   "operator_not_slower_than_chain": {name: med[name] - med["chain"] <= max(spread[name], spread["chain"])
                                                      for name in legs if name != "chain"}}
            print(json.dumps(res), flush=True)
            for pl in plans.values():
                pl.close()


if __name__ == "__main__":
    main()
