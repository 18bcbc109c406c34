"""BFV linear transform (lsa_bfv_linear_transform) against the best composition a caller had before it, and the device slot
encoder against the host encoding, at two shapes: params.BFV_DEFAULT[16384] (N = 2^14, 6 Q + 2 P) at the top level, batch 64, and
params.BFV_DEFAULT[32768] (N = 2^15, 12 Q + 3 P) at the top level, batch 16; dense diagonals 0..D-1 for D in {8, 64, 256}.

Legs per (shape, D), in one process:
(a) rotmac    lsa_bfv_rotate_mac_plain_mul over the D diagonals (one decomposition, one key MAC and one division by P per
              rotation; form-1 plaintexts) -- the single-hoisted composition;
(b) operator  the plan of lsa_bfv_lt_create (baby-step / giant-step, double hoisting; form-2 plaintexts).
Encoder legs per shape: lsa_bfv_encode form 2, batch 256 (device transform mod t, lifted forward transforms) against the host
encoding the tests use (Client.bfv_encode + one oracle transform per row, per plaintext; timed on `--host-encodes` plaintexts).

Inputs, diagonals and keys are uniform random words (one key's words serve every Galois element); timing does not depend on
them.  After `--warmup` calls of each, the legs are alternated `--rounds` times; HIP events on the launch stream; per leg the median,
the minimum and the maximum of the rounds.  Every timed call runs under `--leg-timeout` seconds: when a call does not come back the
process dumps its stack and exits.  Prints one JSON line per (shape, D) and one per shape for the encoder.

    python tools/bench_bfv_lt.py [--shapes 16384,32768] [--diags 8,64,256] [--steps 2] [--warmup 1] [--rounds 3]
                                 [--leg-timeout 120] [--host-encodes 4] [--dry-run]

--dry-run: needs no GPU; prints the plan counts of each leg (decompositions, key MACs, divisions by P, Galois keys)."""
import argparse
import ctypes
import faulthandler
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lattisense_amd import params  # noqa: E402

SHAPES = {16384: {"batch": 64}, 32768: {"batch": 16}}
DIAGS = (8, 64, 256)
ENCODE_BATCH = 256


def plan_counts(n, d):
    from lattisense_amd.device import bfv_lt_plan
    p = bfv_lt_plan(n, n // 2, list(range(d)))
    rot_b, rot_g = len([b for b in p["babies"] if b]), len([g for g in p["giants"] if g])
    return {"plan": {"n1": p["n1"], "babies": len(p["babies"]), "giants": len(p["giants"]), "decompositions": 1 + rot_g,
                     "key_macs": rot_b + rot_g, "moddowns": p["moddowns"], "galois_keys": len(p["galois_elements"])},
            "composition": {"decompositions": 1, "key_macs": d - 1, "moddowns": d - 1, "galois_keys": d - 1}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(map(str, SHAPES)))
    ap.add_argument("--diags", default=",".join(map(str, DIAGS)))
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg-timeout", type=float, default=120.0)
    ap.add_argument("--host-encodes", type=int, default=4)
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    shapes = [int(t) for t in a.shapes.split(",")]
    diags = [int(t) for t in a.diags.split(",")]
    if a.dry_run:
        from lattisense_amd import build
        build.build_native()
        for n in shapes:
            B = params.BFV_DEFAULT[n]
            for d in diags:
                print(json.dumps({"tool": "bench_bfv_lt", "kind": "lt", "n": n, "level": len(B["q"]) - 1, "D": d, "batch": SHAPES[n]["batch"],
                                  "dry_run": True, **plan_counts(n, d)}))
            print(json.dumps({"tool": "bench_bfv_lt", "kind": "encode", "n": n, "level": len(B["q"]) - 1, "form": 2, "batch": ENCODE_BATCH,
                              "rows": len(B["q"]) + len(B["p"]), "dry_run": True}))
        return
    for n in shapes:
        run_shape(a, n, diags)


def run_shape(a, N, diags):
    import numpy as np
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_BFV, BfvLinearTransformPlan, DeviceContext
    B = params.BFV_DEFAULT[N]
    q, p, t, batch = B["q"], B["p"], B["t"], SHAPES[N]["batch"]
    level, k = len(q) - 1, len(p)
    L = level + 1
    rng = np.random.default_rng(1)
    ctx = DeviceContext(ALGO_BFV, N, q, p, t)
    st = ctypes.c_void_p()
    check(lib().lsa_stream_create(ctx.h, ctypes.byref(st)))
    ctx.stream = st
    S = ctx.stream
    beta = -(-L // k)
    mods = ctx.moduli[:L] + ctx.moduli[len(q): len(q) + k]
    key = np.empty((beta, 2, L + k, N), dtype=np.uint64)
    for j, m in enumerate(mods):
        key[:, :, j, :] = rng.integers(0, m, size=(beta, 2, N), dtype=np.uint64)
    shared_key = ctx.upload_key(key, level)        # one key's words serve every Galois element
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

    def alternate(legs):
        for fn in legs.values():
            timed(fn, a.warmup)
        ms = {name: [] for name in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                ms[name].append(timed(fn, a.steps))
        return ms

    w = 2 * L * N
    x = np.empty((batch, 2, L, N), dtype=np.uint64)
    for j in range(L):
        x[:, :, j, :] = rng.integers(0, ctx.moduli[j], size=(batch, 2, N), dtype=np.uint64)
    xin = ctx.upload(x)
    del x
    out = ctx.alloc(batch * w)
    period = N // 2
    for D in diags:
        vals = {i: rng.integers(0, t, (2, period)).astype(np.uint64) for i in range(D)}
        plan = BfvLinearTransformPlan(ctx, level, vals, period)
        glk = {e: shared_key for e in plan.galois_elements}
        slots = np.stack([np.concatenate([vals[i][0], vals[i][1]]) for i in range(D)])
        pts = ctx.bfv_encode(level, 1, slots)      # the composition's form-1 plaintexts, one per diagonal, shared by the batch
        n = D
        els = (ctypes.c_uint64 * n)(*[pow(5, i, 2 * N) for i in range(D)])
        hk = (ctypes.c_void_p * n)(*[None if i == 0 else shared_key.value for i in range(D)])
        pp = (ctypes.c_void_p * n)(*[pts.ptr + 8 * i * L * N for i in range(D)])
        sp = (ctypes.c_longlong * n)(*([0] * n))

        def leg_rotmac():
            check(lib().lsa_bfv_rotate_mac_plain_mul(ctx.h, level, xin.ptr, n, els, hk, pp, sp, None, w, out.ptr, batch, w, w, S))

        def leg_operator():
            plan.run(xin, batch, glk, out=out)

        ms = alternate({"rotmac": leg_rotmac, "operator": leg_operator})
        med = {name: statistics.median(v) for name, v in ms.items()}
        spread = {name: max(v) - min(v) for name, v in ms.items()}
        print(json.dumps({"tool": "bench_bfv_lt", "kind": "lt", "n": N, "level": level, "special_primes": k, "D": D, "batch": batch,
                          "dry_run": False, **plan_counts(N, D), "ms_rounds": ms,
                          "ms_per_call": {name: {"median": med[name], "min": min(v), "max": max(v)} for name, v in ms.items()},
                          "rotmac_over_operator": med["rotmac"] / med["operator"],
                          "operator_beats_rotmac_by_more_than_spread": med["rotmac"] - med["operator"] > max(spread.values()),
                          "rotmac_beats_operator_by_more_than_spread": med["operator"] - med["rotmac"] > max(spread.values())}), flush=True)
        plan.close()
        pts.free()
    # the encoder: form 2, batch 256, against the host encoding of the tests
    T = L + k
    slots = rng.integers(0, t, (ENCODE_BATCH, N)).astype(np.uint64)
    enc_out = ctx.alloc(ENCODE_BATCH * T * N)
    ms = alternate({"device": lambda: ctx.bfv_encode(level, 2, slots, out=enc_out)})["device"]
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    from tests.bfv_lt_model import encode_ext
    o = Oracle(N, q, p, t)
    c = Client(o, seed=1)
    encode_ext(o, c, level, slots[0])              # warm: the client's tables
    t0 = time.perf_counter()
    for i in range(a.host_encodes):
        encode_ext(o, c, level, slots[i])
    host_ms = (time.perf_counter() - t0) * 1e3 / a.host_encodes
    med = statistics.median(ms)
    print(json.dumps({"tool": "bench_bfv_lt", "kind": "encode", "n": N, "level": level, "form": 2, "batch": ENCODE_BATCH, "rows": T, "dry_run": False,
                      "device_ms_per_call": {"median": med, "min": min(ms), "max": max(ms)}, "device_ms_per_plaintext": med / ENCODE_BATCH,
                      "host_ms_per_plaintext": host_ms, "host_over_device": host_ms / (med / ENCODE_BATCH)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
