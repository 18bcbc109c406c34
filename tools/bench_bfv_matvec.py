"""BFV plaintext matrix x ciphertext vector product (lsa_bfv_matvec_plain_mul) on params.BFV_DEFAULT[N] at the top level,
N = 2^12 / 2^13 / 2^14, (rows, cols) = (64, 64), (256, 128), (1024, 256), batch 1 and 16, one database shared by the batch (spt == 0).
Legs per (shape, matrix, batch), in one process and on the same buffers:

(a) default       the operator at the plan's own blocks;
(b) rb1 .. rb8    lsa_set_bfv_matvec_block(ctx, row_block, 0) for every row block;
(c) composition   `rows` calls of lsa_bfv_mac_plain_mul, one per output row: the reference to beat.

A shape whose database (rows * cols * L * N * 8 bytes) exceeds --max-db-gib is dropped and named in a line of its own.  The database is
one block of uniform random plaintexts copied over and over on the device (the kernels have no data-dependent path; the addresses, and
so the traffic, are those of a real database).  After `--warmup` calls of each, the legs are alternated `--rounds` times; HIP events on
the launch stream; per leg the median, the minimum and the maximum of the rounds.  Every timed call runs under `--leg-timeout` seconds:
when a call does not come back the process dumps its stack and exits.  Prints one JSON line per (shape, matrix, batch) with the
plaintext-stream rate rows * cols * L * N * 8 bytes / time of every operator leg.

    python tools/bench_bfv_matvec.py [--shapes 4096,8192,16384] [--matrices 64x64,256x128,1024x256] [--batches 1,16] [--steps 3]
                                     [--warmup 1] [--rounds 5] [--max-db-gib 32] [--leg-timeout 300] [--dry-run]

--dry-run: needs no GPU; prints the shapes, the plan and the byte accounting (rows of N words moved per call)."""
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
MATRICES = ((64, 64), (256, 128), (1024, 256))
BATCHES = (1, 16)
ROW_BLOCKS = (1, 2, 4, 8)


def accounting(n, L, rows, cols, batch, plan, two_pass):
    """rows of N words moved per call, derived from the code: the composition per term reads the ciphertext in its transform (twice on
    two-pass rings), the plaintext, and reads and writes the running sum; the operator reads every plaintext once, transforms every
    ciphertext once and re-reads the transformed ciphertext once per row block"""
    t = 2 if two_pass else 1
    comp = batch * rows * cols * (2 * L * t + 4 * L) + rows * cols * L + batch * rows * 2 * L * 2 * t
    rb = plan["row_block"]
    op = rows * cols * L + batch * (cols * 2 * L * 2 * t + cols * 2 * L * -(-rows // rb) + rows * 2 * L * (1 + 2 * t))
    return {"composition_rows": comp, "operator_rows": op, "database_bytes": rows * cols * L * n * 8,
            "composition_launches_at_least": rows * (cols + 1), "row_bytes": n * 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(map(str, SHAPES)))
    ap.add_argument("--matrices", default=",".join("%dx%d" % m for m in MATRICES))
    ap.add_argument("--batches", default=",".join(map(str, BATCHES)))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-db-gib", type=float, default=32.0)
    ap.add_argument("--leg-timeout", type=float, default=300.0)
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    shapes = [int(t) for t in a.shapes.split(",")]
    matrices = [tuple(int(v) for v in t.split("x")) for t in a.matrices.split(",")]
    batches = [int(t) for t in a.batches.split(",")]
    if a.dry_run:
        from lattisense_amd import build
        from lattisense_amd.device import bfv_matvec_plan
        build.build_native()
        for n in shapes:
            L = len(params.BFV_DEFAULT[n]["q"])
            for rows, cols in matrices:
                for batch in batches:
                    plan = bfv_matvec_plan(n, L, rows, cols, batch)
                    acc = accounting(n, L, rows, cols, batch, plan, n > 16384)                  # N <= 2^14: one pass (the wide plan above 2^12)
                    print(json.dumps({"tool": "bench_bfv_matvec", "n": n, "level": L - 1, "rows": rows, "cols": cols, "batch": batch,
                                      "dry_run": True, "plan": plan, "dropped": acc["database_bytes"] > a.max_db_gib * 2 ** 30, **acc}))
        return

    import numpy as np
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_BFV, DeviceContext, bfv_matvec_plan
    for N in shapes:
        run_shape(a, N, matrices, batches, np, check, lib, ALGO_BFV, DeviceContext, bfv_matvec_plan)


def run_shape(a, N, matrices, batches, np, check, lib, ALGO_BFV, DeviceContext, bfv_matvec_plan):
    B = params.BFV_DEFAULT[N]
    q, p = B["q"], B["p"]
    rng = np.random.default_rng(1)
    ctx = DeviceContext(ALGO_BFV, N, q, p, B["t"])
    st = ctypes.c_void_p()
    check(lib().lsa_stream_create(ctx.h, ctypes.byref(st)))
    ctx.stream = st
    S = ctx.stream
    level = len(q) - 1
    L = level + 1
    wct, wpt = 2 * L * N, L * N
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
        ctx.set_bfv_matvec_block(0, 0)
        return ms

    def residues(shape_head, rows_):
        x = np.empty(shape_head + (rows_, N), dtype=np.uint64)
        for j in range(rows_):
            x[..., j, :] = rng.integers(0, ctx.moduli[j % L], size=shape_head + (N,), dtype=np.uint64)
        return x

    head = {"tool": "bench_bfv_matvec", "n": N, "level": level, "dry_run": False}
    for rows, cols in matrices:
        db_bytes = rows * cols * wpt * 8
        if db_bytes > a.max_db_gib * 2 ** 30:
            print(json.dumps({**head, "rows": rows, "cols": cols, "dropped": True, "database_bytes": db_bytes}), flush=True)
            continue
        block = min(rows * cols, 64)                                  # plaintexts uploaded; the rest are device copies of them
        db = ctx.alloc(rows * cols * wpt)
        seed = ctx.upload(residues((block,), L))
        for i in range(0, rows * cols, block):
            k = min(block, rows * cols - i)
            check(lib().lsa_probe_copy(ctx.h, db.ptr + 8 * i * wpt, seed.ptr, k * wpt, S))
        ctx.sync()
        seed.free()
        for batch in batches:
            cts = ctx.upload(residues((cols, batch), 2 * L))
            out = ctx.alloc(rows * batch * wct)
            pc = (ctypes.c_void_p * cols)(*[cts.ptr + 8 * c * batch * wct for c in range(cols)])
            sc = (ctypes.c_longlong * cols)(*([wct] * cols))
            sp = (ctypes.c_longlong * cols)(*([0] * cols))
            pps = [(ctypes.c_void_p * cols)(*[db.ptr + 8 * (r * cols + c) * wpt for c in range(cols)]) for r in range(rows)]

            def leg_op(rb):
                def fn():
                    ctx.set_bfv_matvec_block(rb, 0)
                    ctx.bfv_matvec_plain_mul(level, cts, db, rows, cols, batch, out=out)
                return fn

            def leg_comp():
                for r in range(rows):
                    check(lib().lsa_bfv_mac_plain_mul(ctx.h, level, cols, pc, sc, pps[r], sp, None, 0, out.ptr + 8 * r * batch * wct, batch,
                                                      wct, S))

            legs = {"default": leg_op(0)}
            legs.update({"rb%d" % rb: leg_op(rb) for rb in ROW_BLOCKS})
            legs["composition"] = leg_comp
            ms = measure(legs)
            med = {name: statistics.median(t) for name, t in ms.items()}
            spread = {name: max(t) - min(t) for name, t in ms.items()}
            plan = bfv_matvec_plan(N, L, rows, cols, batch)
            print(json.dumps({**head, "rows": rows, "cols": cols, "batch": batch, "plan": plan, "database_bytes": db_bytes,
                              "ms_rounds": ms,
                              "ms_per_call": {name: {"median": med[name], "min": min(t), "max": max(t)} for name, t in ms.items()},
                              "composition_over_default": med["composition"] / med["default"],
                              "default_slower_than_composition_by_more_than_spread":
                                  med["default"] - med["composition"] > max(spread["default"], spread["composition"]),
                              "plaintext_stream_gb_per_s": {name: db_bytes / (med[name] * 1e-3) / 1e9 for name in legs if name != "composition"}}),
                  flush=True)
            ctx.sync()
            cts.free()
            out.free()
        db.free()
    ctx.close()


if __name__ == "__main__":
    main()
