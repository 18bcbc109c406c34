"""BFV ring-t plaintext operands (lsa_bfv_addsub_plain / lsa_bfv_mult_plain) at N = 2^14 on the six-prime set
(params.BFV_DEFAULT[16384], top level), batch 64, legs interleaved in one process:

(a)  addsub           lsa_bfv_addsub_plain out of place: one launch, the plaintext scaled up as c0 is read, c1 copied by the same lanes;
(a') addsub_inplace   the same in place: c1 is not touched;
(b)  prescaled        what a caller holding an ALREADY SCALED [L][N] plaintext could do before this operator: lsa_poly_addsub
                      (polys = 1) on c0 plus lsa_memcpy_d2d of c1 (the scale-up itself is not in the leg: it had no entry point);
(b') prescaled_inplace  the add alone;
(b") prescaled_copy_all  the other composition of the same caller: ONE lsa_memcpy_d2d of the whole batch, then the add in place on
                      the copy (7L rows, two calls instead of batch + 1);
(c)  copy             lsa_probe_copy of (a)'s bytes: the HBM yardstick;
(d)  mult_shared / mult_per_item   lsa_bfv_mult_plain with one plaintext for the batch / one per item (lift to pt_mul + product);
(e)  mult_prelifted   lsa_bfv_mult_plain_mul on a pt_mul plaintext lifted beforehand.

Byte model, in rows of N words per batch item, L = level + 1: (a) 4L + 1 (pt, c0 and c1 read, c0 and c1 written), (a') 2L + 1,
(b) 5L (3L for the add, 2L for the copy), (b') 3L, (b") 7L, (c) as (a).  For (d) and (e) the rows are the operands alone (ct read, result
written, plaintext read); the transforms' intermediate traffic is not modelled.

Inputs are uniform random residues; timing does not depend on them.  After `--warmup` calls of each, every leg is timed once
over 10 calls to size its window -- as many calls as fill `--window-ms` (a call takes tens of microseconds: a fixed count would time
the clock) -- then the legs are alternated `--rounds` times; HIP events on the launch stream; per leg the median, the minimum and
the maximum of the rounds, in ms per call.  At batch 64 a leg's buffers (2 x 100 MB) are of the size of the last-level cache, for
the copy yardstick as for the operator: the rates are those of repeated calls on the same buffers.  Every timed window runs under
`--leg-timeout` seconds: when a call does not come back the process dumps its stack and exits.  Prints one JSON line.

    python tools/bench_bfv_plain.py [--batch 64] [--window-ms 200] [--warmup 2] [--rounds 7] [--leg-timeout 120] [--dry-run]

--dry-run: needs no GPU and loads no library; prints the byte model per leg.
"""
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

N, SET = 1 << 14, 16384


def byte_model(L, batch, n=N):
    """rows of n words per batch item and bytes per call of every leg"""
    rows = {"addsub": 4 * L + 1, "addsub_inplace": 2 * L + 1, "prescaled": 5 * L, "prescaled_inplace": 3 * L, "prescaled_copy_all": 7 * L,
            "copy": 4 * L + 1,
            "mult_shared": 4 * L, "mult_per_item": 4 * L + 1, "mult_prelifted": 5 * L}
    model = {k: {"rows": r, "bytes": 8 * n * r * batch} for k, r in rows.items()}
    model["mult_shared"]["bytes"] += 8 * n                      # the one plaintext row of the call
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--window-ms", type=float, default=200.0, help="length of a timed window; the calls per window follow from it")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--leg-timeout", type=float, default=120.0)
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    P = params.BFV_DEFAULT[SET]
    q, p, t = P["q"], P["p"], P["t"]
    level, batch = len(q) - 1, a.batch
    L = level + 1
    model = byte_model(L, batch)
    res = {"tool": "bench_bfv_plain", "n": N, "level": level, "q_limbs": L, "batch": batch, "t": t, "dry_run": bool(a.dry_run),
           "model": model}
    if a.dry_run:
        print(json.dumps(res))
        return

    import numpy as np
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    ctx = DeviceContext(ALGO_BFV, N, q, p, t)
    st = ctypes.c_void_p()
    check(lib().lsa_stream_create(ctx.h, ctypes.byref(st)))
    ctx.stream = st
    S = ctx.stream
    rng = np.random.default_rng(14)
    x = np.empty((batch, 2, L, N), dtype=np.uint64)
    for j in range(L):
        x[:, :, j, :] = rng.integers(0, ctx.moduli[j], size=(batch, 2, N), dtype=np.uint64)
    ct = ctx.upload(x)
    scaled = ctx.upload(np.ascontiguousarray(x[:, 0]))          # any canonical residues serve as the scaled plaintext of (b)
    del x
    pt = ctx.upload(rng.integers(0, t, size=(batch, N), dtype=np.uint64))
    w, wp = 2 * L * N, L * N
    out, work = ctx.alloc(batch * w), ctx.alloc(batch * w)
    check(lib().lsa_memcpy_d2d(ctx.h, work.ptr, ct.ptr, batch * w * 8, S))
    lifted = ctx.bfv_plain_lift(level, 1, pt, batch)
    n_copy = model["copy"]["bytes"] // 16                        # a copy of n words moves 2 n words
    csrc, cdst = ctx.alloc(n_copy), ctx.alloc(n_copy)

    def leg_prescaled():
        check(lib().lsa_poly_addsub(ctx.h, 0, level, 1, ct.ptr, scaled.ptr, out.ptr, batch, w, wp, w, S))
        for b in range(batch):                                   # c1 of every item: the rows after c0
            check(lib().lsa_memcpy_d2d(ctx.h, out.ptr + (b * w + wp) * 8, ct.ptr + (b * w + wp) * 8, wp * 8, S))

    def leg_copy_all():
        check(lib().lsa_memcpy_d2d(ctx.h, out.ptr, ct.ptr, batch * w * 8, S))
        check(lib().lsa_poly_addsub(ctx.h, 0, level, 1, out.ptr, scaled.ptr, out.ptr, batch, w, wp, w, S))

    legs = {
        "addsub": lambda: ctx.bfv_addsub_plain(0, level, ct, pt, batch, out=out),
        "addsub_inplace": lambda: ctx.bfv_addsub_plain(0, level, work, pt, batch, out=work),
        "prescaled": leg_prescaled,
        "prescaled_inplace": lambda: check(lib().lsa_poly_addsub(ctx.h, 0, level, 1, work.ptr, scaled.ptr, work.ptr, batch, w, wp, w, S)),
        "prescaled_copy_all": leg_copy_all,
        "copy": lambda: check(lib().lsa_probe_copy(ctx.h, cdst.ptr, csrc.ptr, n_copy, S)),
        "mult_shared": lambda: ctx.bfv_mult_plain(level, ct, pt, batch, out=out, spt=0),
        "mult_per_item": lambda: ctx.bfv_mult_plain(level, ct, pt, batch, out=out),
        "mult_prelifted": lambda: ctx.bfv_mult_plain_mul(level, ct, lifted, batch, out=out),
    }

    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib().lsa_event_create(ctx.h, ctypes.byref(e0)))
    check(lib().lsa_event_create(ctx.h, ctypes.byref(e1)))

    def timed(fn, steps):
        faulthandler.dump_traceback_later(a.leg_timeout, exit=True)   # the leg's own time limit
        try:
            check(lib().lsa_event_record(ctx.h, e0, ctx.stream))
            for _ in range(steps):
                fn()
            check(lib().lsa_event_record(ctx.h, e1, ctx.stream))
            ctx.sync()
            ms = ctypes.c_float()
            check(lib().lsa_event_elapsed_ms(ctx.h, e0, e1, ctypes.byref(ms)))
        finally:
            faulthandler.cancel_dump_traceback_later()
        return ms.value / steps

    for fn in legs.values():
        timed(fn, a.warmup)
    steps = {name: max(10, min(20000, int(a.window_ms / max(timed(fn, 10), 1e-4)))) for name, fn in legs.items()}
    res["calls_per_window"] = steps
    ms = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, fn in legs.items():
            ms[name].append(timed(fn, steps[name]))
    med = {name: statistics.median(v) for name, v in ms.items()}
    res["ms_per_call"] = {name: {"median": med[name], "min": min(v), "max": max(v)} for name, v in ms.items()}
    res["tb_per_s"] = {name: model[name]["bytes"] / (med[name] * 1e-3) / 1e12 for name in ("addsub", "addsub_inplace", "prescaled",
                                                                                        "prescaled_inplace", "prescaled_copy_all", "copy")}
    spread = {name: max(ms[name]) - min(ms[name]) for name in ("prescaled", "prescaled_inplace")}
    res["measured"] = {"addsub_share_of_copy_ceiling": med["copy"] / med["addsub"],
                       "addsub_slower_than_prescaled_by_more_than_its_spread": med["addsub"] - med["prescaled"] > spread["prescaled"],
                       "addsub_inplace_slower_than_prescaled_inplace_by_more_than_its_spread":
                           med["addsub_inplace"] - med["prescaled_inplace"] > spread["prescaled_inplace"],
                       "prescaled_copy_all_over_addsub": med["prescaled_copy_all"] / med["addsub"],
                       "mult_per_item_over_prelifted": med["mult_per_item"] / med["mult_prelifted"],
                       "mult_shared_over_prelifted": med["mult_shared"] / med["mult_prelifted"]}
    ctx.sync()
    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
