"""BFV encrypted inner product (lsa_bfv_dot) at the reference bench shape N = 2^14 level 3 (params.BFV_DEFAULT[16384], batch 256)
and at N = 2^15 with 12 Q + 3 P (params.BFV_DEFAULT[32768], top level, batch 32), n in {2, 4, 16, 64} pairs of ciphertexts, legs
interleaved in one process:

(a) dot               lsa_bfv_dot at its defaults: the pairs extended to Q u QMul in chunks, one k_tensor_sum launch per chunk, ONE
                      inverse transform, ONE set of six base conversions, ONE key switch;
(b) lazy_by_hand      n x lsa_bfv_mult, n - 1 x lsa_poly_addsub over three polynomials, one lsa_bfv_relin (n scale-downs, one key
                      switch; other words than (a): n roundings);
(c) eager             n x lsa_bfv_mult_relin plus n - 1 additions (n scale-downs, n key switches);
(d) dot_g1 .. dot_g16 (a) with lsa_set_bfv_dot_chunk(g) pairs per tensor launch, the tile pinned to the batch so that the
                      operator does not cut g back to keep lsa_bfv_mult's tile (it does at the default setting): the default chunk
                      size is picked from these.

Legs (b) and (c) call only entry points that exist without lsa_bfv_dot: they are the yardstick, measured on the same box in the
same process.  Inputs and the key are uniform random residues; timing does not depend on them.  After `--warmup` calls of each,
the legs are alternated `--rounds` times; HIP events on the launch stream; per leg the median, the minimum and the maximum of the
rounds.  Every timed call runs under `--leg-timeout` seconds: when a call does not come back the process dumps its stack and
exits.  Prints one JSON line per shape.

    python tools/bench_bfv_dot.py [--shapes 0,1] [--terms 2,4,16,64] [--chunks 1,2,4,8,16] [--steps 1] [--warmup 1] [--rounds 5]
                                  [--leg-timeout 120] [--dry-run]

--dry-run: needs no GPU; prints per shape the plan (lsa_bfv_dot_plan) and the step counts of each leg: operand extensions,
tensor launches, scale-downs (inverse transform + six conversions) and key switches.
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

SHAPES = ({"n": 1 << 14, "set": 16384, "level": 3, "batch": 256}, {"n": 1 << 15, "set": 32768, "level": 11, "batch": 32})
TERMS = (2, 4, 16, 64)
CHUNKS = (1, 2, 4, 8, 16)
DEFAULT_CHUNK = 4   # LSA_BFV_DOT_CHUNK (csrc/ops.hip)


def rule(n, q, level, terms):
    """the headroom rule of include/lattisense_amd.h on Python integers (the dry run loads no library)"""
    logn = n.bit_length() - 1

    def prod(vals):
        out = 1
        for v in vals:
            out *= int(v)
        return out

    bl = prod(q[: level + 1]).bit_length()
    nmul = (prod(q).bit_length() + logn + 60) // 61
    g = min(30, 61 * nmul - bl - logn)
    m = min(terms, 1 << g)
    return {"max_terms": 1 << g, "groups": -(-terms // (1 << g)), "aux_limbs": (bl + logn + (m - 1).bit_length() + 60) // 61}


def step_model(t, chunk, plan):
    groups = plan["groups"]
    return {"dot": {"extensions": 2 * t, "tensor_launches": -(-t // chunk) + groups - 1, "scale_downs": groups, "key_switches": 1},
            "lazy_by_hand": {"extensions": 2 * t, "tensor_launches": t, "scale_downs": t, "key_switches": 1, "additions": t - 1},
            "eager": {"extensions": 2 * t, "tensor_launches": t, "scale_downs": t, "key_switches": t, "additions": t - 1}}


def run_shape(shape, terms, chunks, a):
    P = params.BFV_DEFAULT[shape["set"]]
    n, q, p, t_mod, level, batch = shape["n"], P["q"], P["p"], P["t"], shape["level"], shape["batch"]
    res = {"tool": "bench_bfv_dot", "n": n, "level": level, "q_limbs": len(q), "special_primes": len(p), "batch": batch,
           "dry_run": bool(a.dry_run), "terms": terms, "chunks": chunks, "default_chunk": DEFAULT_CHUNK,
           "plan": {str(t): rule(n, q, level, t) for t in terms}}
    res["steps"] = {str(t): step_model(t, DEFAULT_CHUNK, res["plan"][str(t)]) for t in terms}
    if a.dry_run:
        print(json.dumps(res))
        return

    import numpy as np
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_BFV, DeviceContext, bfv_dot_plan
    for t in terms:
        assert bfv_dot_plan(n, q, level, t) == res["plan"][str(t)], t
    rng = np.random.default_rng(1)
    ctx = DeviceContext(ALGO_BFV, n, q, p, t_mod)
    st = ctypes.c_void_p()
    check(lib().lsa_stream_create(ctx.h, ctypes.byref(st)))
    ctx.stream = st
    L, k = level + 1, len(p)
    beta = -(-L // k)
    mods = ctx.moduli[:L] + ctx.moduli[len(q): len(q) + k]
    key = np.empty((beta, 2, L + k, n), dtype=np.uint64)
    for j, m in enumerate(mods):
        key[:, :, j, :] = rng.integers(0, m, size=(beta, 2, n), dtype=np.uint64)
    rlk = ctx.upload_key(key, level)
    del key

    def rand_ct():
        x = np.empty((batch, 2, L, n), dtype=np.uint64)
        for j in range(L):
            x[:, :, j, :] = rng.integers(0, ctx.moduli[j], size=(batch, 2, n), dtype=np.uint64)
        return ctx.upload(x)

    def clone(src):
        dst = ctx.alloc(src.nwords)
        check(lib().lsa_memcpy_d2d(ctx.h, dst.ptr, src.ptr, src.nwords * 8, ctx.stream))
        return dst

    # every term has its own pair of buffers (no cache reuse between terms); the words repeat, timing does not depend on them
    nmax = max(terms)
    A, B = [rand_ct()], [rand_ct()]
    for _ in range(1, nmax):
        A.append(clone(A[0]))
        B.append(clone(B[0]))
    ctx.sync()
    w2, w3 = 2 * L * n, 3 * L * n
    out = ctx.alloc(batch * w2)
    d3a, d3b = ctx.alloc(batch * w3), ctx.alloc(batch * w3)
    ea, eb = ctx.alloc(batch * w2), ctx.alloc(batch * w2)
    S = ctx.stream

    def leg_dot(t):
        ctx.bfv_dot(level, A[:t], B[:t], rlk, batch, out=out)

    def leg_chunk(g):
        def run(t):
            ctx.set_bfv_dot_chunk(g)
            ctx.set_tile_batch(batch)
            try:
                ctx.bfv_dot(level, A[:t], B[:t], rlk, batch, out=out)
            finally:
                ctx.set_bfv_dot_chunk(0)
                ctx.set_tile_batch(0)
        return run

    def leg_lazy(t):
        check(lib().lsa_bfv_mult(ctx.h, level, A[0].ptr, B[0].ptr, d3a.ptr, batch, w2, w2, w3, S))
        for i in range(1, t):
            check(lib().lsa_bfv_mult(ctx.h, level, A[i].ptr, B[i].ptr, d3b.ptr, batch, w2, w2, w3, S))
            check(lib().lsa_poly_addsub(ctx.h, 0, level, 3, d3a.ptr, d3b.ptr, d3a.ptr, batch, w3, w3, w3, S))
        check(lib().lsa_bfv_relin(ctx.h, level, d3a.ptr, rlk, out.ptr, batch, w3, w2, S))

    def leg_eager(t):
        check(lib().lsa_bfv_mult_relin(ctx.h, level, A[0].ptr, B[0].ptr, rlk, ea.ptr, batch, w2, w2, w2, S))
        for i in range(1, t):
            check(lib().lsa_bfv_mult_relin(ctx.h, level, A[i].ptr, B[i].ptr, rlk, eb.ptr, batch, w2, w2, w2, S))
            check(lib().lsa_poly_addsub(ctx.h, 0, level, 2, ea.ptr, eb.ptr, ea.ptr, batch, w2, w2, w2, S))

    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib().lsa_event_create(ctx.h, ctypes.byref(e0)))
    check(lib().lsa_event_create(ctx.h, ctypes.byref(e1)))

    def timed(fn, t, steps):
        faulthandler.dump_traceback_later(a.leg_timeout, exit=True)   # the leg's own time limit
        try:
            check(lib().lsa_event_record(ctx.h, e0, ctx.stream))
            for _ in range(steps):
                fn(t)
            check(lib().lsa_event_record(ctx.h, e1, ctx.stream))
            ctx.sync()
            ms = ctypes.c_float()
            check(lib().lsa_event_elapsed_ms(ctx.h, e0, e1, ctypes.byref(ms)))
        finally:
            faulthandler.cancel_dump_traceback_later()
        return ms.value / steps

    legs = {"dot": leg_dot, "lazy_by_hand": leg_lazy, "eager": leg_eager}
    for g in chunks:
        legs["dot_g%d" % g] = leg_chunk(g)
    res["ms_per_call"], res["measured"] = {}, {}
    for t in terms:
        for fn in legs.values():
            timed(fn, t, a.warmup)
        ms = {name: [] for name in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                ms[name].append(timed(fn, t, a.steps))
        med = {name: statistics.median(v) for name, v in ms.items()}
        res["ms_per_call"][str(t)] = {name: {"median": med[name], "min": min(v), "max": max(v)} for name, v in ms.items()}
        lazy_range = max(ms["lazy_by_hand"]) - min(ms["lazy_by_hand"])
        res["measured"][str(t)] = {"lazy_over_dot": med["lazy_by_hand"] / med["dot"], "eager_over_dot": med["eager"] / med["dot"],
                                   "dot_beats_lazy_by_more_than_its_range": med["lazy_by_hand"] - med["dot"] > lazy_range,
                                   "dot_loses_to_lazy_by_more_than_its_range": med["dot"] - med["lazy_by_hand"] > lazy_range,
                                   "dot_ct_per_s": batch / (med["dot"] / 1e3)}
    ctx.sync()
    print(json.dumps(res), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--terms", default=",".join(map(str, TERMS)))
    ap.add_argument("--chunks", default=",".join(map(str, CHUNKS)))
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--leg-timeout", type=float, default=120.0)
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    terms = [int(t) for t in a.terms.split(",")]
    chunks = [int(g) for g in a.chunks.split(",") if g]
    for i in (int(x) for x in a.shapes.split(",")):
        run_shape(SHAPES[i], terms, chunks, a)


if __name__ == "__main__":
    main()
