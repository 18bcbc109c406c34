"""BFV polynomial evaluator (lsa_bfv_poly_eval) at N = 2^14 on the six-prime set (params.BFV_DEFAULT[16384], top level), dense
polynomials of degree 15 and 31 with uniform coefficients, legs interleaved in one process:

(a) poly          lsa_bfv_poly_eval at the planner's log_baby (or --log-baby): the powers by lsa_bfv_mult_relin, all leaves by k_bfv_poly_leaves,
                  the sum of leaf x giant-power products by lsa_bfv_dot: ONE scale-down and ONE relinearisation for the sum;
(b) horner        acc = c_d x + c_(d-1) by lsa_bfv_affine_const, then d - 1 times acc = acc * x (lsa_bfv_mult_relin) + c_k
                  (lsa_bfv_affine_const in place): depth d - 1;
(c) plan_by_hand  the same plan from public entry points without lsa_bfv_dot: the same powers, every leaf by lsa_bfv_affine_const
                  per term and lsa_poly_addsub, ONE lsa_bfv_mult_relin per pair and lsa_poly_addsub for the sum.  Against (a) this
                  isolates what the single scale-down and relinearisation (and the one-launch leaves) save;
(d) horner_mults  the d - 1 lsa_bfv_mult_relin calls of (b) alone: entry points of the commit before this operator only (it had
                  no BFV constant operand), a lower bound of any Horner composition there.

Legs (b) and (c) are compositions a caller can write today; they compute other words than (a) (one rounding per product) and
decrypt to the same slots.  Inputs and the key are uniform random residues; timing does not depend on them.  After `--warmup`
calls of each, the legs are alternated `--rounds` times, each timed window `--steps` calls (a few tenths of a second); HIP events
on the launch stream; per leg the median, the minimum and the maximum of the rounds, in ms per call.  Every timed call runs under `--leg-timeout` seconds: when a call does not come back the process dumps
its stack and exits.  Prints one JSON line per degree.

    python tools/bench_bfv_poly.py [--degrees 15,31] [--batch 64] [--log-baby 0] [--steps 10] [--warmup 1] [--rounds 5] [--leg-timeout 120] [--dry-run]

--dry-run: needs no GPU and loads no library; prints per degree the plan counts (the planner of tests/bfv_poly_model.py, which
tests/test_bfv_poly_api.py holds equal to lsa_bfv_poly_plan) and the step counts of each leg.
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
DEGREES = (15, 31)


def step_model(plan, degree):
    leaf_terms = sum(len(plan["used"][g]) for g in plan["leaves"])
    powers = len(plan["babies"]) + len(plan["giants"])
    return {"poly": {"key_switches": plan["n_mult"], "scale_downs": plan["n_mult"], "leaf_launches": plan["n_leaf_launches"]},
            "horner": {"key_switches": degree - 1, "scale_downs": degree - 1, "affine_launches": degree, "depth": degree - 1},
            "horner_mults": {"key_switches": degree - 1, "scale_downs": degree - 1},
            "plan_by_hand": {"key_switches": powers + plan["n_pairs"], "scale_downs": powers + plan["n_pairs"],
                             "affine_launches": leaf_terms + sum(1 for g in plan["leaves"] if not plan["used"][g]),
                             "additions": leaf_terms - sum(1 for g in plan["leaves"] if plan["used"][g]) + plan["n_leaves"] - 1}}


def run_degree(degree, a):
    from tests import bfv_poly_model as model
    import numpy as np
    P = params.BFV_DEFAULT[SET]
    q, p, t = P["q"], P["p"], P["t"]
    level, batch = len(q) - 1, a.batch
    rng = np.random.default_rng(degree)
    coeffs = [int(x) for x in rng.integers(1, t, degree + 1)]
    plan = model.plan(coeffs, a.log_baby)
    res = {"tool": "bench_bfv_poly", "n": N, "level": level, "q_limbs": len(q), "special_primes": len(p), "batch": batch,
           "degree": degree, "dry_run": bool(a.dry_run), "plan": {k: plan[k] for k in model.COUNTS}, "steps": step_model(plan, degree)}
    if a.dry_run:
        print(json.dumps(res))
        return

    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_BFV, BfvPolynomialPlan, DeviceContext, bfv_poly_plan
    assert bfv_poly_plan(t, coeffs, a.log_baby) == res["plan"]
    ctx = DeviceContext(ALGO_BFV, N, q, p, t)
    st = ctypes.c_void_p()
    check(lib().lsa_stream_create(ctx.h, ctypes.byref(st)))
    ctx.stream = st
    L, k = level + 1, len(p)
    beta = -(-L // k)
    mods = ctx.moduli[:L] + ctx.moduli[len(q): len(q) + k]
    key = np.empty((beta, 2, L + k, N), dtype=np.uint64)
    for j, m in enumerate(mods):
        key[:, :, j, :] = rng.integers(0, m, size=(beta, 2, N), dtype=np.uint64)
    rlk = ctx.upload_key(key, level)
    del key
    x = np.empty((batch, 2, L, N), dtype=np.uint64)
    for j in range(L):
        x[:, :, j, :] = rng.integers(0, ctx.moduli[j], size=(batch, 2, N), dtype=np.uint64)
    dx = ctx.upload(x)
    del x
    w = 2 * L * N
    S = ctx.stream
    out = ctx.alloc(batch * w)
    poly = BfvPolynomialPlan(ctx, coeffs, level, a.log_baby)
    assert poly.info()["n_mult"] == plan["n_mult"]
    m, cf = plan["m"], plan["coef"]
    # buffers of the two compositions: made once, as the operator's pool is
    acc, tmp = ctx.alloc(batch * w), ctx.alloc(batch * w)
    X = {j: ctx.alloc(batch * w) for j in plan["babies"]}
    X[1] = dx
    Y = {g: ctx.alloc(batch * w) for g in plan["giants"]}
    leaf = {g: ctx.alloc(batch * w) for g in plan["leaves"]}

    def mult(a_buf, b_buf, o_buf):
        check(lib().lsa_bfv_mult_relin(ctx.h, level, a_buf.ptr, b_buf.ptr, rlk, o_buf.ptr, batch, w, w, w, S))

    def add(a_buf, b_buf, o_buf):
        check(lib().lsa_poly_addsub(ctx.h, 0, level, 2, a_buf.ptr, b_buf.ptr, o_buf.ptr, batch, w, w, w, S))

    def leg_poly():
        poly.run(dx, batch, rlk, out=out)

    def leg_horner():
        ctx.bfv_affine_const(level, dx, coeffs[degree], coeffs[degree - 1], batch, out=acc)
        cur, other = acc, tmp
        for kk in range(degree - 2, -1, -1):
            mult(cur, dx, other)
            ctx.bfv_affine_const(level, other, 1, coeffs[kk], batch, out=other)
            cur, other = other, cur

    def leg_horner_mults():
        cur, other = acc, tmp
        for _ in range(degree - 1):
            mult(cur, dx, other)
            cur, other = other, cur

    def leg_by_hand():
        for j in plan["babies"]:
            mult(X[(j + 1) // 2], X[j // 2], X[j])
        for g in plan["giants"]:
            if g == 1:
                mult(X[m // 2], X[m // 2], Y[1])
            else:
                mult(Y[(g + 1) // 2], Y[g // 2], Y[g])
        for g in plan["leaves"]:
            used = plan["used"][g]
            if not used:
                ctx.bfv_affine_const(level, dx, 0, cf[g * m], batch, out=leaf[g])
                continue
            ctx.bfv_affine_const(level, X[used[0]], cf[g * m + used[0]], cf[g * m], batch, out=leaf[g])
            for j in used[1:]:
                ctx.bfv_affine_const(level, X[j], cf[g * m + j], 0, batch, out=tmp)
                add(leaf[g], tmp, leaf[g])
        first = True
        for g in plan["leaves"]:
            if g == 0:
                continue
            mult(leaf[g], Y[g], out if first else tmp)
            if not first:
                add(out, tmp, out)
            first = False
        if 0 in plan["leaves"]:
            add(out, leaf[0], out)

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

    legs = {"poly": leg_poly, "horner": leg_horner, "plan_by_hand": leg_by_hand, "horner_mults": leg_horner_mults}
    for fn in legs.values():
        timed(fn, a.warmup)
    ms = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, fn in legs.items():
            ms[name].append(timed(fn, a.steps))
    med = {name: statistics.median(v) for name, v in ms.items()}
    res["ms_per_call"] = {name: {"median": med[name], "min": min(v), "max": max(v)} for name, v in ms.items()}
    hand_range = max(ms["plan_by_hand"]) - min(ms["plan_by_hand"])
    res["measured"] = {"horner_over_poly": med["horner"] / med["poly"], "plan_by_hand_over_poly": med["plan_by_hand"] / med["poly"],
                       "poly_beats_plan_by_hand_by_more_than_its_range": med["plan_by_hand"] - med["poly"] > hand_range,
                       "poly_loses_to_plan_by_hand_by_more_than_its_range": med["poly"] - med["plan_by_hand"] > hand_range,
                       "poly_ct_per_s": batch / (med["poly"] / 1e3)}
    ctx.sync()
    print(json.dumps(res), flush=True)
    poly.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degrees", default=",".join(map(str, DEGREES)))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--log-baby", type=int, default=0, help="0: the planner's choice (least depth); 1..4 forces the split")
    ap.add_argument("--steps", type=int, default=10, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--leg-timeout", type=float, default=120.0)
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    for d in (int(x) for x in a.degrees.split(",")):
        run_degree(d, a)


if __name__ == "__main__":
    main()
