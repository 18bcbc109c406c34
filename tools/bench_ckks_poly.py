"""CKKS polynomial evaluation (lsa_ckks_poly_eval) of a dense Chebyshev polynomial at N = 2^16 on the headline chain
(params.CKKS_DEFAULT[65536] cut to 13 Q limbs + 4 P, level 12), three readings in one process:

1. the operator at the planner's log_baby and at log_baby = 1 (the binary splitting bootstrapping's EvalMod runs);
2. each of them divided by the sum, over its ciphertext multiplications, of lsa_ckks_mult_relin_rescale's time at that
   multiplication's level, measured here on the same box: what the leaves, the unfused odd powers and the bookkeeping add;
3. the element-wise launches of the planner's operator (k_poly_lincomb, the additions and the row copies; the library's own
   sampled event timing), algorithmic bytes per second next to lsa_probe_copy's.

Inputs and the key are uniform random residues; timing does not depend on them.  The legs are alternated `--rounds` times after
`--warmup` calls of each; HIP events on the launch stream; medians over the rounds.  Prints one JSON line.

    python tools/bench_ckks_poly.py [--degree 31|63] [--batch B] [--steps 3] [--warmup 1] [--rounds 3] [--log-baby b] [--dry-run]

--dry-run: needs no GPU; prints depth, log_baby, multiplications (with their levels), leaves and leaf launches of both plans.
"""
import argparse
import collections
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lattisense_amd import params  # noqa: E402

LEVEL, BATCH = 12, 16


def plans_of(coeffs, log_baby):
    """the library's counts, with the level of every multiplication from the planner model (tests/poly_model.py)"""
    from lattisense_amd.device import plan_polynomial
    from tests import poly_model as pm
    out = {}
    for name, b in (("planner", log_baby), ("binary", 1)):
        pl = plan_polynomial(coeffs, LEVEL, "chebyshev", b)
        st = pm.Structure(coeffs, "chebyshev", pl["log_baby"])
        assert st.mults == pl["mults"] and len(st.mult_levels) == pl["mults"]
        pl["mult_levels"] = dict(sorted(collections.Counter(LEVEL + lv for lv in st.mult_levels).items()))
        out[name] = pl
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree", type=int, default=31)
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log-baby", type=int, default=0)
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    import numpy as np
    rng = np.random.default_rng(1)
    coeffs = rng.uniform(-1, 1, a.degree + 1) / (a.degree + 1)
    P = params.CKKS_DEFAULT[65536]
    n, q, p, batch = 65536, P["q"][:13], P["p"], a.batch
    plans = plans_of(coeffs, a.log_baby)
    res = {"tool": "bench_ckks_poly", "n": n, "level": LEVEL, "degree": a.degree, "batch": batch, "dry_run": bool(a.dry_run),
           "depth": plans["planner"]["depth"], "plans": plans}
    if a.dry_run:
        print(json.dumps(res))
        return

    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_CKKS, DeviceContext, PolynomialPlan
    ctx = DeviceContext(ALGO_CKKS, n, q, p)
    st = ctypes.c_void_p()
    check(lib().lsa_stream_create(ctx.h, ctypes.byref(st)))
    ctx.stream = st
    L, k = LEVEL + 1, len(p)
    beta = -(-L // k)
    mods = ctx.moduli[:L] + ctx.moduli[len(q): len(q) + k]
    key = np.empty((beta, 2, L + k, n), dtype=np.uint64)
    for j, m in enumerate(mods):
        key[:, :, j, :] = rng.integers(0, m, size=(beta, 2, n), dtype=np.uint64)
    rlk = ctx.upload_key(key, LEVEL)
    del key
    x = np.empty((batch, 2, L, n), dtype=np.uint64)
    for j in range(L):
        x[:, :, j, :] = rng.integers(0, ctx.moduli[j], size=(batch, 2, n), dtype=np.uint64)
    xin = ctx.upload(x)
    scale = float(2 ** 45)
    ops = {name: PolynomialPlan(ctx, coeffs, LEVEL, scale, log_baby=plans[name]["log_baby"]) for name in ("planner", "binary")}
    lo = ops["planner"].level_out + 1
    out = ctx.alloc(batch * 2 * L * n)
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib().lsa_event_create(ctx.h, ctypes.byref(e0)))
    check(lib().lsa_event_create(ctx.h, ctypes.byref(e1)))

    def timed(fn, steps):
        check(lib().lsa_event_record(ctx.h, e0, ctx.stream))
        for _ in range(steps):
            fn()
        check(lib().lsa_event_record(ctx.h, e1, ctx.stream))
        ctx.sync()
        t = ctypes.c_float()
        check(lib().lsa_event_elapsed_ms(ctx.h, e0, e1, ctypes.byref(t)))
        return t.value / steps

    levels = sorted({lv for pl in plans.values() for lv in pl["mult_levels"]})
    legs = {name: (lambda pl=pl: pl.run(xin, batch, rlk, out=out)) for name, pl in ops.items()}
    for lv in levels:   # operands: the leading rows of the level-12 input, as the operator's own multiplications read them
        legs["mult_l%d" % lv] = (lambda lv=lv: check(lib().lsa_ckks_mult_relin_rescale(
            ctx.h, lv, xin.ptr, xin.ptr, rlk, out.ptr, batch, 2 * L * n, 2 * L * n, 2 * lv * n, ctx.stream)))
    nwords = batch * 2 * L * n
    legs["probe_copy"] = lambda: check(lib().lsa_probe_copy(ctx.h, out.ptr, xin.ptr, nwords, ctx.stream))
    for fn in legs.values():
        timed(fn, a.warmup)
    ms = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, fn in legs.items():
            ms[name].append(timed(fn, a.steps))
    med = {name: statistics.median(v) for name, v in ms.items()}
    res["ms_per_call"] = med
    res["ms_rounds"] = ms
    res["speedup_planner_over_binary"] = med["binary"] / med["planner"]
    res["mult_count_ratio"] = plans["planner"]["mults"] / plans["binary"]["mults"]
    for name in ops:
        mult_ms = sum(cnt * med["mult_l%d" % lv] for lv, cnt in plans[name]["mult_levels"].items())
        res[name + "_over_its_multiplications"] = med[name] / mult_ms
    res["probe_copy_bytes_per_s"] = 16.0 * nwords / (med["probe_copy"] / 1e3)
    # k_poly_lincomb's share, from the library's sampled element-wise timings of the planner's operator
    check(lib().lsa_profile_begin(ctx.h, 1))
    ops["planner"].run(xin, batch, rlk, out=out)
    ctx.sync()
    check(lib().lsa_profile_end(ctx.h))
    tms, tby, smp, lau = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong(), ctypes.c_longlong()
    check(lib().lsa_profile_read(ctx.h, 4, ctypes.byref(tms), ctypes.byref(tby), ctypes.byref(smp), ctypes.byref(lau)))
    res["elementwise_kind"] = {"ms": tms.value, "algorithmic_bytes_per_s": tby.value / (tms.value / 1e3) if tms.value else 0.0,
                               "launches": lau.value}
    res["out_words"] = batch * 2 * lo * n
    print(json.dumps(res))
    for pl in ops.values():
        pl.close()


if __name__ == "__main__":
    main()
