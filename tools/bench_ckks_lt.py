"""CKKS linear transform (lsa_ckks_linear_transform) on D dense diagonals 0..D-1: the double-hoisted operator, the same with
LSA_LT_BLOCKED_MAC=0 (inner sums by one multiply-accumulate launch per giant step), and the composition a caller had before
the operator: lsa_ckks_rotate_many over the D-1 non-zero diagonals (one decomposition, one division by P per rotation), a
multiply-add per term, lsa_ckks_rescale.

The C-ABI has no CKKS ciphertext x plaintext kernel, so the composition leg times lsa_ckks_rotate_many + lsa_ckks_rescale only
and leaves the caller's D multiply-adds out: `composition_lower_bound` is a LOWER bound of that composition's time.
--single-hoisted adds the library's own evaluator with double_hoist = 0 (baby-step / giant-step, one division per rotation).

Shapes: `--shape n16` is params.CKKS_DEFAULT[65536] cut to 13 Q limbs + 4 P at level 12 (the headline chain), `--shape n14`
params.CKKS_DEFAULT[16384] at its top level (10 Q + 2 P).  Inputs and keys are uniform random residues, the diagonals uniform
in [-1/D, 1/D]; timing does not depend on them.  The legs are alternated `--rounds` times in one process after `--warmup`
calls of each; HIP events on the launch stream; medians over the rounds.  Prints one JSON line.

    python tools/bench_ckks_lt.py [--shape n14|n16] [--diagonals D] [--batch B] [--steps 5] [--warmup 2] [--rounds 3]
                                  [--ratio 2.0] [--giant-ab] [--single-hoisted] [--dry-run]

--giant-ab: also times the operator with LSA_LT_GIANT_SCATTER=0 and =1 (giant-step rotations by MAC + permutation kernel or by
the accumulating scatter of the key MAC).
--dry-run: needs no GPU; prints n1, the baby / giant step counts, divisions by P and the limb-stream model of the inner sums
(per limb piece; fallback: terms*(2+1) + 2*ng; blocked: 2*nb*ceil(ng/8) + terms + 2*ng*ceil(nb/8)).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lattisense_amd import params  # noqa: E402


def shape_of(name):
    if name == "n14":
        P = params.CKKS_DEFAULT[16384]
        return {"n": 16384, "q": P["q"], "p": P["p"], "level": len(P["q"]) - 1, "batch": 64}
    P = params.CKKS_DEFAULT[65536]
    return {"n": 65536, "q": P["q"][:13], "p": P["p"], "level": 12, "batch": 16}


def model(n, d, ratio):
    from lattisense_amd.device import plan_rotations
    period = n // 2
    n1, rot = plan_rotations(period, list(range(d)), ratio)
    if n1 == 0:
        babies, giants = sorted(set(range(d))), [0]
    else:
        babies = sorted({k % n1 for k in range(d)})
        giants = sorted({(k // n1) * n1 for k in range(d)})
    nb, ng = len(babies), len(giants)
    cd = lambda a, b: -(-a // b)
    return {"n1": n1, "babies": nb, "giants": ng, "rotations": len(rot),
            "divisions_by_p": {"operator": ng + 1 if n1 else len(rot), "composition": d - 1},
            "inner_sum_streams": {"fallback": d * 3 + 2 * ng, "blocked": 2 * nb * cd(ng, 8) + d + 2 * ng * cd(nb, 8)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["n14", "n16"], default="n14")
    ap.add_argument("--diagonals", type=int, default=64)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ratio", type=float, default=2.0)
    ap.add_argument("--giant-ab", action="store_true")
    ap.add_argument("--single-hoisted", action="store_true")
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    S = shape_of(a.shape)
    n, level, d = S["n"], S["level"], a.diagonals
    batch = a.batch or S["batch"]
    assert 1 <= d <= n // 2
    res = {"tool": "bench_ckks_lt", "shape": a.shape, "n": n, "level": level, "q_limbs": level + 1, "p_limbs": len(S["p"]),
           "diagonals": d, "batch": batch, "ratio": a.ratio, "dry_run": bool(a.dry_run)}
    res.update(model(n, d, a.ratio))
    if a.dry_run:
        print(json.dumps(res))
        return

    import numpy as np
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_CKKS, DeviceContext, LinearTransformPlan
    ctx = DeviceContext(ALGO_CKKS, n, S["q"], S["p"])
    st = ctypes.c_void_p()
    check(lib().lsa_stream_create(ctx.h, ctypes.byref(st)))
    ctx.stream = st
    rng = np.random.default_rng(1)
    period = n // 2
    diags = {k: (rng.uniform(-1, 1, period) + 1j * rng.uniform(-1, 1, period)) / d for k in range(d)}
    plan_dh = LinearTransformPlan(ctx, level, diags, ratio=a.ratio, double_hoist=True)
    plan_sh = LinearTransformPlan(ctx, level, diags, ratio=a.ratio, double_hoist=False) if a.single_hoisted else None
    assert plan_dh.n1 == res["n1"]
    L, k = level + 1, len(S["p"])
    beta = -(-L // k)
    mods = ctx.moduli[:L] + ctx.moduli[len(S["q"]): len(S["q"]) + k]
    key = np.empty((beta, 2, L + k, n), dtype=np.uint64)
    for j, q in enumerate(mods):
        key[:, :, j, :] = rng.integers(0, q, size=(beta, 2, n), dtype=np.uint64)
    one_key = ctx.upload_key(key, level)          # every element gets the same words: the timing does not depend on them
    del key
    glk = {e: one_key for e in plan_dh.galois_elements}
    comp_elements = [pow(5, r, 2 * n) for r in range(1, d)]
    comp_outs = [ctx.alloc(batch * 2 * L * n) for _ in comp_elements]      # allocated once, outside the timed region
    c_els = (ctypes.c_uint64 * max(1, d - 1))(*comp_elements)
    c_keys = (ctypes.c_void_p * max(1, d - 1))(*([one_key.value] * (d - 1)))
    c_outs = (ctypes.c_void_p * max(1, d - 1))(*[o.ptr for o in comp_outs])
    x = np.empty((batch, 2, L, n), dtype=np.uint64)
    for j in range(L):
        x[:, :, j, :] = rng.integers(0, ctx.moduli[j], size=(batch, 2, n), dtype=np.uint64)
    xin = ctx.upload(x)
    out = ctx.alloc(batch * 2 * level * n)

    legs = [("operator", plan_dh, {}), ("blocked_mac_off", plan_dh, {"LSA_LT_BLOCKED_MAC": "0"}), ("composition_lower_bound", None, {})]
    if a.single_hoisted:
        legs.append(("single_hoisted", plan_sh, {}))
    if a.giant_ab:
        legs += [("giant_permute", plan_dh, {"LSA_LT_GIANT_SCATTER": "0"}), ("giant_scatter", plan_dh, {"LSA_LT_GIANT_SCATTER": "1"})]
    switches = ("LSA_LT_BLOCKED_MAC", "LSA_LT_GIANT_SCATTER")

    def call(plan, env, times):
        saved = {s: os.environ.pop(s, None) for s in switches}
        os.environ.update(env)
        try:
            for _ in range(times):
                if plan is None:
                    check(lib().lsa_ckks_rotate_many(ctx.h, level, xin.ptr, d - 1, c_els, c_keys, c_outs, batch, 2 * L * n, 2 * L * n,
                                                     ctx.stream))
                    first = comp_outs[0] if comp_outs else xin
                    check(lib().lsa_ckks_rescale(ctx.h, level, 2, first.ptr, out.ptr, batch, 2 * L * n, 2 * level * n, ctx.stream))
                else:
                    plan.run(xin, batch, glk, rescale=True, out=out)
        finally:
            for s in switches:
                os.environ.pop(s, None)
                if saved[s] is not None:
                    os.environ[s] = saved[s]

    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib().lsa_event_create(ctx.h, ctypes.byref(e0)))
    check(lib().lsa_event_create(ctx.h, ctypes.byref(e1)))
    words = {}
    for name, plan, env in legs:
        call(plan, env, a.warmup)
        ctx.sync()
        words[name] = ctx.download(out, (batch, 2, level, n))
    # the switches change no word; the single-hoisted form rounds its divisions by P elsewhere and is not compared
    res["identical"] = all(np.array_equal(words["operator"], words[name]) for name, plan, _ in legs if plan is plan_dh)
    ms = {name: [] for name, _, _ in legs}
    for _ in range(a.rounds):
        for name, plan, env in legs:
            check(lib().lsa_event_record(ctx.h, e0, ctx.stream))
            call(plan, env, a.steps)
            check(lib().lsa_event_record(ctx.h, e1, ctx.stream))
            ctx.sync()
            t = ctypes.c_float()
            check(lib().lsa_event_elapsed_ms(ctx.h, e0, e1, ctypes.byref(t)))
            ms[name].append(t.value / a.steps)
    res["ms_per_call"] = {name: statistics.median(v) for name, v in ms.items()}
    res["ms_rounds"] = ms
    res["ct_per_s"] = {name: batch / (v / 1e3) for name, v in res["ms_per_call"].items()}
    print(json.dumps(res))
    plan_dh.close()
    if plan_sh is not None:
        plan_sh.close()


if __name__ == "__main__":
    main()
