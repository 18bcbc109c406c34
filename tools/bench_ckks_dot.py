"""CKKS encrypted inner product (lsa_ckks_dot) at N = 2^16 on the headline chain (params.CKKS_DEFAULT[65536] cut to 13 Q limbs +
4 P, level 12), n in {2, 4, 8, 16, 32} pairs of ciphertexts, three legs per n in one process:

(a) lsa_ckks_dot: one k_tensor_sum pass over the pairs, ONE key switch, ONE rescale;
(b) the lazy composition from the existing entry points: n x lsa_ckks_mult, n - 1 x lsa_poly_addsub over three polynomials,
    lsa_ckks_relin, lsa_ckks_rescale -- the same words as (a);
(c) the eager form: n x lsa_ckks_mult_relin_rescale plus n - 1 additions (n key switches; different words).

Legs (b) and (c) call only entry points that exist without lsa_ckks_dot: they are the yardstick, measured on the same box in the
same process.  Inputs and the key are uniform random residues; timing does not depend on them.  After `--warmup` calls of each,
the legs are alternated `--rounds` times; HIP events on the launch stream; per leg the median, the minimum and the maximum of the
rounds.  Every timed call of a leg runs under `--leg-timeout` seconds: when a call does not come back the process dumps its
stack and exits.  Prints one JSON line.

    python tools/bench_ckks_dot.py [--terms 2,4,8,16,32] [--batch B] [--steps 3] [--warmup 1] [--rounds 5] [--leg-timeout 120] [--dry-run]

--dry-run: needs no GPU; prints the limb-stream model of each leg (rows of N words read and written per ciphertext of the
batch) and the ratios it predicts.

The model (two-pass transforms, fused key MAC, fused tails; L = level + 1, k special primes, T = L + k, beta = ceil(L / k),
E = beta T - L extended rows; the key's rows are shared by the whole batch and not counted):
  tensor              7L                      k_tensor: four operand rows read, three written
  tensor sum          4L n + 3L               k_tensor_sum (+ 6L for every accumulating launch past LSA_DOT_MAX_TERMS pairs)
  addition            3 rows per limb         k_elementwise
  decompose + MAC     4L + (L + E) + 2E + (E + L + 2T)      inverse transform, ModUp, extension first pass, second pass + MAC
  ModDown             8k + (2k + 2L) + 12L                    P rows out of the NTT domain, conversion, forward transform + tail
  ModDown + rescale   4(2k + 2) + (2k + 2L) + 8 + 8 + 14(L - 1)   the merged tail (KsOut::RESCALE) with d0 / d1 as base
  rescale             4 + 8 + 10(L - 1)       last rows copied and transformed, one forward transform with fused ends
  folded HMult        5L + (L + E) + 2E + (E + 4L + 2T) + 4(2k + 2) + (2k + 2L) + 6 + 12(L - 1)   lsa_ckks_mult_relin_rescale's default
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

LEVEL, BATCH = 12, 16
TERMS = (2, 4, 8, 16, 32)
DOT_MAX_TERMS = 16   # LSA_DOT_MAX_TERMS (csrc/tensor_sum.h)


def stream_model(n, level, k, max_terms=DOT_MAX_TERMS):
    """limb streams (rows read + rows written) per ciphertext of the three legs for n terms"""
    L = level + 1
    T, beta = L + k, -(-L // k)
    E = beta * T - L
    mac = 4 * L + (L + E) + 2 * E + (E + L + 2 * T)
    moddown = 8 * k + (2 * k + 2 * L) + 12 * L
    moddown_rescale = 4 * (2 * k + 2) + (2 * k + 2 * L) + 8 + 8 + 14 * (L - 1)
    rescale = 4 + 8 + 10 * (L - 1)
    hmult_folded = 5 * L + (L + E) + 2 * E + (E + 4 * L + 2 * T) + 4 * (2 * k + 2) + (2 * k + 2 * L) + 6 + 12 * (L - 1)
    launches = -(-n // max_terms)
    a = 4 * L * n + 3 * L + 6 * L * (launches - 1) + mac + moddown_rescale
    b = 7 * L * n + 9 * L * (n - 1) + mac + moddown + rescale
    c = hmult_folded * n + 6 * (L - 1) * (n - 1)
    return {"dot": a, "lazy_composition": b, "eager": c, "predicted_lazy_over_dot": b / a, "predicted_eager_over_dot": c / a,
            "tensor_sum_launches": launches}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--terms", default=",".join(map(str, TERMS)))
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--leg-timeout", type=float, default=120.0)
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    terms = [int(t) for t in a.terms.split(",")]
    P = params.CKKS_DEFAULT[65536]
    n, q, p, batch = 65536, P["q"][:13], P["p"][:4], a.batch
    res = {"tool": "bench_ckks_dot", "n": n, "level": LEVEL, "special_primes": len(p), "batch": batch, "dry_run": bool(a.dry_run),
           "terms": terms, "streams_per_ct": {str(t): stream_model(t, LEVEL, len(p)) for t in terms}}
    if a.dry_run:
        print(json.dumps(res))
        return

    import numpy as np
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    rng = np.random.default_rng(1)
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
    w2, w3, wo = 2 * L * n, 3 * L * n, 2 * LEVEL * n
    out = ctx.alloc(batch * wo)
    d3a, d3b, r2 = ctx.alloc(batch * w3), ctx.alloc(batch * w3), ctx.alloc(batch * w2)
    ea, eb = ctx.alloc(batch * wo), ctx.alloc(batch * wo)
    S = ctx.stream

    def leg_dot(t):
        ctx.ckks_dot(LEVEL, A[:t], B[:t], rlk, batch, out=out)

    def leg_lazy(t):
        check(lib().lsa_ckks_mult(ctx.h, LEVEL, A[0].ptr, B[0].ptr, d3a.ptr, batch, w2, w2, w3, S))
        for i in range(1, t):
            check(lib().lsa_ckks_mult(ctx.h, LEVEL, A[i].ptr, B[i].ptr, d3b.ptr, batch, w2, w2, w3, S))
            check(lib().lsa_poly_addsub(ctx.h, 0, LEVEL, 3, d3a.ptr, d3b.ptr, d3a.ptr, batch, w3, w3, w3, S))
        check(lib().lsa_ckks_relin(ctx.h, LEVEL, d3a.ptr, rlk, r2.ptr, batch, w3, w2, S))
        check(lib().lsa_ckks_rescale(ctx.h, LEVEL, 2, r2.ptr, out.ptr, batch, w2, wo, S))

    def leg_eager(t):
        check(lib().lsa_ckks_mult_relin_rescale(ctx.h, LEVEL, A[0].ptr, B[0].ptr, rlk, ea.ptr, batch, w2, w2, wo, S))
        for i in range(1, t):
            check(lib().lsa_ckks_mult_relin_rescale(ctx.h, LEVEL, A[i].ptr, B[i].ptr, rlk, eb.ptr, batch, w2, w2, wo, S))
            check(lib().lsa_poly_addsub(ctx.h, 0, LEVEL - 1, 2, ea.ptr, eb.ptr, ea.ptr, batch, wo, wo, wo, S))

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

    legs = {"dot": leg_dot, "lazy_composition": leg_lazy, "eager": leg_eager}
    res["ms_per_call"], res["ms_rounds"], res["measured"] = {}, {}, {}
    for t in terms:
        for fn in legs.values():
            timed(fn, t, a.warmup)
        ms = {name: [] for name in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                ms[name].append(timed(fn, t, a.steps))
        med = {name: statistics.median(v) for name, v in ms.items()}
        res["ms_rounds"][str(t)] = ms
        res["ms_per_call"][str(t)] = {name: {"median": med[name], "min": min(v), "max": max(v)} for name, v in ms.items()}
        lazy_range = max(ms["lazy_composition"]) - min(ms["lazy_composition"])
        res["measured"][str(t)] = {"lazy_over_dot": med["lazy_composition"] / med["dot"], "eager_over_dot": med["eager"] / med["dot"],
                                   "dot_beats_lazy_by_more_than_its_range": med["lazy_composition"] - med["dot"] > lazy_range,
                                   "dot_ct_per_s": batch / (med["dot"] / 1e3)}
    # k_tensor_sum on its own: the library's sampled event timing of the tensor kind during one call at the largest n
    check(lib().lsa_profile_begin(ctx.h, 1))
    leg_dot(nmax)
    ctx.sync()
    check(lib().lsa_profile_end(ctx.h))
    tms, tby, smp, lau = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong(), ctypes.c_longlong()
    check(lib().lsa_profile_read(ctx.h, 3, ctypes.byref(tms), ctypes.byref(tby), ctypes.byref(smp), ctypes.byref(lau)))
    res["tensor_sum_kind"] = {"terms": nmax, "ms": tms.value, "launches": lau.value,
                              "algorithmic_bytes_per_s": tby.value / (tms.value / 1e3) if tms.value else 0.0}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
