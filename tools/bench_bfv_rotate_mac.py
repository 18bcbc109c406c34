"""Hoisted BFV rotate-and-MAC (lsa_bfv_rotate_mac_plain_mul) against the composition it replaces: lsa_bfv_rotate_many over
the rotation elements, then lsa_bfv_mac_plain_mul over the identity term and the rotated ciphertexts.

Shapes: `--shape n14` is params.BFV_DEFAULT[16384] at the top level (6 Q + 2 P limbs), batch 64; `--shape n16` is
params.bfv_n16_chain() at level 23 (24 Q + 4 P limbs), batch 4.  `--m` column rotations by steps 1..m plus one identity term
(g = 1), i.e. m + 1 products: the diagonal (Halevi-Shoup) matrix-vector product.

Timed regions, alternated `--rounds` times in one process after `--warmup` calls of each: `--steps` calls of the fused
operator (LSA_ROTMAC_FUSED=1), of its two-step form (LSA_ROTMAC_FUSED=0) and of the composition; HIP events on the launch
stream, operator tiles on two streams as in bench.py.  Reported per form: ms per call (median over the rounds), ciphertexts
per second, the limb-transform counts and the algorithmic byte model, and whether all three results are bit-identical on
the timed data.  Inputs, plaintexts and keys are uniform random residues (the timing does not depend on them).  Prints one
JSON line.

    python tools/bench_bfv_rotate_mac.py [--shape n14|n16] [--m 4|8|16] [--batch B] [--steps 10] [--warmup 3] [--rounds 3]
                                         [--fused-only] [--dry-run]

--fused-only: warm-up and the fused calls only (a kernel trace of one form; LSA_ROTMAC_FUSED=0 in the environment traces
the two-step form).
--dry-run: the shape, the transform counts and the byte model; no GPU.
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
        P = params.BFV_DEFAULT[16384]
        return {"n": 16384, "q": P["q"], "p": P["p"], "t": P["t"], "level": len(P["q"]) - 1, "batch": 64}
    C = params.bfv_n16_chain()
    return {"n": C["n"], "q": C["q"], "p": C["p"], "t": C["t"], "level": len(C["q"]) - 1, "batch": 4}


def transform_counts(L, k, m):
    """limb transforms per ciphertext for m rotation terms and one identity term"""
    comp = L + m * (2 * (L + k)) + (m + 1) * 2 * L + 2 * L   # NTT(c1); ModDown on coefficients; MAC forward; one inverse
    fused = 2 * L + m * (2 * k + 2 * L) + 2 * L              # NTT(c0, c1); P rows + conversion per term; one inverse
    return {"per_rotation_term_composition": 2 * (L + k) + 2 * L, "per_rotation_term_fused": 2 * k + 2 * L,
            "per_ct_composition": comp, "per_ct_fused": fused}


def byte_model(n, L, k, m):
    """algorithmic limb streams (one limb of N words read or written = one stream) of ONE ciphertext.  Both forms:
    decomposition 3*beta*T, per key MAC (beta*T digits + 2*beta*T key in, 2T out) and the P -> Q conversion (2k in, 2L out),
    one inverse transform of the sum (4L).  Composition: forward NTT of c1 (2L); per key the coefficient-domain ModDown
    (2T rows transformed, 4T; tail: acc, conv 2L each + c0 L in, 2L out); per product the forward transform with the pt_mul
    epilogue (2L in; pt 2L, running sum 2L in; 2L out).  Fused: forward NTT of c0 and c1 (4L); per key the P rows (4k) and the
    conversion's forward transform whose store reads acc 2L, base L, pt 2L, running sum 2L and writes 2L; the identity term
    reads NTT(ct) 2L, pt 2L, the sum 2L and writes 2L."""
    T, beta = L + k, (L + k - 1) // k
    decomp = 3 * beta * T
    mac = 3 * beta * T + 2 * T
    conv = 2 * k + 2 * L
    comp = 2 * L + decomp + m * (mac + 4 * T + conv + 7 * L) + (m + 1) * 8 * L + 4 * L
    fused = 4 * L + decomp + m * (mac + 4 * k + conv + 2 * L + 9 * L) + 8 * L + 4 * L
    w = 8 * n
    return {"streams_composition_per_ct": comp, "streams_fused_per_ct": fused, "bytes_composition_per_ct": comp * w,
            "bytes_fused_per_ct": fused * w, "byte_ratio_composition_over_fused": comp / fused}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["n14", "n16"], default="n14")
    ap.add_argument("--m", type=int, default=8, choices=[4, 8, 16])
    ap.add_argument("--batch", type=int, default=0, help="ciphertexts per call (0 = the shape's default)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--dry-run", action="store_true", help="print the shape and the models; no GPU")
    args = ap.parse_args()
    S = shape_of(args.shape)
    n, q, p, t, lvl = S["n"], S["q"], S["p"], S["t"], S["level"]
    L, k = lvl + 1, len(p)
    B = args.batch or S["batch"]
    m = args.m
    els = [pow(5, s, 2 * n) for s in range(1, m + 1)]
    terms = [1] + els
    model, counts = byte_model(n, L, k, m), transform_counts(L, k, m)
    shape = {"shape": args.shape, "ring_degree": n, "level": lvl, "q_limbs": L, "special_primes": k, "t": t, "batch": B,
             "rotations": m, "identity_terms": 1, "galois_elements": terms}
    if args.dry_run:
        print(json.dumps({"config": shape, "transforms": counts, "byte_model": model}))
        return 0

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bfv_rotate_mac.py needs an MI355X: no HIP device visible and there is no CPU fallback")
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    L_ = lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = DeviceContext(ALGO_BFV, n, q, p, t, device=0)
    stream = torch.cuda.current_stream()
    ctx.stream = ctypes.c_void_p(stream.cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1406 if args.shape == "n14" else 1606)

    def uniform(prefix, mods):
        out = torch.empty(*prefix, len(mods), n, dtype=torch.int64, device=dev)
        for i, mod in enumerate(mods):
            out[..., i, :] = torch.randint(0, mod, (*prefix, n), dtype=torch.int64, device=dev, generator=gen)
        return out

    beta = (L + k - 1) // k
    key_ts = [uniform((beta, 2), q[:L] + p) for _ in els]
    torch.cuda.synchronize()
    keys = []
    for kt in key_ts:
        assert kt.numel() * 8 == ctx.key_bytes(lvl)
        keys.append(ctx.adopt_key(kt.data_ptr(), lvl))
    a = uniform((B, 2), q[:L])
    pts = [uniform((B,), q[:L]) for _ in terms]
    rotated = [torch.empty(B, 2, L, n, dtype=torch.int64, device=dev) for _ in els]
    res = {f: torch.empty(B, 2, L, n, dtype=torch.int64, device=dev) for f in ("fused", "two_step", "composition")}
    s_ct, s_pt = 2 * L * n, L * n
    nt = m + 1
    c_terms = (ctypes.c_uint64 * nt)(*terms)
    c_tkeys = (ctypes.c_void_p * nt)(*([None] + [kh.value for kh in keys]))
    c_pts = (ctypes.c_void_p * nt)(*[x.data_ptr() for x in pts])
    c_spts = (ctypes.c_longlong * nt)(*([s_pt] * nt))
    c_els = (ctypes.c_uint64 * m)(*els)
    c_keys = (ctypes.c_void_p * m)(*[kh.value for kh in keys])
    c_rot = (ctypes.c_void_p * m)(*[x.data_ptr() for x in rotated])
    c_cts = (ctypes.c_void_p * nt)(*([a.data_ptr()] + [x.data_ptr() for x in rotated]))
    c_scts = (ctypes.c_longlong * nt)(*([s_ct] * nt))
    check(L_.lsa_set_dual_stream(ctx.h, 1))
    env0 = os.environ.get("LSA_ROTMAC_FUSED")

    def run_op(form):
        def fn():
            if not args.fused_only:   # (--fused-only keeps the environment's choice)
                os.environ["LSA_ROTMAC_FUSED"] = "1" if form == "fused" else "0"
            check(L_.lsa_bfv_rotate_mac_plain_mul(ctx.h, lvl, a.data_ptr(), nt, c_terms, c_tkeys, c_pts, c_spts, None, 0,
                                                  res[form].data_ptr(), B, s_ct, s_ct, ctx.stream))
        return fn

    def run_composition():
        check(L_.lsa_bfv_rotate_many(ctx.h, lvl, a.data_ptr(), m, c_els, c_keys, c_rot, B, s_ct, s_ct, ctx.stream))
        check(L_.lsa_bfv_mac_plain_mul(ctx.h, lvl, nt, c_cts, c_scts, c_pts, c_spts, None, 0, res["composition"].data_ptr(), B,
                                       s_ct, ctx.stream))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    fns = {"fused": run_op("fused")} if args.fused_only else {"fused": run_op("fused"), "two_step": run_op("two_step"),
                                                              "composition": run_composition}
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {f: [] for f in fns}
    for _ in range(args.rounds):
        for f, fn in fns.items():
            ms[f].append(timed(fn))
    if env0 is None:
        os.environ.pop("LSA_ROTMAC_FUSED", None)
    else:
        os.environ["LSA_ROTMAC_FUSED"] = env0
    med = {f: statistics.median(v) for f, v in ms.items()}
    line = {"metric": "bfv_rotate_mac_fused_over_composition" if not args.fused_only else "bfv_rotate_mac_fused_only",
            "config": shape, "transforms": counts, "byte_model": model, "steps": args.steps, "warmup": args.warmup,
            "rounds": args.rounds, "data": "synthetic",
            "timing": "HIP events on the launch stream after warm-up; the forms alternated, medians of the rounds"}
    for f in fns:
        line[f + "_ms"] = med[f]
        line[f + "_ms_rounds"] = ms[f]
        line[f + "_ct_per_s"] = 1e3 * B / med[f]
    line["fused_algorithmic_GBps"] = model["bytes_fused_per_ct"] * B / (med["fused"] * 1e6)
    ok = True
    if not args.fused_only:
        line["value"] = med["composition"] / med["fused"]
        line["unit"] = "x"
        line["two_step_over_composition"] = med["composition"] / med["two_step"]
        line["fused_over_two_step"] = med["two_step"] / med["fused"]
        line["composition_algorithmic_GBps"] = model["bytes_composition_per_ct"] * B / (med["composition"] * 1e6)
        ok = torch.equal(res["fused"], res["composition"]) and torch.equal(res["two_step"], res["composition"])
        line["bit_identical"] = ok
    else:
        line["value"] = 1e3 * B / med["fused"]
        line["unit"] = "ct/s"
    print(json.dumps(line), flush=True)
    for kh in keys:
        ctx.destroy_key(kh)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
