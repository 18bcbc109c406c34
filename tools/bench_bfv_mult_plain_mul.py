"""BFV ct x pt_mul (lsa_bfv_mult_plain_mul / lsa_bfv_mac_plain_mul): the fused form (the Montgomery product on the store of
the forward transform's last pass) against the unfused one (LSA_PTMUL_FUSED=0: forward transform, k_mont_muladd, inverse
transform), in one process.

Shapes: `--shape n14` is params.BFV_DEFAULT[16384] at its top level (6 Q limbs), batch 256; `--shape n16` is
params.bfv_n16_chain() at level 23 (24 Q limbs), batch 8.  `--op mult` multiplies each ciphertext by its plaintext;
`--op mac` sums `--terms` products plus a partial-sum ciphertext (the task graph's cmpac_sum).

Timed regions, alternated `--rounds` times after `--warmup` calls of each form: `--steps` calls of the operator on `--batch`
ciphertexts; HIP events on the launch stream, operator tiles on two streams as in bench.py.  Reported: ciphertexts (outputs)
per second of both forms (median over the rounds), their ratio, the algorithmic byte model and TB/s, and whether both forms
gave bit-identical results on the timed data (uniform random residues: the timing does not depend on them).  One JSON line.

    python tools/bench_bfv_mult_plain_mul.py [--shape n14|n16] [--op mult|mac] [--terms 16] [--batch B] [--steps 10]
                                             [--warmup 3] [--rounds 3] [--dry-run]

--dry-run: the shape and the byte model; no GPU.
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
        return {"n": 16384, "q": P["q"], "p": P["p"], "t": P["t"], "level": len(P["q"]) - 1, "batch": 256}
    C = params.bfv_n16_chain()
    return {"n": C["n"], "q": C["q"], "p": C["p"], "t": C["t"], "level": 23, "batch": 8}


def byte_model(n, L, op, terms):
    """algorithmic limb streams (one limb of N words read or written = one stream) per output ciphertext, two-pass transforms.
    A forward or inverse pass over both polys reads 2 and writes 2 streams per limb.  Fused: the last forward pass also reads
    the plaintext limb (1) and, from the second term on, the running sum (2).  Unfused: the forward transform's two passes
    (8), then k_mont_muladd reads the transform (2), the plaintext (1), the running sum (2, from the second term on) and
    writes (2).  Both: one inverse transform (8) and, for a MAC, the partial-sum add (2 + 2 in, 2 out)."""
    k = 1 if op == "mult" else terms
    fused = (4 + 5) + (k - 1) * (4 + 5 + 2) + 8
    unfused = (8 + 5) + (k - 1) * (8 + 7) + 8
    if op == "mac":
        fused += 6
        unfused += 6
    w = 8 * n * L
    return {"streams_per_limb_fused": fused, "streams_per_limb_unfused": unfused, "bytes_fused_per_ct": fused * w,
            "bytes_unfused_per_ct": unfused * w, "byte_ratio_unfused_over_fused": unfused / fused}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["n14", "n16"], default="n14")
    ap.add_argument("--op", choices=["mult", "mac"], default="mult")
    ap.add_argument("--terms", type=int, default=16)
    ap.add_argument("--batch", type=int, default=0, help="ciphertexts per call (0 = the shape's default)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dry-run", action="store_true", help="print the shape and the byte model; no GPU")
    args = ap.parse_args()
    S = shape_of(args.shape)
    n, q, p, t, lvl = S["n"], S["q"], S["p"], S["t"], S["level"]
    L = lvl + 1
    B = args.batch or S["batch"]
    k = 1 if args.op == "mult" else args.terms
    model = byte_model(n, L, args.op, k)
    shape = {"shape": args.shape, "ring_degree": n, "level": lvl, "q_limbs": L, "t": t, "batch": B, "op": args.op, "terms": k}
    if args.dry_run:
        print(json.dumps({"config": shape, "byte_model": model}))
        return 0

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bfv_mult_plain_mul.py needs an MI355X: no HIP device visible and there is no CPU fallback")
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    L_ = lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = DeviceContext(ALGO_BFV, n, q, p, t, device=0)
    stream = torch.cuda.current_stream()
    ctx.stream = ctypes.c_void_p(stream.cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1414 if args.shape == "n14" else 1616)

    def uniform(prefix, mods):
        out = torch.empty(*prefix, len(mods), n, dtype=torch.int64, device=dev)
        for i, mod in enumerate(mods):
            out[..., i, :] = torch.randint(0, mod, (*prefix, n), dtype=torch.int64, device=dev, generator=gen)
        return out

    cts = [uniform((B, 2), q[:L]) for _ in range(k)]
    pts = [uniform((B,), q[:L]) for _ in range(k)]
    partial = uniform((B, 2), q[:L])
    outs = {f: torch.empty(B, 2, L, n, dtype=torch.int64, device=dev) for f in ("1", "0")}
    s_ct, s_pt = 2 * L * n, L * n
    check(L_.lsa_set_dual_stream(ctx.h, 1))
    c_cts = (ctypes.c_void_p * k)(*[x.data_ptr() for x in cts])
    c_scts = (ctypes.c_longlong * k)(*([s_ct] * k))
    c_pts = (ctypes.c_void_p * k)(*[x.data_ptr() for x in pts])
    c_spts = (ctypes.c_longlong * k)(*([s_pt] * k))

    def run(fused):
        os.environ["LSA_PTMUL_FUSED"] = fused   # read per call
        if args.op == "mult":
            check(L_.lsa_bfv_mult_plain_mul(ctx.h, lvl, cts[0].data_ptr(), pts[0].data_ptr(), outs[fused].data_ptr(), B, s_ct, s_pt,
                                            s_ct, ctx.stream))
        else:
            check(L_.lsa_bfv_mac_plain_mul(ctx.h, lvl, k, c_cts, c_scts, c_pts, c_spts, partial.data_ptr(), s_ct,
                                           outs[fused].data_ptr(), B, s_ct, ctx.stream))

    def timed(fused):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            run(fused)
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        run("1")
        run("0")
    torch.cuda.synchronize()
    fs, us = [], []
    for _ in range(args.rounds):
        fs.append(timed("1"))
        us.append(timed("0"))
    os.environ.pop("LSA_PTMUL_FUSED", None)
    identical = torch.equal(outs["1"], outs["0"])
    cnt = args.steps * B
    f_cps, u_cps = 1e3 * cnt / statistics.median(fs), 1e3 * cnt / statistics.median(us)
    line = {
        "metric": "bfv_%s_plain_mul_fused_speedup" % args.op, "value": f_cps / u_cps, "unit": "x",
        "fused_ct_per_s": f_cps, "unfused_ct_per_s": u_cps, "fused_ms_rounds": fs, "unfused_ms_rounds": us,
        "fused_algorithmic_TBps": model["bytes_fused_per_ct"] * f_cps / 1e12,
        "unfused_algorithmic_TBps": model["bytes_unfused_per_ct"] * u_cps / 1e12,
        "bit_identical": identical, "config": shape, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
        "byte_model": model, "data": "synthetic",
        "timing": "HIP events on the launch stream after warm-up; fused and unfused regions alternated, medians of the rounds",
    }
    print(json.dumps(line), flush=True)
    return 0 if identical else 1


if __name__ == "__main__":
    sys.exit(main())
