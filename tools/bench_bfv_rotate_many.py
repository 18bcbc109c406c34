"""Hoisted BFV rotations (lsa_bfv_rotate_many) against the same rotations run one by one (lsa_bfv_rotate).

Shapes: `--shape n14` is params.BFV_DEFAULT[16384] at level 3 (4 Q + 2 P limbs), batch 256; `--shape n16` is
params.bfv_n16_chain() at level 23 (24 Q + 4 P limbs), batch 4.  `--m` Galois elements (column rotations by the steps of the
reference's BFV advanced_rotate_col test, unittests/test_gpu_bfv.cpp:493-528).

Timed regions, alternated `--rounds` times in one process after `--warmup` calls of each: `--steps` calls of ONE
bfv_rotate_many over the m elements, and `--steps` x m calls of bfv_rotate; HIP events on the launch stream, operator tiles on
two streams as in bench.py.  Reported: rotations per second of both (median over the rounds), their ratio, the algorithmic
byte model, and whether the hoisted outputs are bit-identical to the separate ones on the timed data.  Inputs and keys are
uniform random residues (the timing does not depend on them).  Prints one JSON line.

    python tools/bench_bfv_rotate_many.py [--shape n14|n16] [--m 5] [--batch B] [--steps 10] [--warmup 3] [--rounds 3]
                                          [--hoisted-only] [--dry-run]

--hoisted-only: warm-up and the hoisted calls only, no comparison (a kernel trace of one hoisted run).
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

STEPS = [-900, 20, 400, 2000, 3009]   # the reference's advanced_rotate_col steps


def shape_of(name):
    if name == "n14":
        P = params.BFV_DEFAULT[16384]
        return {"n": 16384, "q": P["q"], "p": P["p"], "t": P["t"], "level": 3, "batch": 256}
    C = params.bfv_n16_chain()
    return {"n": C["n"], "q": C["q"], "p": C["p"], "t": C["t"], "level": 23, "batch": 4}


def byte_model(n, L, k, m):
    """algorithmic limb streams (one limb of N words read or written = one stream) of rotating ONE ciphertext by m elements.
    Decomposition, once per input: forward NTT of c1 (L in, L out), the digits' conversions (L in, beta*T - L out), the
    extension transform (beta*T - L in and out): 3*beta*T.  Per key: MAC (beta*T digits + 2*beta*T key in, 2T out), ModDown
    inverse transform (2T in and out), P -> Q conversion (2k in, 2L out), tail (acc, conv 2L each + c0 L in, 2L out).
    Separate rotations add the permutation pass (2L in, 2L out) each; hoisted ones fold it into the tail."""
    T, beta = L + k, (L + k - 1) // k
    decomp = 3 * beta * T
    per_key = (3 * beta * T + 2 * T) + 4 * T + (2 * k + 2 * L) + 7 * L
    perm = 4 * L
    separate = m * (decomp + per_key + perm)
    hoisted = decomp + m * per_key
    w = 8 * n
    return {"streams_decomposition": decomp, "streams_per_key": per_key, "streams_permutation": perm,
            "bytes_separate_per_ct": separate * w, "bytes_hoisted_per_ct": hoisted * w,
            "byte_ratio_separate_over_hoisted": separate / hoisted}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["n14", "n16"], default="n14")
    ap.add_argument("--m", type=int, default=5, choices=range(2, len(STEPS) + 1))
    ap.add_argument("--batch", type=int, default=0, help="ciphertexts per call (0 = the shape's default)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--hoisted-only", action="store_true")
    ap.add_argument("--dry-run", action="store_true", help="print the shape and the byte model; no GPU")
    args = ap.parse_args()
    S = shape_of(args.shape)
    n, q, p, t, lvl = S["n"], S["q"], S["p"], S["t"], S["level"]
    L, k = lvl + 1, len(p)
    B = args.batch or S["batch"]
    m = args.m
    steps = STEPS[:m]
    els = [pow(5, s % (n // 2), 2 * n) for s in steps]
    model = byte_model(n, L, k, m)
    shape = {"shape": args.shape, "ring_degree": n, "level": lvl, "q_limbs": L, "special_primes": k, "t": t, "batch": B,
             "m": m, "steps": steps, "galois_elements": els}
    if args.dry_run:
        print(json.dumps({"config": shape, "byte_model": model}))
        return 0

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bfv_rotate_many.py needs an MI355X: no HIP device visible and there is no CPU fallback")
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

    beta = (L + k - 1) // k
    key_ts, keys = [], []
    for _ in els:
        kt = uniform((beta, 2), q[:L] + p)
        key_ts.append(kt)
    torch.cuda.synchronize()
    for kt in key_ts:
        assert kt.numel() * 8 == ctx.key_bytes(lvl)
        keys.append(ctx.adopt_key(kt.data_ptr(), lvl))
    a = uniform((B, 2), q[:L])
    hoisted = [torch.empty(B, 2, L, n, dtype=torch.int64, device=dev) for _ in els]
    separate = [torch.empty(B, 2, L, n, dtype=torch.int64, device=dev) for _ in els]
    s_ct = 2 * L * n
    c_els = (ctypes.c_uint64 * m)(*els)
    c_keys = (ctypes.c_void_p * m)(*[kh.value for kh in keys])
    c_outs = (ctypes.c_void_p * m)(*[o.data_ptr() for o in hoisted])
    check(L_.lsa_set_dual_stream(ctx.h, 1))

    def run_hoisted():
        check(L_.lsa_bfv_rotate_many(ctx.h, lvl, a.data_ptr(), m, c_els, c_keys, c_outs, B, s_ct, s_ct, ctx.stream))

    def run_separate():
        for i in range(m):
            check(L_.lsa_bfv_rotate(ctx.h, lvl, a.data_ptr(), els[i], keys[i], separate[i].data_ptr(), B, s_ct, s_ct, ctx.stream))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.steps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        run_hoisted()
        if not args.hoisted_only:
            run_separate()
    torch.cuda.synchronize()
    if args.hoisted_only:
        ms = timed(run_hoisted)
        line = {"metric": "bfv_rotate_many_hoisted_only", "value": 1e3 * args.steps * B * m / ms, "unit": "rot/s",
                "config": shape, "steps": args.steps, "warmup": args.warmup, "byte_model": model, "data": "synthetic"}
        print(json.dumps(line), flush=True)
    else:
        hs, ss = [], []
        for _ in range(args.rounds):
            hs.append(timed(run_hoisted))
            ss.append(timed(run_separate))
        identical = all(torch.equal(hoisted[i], separate[i]) for i in range(m))
        rot = args.steps * B * m
        h_rps, s_rps = 1e3 * rot / statistics.median(hs), 1e3 * rot / statistics.median(ss)
        bph, bps = model["bytes_hoisted_per_ct"], model["bytes_separate_per_ct"]
        line = {
            "metric": "bfv_rotate_many_speedup", "value": h_rps / s_rps, "unit": "x",
            "hoisted_rot_per_s": h_rps, "separate_rot_per_s": s_rps,
            "hoisted_ms_rounds": hs, "separate_ms_rounds": ss,
            "hoisted_algorithmic_GBps": bph * B * args.steps / (statistics.median(hs) * 1e6),
            "separate_algorithmic_GBps": bps * B * args.steps / (statistics.median(ss) * 1e6),
            "bit_identical": identical, "config": shape, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
            "byte_model": model, "data": "synthetic",
            "timing": "HIP events on the launch stream after warm-up; hoisted and separate regions alternated, medians of the rounds",
        }
        print(json.dumps(line), flush=True)
        if not identical:
            return 1
    for kh in keys:
        ctx.destroy_key(kh)
    return 0


if __name__ == "__main__":
    sys.exit(main())
