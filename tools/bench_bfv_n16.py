"""Throughput of BFV multiply + relinearise at N = 2^16 (params.bfv_n16_chain, 24 Q + 4 P limbs, top level): the shape
whose two exact base conversions have 24 source limbs (kernels.hip k_baseconv_wide).  bench.py's bfv_hmult workload stays at
N = 2^14; this is a separate tool.

Timed region: `--steps` calls of bfv_mult_relin on a batch of `--batch` ciphertext pairs after `--warmup` calls, HIP events
on the launch stream, operator tiles on two streams as in bench.py.  Second region (single stream): bfv_mult alone -- the
only base conversions in it are the multiply's Q -> QMul and QMul -> Q ones -- with every launch timed by the library's
event profiler (lsa_profile_*), giving the conversions' time, their achieved algorithmic bandwidth and their share of
mult + relin.  Prints one JSON line.  Inputs and key are uniform random residues (the timing does not depend on them).

    python tools/bench_bfv_n16.py [--batch 4] [--steps 10] [--warmup 3] [--dry-run]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lattisense_amd import params  # noqa: E402


def bfv_aux_count(q, logn):
    """auxiliary limbs of a BFV multiply with Q = prod(q) (tables.cpp bfv_aux_count)"""
    prod = 1
    for m in q:
        prod *= m
    return (prod.bit_length() + logn + 60) // 61


def conversion_bytes(n, L, M):
    """algorithmic bytes (each source limb read once, each target limb written once) of the base conversions of one
    folded bfv_mult: 2 operands x 2 polynomials + 3 tensor polynomials Q -> QMul (L sources, M targets), 3 QMul -> Q whose
    source load also reads the subtrahend (2M sources, L targets)"""
    qa = 7 * 8 * n * (L + M)
    aq = 3 * 8 * n * (2 * M + L)
    return qa, aq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--level", type=int, default=23)
    ap.add_argument("--dry-run", action="store_true", help="print the shape and byte counts; no GPU")
    args = ap.parse_args()
    C = params.bfv_n16_chain()
    n, q, p, t = C["n"], C["q"], C["p"], C["t"]
    lvl = args.level
    L = lvl + 1
    M = bfv_aux_count(q[:L], n.bit_length() - 1)
    qa, aq = conversion_bytes(n, L, M)
    shape = {"ring_degree": n, "level": lvl, "q_limbs": L, "aux_limbs": M, "special_primes": len(p), "t": t,
             "batch": args.batch}
    if args.dry_run:
        print(json.dumps({"config": shape, "conv_bytes_per_ct": qa + aq, "conv_bytes_per_ct_q_to_aux": qa,
                          "conv_bytes_per_ct_aux_to_q": aq}))
        return 0

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bfv_n16.py needs an MI355X: no HIP device visible and there is no CPU fallback")
    from lattisense_amd._native import check, lib
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    L_ = lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = DeviceContext(ALGO_BFV, n, q, p, t, device=0)
    stream = torch.cuda.current_stream()
    ctx.stream = ctypes.c_void_p(stream.cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1616)

    def uniform(prefix, mods):
        out = torch.empty(*prefix, len(mods), n, dtype=torch.int64, device=dev)
        for i, m in enumerate(mods):
            out[..., i, :] = torch.randint(0, m, (*prefix, n), dtype=torch.int64, device=dev, generator=gen)
        return out

    class Buf:
        def __init__(self, x):
            self.t, self.ptr = x, x.data_ptr()

    B = args.batch
    beta = (L + len(p) - 1) // len(p)
    key_t = uniform((beta, 2), q[:L] + p)
    torch.cuda.synchronize()
    assert key_t.numel() * 8 == ctx.key_bytes(lvl)
    key = ctx.adopt_key(key_t.data_ptr(), lvl)
    a, b = uniform((B, 2), q[:L]), uniform((B, 2), q[:L])
    out = torch.empty(B, 2, L, n, dtype=torch.int64, device=dev)
    d3 = torch.empty(B, 3, L, n, dtype=torch.int64, device=dev)

    # ---- timed region: mult + relin, two tile streams (as bench.py)
    check(L_.lsa_set_dual_stream(ctx.h, 1))
    for _ in range(args.warmup):
        ctx.bfv_mult_relin(lvl, Buf(a), Buf(b), key, B, out=Buf(out))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(args.steps):
        ctx.bfv_mult_relin(lvl, Buf(a), Buf(b), key, B, out=Buf(out))
    e1.record(stream)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    ms_per_ct = ms / (args.steps * B)

    # ---- second region: multiply alone, one stream, every launch timed by the library's profiler
    check(L_.lsa_set_dual_stream(ctx.h, 0))

    def mult():
        check(L_.lsa_bfv_mult(ctx.h, lvl, a.data_ptr(), b.data_ptr(), d3.data_ptr(), B, 2 * L * n, 2 * L * n, 3 * L * n,
                              ctx.stream))

    for _ in range(args.warmup):
        mult()
    torch.cuda.synchronize()
    k2 = max(2, min(args.steps, 10))
    check(L_.lsa_profile_begin(ctx.h, 1))
    m0, m1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    m0.record(stream)
    for _ in range(k2):
        mult()
    m1.record(stream)
    torch.cuda.synchronize()
    check(L_.lsa_profile_end(ctx.h))
    mult_ms_per_ct = m0.elapsed_time(m1) / (k2 * B)
    pms, pby = ctypes.c_double(), ctypes.c_double()
    ns_, nl_ = ctypes.c_longlong(), ctypes.c_longlong()
    check(L_.lsa_profile_read(ctx.h, 1, ctypes.byref(pms), ctypes.byref(pby), ctypes.byref(ns_), ctypes.byref(nl_)))
    conv_ms_per_ct = pms.value / ns_.value * nl_.value / (k2 * B) if ns_.value else None
    conv_gbps = pby.value / pms.value / 1e6 if pms.value else None
    ctx.destroy_key(key)
    line = {
        "metric": "bfv_mult_relin_n65536_throughput", "value": 1e3 / ms_per_ct, "unit": "ct/s", "ms_per_ct": ms_per_ct,
        "steps": args.steps, "warmup": args.warmup, "config": shape, "data": "synthetic",
        "conv_bytes_per_ct": qa + aq, "conv_bytes_per_ct_q_to_aux": qa, "conv_bytes_per_ct_aux_to_q": aq,
        "mult_only_ms_per_ct": mult_ms_per_ct,
        "conv_ms_per_ct": conv_ms_per_ct, "conv_launches_per_call": nl_.value / k2,
        "conv_achieved_GBps": conv_gbps,
        "conv_share_of_mult_relin": conv_ms_per_ct / ms_per_ct if conv_ms_per_ct else None,
        "conv_share_of_mult": conv_ms_per_ct / mult_ms_per_ct if conv_ms_per_ct else None,
        "timing": "HIP events on the launch stream after warm-up; conversion time from the library's per-launch event "
                  "profiler in a separate single-stream region of bfv_mult alone",
    }
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
