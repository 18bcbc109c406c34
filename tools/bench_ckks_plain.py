"""CKKS plaintext and constant operands (lsa_ckks_encode / _mult_plain / _mult_const / _add_const / _affine_const) at N = 2^16 on
the headline chain (params.CKKS_DEFAULT[65536] cut to 13 Q limbs + 4 P, level 12).  Three comparisons, each pair alternated in
one process:

(a) multiplication by i: lsa_ckks_mult_const(re = 0, im = 1, const_scale = 1), which reads no plaintext (k_cconst), against
    lsa_ckks_mult_plain with the encoded monomial X^(N/2) as a shared plaintext (k_mac_plain) -- the same words;
(b) lsa_ckks_affine_const (one pass) against lsa_ckks_mult_const followed by lsa_ckks_add_const in place -- the same words;
(c) lsa_ckks_encode (8 N bytes uploaded per plaintext, residue rows formed by k_lift_i64) against an upload of (level + 1) rows
    the host has reduced already (lsa_memcpy_h2d + lsa_ntt); the host's floating-point encoding is common to both and is timed
    with (c)'s first leg only, so the second leg is a LOWER bound for the path it stands for.

After `--warmup` calls of each, the legs of a pair are alternated `--rounds` times (default 3); HIP events on the launch stream for
(a) and (b), wall clock around the synchronous calls for (c); per leg the median, the minimum and the maximum.  Prints one JSON line.

    python tools/bench_ckks_plain.py [--batch B] [--steps 5] [--warmup 1] [--rounds 3] [--leg-timeout 120] [--dry-run]

--dry-run: needs no GPU; prints the limb-stream model (rows of N words read + written per ciphertext, L = level + 1):
  mult_plain      6L          k_mac_plain, one term: the ciphertext row and the plaintext row read, one row written, 2L rows
  mult_const      4L          k_cconst: one read and one write per row
  add_const       2L | 4L     in place (c0 only) | out of place (c1 copied)
  addsub_plain    3L | 5L     in place | out of place
  affine_const    4L          against mult_const + add_const in place: 6L
  mac_plain       4L n + 2L launches + 2L (launches - 1) (+ 2L addend), launches = ceil(n / 16)
  rescale         4 + 8 + 10 (L - 1)      the existing lsa_ckks_rescale, unchanged
  encode          upload N words per plaintext (against L N), k_lift_i64 1 + L rows, then the forward transform
"""
import argparse
import ctypes
import faulthandler
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lattisense_amd import params  # noqa: E402

LEVEL, BATCH = 12, 16
MAC_MAX_TERMS = 16   # LSA_MAC_MAX_TERMS (csrc/lsa_internal.h)


def stream_model(level, mac_terms=(1, 16, 17)):
    L = level + 1
    m = {"mult_plain": 6 * L, "mult_const": 4 * L, "add_const_in_place": 2 * L, "add_const": 4 * L, "addsub_plain_in_place": 3 * L,
         "addsub_plain": 5 * L, "affine_const": 4 * L, "mult_const_then_add_const": 6 * L, "rescale": 4 + 8 + 10 * (L - 1),
         "encode_upload_words_per_n": 1, "rows_upload_words_per_n": L, "lift_i64": 1 + L, "mac_plain": {}}
    for n in mac_terms:
        launches = -(-n // MAC_MAX_TERMS)
        m["mac_plain"][str(n)] = 4 * L * n + 2 * L * launches + 2 * L * (launches - 1)
    m["predicted_mult_plain_over_mult_const"] = m["mult_plain"] / m["mult_const"]
    m["predicted_two_calls_over_affine"] = m["mult_const_then_add_const"] / m["affine_const"]
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg-timeout", type=float, default=120.0)
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    P = params.CKKS_DEFAULT[65536]
    n, q, p, batch = 65536, P["q"][:13], P["p"][:4], a.batch
    res = {"tool": "bench_ckks_plain", "n": n, "level": LEVEL, "batch": batch, "dry_run": bool(a.dry_run),
           "streams_per_ct": stream_model(LEVEL)}
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
    L = LEVEL + 1
    x = np.empty((batch, 2, L, n), dtype=np.uint64)
    for j in range(L):
        x[:, :, j, :] = rng.integers(0, ctx.moduli[j], size=(batch, 2, n), dtype=np.uint64)
    ct = ctx.upload(x)
    del x
    out, tmp = ctx.alloc(batch * 2 * L * n), ctx.alloc(batch * 2 * L * n)
    mono = ctx.ckks_encode(LEVEL, np.full(n // 2, 1j), 1.0)           # the plaintext X^(N/2)
    got_c = ctx.download(ctx.ckks_mult_const(LEVEL, ct, 1j, 1.0, batch, out=out), (batch, 2, L, n))
    got_p = ctx.download(ctx.ckks_mult_plain(LEVEL, ct, mono, batch, out=tmp, spt=0), (batch, 2, L, n))
    res["mult_const_equals_mult_plain"] = bool(np.array_equal(got_c, got_p))
    del got_c, got_p
    # beta is encoded at ct_scale * const_scale and a rounded constant has to stay below 2^62: 2^30 x 2^30 leaves room, the
    # library's usual 2^40 x 2^40 would not (include/lattisense_amd.h, lsa_ckks_affine_const)
    alpha, beta, d30, d40 = 0.37 - 0.81j, -0.25 + 0.5j, float(2 ** 30), float(2 ** 40)
    z = rng.uniform(-1, 1, (batch, n // 2)) + 1j * rng.uniform(-1, 1, (batch, n // 2))
    pt_out = ctx.alloc(batch * L * n)

    def leg_mult_const():
        ctx.ckks_mult_const(LEVEL, ct, 1j, 1.0, batch, out=out)

    def leg_mult_plain():
        ctx.ckks_mult_plain(LEVEL, ct, mono, batch, out=out, spt=0)

    def leg_affine():
        ctx.ckks_affine_const(LEVEL, ct, alpha, d30, beta, d30, batch, out=out)

    def leg_two_calls():
        ctx.ckks_mult_const(LEVEL, ct, alpha, d30, batch, out=out)
        ctx.ckks_add_const(LEVEL, out, beta, d30 * d30, batch, out=out)

    leg_affine()                                                      # the pair's legs give the same words, checked before timing
    got_a = ctx.download(out, (batch, 2, L, n))
    leg_two_calls()
    res["affine_const_equals_two_calls"] = bool(np.array_equal(got_a, ctx.download(out, (batch, 2, L, n))))
    del got_a
    assert res["mult_const_equals_mult_plain"] and res["affine_const_equals_two_calls"], res

    def leg_encode():
        ctx.ckks_encode(LEVEL, z, d40, batch=batch, out=pt_out)

    rows = np.empty((batch, L, n), dtype=np.uint64)
    for j in range(L):
        rows[:, j, :] = rng.integers(0, ctx.moduli[j], size=(batch, n), dtype=np.uint64)
    mod_of = (ctypes.c_int * L)(*range(L))

    def leg_rows_upload():
        check(lib().lsa_memcpy_h2d(ctx.h, pt_out.ptr, rows.ctypes.data, rows.nbytes, ctx.stream))
        check(lib().lsa_ntt(ctx.h, pt_out.ptr, batch, L * n, L, mod_of, L, 0, ctx.stream))
        ctx.sync()

    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib().lsa_event_create(ctx.h, ctypes.byref(e0)))
    check(lib().lsa_event_create(ctx.h, ctypes.byref(e1)))

    def timed(fn, steps, wall=False):
        faulthandler.dump_traceback_later(a.leg_timeout, exit=True)   # the leg's own time limit
        try:
            ctx.sync()
            t0 = time.perf_counter()
            check(lib().lsa_event_record(ctx.h, e0, ctx.stream))
            for _ in range(steps):
                fn()
            check(lib().lsa_event_record(ctx.h, e1, ctx.stream))
            ctx.sync()
            t1 = time.perf_counter()
            ms = ctypes.c_float()
            check(lib().lsa_event_elapsed_ms(ctx.h, e0, e1, ctypes.byref(ms)))
        finally:
            faulthandler.cancel_dump_traceback_later()
        return ((t1 - t0) * 1e3 if wall else ms.value) / steps

    pairs = {"times_i": ({"mult_const": leg_mult_const, "mult_plain_monomial": leg_mult_plain}, False),
             "affine": ({"affine_const": leg_affine, "mult_const_then_add_const": leg_two_calls}, False),
             "encode": ({"encode_device_lift": leg_encode, "host_rows_upload": leg_rows_upload}, True)}
    res["ms_per_call"], res["measured"] = {}, {}
    for pname, (legs, wall) in pairs.items():
        steps = 1 if wall else a.steps
        for fn in legs.values():
            timed(fn, max(a.warmup, 1), wall)
        ms = {name: [] for name in legs}
        for _ in range(a.rounds):
            for name, fn in legs.items():
                ms[name].append(timed(fn, steps, wall))
        res["ms_per_call"][pname] = {name: {"median": statistics.median(v), "min": min(v), "max": max(v)} for name, v in ms.items()}
        first, second = list(legs)
        res["measured"][pname] = {second + "_over_" + first: statistics.median(ms[second]) / statistics.median(ms[first])}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
