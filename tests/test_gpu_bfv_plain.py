"""lsa_bfv_addsub_plain / lsa_bfv_plain_lift / lsa_bfv_mult_plain (csrc/bfv_plain.hip) against the CPU oracle, word for word on
every batch item.

addsub: Oracle.plain_ringt(0 | 1) (op 2: its word-wise negation) on the chains fp, mixed and ceiling of tests/boundary.py at
N = 2^11 with t = 65537 -- every limb on the FP64 engine, both engines, 61-bit primes -- at level 0, the odd-limb level and the
top; ciphertexts batch 3 in the patterns max / top / uniform; plaintext rows all 0, all t - 1, floor(t/2) and floor(t/2) + 1
alternating, random below t and random 64-bit words; per item and one for the batch; out of place with padded strides (the padding
asserted untouched) and in place; batch 0.  t at the 2^32 edge (4294828033 on BFV_DEFAULT[4096]): words at levels 0 and 1, the
decrypted sum and differences at level 1.  N = 2^16 (two Q limbs of the N = 2^16 chain, t = 786433): the largest ring's index
arithmetic.  One oracle call per (plaintext row, item, level, add | sub) serves every layout and op 2.

lift: forms 1 and 2 equal lsa_bfv_encode of the same values, N = 2^12 (single pass) and 2^13 (two passes), both engine settings,
padded strides, one plaintext for the batch.  mult: Oracle.plain_ringt(2) at N = 2^12 and 2^13, level 0 and top, shared and
per-item plaintexts, in and out of place, and with LSA_PTMUL_FUSED=0; at the top level the product decrypts to m v mod t.
Refusals: code 1, the entry point's name first, nothing written.  Task runtime: the bfv_n4096_cap_ringt graph, whose ADD nodes run
k_bfv_addsub_plain, against the oracle."""
import ctypes
import json
import os

import numpy as np
import pytest

from lattisense_amd import params
from tests.bfv_chain_cases import CHAINS, T, levels
from tests.boundary import bfv_operator_chain, pattern_ct
from tests.gpu_util import env, need_gpu, rand_ct

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_EDGE = 4294828033
PATTERNS = ("max", "top", "uniform")
BATCH = 3
FILL = 7


def _rig(n, q, p, t, seed=0):
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    o = Oracle(n, q, p, t)
    return DeviceContext(ALGO_BFV, n, q, p, t), o, Client(o, seed=seed)


def _pt_rows(t, n, rng, full64=True):
    """the plaintext rows of the header: 0, t - 1, floor(t/2) | floor(t/2) + 1, random below t (, random 64-bit words)"""
    alt = np.empty(n, dtype=np.uint64)
    alt[0::2], alt[1::2] = t // 2, t // 2 + 1
    rows = [np.zeros(n, dtype=np.uint64), np.full(n, t - 1, dtype=np.uint64), alt, rng.integers(0, t, n).astype(np.uint64)]
    if full64:
        rows.append(rng.integers(0, 1 << 64, n, dtype=np.uint64))
    return rows


def _negate(words, q):
    """word-wise negation of [2][L][n] canonical residues"""
    qs = np.array(q[: words.shape[1]], dtype=np.uint64)[None, :, None]
    return np.where(words == 0, words, qs - words)


class Ref:
    """Oracle.plain_ringt(0 | 1) per (level, op, plaintext row, ciphertext item), computed once"""

    def __init__(self, o, q):
        self.o, self.q, self.cache = o, q, {}

    def want(self, op, lvl, ct, ct_id, row, row_id):
        key = (min(op, 1), lvl, ct_id, row_id)
        if key not in self.cache:
            self.cache[key] = self.o.plain_ringt(min(op, 1), lvl, ct, row)
        w = self.cache[key]
        return _negate(w, self.q) if op == 2 else w


def _addsub(ctx, op, lvl, cts, pts, shared, in_place, n):
    """runs one call; cts [B][2][L][n], pts [B][n] (shared: [1][n]); out of place with padded strides everywhere, the padding
    pre-filled and asserted untouched; returns [B][2][L][n]"""
    B, w = cts.shape[0], 2 * (lvl + 1) * n
    if in_place:
        sct, spt = w + 2 * n, 0 if shared else n
        host = np.full((B, sct), FILL, dtype=np.uint64)
        host[:, :w] = cts.reshape(B, w)
        buf = ctx.upload(host)
        ctx.bfv_addsub_plain(op, lvl, buf, ctx.upload(pts), B, out=buf, spt=spt, sct=sct, sout=sct)
        got = ctx.download(buf, (B, sct))
        assert np.all(got[:, w:] == FILL), "in place: the padding between the items was written"
        return got[:, :w].reshape(cts.shape)
    sct, spt, sout = w + 4 * n, 0 if shared else n + 16, w + 64
    hc = np.full((B, sct), FILL, dtype=np.uint64)
    hc[:, :w] = cts.reshape(B, w)
    hp = np.full((pts.shape[0], n + 16), FILL, dtype=np.uint64)
    hp[:, :n] = pts
    dc, dp = ctx.upload(hc), ctx.upload(hp)
    out = ctx.upload(np.full((B, sout), FILL, dtype=np.uint64))
    ctx.bfv_addsub_plain(op, lvl, dc, dp, B, out=out, spt=spt, sct=sct, sout=sout)
    got = ctx.download(out, (B, sout))
    assert np.all(got[:, w:] == FILL), "the padding of the output was written"
    assert np.array_equal(ctx.download(dc, (B, sct)), hc) and np.array_equal(ctx.download(dp, hp.shape), hp), "an input was written"
    return got[:, :w].reshape(cts.shape)


_CHAIN_RIGS = {}


def _chain_rig(kind):
    if kind not in _CHAIN_RIGS:
        n = 1 << 11
        q, p = bfv_operator_chain(kind, n)
        ctx, o, c = _rig(n, q, p, T)
        rng = np.random.default_rng(1100 + CHAINS.index(kind))
        _CHAIN_RIGS[kind] = (ctx, o, Ref(o, q), pattern_ct(PATTERNS, q, 2, n, rng), _pt_rows(T, n, rng), q, n)
    return _CHAIN_RIGS[kind]


@pytest.mark.parametrize("which", ["zero", "odd", "top"])
@pytest.mark.parametrize("kind", CHAINS)
def test_addsub_on_the_operator_chains(kind, which):
    need_gpu()
    ctx, o, ref, A, rows, q, n = _chain_rig(kind)
    top, odd = levels(kind, n)
    lvl = {"zero": 0, "odd": odd, "top": top}[which]
    assert which != "odd" or (lvl + 1) % 2 == 1
    cts = np.ascontiguousarray(A[:, :, : lvl + 1])
    per_item = [(0, 1, 2), (2, 3, 4), (4, 0, 3)]                     # plaintext row of each batch item
    for op in (0, 1, 2):
        for in_place in (False, True):
            for ids in per_item:
                got = _addsub(ctx, op, lvl, cts, np.stack([rows[i] for i in ids]), False, in_place, n)
                for b in range(BATCH):
                    assert np.array_equal(got[b], ref.want(op, lvl, cts[b], b, rows[ids[b]], ids[b])), (kind, lvl, op, in_place, ids, b)
            for i, row in enumerate(rows):                            # one plaintext for the whole batch
                got = _addsub(ctx, op, lvl, cts, row[None], True, in_place, n)
                for b in range(BATCH):
                    assert np.array_equal(got[b], ref.want(op, lvl, cts[b], b, row, i)), (kind, lvl, op, in_place, "shared", i, b)
    # batch 0: nothing is written
    w = 2 * (lvl + 1) * n
    out = ctx.upload(np.full(w, FILL, dtype=np.uint64))
    ctx.bfv_addsub_plain(0, lvl, ctx.upload(cts[0]), ctx.upload(rows[3]), 0, out=out)
    assert np.all(ctx.download(out, (w,)) == FILL)


def test_addsub_with_t_at_the_2_32_edge():
    """t = 4294828033 on the two 39-bit limbs of BFV_DEFAULT[4096]: (t - 1)^2 + t/2 is the largest value the reduction mod t
    sees.  Level 0 (Q / t is 7 bits) has no noise room: words only, on pattern ciphertexts.  Level 1: real encryptions, and the
    result decrypts to (m + v), (m - v) and (v - m) mod t."""
    need_gpu()
    n = 4096
    B = params.BFV_DEFAULT[n]
    assert T_EDGE % (2 * n) == 1 and all(T_EDGE < m for m in B["q"])
    ctx, o, c = _rig(n, B["q"], B["p"], T_EDGE, seed=5)
    try:
        rng = np.random.default_rng(32)
        ref = Ref(o, B["q"])
        rows = _pt_rows(T_EDGE, n, rng)
        A = pattern_ct(PATTERNS, B["q"], 2, n, rng)
        for lvl in (0, 1):
            cts = np.ascontiguousarray(A[:, :, : lvl + 1])
            for op in (0, 1, 2):
                for ids in ((0, 1, 2), (2, 3, 4)):
                    got = _addsub(ctx, op, lvl, cts, np.stack([rows[i] for i in ids]), False, op == 1, n)
                    for b in range(BATCH):
                        assert np.array_equal(got[b], ref.want(op, lvl, cts[b], (lvl, b), rows[ids[b]], ids[b])), (lvl, op, ids, b)
        tm = np.uint64(T_EDGE)
        m = rng.integers(0, T_EDGE, (BATCH, n)).astype(np.uint64)
        v = np.stack([rng.integers(0, T_EDGE, n).astype(np.uint64), np.full(n, T_EDGE - 1, dtype=np.uint64), np.zeros(n, dtype=np.uint64)])
        enc = np.stack([c.bfv_encrypt(x, 1) for x in m])
        pts = np.stack([c.bfv_encode(x) for x in v])
        for op, fn in ((0, lambda x, y: (x + y) % tm), (1, lambda x, y: (x + tm - y) % tm), (2, lambda x, y: (y + tm - x) % tm)):
            got = _addsub(ctx, op, 1, enc, pts, False, False, n)
            for b in range(BATCH):
                assert np.array_equal(got[b], ref.want(op, 1, enc[b], ("enc", b), pts[b], ("enc", b))), (op, b)
                assert np.array_equal(c.bfv_decrypt(got[b]), fn(m[b], v[b])), ("decryption", op, b)
    finally:
        ctx.close()


def test_addsub_at_the_largest_ring():
    need_gpu()
    n = 65536
    C = params.bfv_n16_chain()
    q, p, t = C["q"][:2], C["p"][:1], C["t"]
    assert t == 786433
    ctx, o, c = _rig(n, q, p, t)
    try:
        rng = np.random.default_rng(16)
        cts = rand_ct(rng, q, 2, n, 2)
        cts[0, :, :, -2:] = np.array(q, dtype=np.uint64)[None, :, None] - np.uint64(1)       # the last lane of the last block
        pts = np.stack([rng.integers(0, t, n).astype(np.uint64), rng.integers(0, 1 << 64, n, dtype=np.uint64)])
        for op, in_place in ((1, False), (0, True)):
            got = _addsub(ctx, op, 1, cts, pts, False, in_place, n)
            for b in range(2):
                assert np.array_equal(got[b], o.plain_ringt(op, 1, cts[b], pts[b])), (op, b)
    finally:
        ctx.close()


# ---------------------------------------------------------------- lift and multiply

def _default_rig(n, seed=0):
    B = params.BFV_DEFAULT[n]
    return _rig(n, B["q"], B["p"], B["t"], seed) + (B,)


@pytest.mark.parametrize("n", [4096, 8192])
def test_lift_equals_the_encoder(n):
    need_gpu()
    ctx, o, c, B = _default_rig(n)
    try:
        t, rng = B["t"], np.random.default_rng(n + 7)
        vals = np.stack([rng.integers(0, t, n).astype(np.uint64), np.full(n, t - 1, dtype=np.uint64), np.zeros(n, dtype=np.uint64)])
        coef = ctx.bfv_encode(0, 0, vals)
        hcoef = ctx.download(coef, (3, n))
        assert np.array_equal(hcoef, np.stack([c.bfv_encode(v) for v in vals]))
        top = len(B["q"]) - 1
        for lvl in (0, top):
            for form in (1, 2):
                rows = ctx.bfv_pt_rows(lvl, form)
                want = ctx.download(ctx.bfv_encode(lvl, form, vals), (3, rows, n))
                for engine in (1, 0):
                    ctx.set_fp64_ntt(engine)
                    try:
                        got = ctx.download(ctx.bfv_plain_lift(lvl, form, coef, 3), (3, rows, n))
                    finally:
                        ctx.set_fp64_ntt(1)
                    assert np.array_equal(got, want), (n, lvl, form, engine)
                spt, sout = n + 32, rows * n + 2 * n                   # padded on both sides
                hp = np.full((3, spt), FILL, dtype=np.uint64)
                hp[:, :n] = hcoef
                out = ctx.upload(np.full((3, sout), FILL, dtype=np.uint64))
                ctx.bfv_plain_lift(lvl, form, ctx.upload(hp), 3, out=out, spt=spt, sout=sout)
                pad = ctx.download(out, (3, sout))
                assert np.array_equal(pad[:, : rows * n].reshape(3, rows, n), want) and np.all(pad[:, rows * n:] == FILL), (n, lvl, form)
                one = ctx.download(ctx.bfv_plain_lift(lvl, form, coef, 2, spt=0), (2, rows, n))   # one plaintext for the batch
                assert np.array_equal(one[0], want[0]) and np.array_equal(one[1], want[0]), (n, lvl, form, "shared")
                ctx.bfv_plain_lift(lvl, form, coef, 0, out=out, spt=n, sout=sout)                  # batch 0
                assert np.array_equal(ctx.download(out, (3, sout)), pad)
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [4096, 8192])
def test_mult_equals_the_oracle_and_multiplies_messages(n):
    need_gpu()
    ctx, o, c, B = _default_rig(n, seed=3)
    try:
        t, rng = B["t"], np.random.default_rng(n + 9)
        tm, top = np.uint64(t), len(B["q"]) - 1
        m = rng.integers(0, t, (2, n)).astype(np.uint64)
        v = np.stack([rng.integers(0, t, n).astype(np.uint64), np.full(n, t - 1, dtype=np.uint64)])
        pts = np.stack([c.bfv_encode(x) for x in v])
        dp = ctx.upload(pts)
        for lvl in (0, top):
            w = 2 * (lvl + 1) * n
            # level 0 has no noise room for a product: uniform words; at the top real encryptions
            cts = np.stack([c.bfv_encrypt(x, lvl) for x in m]) if lvl == top else rand_ct(rng, B["q"][:1], 2, n, 2)
            want = {(b, k): o.plain_ringt(2, lvl, cts[b], pts[k]) for b in range(2) for k in range(2)}
            dc = ctx.upload(cts)
            per_item = ctx.download(ctx.bfv_mult_plain(lvl, dc, dp, 2), (2, 2, lvl + 1, n))
            shared = ctx.download(ctx.bfv_mult_plain(lvl, dc, dp, 2, spt=0), (2, 2, lvl + 1, n))
            for b in range(2):
                assert np.array_equal(per_item[b], want[(b, b)]), (n, lvl, "per item", b)
                assert np.array_equal(shared[b], want[(b, 0)]), (n, lvl, "shared", b)
            with env(LSA_PTMUL_FUSED="0"):
                assert np.array_equal(ctx.download(ctx.bfv_mult_plain(lvl, dc, dp, 2), (2, 2, lvl + 1, n)), per_item), (n, lvl, "unfused")
                assert np.array_equal(ctx.download(ctx.bfv_mult_plain(lvl, dc, dp, 2, spt=0), (2, 2, lvl + 1, n)), shared), (n, lvl, "unfused")
            ctx.set_tile_batch(1)                                      # one item per tile: a lift and a product per tile
            try:
                assert np.array_equal(ctx.download(ctx.bfv_mult_plain(lvl, dc, dp, 2), (2, 2, lvl + 1, n)), per_item), (n, lvl, "tiles of 1")
            finally:
                ctx.set_tile_batch(0)
            for spt, ref in ((None, per_item), (0, shared)):           # in place
                buf = ctx.upload(cts)
                ctx.bfv_mult_plain(lvl, buf, dp, 2, out=buf, spt=spt)
                assert np.array_equal(ctx.download(buf, (2, 2, lvl + 1, n)), ref), (n, lvl, "in place", spt)
            out = ctx.upload(np.full(2 * w, FILL, dtype=np.uint64))    # batch 0
            ctx.bfv_mult_plain(lvl, dc, dp, 0, out=out)
            assert np.all(ctx.download(out, (2 * w,)) == FILL)
            if lvl == top:
                for b in range(2):
                    assert np.array_equal(c.bfv_decrypt(per_item[b]), m[b] * v[b] % tm), (n, "decryption", b)
                    assert np.array_equal(c.bfv_decrypt(shared[b]), m[b] * v[0] % tm), (n, "decryption, shared", b)
    finally:
        ctx.close()


# ---------------------------------------------------------------- refusals

def _message(err):
    return str(err).split(": ", 1)[1]


def test_refusals_arrive_before_anything_is_written():
    need_gpu()
    from lattisense_amd._native import LsaError, check, lib
    from lattisense_amd.device import ALGO_BFV, ALGO_CKKS, DeviceContext
    n = 4096
    ctx, o, c, B = _default_rig(n)
    try:
        L = len(B["q"])
        w = 2 * L * n
        ct = ctx.upload(rand_ct(np.random.default_rng(4), B["q"], 2, n, 2))
        pt = ctx.upload(np.zeros(4 * w, dtype=np.uint64))                # two plaintexts, and room for an output that starts in them
        out = ctx.upload(np.full(4 * w, FILL, dtype=np.uint64))
        S = ctx.stream

        def fails(who, fn, needle):
            with pytest.raises(LsaError) as e:
                fn()
            assert e.value.code == 1 and _message(e.value).startswith(who) and needle in _message(e.value), e.value
            assert np.all(ctx.download(out, (4 * w,)) == FILL), (who, needle)

        def addsub(h=ctx.h, op=0, lvl=L - 1, ct_=ct.ptr, sct=w, pt_=pt.ptr, spt=n, out_=out.ptr, sout=w, b=2):
            check(lib().lsa_bfv_addsub_plain(h, op, lvl, ct_, sct, pt_, spt, out_, sout, b, S))

        def lift(h=ctx.h, lvl=L - 1, form=1, pt_=pt.ptr, spt=n, out_=out.ptr, sout=L * n, b=2):
            check(lib().lsa_bfv_plain_lift(h, lvl, form, pt_, spt, out_, sout, b, S))

        def mult(h=ctx.h, lvl=L - 1, ct_=ct.ptr, sct=w, pt_=pt.ptr, spt=n, out_=out.ptr, sout=w, b=2):
            check(lib().lsa_bfv_mult_plain(h, lvl, ct_, sct, pt_, spt, out_, sout, b, S))

        P = params.CKKS_DEFAULT[4096]
        ckks = DeviceContext(ALGO_CKKS, n, P["q"], P["p"])
        for who, fn in (("lsa_bfv_addsub_plain", addsub), ("lsa_bfv_plain_lift", lift), ("lsa_bfv_mult_plain", mult)):
            fails(who, lambda: fn(h=ckks.h, lvl=0), "not BFV")
            fails(who, lambda: fn(lvl=L), "level")
            fails(who, lambda: fn(lvl=-1), "level")
            fails(who, lambda: fn(pt_=None), "null")
            fails(who, lambda: fn(out_=None), "null")
            fails(who, lambda: fn(pt_=pt.ptr + 8), "16-byte")
            fails(who, lambda: fn(out_=out.ptr + 8), "16-byte")
            fails(who, lambda: fn(spt=n + 1), "even")
            fails(who, lambda: fn(spt=n - 2), "stride")
            fails(who, lambda: fn(sout=0), "stride")                  # a shared output is no layout
            fails(who, lambda: fn(sout=2), "stride")
            fails(who, lambda: fn(out_=pt.ptr, b=1), "overlaps")
            fails(who, lambda: fn(lvl=L, b=0), "level")               # batch 0: still checked
            fails(who, lambda: fn(out_=None, b=0), "null")
        for who, fn in (("lsa_bfv_addsub_plain", addsub), ("lsa_bfv_mult_plain", mult)):
            fails(who, lambda: fn(ct_=None), "null")
            fails(who, lambda: fn(ct_=ct.ptr + 8), "16-byte")
            fails(who, lambda: fn(sct=w + 1), "even")
            fails(who, lambda: fn(sct=w - 2), "stride")
            fails(who, lambda: fn(sct=0), "stride")                   # the ciphertext is never shared
            fails(who, lambda: fn(out_=ct.ptr + 16 * n), "ct itself")   # overlaps ct without being it
            fails(who, lambda: fn(out_=ct.ptr, sout=w + 2, sct=w), "ct itself")
        ckks.close()
        fails("lsa_bfv_addsub_plain", lambda: addsub(op=3), "op")
        fails("lsa_bfv_addsub_plain", lambda: addsub(op=-1), "op")
        fails("lsa_bfv_plain_lift", lambda: lift(form=0), "form")
        fails("lsa_bfv_plain_lift", lambda: lift(form=3), "form")
        fails("lsa_bfv_plain_lift", lambda: lift(form=2, sout=L * n), "stride")      # extended needs (L + 1) N words
        fails("lsa_bfv_plain_lift", lambda: lift(out_=pt.ptr + 8 * (n - 2), b=1), "overlaps")   # the plaintext's last two words
        # t: 2^32 + 15 is no plaintext modulus for the scale-up; t above a modulus of the chain is none for the lift
        big = DeviceContext(ALGO_BFV, n, B["q"], B["p"], (1 << 32) + 15)
        fails("lsa_bfv_addsub_plain", lambda: addsub(h=big.h), "2^32")
        big.close()
        edge = DeviceContext(ALGO_BFV, n, B["q"], B["p"], T_EDGE)       # above the 30-bit special prime, below both q
        fails("lsa_bfv_plain_lift", lambda: lift(h=edge.h, form=2, sout=(L + 1) * n), "below every modulus")
        ok = ctx.alloc(2 * L * n)
        lift(h=edge.h, form=1, out_=ok.ptr)                              # form 1 writes no special prime's row: accepted
        ctx.sync()
        edge.close()
        wide = DeviceContext(ALGO_BFV, n, B["q"], B["p"], B["q"][0] + 2)
        fails("lsa_bfv_plain_lift", lambda: lift(h=wide.h), "below every modulus")
        fails("lsa_bfv_mult_plain", lambda: mult(h=wide.h), "below every modulus")
        wide.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------- task runtime

def test_task_ringt_add_runs_the_fused_kernel_and_matches_the_oracle():
    """the ADD nodes of bfv_n4096_cap_ringt (a ciphertext plus a ring-t plaintext) go through k_bfv_addsub_plain in the task
    dispatcher: bit-exact against the oracle, and the message is the sum"""
    need_gpu()
    from lattisense_amd.task import Argument, Ciphertext, FheTaskGpu, Plaintext
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    name = "bfv_n4096_cap_ringt"
    path = os.path.join(ROOT, "tests", "golden", "tasks", name)
    P = json.load(open(os.path.join(path, "mega_ag.json")))["parameter"]
    o = Oracle(P["n"], P["q"][: P["max_level"] + 1], P["p"], P["t"])
    c = Client(o, seed=11)
    n, lvl, tm = P["n"], 2, np.uint64(P["t"])
    rng = np.random.default_rng(77)
    xm = [rng.integers(0, P["t"], size=n, dtype=np.uint64) for _ in range(4)]
    ym = [rng.integers(0, P["t"], size=n, dtype=np.uint64) for _ in range(3)] + [np.full(n, P["t"] - 1, dtype=np.uint64)]
    xs = [c.bfv_encrypt(m, lvl) for m in xm]
    ys = [c.bfv_encode(m) for m in ym]
    t = FheTaskGpu(path)
    try:
        zs = [Ciphertext.empty(1, lvl, n) for _ in range(4)]
        t.run([Argument("xs", [Ciphertext(x) for x in xs]), Argument("ys", [Plaintext(y[None]) for y in ys])], [Argument("zs", zs)])
        for i in range(4):
            assert np.array_equal(zs[i].data, o.plain_ringt(0, lvl, xs[i], ys[i])), i
            assert np.array_equal(c.bfv_decrypt(zs[i].data), (xm[i] + ym[i]) % tm), i
    finally:
        t.close()
