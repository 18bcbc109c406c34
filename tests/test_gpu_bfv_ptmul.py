"""BFV ciphertext x pt_mul plaintext (lsa_bfv_mult_plain_mul / lsa_bfv_mac_plain_mul): the plaintext is NTT-domain and in
Montgomery form, and per poly and limb the result is INTT(NTT(ct) . pt . 2^-64 mod q), Lattigo v4's mulPlaintextMul.
Every result is compared bit for bit with that expression built from the unchanged CPU oracle (Oracle.ntt, Oracle.vec "mul"
by pt * 2^-64 mod q, Oracle.intt), under both forms (LSA_PTMUL_FUSED=1 / 0), both butterfly engines, tile batch default and
1, in place and batch-position independent; at N = 2^12 (FP64 engine), 2^14 and 2^15 at every level and the full N = 2^16
chain; at message level (decrypt == m1 * m2 mod t); and through the task runtime on the frontend's pt_mul graphs."""
import json
import os

import numpy as np
import pytest

from lattisense_amd import params
from tests.gpu_util import env, need_gpu, rand_ct

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASKS = os.path.join(ROOT, "tests", "golden", "tasks")


def _minv(q):
    return np.uint64(pow(2 ** 64, -1, int(q)))


def _want_mac(o, L, cts, pts, partial=None):
    """sum_i INTT(NTT(ct_i) . pt_i . 2^-64) (+ partial) for one batch item: cts [2][L][N], pts [L][N]"""
    n = o.n
    out = np.empty((2, L, n), dtype=np.uint64)
    for j in range(L):
        r = np.full(n, _minv(o.q[j]), dtype=np.uint64)
        for pl in range(2):
            acc = np.zeros(n, dtype=np.uint64)
            for ct, pt in zip(cts, pts):
                acc = o.vec("add", j, acc, o.vec("mul", j, o.ntt(j, ct[pl, j]), o.vec("mul", j, pt[j], r)))
            v = o.intt(j, acc)
            out[pl, j] = o.vec("add", j, v, partial[pl, j]) if partial is not None else v
    return out


def _rand_pt(rng, mods, n, batch):
    return rand_ct(rng, mods, 1, n, batch)[:, 0]


def _ctx(n, q, p, t):
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    from oracle.pyoracle import Oracle
    return DeviceContext(ALGO_BFV, n, q, p, t), Oracle(n, q, p, t)


def _check_level(ctx, o, lvl, batch, rng, terms=(1, 2)):
    """multiply (fresh output and in place) and MACs of the given term counts, with and without a partial sum, against the
    oracle; every batch item checked"""
    n = ctx.n
    L = lvl + 1
    mods = o.q[:L]
    A = rand_ct(rng, mods, 2, n, batch)
    Pt = _rand_pt(rng, mods, n, batch)
    da, dp = ctx.upload(A), ctx.upload(Pt)
    got = ctx.download(ctx.bfv_mult_plain_mul(lvl, da, dp, batch), (batch, 2, L, n))
    for b in range(batch):
        assert np.array_equal(got[b], _want_mac(o, L, [A[b]], [Pt[b]])), ("mult", n, lvl, b)
    ctx.bfv_mult_plain_mul(lvl, da, dp, batch, out=da)   # in place
    assert np.array_equal(ctx.download(da, (batch, 2, L, n)), got), ("mult in place", n, lvl)
    for k in terms:
        Cs = [rand_ct(rng, mods, 2, n, batch) for _ in range(k)]
        Ps = [_rand_pt(rng, mods, n, batch) for _ in range(k)]
        Pa = rand_ct(rng, mods, 2, n, batch)
        dcs, dps = [ctx.upload(x) for x in Cs], [ctx.upload(x) for x in Ps]
        dpa = ctx.upload(Pa)
        for partial in (None, dpa):
            got = ctx.download(ctx.bfv_mac_plain_mul(lvl, dcs, dps, batch, partial=partial), (batch, 2, L, n))
            for b in range(batch):
                want = _want_mac(o, L, [c[b] for c in Cs], [p[b] for p in Ps], Pa[b] if partial is not None else None)
                assert np.array_equal(got[b], want), ("mac", n, lvl, k, partial is not None, b)


@pytest.mark.parametrize("fused", ["1", "0"])
def test_n4096_fp64_engine_terms_and_switches(fused):
    """N = 2^12 on BFV_DEFAULT[4096] (primes below 2^47: the FP64 engine, single-pass plan), engine on and off, tile batch
    default and 1, n in {1, 2, 4, 16}"""
    need_gpu()
    P = params.BFV_DEFAULT[4096]
    ctx, o = _ctx(4096, P["q"], P["p"], P["t"])
    rng = np.random.default_rng(4096 + int(fused))
    try:
        with env(LSA_PTMUL_FUSED=fused):
            for fp64 in (1, 0):
                ctx.set_fp64_ntt(fp64)
                for tile in (0, 1):
                    ctx.set_tile_batch(tile)
                    _check_level(ctx, o, 1, 3, rng, terms=(1, 2, 4, 16) if tile == 0 and fp64 else (1, 2))
                    _check_level(ctx, o, 0, 2, rng, terms=(2,))
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [16384, 32768])
@pytest.mark.parametrize("fused", ["1", "0"])
def test_default_chains_every_level(n, fused):
    need_gpu()
    P = params.BFV_DEFAULT[n]
    ctx, o = _ctx(n, P["q"], P["p"], P["t"])
    rng = np.random.default_rng(n + int(fused))
    try:
        with env(LSA_PTMUL_FUSED=fused):
            for lvl in range(len(P["q"])):
                _check_level(ctx, o, lvl, 2, rng, terms=(2,))
            top = len(P["q"]) - 1
            ctx.set_tile_batch(1)
            _check_level(ctx, o, top, 3, rng, terms=(1, 4))
            ctx.set_tile_batch(0)
    finally:
        ctx.close()


def test_n16_chain_full_ring():
    """the full N = 2^16 chain (24 limbs of 59 bits): multiply and a 4-term MAC with a partial sum, both forms"""
    need_gpu()
    C = params.bfv_n16_chain()
    ctx, o = _ctx(C["n"], C["q"], C["p"], C["t"])
    rng = np.random.default_rng(65536)
    try:
        for fused in ("1", "0"):
            with env(LSA_PTMUL_FUSED=fused):
                _check_level(ctx, o, len(C["q"]) - 1, 1, rng, terms=(4,))
    finally:
        ctx.close()


def test_fused_equals_unfused_and_batch_position_independent():
    """the same ciphertext gives the same result at every batch position, and both forms agree bit for bit"""
    need_gpu()
    P = params.BFV_DEFAULT[16384]
    ctx, o = _ctx(16384, P["q"], P["p"], P["t"])
    n, lvl, batch = 16384, 3, 5
    L = lvl + 1
    rng = np.random.default_rng(7)
    try:
        one = rand_ct(rng, o.q[:L], 2, n, 1)[0]
        pt = _rand_pt(rng, o.q[:L], n, 1)[0]
        A = np.stack([one] * batch)
        Pt = np.stack([pt] * batch)
        res = {}
        for fused in ("1", "0"):
            with env(LSA_PTMUL_FUSED=fused):
                res[fused] = ctx.download(ctx.bfv_mult_plain_mul(lvl, ctx.upload(A), ctx.upload(Pt), batch), (batch, 2, L, n))
                mac = ctx.download(ctx.bfv_mac_plain_mul(lvl, [ctx.upload(A)] * 3, [ctx.upload(Pt)] * 3, batch), (batch, 2, L, n))
                for b in range(batch):
                    assert np.array_equal(res[fused][b], res[fused][0]), (fused, b)
                    assert np.array_equal(mac[b], mac[0]), (fused, b)
        assert np.array_equal(res["1"], res["0"])
        assert np.array_equal(res["1"][0], _want_mac(o, L, [one], [pt]))
    finally:
        ctx.close()


def test_decrypts_to_product():
    """encrypt m1; pt_mul = bfv_encode(m2) lifted to Q, NTT'd, times 2^64 (Montgomery form); decrypt(ct x pt) = m1 * m2 mod t,
    and a 3-term MAC with a partial sum decrypts to the dot product plus the partial message"""
    need_gpu()
    from oracle.client import Client
    P = params.BFV_DEFAULT[16384]
    ctx, o = _ctx(16384, P["q"], P["p"], P["t"])
    c = Client(o, seed=11)
    n, lvl, t = 16384, 2, P["t"]
    L = lvl + 1
    rng = np.random.default_rng(12)
    tm = np.uint64(t)

    def pt_mul(m):
        e = c.bfv_encode(m)
        return np.stack([o.vec("mul", j, o.ntt(j, e % np.uint64(o.q[j])), np.full(n, np.uint64(2 ** 64 % o.q[j]), dtype=np.uint64))
                         for j in range(L)])
    try:
        m1 = [rng.integers(0, t, size=n, dtype=np.uint64) for _ in range(3)]
        m2 = [rng.integers(0, t, size=n, dtype=np.uint64) for _ in range(3)]
        mp = rng.integers(0, t, size=n, dtype=np.uint64)
        cts = [c.bfv_encrypt(m, lvl) for m in m1]
        pts = [pt_mul(m) for m in m2]
        for fused in ("1", "0"):
            with env(LSA_PTMUL_FUSED=fused):
                got = ctx.download(ctx.bfv_mult_plain_mul(lvl, ctx.upload(cts[0][None]), ctx.upload(pts[0][None]), 1), (1, 2, L, n))[0]
                assert np.array_equal(c.bfv_decrypt(got), m1[0] * m2[0] % tm), fused
                part = c.bfv_encrypt(mp, lvl)
                mac = ctx.bfv_mac_plain_mul(lvl, [ctx.upload(x[None]) for x in cts], [ctx.upload(x[None]) for x in pts], 1,
                                            partial=ctx.upload(part[None]))
                got = ctx.download(mac, (1, 2, L, n))[0]
                exp = mp.copy()
                for a, b in zip(m1, m2):
                    exp = (exp + a * b % tm) % tm
                assert np.array_equal(c.bfv_decrypt(got), exp), fused
    finally:
        ctx.close()


def _load(name):
    from oracle.client import Client
    from oracle.pyoracle import Oracle
    g = json.load(open(os.path.join(TASKS, name, "mega_ag.json")))
    P = g["parameter"]
    o = Oracle(P["n"], P["q"][: P["max_level"] + 1], P["p"], P.get("t", 0))
    return g, P, o, Client(o, seed=len(name))


def _task(name):
    from lattisense_amd.task import FheTaskGpu
    return FheTaskGpu(os.path.join(TASKS, name))


@pytest.mark.parametrize("fused", ["1", "0"])
def test_task_fixtures(fused):
    """bfv_n4096_cmp_mul (4 x ct * pt_mul), bfv_n4096_cmpac_mul (3-term dot product: mult + cmpac_sum) and
    bfv_n16384_cmpac_mul20 (20 terms: 16-term cmp_sum + 4-term cmpac_sum) through FheTaskGpu"""
    need_gpu()
    from lattisense_amd.task import Argument, Ciphertext, Plaintext
    with env(LSA_PTMUL_FUSED=fused):
        g, P, o, c = _load("bfv_n4096_cmp_mul")
        n, lvl = P["n"], 2
        L = lvl + 1
        rng = np.random.default_rng(31)
        xs = [rand_ct(rng, o.q[:L], 2, n, 1)[0] for _ in range(4)]
        ys = [_rand_pt(rng, o.q[:L], n, 1)[0] for _ in range(4)]
        t = _task("bfv_n4096_cmp_mul")
        zs = [Ciphertext.empty(1, lvl, n) for _ in range(4)]
        t.run([Argument("xs", [Ciphertext(x) for x in xs]), Argument("ys", [Plaintext(y) for y in ys])], [Argument("zs", zs)])
        for i in range(4):
            assert np.array_equal(zs[i].data, _want_mac(o, L, [xs[i]], [ys[i]])), ("cmp_mul", i)
        t.close()
        for name, k, lvl in (("bfv_n4096_cmpac_mul", 3, 2), ("bfv_n16384_cmpac_mul20", 20, 5)):
            g, P, o, c = _load(name)
            n = P["n"]
            L = lvl + 1
            rng = np.random.default_rng(k)
            cs = [rand_ct(rng, o.q[:L], 2, n, 1)[0] for _ in range(k)]
            ps = [_rand_pt(rng, o.q[:L], n, 1)[0] for _ in range(k)]
            t = _task(name)
            z = [Ciphertext.empty(1, lvl, n)]
            t.run([Argument("cs", [Ciphertext(x) for x in cs]), Argument("ps", [Plaintext(p) for p in ps])], [Argument("zs", z)])
            want = np.zeros((2, L, n), dtype=np.uint64)
            for i in range(k):   # Lattigo's per-term multiply followed by adds
                prod = _want_mac(o, L, [cs[i]], [ps[i]])
                want = np.stack([np.stack([o.vec("add", j, want[pl, j], prod[pl, j]) for j in range(L)]) for pl in range(2)])
            assert np.array_equal(z[0].data, want), name
            t.close()
