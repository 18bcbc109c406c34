"""CKKS encrypted inner product on the device (lsa_ckks_mult_sum / lsa_ckks_dot; ops.hip ckks_mult_sum / ckks_dot, k_tensor_sum)
against the composition of the entry points that existed before it -- lsa_ckks_mult per pair, lsa_poly_addsub (three
polynomials; two for the addend), lsa_ckks_relin, lsa_ckks_rescale -- run in the same process, and against the same composition
on the CPU oracle (o.ckks_mult, o.vec("add", ...), o.ckks_relin, o.ckks_rescale) on one batch item.  Every comparison is word for
word.  Random residues as in tests/test_gpu_hmult_fold.py; the worst case runs every input residue at q - 1 on the 60-bit limbs of
the bootstrap chain, past the launch bound LSA_DOT_MAX_TERMS.  The last test encrypts real messages and holds the decrypted
precision of the lazy sum (one key-switch error) to that of the oracle's eager sum of HMults (one per term)."""
import ctypes
import re
import os

import numpy as np
import pytest

from lattisense_amd import params
from tests.gpu_util import need_gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSA_ERR_ARG = 1


def _max_terms():
    text = open(os.path.join(ROOT, "lattisense_amd", "csrc", "tensor_sum.h")).read()
    return int(re.search(r"#define LSA_DOT_MAX_TERMS (\d+)", text).group(1))


MAX_TERMS = _max_terms()


def _rand(rng, mods, shape, n):
    out = np.empty((*shape, len(mods), n), dtype=np.uint64)
    for i, m in enumerate(mods):
        out[..., i, :] = rng.integers(0, m, size=(*shape, n), dtype=np.uint64)
    return out


class Rig:
    def __init__(self, n, q, p, klvl, seed, fp64=True, fuse_tails=True):
        from lattisense_amd._native import check, lib
        from lattisense_amd.device import ALGO_CKKS, DeviceContext
        self.n, self.q, self.p, self.klvl = n, list(q), list(p), klvl
        self.rng = np.random.default_rng(seed)
        self.ctx = DeviceContext(ALGO_CKKS, n, q, p)
        if not fp64:
            self.ctx.set_fp64_ntt(0)
        if not fuse_tails:
            check(lib().lsa_set_fuse_tails(self.ctx.h, 0))
        beta = (klvl + 1 + len(p) - 1) // len(p)
        self.key = _rand(self.rng, self.q[: klvl + 1] + self.p, (beta, 2), n)
        self.k = self.ctx.upload_key(self.key, klvl)
        self._o = None

    @property
    def o(self):
        if self._o is None:
            from oracle.pyoracle import Oracle
            self._o = Oracle(self.n, self.q, self.p, 0)
        return self._o

    def ct(self, lvl, batch, polys=2):
        return _rand(self.rng, self.q[: lvl + 1], (batch, polys), self.n)

    def close(self):
        self.ctx.close()


def _arr(ctype, values):
    return (ctype * max(len(values), 1))(*values)


def raw_dot(ctx, lvl, a_ptrs, sas, a_rpp, b_ptrs, sbs, b_rpp, addend, s_addend, rlk, out_ptr, batch, sout, rescale):
    """lsa_ckks_dot with explicit pointers, strides and rows per polynomial; returns (return code, message)"""
    from lattisense_amd._native import lib
    n = len(a_ptrs)
    rc = lib().lsa_ckks_dot(ctx.h, lvl, n, _arr(ctypes.c_void_p, a_ptrs), _arr(ctypes.c_longlong, sas),
                            _arr(ctypes.c_int, a_rpp) if a_rpp is not None else None, _arr(ctypes.c_void_p, b_ptrs),
                            _arr(ctypes.c_longlong, sbs), _arr(ctypes.c_int, b_rpp) if b_rpp is not None else None, addend, s_addend,
                            rlk, out_ptr, batch, sout, int(rescale), ctx.stream)
    return rc, lib().lsa_last_error().decode()


def compose(ctx, lvl, dA, dB, k, batch, rescale, addend=None, want_d3=False):
    """the same sum from the entry points that existed before: mult per pair, additions, relin, rescale"""
    from lattisense_amd._native import check, lib
    L, N = lvl + 1, ctx.n
    d3 = ctx.ckks_mult(lvl, dA[0], dB[0], batch)
    for a, b in zip(dA[1:], dB[1:]):
        d3 = ctx.addsub(0, lvl, 3, d3, ctx.ckks_mult(lvl, a, b, batch), batch)
    if addend is not None:   # onto polynomials 0 and 1
        check(lib().lsa_poly_addsub(ctx.h, 0, lvl, 2, d3.ptr, addend.ptr, d3.ptr, batch, 3 * L * N, 2 * L * N, 3 * L * N, ctx.stream))
    if want_d3:
        return ctx.download(d3, (batch, 3, L, N))
    r = ctx.ckks_relin(lvl, d3, k, batch)
    if rescale:
        return ctx.download(ctx.ckks_rescale(lvl, 2, r, batch), (batch, 2, lvl, N))
    return ctx.download(r, (batch, 2, L, N))


def oracle_d3(o, lvl, As, Bs, addend=None):
    d = o.ckks_mult(lvl, As[0], Bs[0])
    for a, b in zip(As[1:], Bs[1:]):
        t = o.ckks_mult(lvl, a, b)
        for h in range(3):
            for j in range(lvl + 1):
                d[h, j] = o.vec("add", j, d[h, j], t[h, j])
    if addend is not None:
        for h in range(2):
            for j in range(lvl + 1):
                d[h, j] = o.vec("add", j, d[h, j], addend[h, j])
    return d


def oracle_dot(o, lvl, As, Bs, key, klvl, rescale, addend=None):
    """one batch item: As / Bs lists of [2][lvl+1][N]"""
    r = o.ckks_relin(lvl, oracle_d3(o, lvl, As, Bs, addend), key, klvl)
    return o.ckks_rescale(lvl, r) if rescale else r


def dot(rig, lvl, dA, dB, batch, rescale=True, addend=None):
    out = rig.ctx.ckks_dot(lvl, dA, dB, rig.k, batch, rescale=rescale, addend=addend)
    return rig.ctx.download(out, (batch, 2, lvl if rescale else lvl + 1, rig.n))


def test_headline_shape_tiles_streams_and_batch_positions():
    """N = 2^16, L = 13, k = 4, batch 3; n in {1, 2, 8, LSA_DOT_MAX_TERMS + 1}, with and without rescale and addend; tile batch
    0 / 1 / 2, single and dual stream; items 0 and 2 hold the same pairs; the oracle at n = 8"""
    need_gpu()
    from lattisense_amd._native import check, lib
    C = params.CKKS_DEFAULT[65536]
    rig = Rig(1 << 16, C["q"][:13], C["p"][:4], 12, 1601)
    ctx, lvl, batch = rig.ctx, 12, 3
    try:
        pool = 4   # the terms draw their operands from 4 + 4 ciphertexts: term i is a[i % 4] x b[(3 i + 1) % 4] (16 distinct pairs)
        hA, hB = [rig.ct(lvl, batch) for _ in range(pool)], [rig.ct(lvl, batch) for _ in range(pool)]
        hE = rig.ct(lvl, batch)
        for x in hA + hB + [hE]:
            x[2] = x[0]
        pA, pB, dE = [ctx.upload(x) for x in hA], [ctx.upload(x) for x in hB], ctx.upload(hE)
        ia = lambda i: i % pool                    # noqa: E731
        ib = lambda i: (3 * i + 1) % pool          # noqa: E731
        ref = {}
        for n in (1, 2, 8, MAX_TERMS + 1):
            dA, dB = [pA[ia(i)] for i in range(n)], [pB[ib(i)] for i in range(n)]
            for rescale in (True, False):
                for addend in (None, dE):
                    want = compose(ctx, lvl, dA, dB, rig.k, batch, rescale, addend)
                    got = dot(rig, lvl, dA, dB, batch, rescale, addend)
                    assert np.array_equal(got, want), (n, rescale, addend is not None)
                    assert np.array_equal(got[2], got[0]) and not np.array_equal(got[1], got[0])
                    ref[(n, rescale, addend is not None)] = want
        one = ctx.download(ctx.ckks_mult_relin_rescale(lvl, pA[ia(0)], pB[ib(0)], rig.k, batch), (batch, 2, lvl, rig.n))
        assert np.array_equal(ref[(1, True, False)], one)
        for rescale, addend in ((True, True), (False, False)):
            item = 1
            want = oracle_dot(rig.o, lvl, [hA[ia(i)][item] for i in range(8)], [hB[ib(i)][item] for i in range(8)], rig.key, rig.klvl,
                              rescale, hE[item] if addend else None)
            assert np.array_equal(ref[(8, rescale, addend)][item], want), ("oracle", rescale, addend)
        for dual in (0, 1):
            check(lib().lsa_set_dual_stream(ctx.h, dual))
            for tile in (0, 1, 2):
                ctx.set_tile_batch(tile)
                for n in (1, 2, 8, MAX_TERMS + 1):
                    dA, dB = [pA[ia(i)] for i in range(n)], [pB[ib(i)] for i in range(n)]
                    for rescale, addend in ((True, True), (False, False)):
                        got = dot(rig, lvl, dA, dB, batch, rescale, dE if addend else None)
                        assert np.array_equal(got, ref[(n, rescale, addend)]), (dual, tile, n, rescale)
    finally:
        rig.close()


def test_every_level_small_ring():
    """N = 2^13: levels 1..12 at n = 3; the oracle at levels 1, 4 and 12, there also under lsa_set_ntt_chunk_mib(1)"""
    need_gpu()
    C = params.CKKS_DEFAULT[65536]
    rig = Rig(1 << 13, C["q"][:13], C["p"][:4], 12, 1301)
    try:
        batch = 2
        for lvl in range(1, 13):
            hA, hB = [rig.ct(lvl, batch) for _ in range(3)], [rig.ct(lvl, batch) for _ in range(3)]
            hE = rig.ct(lvl, batch)
            dA, dB, dE = [rig.ctx.upload(x) for x in hA], [rig.ctx.upload(x) for x in hB], rig.ctx.upload(hE)
            for rescale, addend in ((True, None), (False, dE), (True, dE)):
                got = dot(rig, lvl, dA, dB, batch, rescale, addend)
                assert np.array_equal(got, compose(rig.ctx, lvl, dA, dB, rig.k, batch, rescale, addend)), (lvl, rescale)
                if lvl in (1, 4, 12) and rescale:
                    want = oracle_dot(rig.o, lvl, [x[1] for x in hA], [x[1] for x in hB], rig.key, rig.klvl, True,
                                      hE[1] if addend is not None else None)
                    assert np.array_equal(got[1], want), ("oracle", lvl)
                    rig.ctx.set_ntt_chunk_mib(1)          # the two-pass transforms in 1 MiB chunks: item 1 is in a later one
                    try:
                        cut = dot(rig, lvl, dA, dB, batch, rescale, addend)
                    finally:
                        rig.ctx.set_ntt_chunk_mib(0)
                    assert np.array_equal(cut[1], want) and np.array_equal(cut, got), ("ntt chunk", lvl)
    finally:
        rig.close()


def test_mult_sum_alone():
    """lsa_ckks_mult_sum against the oracle's summed ckks_mult and the device's own additions, level 0 included, across the
    launch bound"""
    need_gpu()
    C = params.CKKS_DEFAULT[65536]
    rig = Rig(1 << 13, C["q"][:13], C["p"][:4], 12, 1302)
    try:
        batch = 2
        for lvl, n in ((0, 1), (0, 3), (5, 2), (12, MAX_TERMS), (12, MAX_TERMS + 1), (3, 2 * MAX_TERMS + 3)):
            hA, hB = [rig.ct(lvl, batch) for _ in range(n)], [rig.ct(lvl, batch) for _ in range(n)]
            hE = rig.ct(lvl, batch)
            dA, dB, dE = [rig.ctx.upload(x) for x in hA], [rig.ctx.upload(x) for x in hB], rig.ctx.upload(hE)
            for addend in (None, dE):
                got = rig.ctx.download(rig.ctx.ckks_mult_sum(lvl, dA, dB, batch, addend=addend), (batch, 3, lvl + 1, rig.n))
                assert np.array_equal(got, compose(rig.ctx, lvl, dA, dB, rig.k, batch, False, addend, want_d3=True)), (lvl, n)
                want = oracle_d3(rig.o, lvl, [x[0] for x in hA], [x[0] for x in hB], hE[0] if addend is not None else None)
                assert np.array_equal(got[0], want), ("oracle", lvl, n)
    finally:
        rig.close()


def test_worst_case_residues_on_the_bootstrap_chain():
    """60-bit limbs and 60/61-bit special primes (integer-engine targets) at N = 2^14: every input residue q - 1 -- the largest
    128-bit sums -- at n = 9 and n = 33 (2 LSA_DOT_MAX_TERMS + 1 at the bound chosen here), and one random case"""
    need_gpu()
    P = params.CKKS_BOOTSTRAP_65536
    q, p = P["q"], P["p"]
    lvl = len(q) - 1
    rig = Rig(1 << 14, q, p, lvl, 1401)
    try:
        batch = 2
        top = np.empty((batch, 2, lvl + 1, rig.n), dtype=np.uint64)
        for j, m in enumerate(q):
            top[:, :, j, :] = m - 1
        dT = rig.ctx.upload(top)
        for n in (9, 33):
            for rescale, addend in ((True, dT), (False, None)):
                got = dot(rig, lvl, [dT] * n, [dT] * n, batch, rescale, addend)
                assert np.array_equal(got, compose(rig.ctx, lvl, [dT] * n, [dT] * n, rig.k, batch, rescale, addend)), (n, rescale)
                want = oracle_dot(rig.o, lvl, [top[0]] * n, [top[0]] * n, rig.key, rig.klvl, rescale, top[0] if addend is not None else None)
                assert np.array_equal(got[0], want), ("oracle", n, rescale)
        hA, hB = [rig.ct(lvl, batch) for _ in range(5)], [rig.ct(lvl, batch) for _ in range(5)]
        dA, dB = [rig.ctx.upload(x) for x in hA], [rig.ctx.upload(x) for x in hB]
        got = dot(rig, lvl, dA, dB, batch)
        assert np.array_equal(got, compose(rig.ctx, lvl, dA, dB, rig.k, batch, True))
        assert np.array_equal(got[1], oracle_dot(rig.o, lvl, [x[1] for x in hA], [x[1] for x in hB], rig.key, rig.klvl, True))
    finally:
        rig.close()


def test_mixed_levels_shared_operands_and_squares():
    """operands allocated two levels above `level` and read through their rows per polynomial; stride 0 on the b side (one
    ciphertext for the whole batch); as[i] == bs[i]"""
    need_gpu()
    C = params.CKKS_DEFAULT[65536]
    rig = Rig(1 << 13, C["q"][:13], C["p"][:4], 12, 1303)
    ctx, N = rig.ctx, rig.n
    try:
        lvl, batch, n = 6, 3, 4
        L, up = lvl + 1, lvl + 3
        # mixed levels: a_0, a_2 and b_1 sit at level + 2 (rows per polynomial `up`), the others at `level`
        high_a, high_b = (0, 2), (1,)
        hA = [rig.ct(lvl + 2 if i in high_a else lvl, batch) for i in range(n)]
        hB = [rig.ct(lvl + 2 if i in high_b else lvl, batch) for i in range(n)]
        dA, dB = [ctx.upload(x) for x in hA], [ctx.upload(x) for x in hB]
        lowA = [np.ascontiguousarray(x[:, :, :L, :]) for x in hA]
        lowB = [np.ascontiguousarray(x[:, :, :L, :]) for x in hB]
        cA, cB = [ctx.upload(x) for x in lowA], [ctx.upload(x) for x in lowB]
        for rescale in (True, False):
            rows = lvl if rescale else L
            out = ctx.alloc(batch * 2 * rows * N)
            rc, msg = raw_dot(ctx, lvl, [x.ptr for x in dA], [2 * (up if i in high_a else L) * N for i in range(n)],
                              [up if i in high_a else 0 for i in range(n)], [x.ptr for x in dB],
                              [2 * (up if i in high_b else L) * N for i in range(n)], [up if i in high_b else L for i in range(n)],
                              None, 0, rig.k, out.ptr, batch, 2 * rows * N, rescale)
            assert rc == 0, msg
            got = ctx.download(out, (batch, 2, rows, N))
            assert np.array_equal(got, compose(ctx, lvl, cA, cB, rig.k, batch, rescale)), ("mixed levels", rescale)
            want = oracle_dot(rig.o, lvl, [x[2] for x in lowA], [x[2] for x in lowB], rig.key, rig.klvl, rescale)
            assert np.array_equal(got[2], want), ("mixed levels, oracle", rescale)
        # shared operands: every b is ONE ciphertext (batch stride 0), e.g. an encrypted weight
        hW = [rig.ct(lvl, 1) for _ in range(n)]
        dW = [ctx.upload(x) for x in hW]
        wide = [ctx.upload(np.repeat(x, batch, axis=0)) for x in hW]
        out = ctx.alloc(batch * 2 * lvl * N)
        rc, msg = raw_dot(ctx, lvl, [x.ptr for x in cA], [2 * L * N] * n, None, [x.ptr for x in dW], [0] * n, None, None, 0, rig.k,
                          out.ptr, batch, 2 * lvl * N, True)
        assert rc == 0, msg
        got = ctx.download(out, (batch, 2, lvl, N))
        assert np.array_equal(got, compose(ctx, lvl, cA, wide, rig.k, batch, True)), "stride 0"
        assert np.array_equal(got[1], oracle_dot(rig.o, lvl, [x[1] for x in lowA], [x[0] for x in hW], rig.key, rig.klvl, True))
        # squares: the squared norm sum_i a_i^2
        got = dot(rig, lvl, cA, cA, batch)
        assert np.array_equal(got, compose(ctx, lvl, cA, cA, rig.k, batch, True)), "squares"
        assert np.array_equal(got[0], oracle_dot(rig.o, lvl, [x[0] for x in lowA], [x[0] for x in lowA], rig.key, rig.klvl, True))
    finally:
        rig.close()


@pytest.mark.parametrize("mode", ["fp64_off", "LSA_KS_FUSED=0", "fuse_tails_off"])
def test_switches(mode, monkeypatch):
    """the same words as the default and as the oracle under the switches that select other kernels below the operator: the
    integer NTT engine (a context setting), the unfused key MAC (LSA_KS_FUSED, read per call) and unfused tails (a context
    setting: key switch and rescale as two steps)"""
    need_gpu()
    C = params.CKKS_DEFAULT[65536]
    n, q, p = 1 << 16, C["q"][:6], C["p"][:2]
    lvl, batch, terms = 5, 2, 3
    base = Rig(n, q, p, lvl, 77)
    hA, hB = [base.ct(lvl, batch) for _ in range(terms)], [base.ct(lvl, batch) for _ in range(terms)]
    hE = base.ct(lvl, batch)
    ref = {}
    try:
        dA, dB, dE = [base.ctx.upload(x) for x in hA], [base.ctx.upload(x) for x in hB], base.ctx.upload(hE)
        for rescale in (True, False):
            ref[rescale] = dot(base, lvl, dA, dB, batch, rescale, dE)
            want = oracle_dot(base.o, lvl, [x[1] for x in hA], [x[1] for x in hB], base.key, lvl, rescale, hE[1])
            assert np.array_equal(ref[rescale][1], want), ("default against the oracle", rescale)
    finally:
        base.close()
    if mode == "LSA_KS_FUSED=0":
        monkeypatch.setenv("LSA_KS_FUSED", "0")
    rig = Rig(n, q, p, lvl, 77, fp64=mode != "fp64_off", fuse_tails=mode != "fuse_tails_off")   # the same seed: the same key
    try:
        assert np.array_equal(rig.key, base.key)
        dA, dB, dE = [rig.ctx.upload(x) for x in hA], [rig.ctx.upload(x) for x in hB], rig.ctx.upload(hE)
        for rescale in (True, False):
            got = dot(rig, lvl, dA, dB, batch, rescale, dE)
            assert np.array_equal(got, ref[rescale]), (mode, rescale)
            assert np.array_equal(got, compose(rig.ctx, lvl, dA, dB, rig.k, batch, rescale, dE)), (mode, rescale)
    finally:
        rig.close()


def test_argument_errors():
    """every argument error returns LSA_ERR_ARG with a message that begins "dot", queues nothing, and leaves the context usable"""
    need_gpu()
    from lattisense_amd._native import lib
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    C = params.CKKS_DEFAULT[65536]
    rig = Rig(1 << 12, C["q"][:6], C["p"][:2], 5, 1201)
    ctx, N = rig.ctx, rig.n
    try:
        lvl, batch, n = 3, 2, 2
        L = lvl + 1
        w, wo, w3 = 2 * L * N, 2 * lvl * N, 3 * L * N
        hA, hB = [rig.ct(lvl, batch) for _ in range(n)], [rig.ct(lvl, batch) for _ in range(n)]
        dA, dB, dE = [ctx.upload(x) for x in hA], [ctx.upload(x) for x in hB], ctx.upload(rig.ct(lvl, batch))
        ref = dot(rig, lvl, dA, dB, batch, True, dE)
        out = ctx.upload(np.full(batch * w3, 7, dtype=np.uint64))   # large enough for either entry point
        pa, pb = [x.ptr for x in dA], [x.ptr for x in dB]

        def call(which, c=ctx, level=lvl, a=pa, sa=(w, w), ra=None, b=pb, sb=(w, w), rb=None, e=dE.ptr, se=w, o=out.ptr, bt=batch, so=None,
                 rescale=1, drop_arrays=()):
            nn = len(a)
            A = None if "as" in drop_arrays else _arr(ctypes.c_void_p, list(a))
            SA = None if "sas" in drop_arrays else _arr(ctypes.c_longlong, list(sa))
            B = None if "bs" in drop_arrays else _arr(ctypes.c_void_p, list(b))
            SB = None if "sbs" in drop_arrays else _arr(ctypes.c_longlong, list(sb))
            RA = _arr(ctypes.c_int, list(ra)) if ra is not None else None
            RB = _arr(ctypes.c_int, list(rb)) if rb is not None else None
            if which == "dot":
                so_ = so if so is not None else (2 * level * N if rescale else 2 * (level + 1) * N)
                rc = lib().lsa_ckks_dot(c.h, level, nn, A, SA, RA, B, SB, RB, e, se, rig.k, o, bt, so_, rescale, ctx.stream)
            else:
                so_ = so if so is not None else 3 * (level + 1) * N
                rc = lib().lsa_ckks_mult_sum(c.h, level, nn, A, SA, RA, B, SB, RB, e, se, o, bt, so_, ctx.stream)
            return rc, lib().lsa_last_error().decode()

        def fails(needle="", **kw):
            for which in ("dot", "sum"):
                if which == "sum" and kw.get("rescale_only"):
                    continue
                args = {k: v for k, v in kw.items() if k != "rescale_only"}
                rc, msg = call(which, **args)
                assert rc == LSA_ERR_ARG, (which, kw, rc, msg)
                assert msg.startswith("dot") and needle in msg, (which, kw, msg)

        B = params.BFV_DEFAULT[8192]
        bfv = DeviceContext(ALGO_BFV, 8192, B["q"], B["p"], B["t"])
        fails("CKKS", c=bfv, level=0)
        bfv.close()
        fails("term", a=[], b=[], sa=[], sb=[])                       # n < 1
        fails("level", level=6)
        fails("level", level=-1)
        fails("rescale", level=0, rescale_only=True)                  # rescale with level < 1
        fails("rows per polynomial", ra=(L - 1, 0))
        fails("rows per polynomial", rb=(0, 1))
        fails("stride", sa=(w - 1, w))
        fails("stride", sb=(w, -w))
        fails("stride", ra=(L + 1, 0))                                # a stride of 2 L N under rows per polynomial L + 1
        fails("stride", se=w - 1)
        fails("null", a=(pa[0], None))
        fails("null", b=(None, pb[1]))
        fails("null", drop_arrays=("as",))
        fails("null", drop_arrays=("sbs",))
        fails("null", o=None)
        fails("overlap", o=pa[1])
        fails("overlap", o=pb[0] + 8 * N)
        fails("overlap", o=dE.ptr)
        fails("overlap", o=pb[0], sb=(0, w))                          # a shared operand is still an input
        rc, msg = raw_dot(ctx, lvl, pa, [w, w], None, pb, [w, w], None, None, 0, None, out.ptr, batch, wo, True)
        assert rc == LSA_ERR_ARG and msg.startswith("dot"), msg       # no key
        assert np.all(ctx.download(out, (batch * w3,)) == 7)           # nothing was queued
        for which in ("dot", "sum"):                                  # batch <= 0: a no-op
            for bt in (0, -1):
                rc, msg = call(which, bt=bt)
                assert rc == 0, msg
        assert np.all(ctx.download(out, (batch * w3,)) == 7)
        assert np.array_equal(dot(rig, lvl, dA, dB, batch, True, dE), ref)   # the context stays usable
    finally:
        rig.close()


def test_semantics_and_precision_against_the_eager_sum():
    """N = 2^12, 6 pairs of encrypted random complex vectors: the device words equal the oracle composition's, the message is
    sum_i x_i y_i, and the lazy sum (one key-switch error) decrypts at least as precisely as the oracle's eager sum of six
    ckks_mult_relin_rescale (six key-switch errors), less 1 bit for the different rounding terms"""
    need_gpu()
    from lattisense_amd.device import ALGO_CKKS, DeviceContext
    from oracle.client import Client, mean_precision_bits
    from oracle.pyoracle import Oracle
    C = params.CKKS_DEFAULT[65536]
    N, q, p = 1 << 12, C["q"][:6], C["p"][:2]
    lvl, terms = 5, 6
    scale = float(q[lvl])
    o = Oracle(N, q, p, 0)
    c = Client(o, seed=12)
    rlk = c.gen_relin_key(lvl)
    rng = np.random.default_rng(12)
    xs = [rng.uniform(-1, 1, N // 2) + 1j * rng.uniform(-1, 1, N // 2) for _ in range(terms)]
    ys = [rng.uniform(-1, 1, N // 2) + 1j * rng.uniform(-1, 1, N // 2) for _ in range(terms)]
    A = [c.ckks_encrypt(x, lvl, scale) for x in xs]
    B = [c.ckks_encrypt(y, lvl, scale) for y in ys]
    ctx = DeviceContext(ALGO_CKKS, N, q, p)
    try:
        k = ctx.upload_key(rlk, lvl)
        out = ctx.ckks_dot(lvl, [ctx.upload(a[None]) for a in A], [ctx.upload(b[None]) for b in B], k, 1)
        got = ctx.download(out, (1, 2, lvl, N))[0]
    finally:
        ctx.close()
    assert np.array_equal(got, oracle_dot(o, lvl, A, B, rlk, lvl, True))
    eager = o.ckks_mult_relin_rescale(lvl, A[0], B[0], rlk, lvl)
    for a, b in zip(A[1:], B[1:]):
        t = o.ckks_mult_relin_rescale(lvl, a, b, rlk, lvl)
        for h in range(2):
            for j in range(lvl):
                eager[h, j] = o.vec("add", j, eager[h, j], t[h, j])
    assert not np.array_equal(got, eager)          # a new operator, not a re-expression of the eager sum
    want = sum(x * y for x, y in zip(xs, ys))
    out_scale = scale * scale / q[lvl]
    lazy_bits = mean_precision_bits(want, c.ckks_decrypt(got, out_scale))
    eager_bits = mean_precision_bits(want, c.ckks_decrypt(eager, out_scale))
    print("lazy %.2f / %.2f bits, eager %.2f / %.2f bits (real / imaginary)" % (*lazy_bits, *eager_bits))
    assert min(lazy_bits) >= 10
    assert lazy_bits[0] >= eager_bits[0] - 1 and lazy_bits[1] >= eager_bits[1] - 1, (lazy_bits, eager_bits)
