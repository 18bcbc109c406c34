"""Hoisted BFV rotate-and-MAC (lsa_bfv_rotate_mac_plain_mul): out = sum_i rot_{g_i}(ct) . pt_i (+ partial), the rotations
kept in the NTT domain (the fz_epi = 4 epilogue: ModDown tail, automorphism, pt_mul product and running sum in the last
store of the conversion's forward transform).  Every result is compared bit for bit with the GPU composition
lsa_bfv_rotate_many + lsa_bfv_mac_plain_mul and with the CPU oracle (Oracle.bfv_rotate per term, then
sum INTT(NTT(.) . pt . 2^-64)), under both forms (LSA_ROTMAC_FUSED), fused and unfused tails, LSA_ROT_SCATTER, both
butterfly engines and tile batch default and 1; at N = 2^12 (FP64 engine), every level of the N = 2^14 chain, the full
N = 2^15 and N = 2^16 rings; at message level; and for every refusal."""
import ctypes
import os

import numpy as np
import pytest

from lattisense_amd import params
from tests.gpu_util import env, need_gpu, rand_ct

pytestmark = pytest.mark.gpu


def _minv(q):
    return np.uint64(pow(2 ** 64, -1, int(q)))


def _rand_key(rng, q, p, klvl, n):
    beta = (klvl + 1 + len(p) - 1) // len(p)
    key = np.empty((beta, 2, klvl + 1 + len(p), n), dtype=np.uint64)
    for j, m in enumerate(q[: klvl + 1] + p):
        key[:, :, j, :] = rng.integers(0, m, size=(beta, 2, n), dtype=np.uint64)
    return key


def _rand_pt(rng, mods, n, batch):
    return rand_ct(rng, mods, 1, n, batch)[:, 0]


class _Ring:
    """a BFV context, its oracle, random Galois keys at the top level (uploaded and raw) and helpers for one level"""

    def __init__(self, n, q, p, t, els, seed):
        from lattisense_amd.device import ALGO_BFV, DeviceContext
        from oracle.pyoracle import Oracle
        self.ctx = DeviceContext(ALGO_BFV, n, q, p, t)
        self.o = Oracle(n, q, p, t)
        self.n, self.q, self.p = n, q, p
        self.klvl = len(q) - 1
        self.rng = np.random.default_rng(seed)
        self.raw = {g: _rand_key(self.rng, q, p, self.klvl, n) for g in els}
        self.keys = {g: self.ctx.upload_key(self.raw[g], self.klvl) for g in els}

    def close(self):
        for k in self.keys.values():
            self.ctx.destroy_key(k)
        self.ctx.close()

    def data(self, lvl, k, batch, partial):
        L = lvl + 1
        A = rand_ct(self.rng, self.q[:L], 2, self.n, batch)
        Ps = [_rand_pt(self.rng, self.q[:L], self.n, batch) for _ in range(k)]
        Pa = rand_ct(self.rng, self.q[:L], 2, self.n, batch) if partial else None
        return A, Ps, Pa

    def fused(self, lvl, da, els, dps, batch, dpa):
        terms = [(g, None if g == 1 else self.keys[g], dp) for g, dp in zip(els, dps)]
        out = self.ctx.bfv_rotate_mac_plain_mul(lvl, da, terms, batch, partial=dpa)
        return self.ctx.download(out, (batch, 2, lvl + 1, self.n))

    def composition(self, lvl, da, els, dps, batch, dpa):
        rot = sorted({g for g in els if g != 1})
        outs = self.ctx.bfv_rotate_many(lvl, da, {g: self.keys[g] for g in rot}, batch) if rot else {}
        cts = [da if g == 1 else outs[g] for g in els]
        out = self.ctx.bfv_mac_plain_mul(lvl, cts, dps, batch, partial=dpa)
        return self.ctx.download(out, (batch, 2, lvl + 1, self.n))

    def want(self, lvl, A, els, pts, Pa):
        """the oracle for one batch item: Oracle.bfv_rotate per term, sum_i INTT(NTT(rot_i) . pt_i . 2^-64) (+ partial)"""
        o, L = self.o, lvl + 1
        rots = [A if g == 1 else o.bfv_rotate(lvl, A, g, self.raw[g], self.klvl) for g in els]
        out = np.empty((2, L, self.n), dtype=np.uint64)
        for j in range(L):
            r = np.full(self.n, _minv(o.q[j]), dtype=np.uint64)
            for pl in range(2):
                acc = np.zeros(self.n, dtype=np.uint64)
                for ct, pt in zip(rots, pts):
                    acc = o.vec("add", j, acc, o.vec("mul", j, o.ntt(j, ct[pl, j]), o.vec("mul", j, pt[j], r)))
                v = o.intt(j, acc)
                out[pl, j] = o.vec("add", j, v, Pa[pl, j]) if Pa is not None else v
        return out

    def check(self, lvl, els, batch=2, partial=True, oracle_items=(0,), tag=()):
        A, Ps, Pa = self.data(lvl, len(els), batch, partial)
        da, dps = self.ctx.upload(A), [self.ctx.upload(x) for x in Ps]
        dpa = self.ctx.upload(Pa) if partial else None
        got = self.fused(lvl, da, els, dps, batch, dpa)
        ref = self.composition(lvl, da, els, dps, batch, dpa)
        assert np.array_equal(got, ref), ("composition",) + tuple(tag)
        for b in oracle_items:
            want = self.want(lvl, A[b], els, [p[b] for p in Ps], Pa[b] if partial else None)
            assert np.array_equal(got[b], want), ("oracle", b) + tuple(tag)
        return got


def _els(n, steps, row=True):
    from oracle.client import galois_element_for_col_rotation, galois_element_for_row_rotation
    return [galois_element_for_col_rotation(s, n) for s in steps] + ([galois_element_for_row_rotation(n)] if row else [])


@pytest.mark.parametrize("form", ["1", "0"])
def test_n4096_fp64_engine(form):
    """N = 2^12 (primes below 2^47: the FP64 engine, single-pass plan), engine on and off, tile batch default and 1"""
    need_gpu()
    P = params.BFV_DEFAULT[4096]
    els = _els(4096, [1, 3, -7])
    r = _Ring(4096, P["q"], P["p"], P["t"], els, 4096 + int(form))
    try:
        with env(LSA_ROTMAC_FUSED=form):
            for fp64 in (1, 0):
                r.ctx.set_fp64_ntt(fp64)
                for tile in (0, 1):
                    r.ctx.set_tile_batch(tile)
                    top = len(P["q"]) - 1
                    r.check(top, [1] + els, batch=3, tag=(form, fp64, tile))
                    r.check(0, [els[1], 1, els[3]], batch=2, partial=False, oracle_items=(), tag=(form, fp64, tile, 0))
    finally:
        r.ctx.set_fp64_ntt(1)
        r.ctx.set_tile_batch(0)
        r.close()


@pytest.fixture(scope="module")
def n14():
    P = params.BFV_DEFAULT[16384]
    els = _els(16384, [1, 2, 3, -900, 4095])
    r = _Ring(16384, P["q"], P["p"], P["t"], els, 16384)
    yield r, els
    r.close()


def test_n14_every_level(n14):
    """the default N = 2^14 chain at every level: identity and four rotations plus the row rotation, with a partial sum"""
    need_gpu()
    r, els = n14
    for lvl in range(len(r.q)):
        r.check(lvl, [1] + els, batch=2, oracle_items=(1,) if lvl in (0, len(r.q) - 1) else (), tag=(lvl,))


def test_n14_switches(n14):
    """both forms x fused / unfused tails x LSA_ROT_SCATTER x tile batch: the same residues as the composition"""
    need_gpu()
    from lattisense_amd._native import check, lib
    r, els = n14
    lvl = 3
    terms = [1, els[0], els[3], els[-1], els[0]]
    A, Ps, Pa = r.data(lvl, len(terms), 3, True)
    da, dps, dpa = r.ctx.upload(A), [r.ctx.upload(x) for x in Ps], r.ctx.upload(Pa)
    ref = r.composition(lvl, da, terms, dps, 3, dpa)
    assert np.array_equal(ref[2], r.want(lvl, A[2], terms, [p[2] for p in Ps], Pa[2]))
    try:
        for form in ("1", "0"):
            for scatter in ("1", "0"):
                with env(LSA_ROTMAC_FUSED=form, LSA_ROT_SCATTER=scatter):
                    for fuse in (1, 0):
                        check(lib().lsa_set_fuse_tails(r.ctx.h, fuse))
                        for tile in (0, 1):
                            r.ctx.set_tile_batch(tile)
                            got = r.fused(lvl, da, terms, dps, 3, dpa)
                            assert np.array_equal(got, ref), (form, scatter, fuse, tile)
    finally:
        check(lib().lsa_set_fuse_tails(r.ctx.h, 1))
        r.ctx.set_tile_batch(0)


def test_n14_term_shapes(n14):
    """identity first / later / absent / alone, a repeated element, the row rotation, n = 1, with and without partial"""
    need_gpu()
    r, els = n14
    lvl = 5
    row = els[-1]
    shapes = [[els[1]], [1], [row], [els[0], 1, els[2]], [els[0], els[0], els[0]], [1, 1, row], [row, els[3], 1, els[1]]]
    for i, sh in enumerate(shapes):
        for partial in (False, True):
            r.check(lvl, sh, batch=2, partial=partial, oracle_items=(0,) if i in (0, 3, 5) else (), tag=(i, partial))


def test_n14_batch_position_independent(n14):
    """the same ciphertext gives the same result at every batch position, both forms"""
    need_gpu()
    r, els = n14
    lvl, batch = 4, 5
    L = lvl + 1
    one = rand_ct(r.rng, r.q[:L], 2, r.n, 1)
    pts = [_rand_pt(r.rng, r.q[:L], r.n, 1) for _ in range(3)]
    da = r.ctx.upload(np.repeat(one, batch, axis=0))
    dps = [r.ctx.upload(np.repeat(p, batch, axis=0)) for p in pts]
    terms = [els[2], 1, els[4]]
    res = {}
    for form in ("1", "0"):
        with env(LSA_ROTMAC_FUSED=form):
            res[form] = r.fused(lvl, da, terms, dps, batch, None)
            for b in range(batch):
                assert np.array_equal(res[form][b], res[form][0]), (form, b)
    assert np.array_equal(res["1"], res["0"])
    assert np.array_equal(res["1"][0], r.want(lvl, one[0], terms, [p[0] for p in pts], None))


def test_n14_refusals(n14):
    """bad arguments raise LSA_ERR_ARG-class errors and leave the device usable; batch <= 0 is a no-op"""
    need_gpu()
    from lattisense_amd._native import LsaError, check, lib
    r, els = n14
    ctx, n = r.ctx, r.n
    lvl, batch = 2, 2
    L = lvl + 1
    s = 2 * L * n
    A, Ps, Pa = r.data(lvl, 2, batch, True)
    da, dp, dpa = ctx.upload(A), ctx.upload(Ps[0]), ctx.upload(Pa)
    out = ctx.alloc(batch * s)

    def call(gs, keys, pts, partial, o, b=batch, cnt=None):
        m = len(gs) if cnt is None else cnt
        k = max(len(gs), 1)
        return lib().lsa_bfv_rotate_mac_plain_mul(ctx.h, lvl, da.ptr, m, (ctypes.c_uint64 * k)(*gs),
                                                  (ctypes.c_void_p * k)(*[x.value if x is not None else None for x in keys]),
                                                  (ctypes.c_void_p * k)(*pts), (ctypes.c_longlong * k)(*([L * n] * k)),
                                                  partial, s, o, b, s, s, ctx.stream)

    g = els[0]
    cases = {
        "no terms": ([g], [r.keys[g]], [dp.ptr], None, out.ptr, batch, 0),
        "null key": ([g], [None], [dp.ptr], None, out.ptr, batch, None),
        "even element": ([4], [r.keys[g]], [dp.ptr], None, out.ptr, batch, None),
        "element out of range": ([2 * n + 1], [r.keys[g]], [dp.ptr], None, out.ptr, batch, None),
        "out is the input": ([g], [r.keys[g]], [dp.ptr], None, da.ptr, batch, None),
        "out is a plaintext": ([1, g], [None, r.keys[g]], [out.ptr, dp.ptr], None, out.ptr, batch, None),
        "out is the partial": ([g], [r.keys[g]], [dp.ptr], out.ptr, out.ptr, batch, None),
    }
    for name, (gs, keys, pts, partial, o, b, cnt) in cases.items():
        with pytest.raises(LsaError) as e:
            check(call(gs, keys, pts, partial, o, b, cnt))
        assert e.value.code == 1, (name, e.value)   # LSA_ERR_ARG
    assert call([g], [r.keys[g]], [dp.ptr], None, out.ptr, b=0) == 0
    # still usable
    r.check(lvl, [1, g], batch=1, partial=False, oracle_items=(0,))


def test_n15_full_ring():
    """the reference's N = 2^15 set (12 Q + 3 P) at the full ring: identity plus three rotations with a partial sum"""
    need_gpu()
    P = params.BFV_DEFAULT[32768]
    els = _els(32768, [1, -5], row=True)
    r = _Ring(32768, P["q"], P["p"], P["t"], els, 32768)
    try:
        for form in ("1", "0"):
            with env(LSA_ROTMAC_FUSED=form):
                r.rng = np.random.default_rng(15)
                r.check(len(P["q"]) - 1, [1] + els, batch=1, tag=(form,))
    finally:
        r.close()


def test_n16_chain_full_ring():
    """the N = 2^16 chain (24 Q + 4 P) at the full ring: three rotations and an identity term, both forms"""
    need_gpu()
    C = params.bfv_n16_chain()
    els = _els(C["n"], [1, 7], row=True)
    r = _Ring(C["n"], C["q"], C["p"], C["t"], els, 65536)
    try:
        for form in ("1", "0"):
            with env(LSA_ROTMAC_FUSED=form):
                r.check(len(C["q"]) - 1, els + [1], batch=1, tag=(form,))
    finally:
        r.close()


def test_decrypts_to_rotated_dot_product():
    """oracle client keys: decrypt(out) == sum_i rot_i(m) * m_i + m_partial mod t, slot for slot"""
    need_gpu()
    from oracle.client import Client
    P = params.BFV_DEFAULT[16384]
    n, t, lvl = 16384, P["t"], 3
    L = lvl + 1
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    from oracle.pyoracle import Oracle
    ctx = DeviceContext(ALGO_BFV, n, P["q"], P["p"], t)
    o = Oracle(n, P["q"], P["p"], t)
    c = Client(o, seed=77)
    rng = np.random.default_rng(78)
    tm = np.uint64(t)
    steps = [None, 1, 5, -300, "row"]
    els = [1] + _els(n, [1, 5, -300])
    klvl = len(P["q"]) - 1
    raw = {g: c.gen_galois_key(g, klvl) for g in els if g != 1}
    keys = {g: ctx.upload_key(raw[g], klvl) for g in raw}

    def pt_mul(m):
        e = c.bfv_encode(m)
        return np.stack([o.vec("mul", j, o.ntt(j, e % np.uint64(o.q[j])), np.full(n, np.uint64(2 ** 64 % o.q[j]), dtype=np.uint64))
                         for j in range(L)])
    try:
        x = rng.integers(0, t, size=n, dtype=np.uint64)
        ms = [rng.integers(0, t, size=n, dtype=np.uint64) for _ in els]
        mp = rng.integers(0, t, size=n, dtype=np.uint64)
        A = c.bfv_encrypt(x, lvl)[None]
        part = c.bfv_encrypt(mp, lvl)[None]
        h = n // 2
        exp = mp.copy()
        for s, m in zip(steps, ms):
            if s is None:
                r = x
            elif s == "row":
                r = np.concatenate([x[h:], x[:h]])
            else:
                r = np.concatenate([np.roll(x[:h], -s), np.roll(x[h:], -s)])
            exp = (exp + r * m % tm) % tm
        for form in ("1", "0"):
            with env(LSA_ROTMAC_FUSED=form):
                terms = [(g, keys.get(g), ctx.upload(pt_mul(m)[None])) for g, m in zip(els, ms)]
                out = ctx.bfv_rotate_mac_plain_mul(lvl, ctx.upload(A), terms, 1, partial=ctx.upload(part))
                got = ctx.download(out, (1, 2, L, n))[0]
                assert np.array_equal(c.bfv_decrypt(got), exp), form
    finally:
        for k in keys.values():
            ctx.destroy_key(k)
        ctx.close()


# ---------------------------------------------------------------- task runtime: the FUSED_ROTATE_MAC peephole
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASKS = os.path.join(ROOT, "tests", "golden", "tasks")
# fixture: GPU batches with the peephole (one per FUSED_ROTATE_MAC node) and without it (LSA_NO_GRAPH_FUSION=1: the hoisted
# rotations, the product and the MAC nodes)
RUNTIME = {"bfv_n4096_rotmac4": (2, 4), "bfv_n4096_rotmac_row_partial": (1, 2), "bfv_n4096_rotmac_shared": (2, 2),
           "bfv_n16384_rotmac20": (2, 3)}


def _run_fixture(name, seed):
    """runs the fixture through FheTaskGpu with random inputs; returns (outputs, oracle outputs node by node, stats)"""
    import copy
    import json
    from lattisense_amd.task import FheTaskGpu
    from tests import ref_suite as rs
    path = os.path.join(TASKS, name)
    g = json.load(open(os.path.join(path, "mega_ag.json")))
    o = rs.oracle_for(g)
    g2 = copy.deepcopy(g)   # pt_mul inputs have a pt's shape: the suite's input helpers take them as pt
    for d in g2["data"].values():
        if d["type"] == "pt_mul":
            d["type"] = "pt"
    vals, keys = rs.random_inputs(g2, o, np.random.default_rng(seed))
    ins, outs, out_cts = rs.arguments(g2, vals, keys)
    t = FheTaskGpu(path)
    try:
        t.run(ins, outs)
        st = t.last_run_stats()
    finally:
        t.close()
    data, v = g["data"], dict(vals)

    def ptmul(lvl, ct, pt):   # INTT(NTT(ct) . pt . 2^-64) per poly and limb
        r = np.empty_like(ct)
        for j in range(lvl + 1):
            w = o.vec("mul", j, pt[j], np.full(o.n, _minv(o.q[j]), dtype=np.uint64))
            for pl in range(ct.shape[0]):
                r[pl, j] = o.intt(j, o.vec("mul", j, o.ntt(j, ct[pl, j]), w))
        return r

    def add(lvl, a, b):
        return np.stack([np.stack([o.vec("add", j, a[pl, j], b[pl, j]) for j in range(lvl + 1)]) for pl in range(a.shape[0])])

    for node in rs.order(g):   # the oracle node by node, on the graph as the frontend wrote it
        ins_, out, ty = node["inputs"], node["outputs"][0], node["type"]
        lvl = data[str(ins_[0])]["level"]
        if ty in ("rotate_col", "rotate_row"):
            k, klvl = keys[ins_[1]]
            v[out] = o.bfv_rotate(lvl, v[ins_[0]], data[str(ins_[1])]["galois_element"], k, klvl)
        elif ty == "mult":
            a, b = ins_
            ct, pt = (a, b) if data[str(b)]["type"] == "pt_mul" else (b, a)
            v[out] = ptmul(lvl, v[ct], v[pt])
        elif ty in ("cmp_sum", "cmpac_sum"):
            m = node["sum_cnt"]
            pt0 = m + (1 if ty == "cmpac_sum" else 0)
            r = v[ins_[m]] if ty == "cmpac_sum" else None
            for i in range(m):
                p = ptmul(lvl, v[ins_[i]], v[ins_[pt0 + i]])
                r = p if r is None else add(lvl, r, p)
            v[out] = r
        else:
            raise NotImplementedError(ty)
    return [c.data for c in out_cts], [v[i] for i in g["outputs"]], st


@pytest.mark.parametrize("name", sorted(RUNTIME))
def test_runtime_fixtures(name):
    """each fixture through FheTaskGpu equals the oracle evaluated node by node; the GPU batch count shows the peephole fired
    (or, for _shared, did not); LSA_NO_GRAPH_FUSION=1 gives the same outputs"""
    need_gpu()
    fused, plain = RUNTIME[name]
    got, want, st = _run_fixture(name, 7)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (name, k)
    assert st["gpu_batches"] == fused, (name, st)
    with env(LSA_NO_GRAPH_FUSION="1"):
        got2, _, st2 = _run_fixture(name, 7)
    for a, b in zip(got, got2):
        assert np.array_equal(a, b), name
    assert st2["gpu_batches"] == plain, (name, st2)
    with env(LSA_ROTMAC_FUSED="0"):
        got3, _, _ = _run_fixture(name, 7)
    for a, b in zip(got, got3):
        assert np.array_equal(a, b), name


def test_n14_plaintext_stride_zero(n14):
    """spts[i] == 0: one plaintext for the whole batch, the same result as the plaintext repeated per batch item"""
    need_gpu()
    from lattisense_amd._native import check, lib
    r, els = n14
    ctx, n = r.ctx, r.n
    lvl, batch = 2, 3
    L = lvl + 1
    s = 2 * L * n
    A = rand_ct(r.rng, r.q[:L], 2, n, batch)
    pts = [_rand_pt(r.rng, r.q[:L], n, 1) for _ in range(2)]
    da = ctx.upload(A)
    terms = [1, els[1]]
    want = r.fused(lvl, da, terms, [ctx.upload(np.repeat(p, batch, axis=0)) for p in pts], batch, None)
    one = [ctx.upload(p) for p in pts]
    out = ctx.alloc(batch * s)
    for form in ("1", "0"):
        with env(LSA_ROTMAC_FUSED=form):
            check(lib().lsa_bfv_rotate_mac_plain_mul(ctx.h, lvl, da.ptr, 2, (ctypes.c_uint64 * 2)(*terms),
                                                     (ctypes.c_void_p * 2)(None, r.keys[els[1]].value),
                                                     (ctypes.c_void_p * 2)(*[p.ptr for p in one]), (ctypes.c_longlong * 2)(0, 0),
                                                     None, s, out.ptr, batch, s, s, ctx.stream))
            assert np.array_equal(ctx.download(out, (batch, 2, L, n)), want), form
