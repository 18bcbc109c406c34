"""CKKS plaintext and constant operands on the device (lsa_ckks_encode / _mult_plain / _addsub_plain / _mac_plain / _mult_const /
_add_const / _affine_const) against the frozen oracle (oracle/ckks_bootstrap.py Evaluator.mul_plain / add / sub / rescale /
mul_const / add_const / mul_by_i) and, for the encoder, against lsa_lt_plaintext of the one-diagonal plan.  Everything is integer
arithmetic on the same operands, so every comparison is word for word: no tolerance anywhere.

Rings: N = 2^12 (one-pass transform) on the smallest chain of params.py (CKKS_DEFAULT[4096]: 37- and 32-bit primes, FP64 engine),
N = 2^13 (two-pass transform, so the lifted rows and the selector monomial go through it) on a 60-bit prime followed by three
40-bit primes of the bootstrap chain (integer and FP64 engines side by side), and N = 2^13 on four primes at the 61-bit ceiling
(tests/boundary.py ceiling_chain; the end-to-end scales are chosen for that modulus).  Batch 3, output strides larger than the compact
size (the padding must stay untouched), plaintexts shared by the batch (stride 0) and per item, levels top and 1.
Ciphertext and plaintext words are uniform residues: the operators are exact modular arithmetic on whatever words they get."""
import ctypes

import numpy as np
import pytest

from tests.gpu_util import need_gpu, rand_ct

pytestmark = pytest.mark.gpu

D40 = float(2 ** 40)
D20 = float(2 ** 20)
BATCH = 3
PAD = 6                          # words behind every output item (even: 16-byte alignment holds)
SENT = 0xABCDEF0123456789        # no residue: every modulus is below 2^61
MAC_MAX_TERMS = 16               # LSA_MAC_MAX_TERMS (asserted against the header in tests/test_ckks_plain_api.py)


def _chain(name):
    from lattisense_amd import params
    if name == "n12":
        P = params.CKKS_DEFAULT[4096]
        return 12, P["q"], P["p"]
    if name == "n13c":
        from tests.boundary import ceiling_chain
        C = ceiling_chain(1 << 13, 4, 1)
        return 13, C["q"], C["p"]
    B = params.CKKS_BOOTSTRAP_65536
    return 13, B["q"][:4], B["p"][:1]


class Rig:
    def __init__(self, name):
        from lattisense_amd.device import ALGO_CKKS, DeviceContext
        from oracle.ckks_bootstrap import Evaluator
        from oracle.client import Client
        from oracle.pyoracle import Oracle
        log_n, self.q, self.p = _chain(name)
        self.name = name
        self.N = 1 << log_n
        self.top = len(self.q) - 1
        self.levels = sorted({self.top, 1})
        self.o = Oracle(self.N, self.q, self.p, 0)
        self.c = Client(self.o, seed=log_n)
        self.ctx = DeviceContext(ALGO_CKKS, self.N, self.q, self.p)
        self.ev = Evaluator.__new__(Evaluator)          # no key is needed
        self.ev.o, self.ev.c, self.ev.klvl, self.ev.n = self.o, self.c, self.top, self.N
        self.ev.glk, self.ev.counts = {}, {"rotate": 0, "mult": 0, "mul_plain": 0}
        rng = np.random.default_rng(100 + log_n)
        # operands, made once and never written: three ciphertext batches and four plaintext batches per level
        self.cts, self.pts, self.dcts, self.dpts = {}, {}, {}, {}
        for lvl in self.levels:
            self.cts[lvl] = [rand_ct(rng, self.q[: lvl + 1], 2, self.N, BATCH) for _ in range(3)]
            self.pts[lvl] = [rand_ct(rng, self.q[: lvl + 1], 1, self.N, BATCH)[:, 0] for _ in range(4)]
            self.dcts[lvl] = [self.ctx.upload(x) for x in self.cts[lvl]]
            self.dpts[lvl] = [self.ctx.upload(x) for x in self.pts[lvl]]

    # ---- outputs with a padded stride, pre-filled with a sentinel
    def out_buf(self, rows, batch=BATCH, polys=2):
        so = polys * rows * self.N + PAD
        return self.ctx.upload(np.full(batch * so, SENT, dtype=np.uint64)), so

    def fetch(self, buf, so, rows, batch=BATCH, polys=2):
        a = self.ctx.download(buf, (batch, so))
        w = polys * rows * self.N
        assert np.all(a[:, w:] == SENT), "the padding behind an output item was written"
        return a[:, :w].reshape((batch, polys, rows, self.N) if polys > 1 else (batch, rows, self.N))

    def ct(self, data, lvl, scale=D40):
        from oracle.ckks_bootstrap import Ct
        return Ct(data, lvl, scale)


_RIGS = {}


@pytest.fixture(params=["n12", "n13", "n13c"])
def rig(request):
    need_gpu()
    if request.param not in _RIGS:
        _RIGS[request.param] = Rig(request.param)
    return _RIGS[request.param]


def _lib():
    from lattisense_amd._native import lib
    return lib()


def _check(rc):
    from lattisense_amd._native import check
    check(rc)


def _fails(fn, needle, code=1):
    from lattisense_amd._native import LsaError
    with pytest.raises(LsaError) as e:
        fn()
    assert e.value.code == code, e.value
    assert needle in str(e.value), e.value


def _ptr(buf, words=0):
    return buf.ptr + 8 * words


# ------------------------------------------------------------------------------------------------ encoder
@pytest.mark.parametrize("sparse", [False, True], ids=["full", "log_slots3"])
def test_encode_equals_the_one_diagonal_plan(rig, sparse):
    from lattisense_amd.device import LinearTransformPlan
    ctx, N = rig.ctx, rig.N
    log_slots = 3 if sparse else N.bit_length() - 2
    period = 1 << log_slots
    rng = np.random.default_rng(7 + log_slots)
    z = rng.uniform(-1, 1, (BATCH, period)) + 1j * rng.uniform(-1, 1, (BATCH, period))
    for lvl in rig.levels:
        L = lvl + 1
        for scale in (D40, float(rig.q[lvl])):
            out, so = rig.out_buf(L, polys=1)
            v = np.ascontiguousarray(z).view(np.float64)
            _check(_lib().lsa_ckks_encode(ctx.h, lvl, log_slots, v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), scale, out.ptr, so,
                                          BATCH, ctx.stream))
            got = rig.fetch(out, so, L, polys=1)
            for b in range(BATCH):
                plan = LinearTransformPlan(ctx, lvl, {0: z[b]}, log_slots=log_slots, pt_scale=scale, double_hoist=False)
                assert plan.rows == L and plan.n1 == 0
                want = plan.oracle_plains()[0]
                plan.close()
                assert np.array_equal(got[b], want), (lvl, scale, b)
            # the Python method, compact stride
            again = ctx.download(ctx.ckks_encode(lvl, z, scale, batch=BATCH), (BATCH, L, N))
            assert np.array_equal(again, got)


def test_encode_refusals_write_nothing(rig):
    ctx, N, lvl = rig.ctx, rig.N, rig.top
    L = lvl + 1
    out, so = rig.out_buf(L, batch=2, polys=1)
    ok = np.full(8, 0.5 + 0.25j)
    big = np.full(8, 8.0 + 0j)                                        # 8 * 2^60 = 9.2e18 passes 4.6e18 in coefficient 0
    both = np.stack([ok, big])
    _fails(lambda: ctx.ckks_encode(lvl, both, float(2 ** 60), batch=2, out=out), "lsa_ckks_encode: encoded constant out of range")
    assert np.all(ctx.download(out, (2 * so,)) == SENT), "a refused encoding wrote to the output"
    _fails(lambda: ctx.ckks_encode(lvl, ok, 0.0), "lsa_ckks_encode: scale")
    _fails(lambda: ctx.ckks_encode(lvl, ok, -1.0), "lsa_ckks_encode: scale")
    _fails(lambda: ctx.ckks_encode(lvl + 1, ok, D40), "lsa_ckks_encode: level")
    _fails(lambda: ctx.ckks_encode(-1, ok, D40), "lsa_ckks_encode: level")
    _fails(lambda: ctx.ckks_encode(lvl, np.full(N, 0.5 + 0j), D40), "lsa_ckks_encode: log_slots")
    ctx.ckks_encode(lvl, ok, D40, batch=0, out=out)                   # batch <= 0: a no-op
    assert np.all(ctx.download(out, (2 * so,)) == SENT)


# ------------------------------------------------------------------------------------------------ plaintext operands
def _mul_plain(rig, lvl, ct, pt):
    return rig.ev.mul_plain(rig.ct(ct, lvl), pt, D40)


@pytest.mark.parametrize("rescale", [0, 1])
def test_mult_plain(rig, rescale):
    ctx, N = rig.ctx, rig.N
    for lvl in rig.levels:
        L = lvl + 1
        rows = lvl if rescale else L
        ct, dct = rig.cts[lvl][0], rig.dcts[lvl][0]
        for shared in (False, True):
            pt, dpt = rig.pts[lvl][1], rig.dpts[lvl][1]
            out, so = rig.out_buf(rows)
            _check(_lib().lsa_ckks_mult_plain(ctx.h, lvl, dct.ptr, 2 * L * N, dpt.ptr, 0 if shared else L * N, out.ptr, so, BATCH,
                                              rescale, ctx.stream))
            got = rig.fetch(out, so, rows)
            for b in range(BATCH):
                want = _mul_plain(rig, lvl, ct[b], pt[0 if shared else b])
                if rescale:
                    want = rig.ev.rescale(want)
                assert np.array_equal(got[b], want.data), (lvl, shared, b)
        if not rescale:                                               # out == ct
            mine = ctx.upload(ct)
            assert ctx.ckks_mult_plain(lvl, mine, rig.dpts[lvl][1], BATCH, out=mine) is mine
            want = np.stack([_mul_plain(rig, lvl, ct[b], rig.pts[lvl][1][b]).data for b in range(BATCH)])
            assert np.array_equal(ctx.download(mine, (BATCH, 2, L, N)), want)


@pytest.mark.parametrize("op", [0, 1], ids=["add", "sub"])
def test_addsub_plain(rig, op):
    ctx, N = rig.ctx, rig.N
    for lvl in rig.levels:
        L = lvl + 1
        ct, dct = rig.cts[lvl][1], rig.dcts[lvl][1]
        pt, dpt = rig.pts[lvl][2], rig.dpts[lvl][2]

        def want(b, shared):
            d = ct[b].copy()
            for j in range(L):
                d[0, j] = rig.o.vec("add" if op == 0 else "sub", j, d[0, j], pt[0 if shared else b][j])
            return d
        for shared in (False, True):
            out, so = rig.out_buf(L)
            _check(_lib().lsa_ckks_addsub_plain(ctx.h, op, lvl, dct.ptr, 2 * L * N, dpt.ptr, 0 if shared else L * N, out.ptr, so,
                                                BATCH, ctx.stream))
            got = rig.fetch(out, so, L)
            for b in range(BATCH):
                assert np.array_equal(got[b], want(b, shared)), (lvl, shared, b)     # c1 copied
        mine = ctx.upload(ct)                                         # in place: c1 is left alone
        ctx.ckks_addsub_plain(op, lvl, mine, dpt, BATCH, out=mine)
        assert np.array_equal(ctx.download(mine, (BATCH, 2, L, N)), np.stack([want(b, False) for b in range(BATCH)]))


@pytest.mark.parametrize("n,addend,rescale", [(1, False, 0), (MAC_MAX_TERMS, True, 1), (MAC_MAX_TERMS + 1, True, 0),
                                              (MAC_MAX_TERMS + 1, False, 1)],
                         ids=["one", "limit-addend-rescale", "limit+1-addend", "limit+1-rescale"])
def test_mac_plain(rig, n, addend, rescale):
    """term i: ciphertext batch i % 2, plaintext batch i % 4, every third plaintext shared by the batch; the addend is ciphertext 2"""
    ctx, N, ev = rig.ctx, rig.N, rig.ev
    for lvl in rig.levels:
        L = lvl + 1
        rows = lvl if rescale else L
        shared = [i % 3 == 2 for i in range(n)]
        pc = (ctypes.c_void_p * n)(*[rig.dcts[lvl][i % 2].ptr for i in range(n)])
        sc = (ctypes.c_longlong * n)(*([2 * L * N] * n))
        pp = (ctypes.c_void_p * n)(*[rig.dpts[lvl][i % 4].ptr for i in range(n)])
        sp = (ctypes.c_longlong * n)(*[0 if s else L * N for s in shared])
        out, so = rig.out_buf(rows)
        _check(_lib().lsa_ckks_mac_plain(ctx.h, lvl, n, pc, sc, pp, sp, rig.dcts[lvl][2].ptr if addend else None, 2 * L * N, out.ptr, so,
                                         BATCH, rescale, ctx.stream))
        got = rig.fetch(out, so, rows)
        for b in range(BATCH):
            memo = {}
            acc = None
            for i in range(n):
                key = (i % 2, i % 4, shared[i])
                if key not in memo:
                    memo[key] = _mul_plain(rig, lvl, rig.cts[lvl][i % 2][b], rig.pts[lvl][i % 4][0 if shared[i] else b])
                acc = memo[key] if acc is None else ev.add(acc, memo[key])
            if addend:
                acc = ev.add(acc, rig.ct(rig.cts[lvl][2][b], lvl, D40 * D40))
            if rescale:
                acc = ev.rescale(acc)
            assert np.array_equal(got[b], acc.data), (lvl, b)


# ------------------------------------------------------------------------------------------------ constants
def _raw_const(rig, name, lvl, dct, args, rows, rescale=None):
    """one of the three constant entry points into a padded output"""
    ctx, N = rig.ctx, rig.N
    out, so = rig.out_buf(rows)
    tail = (out.ptr, so, BATCH) + (() if rescale is None else (rescale,)) + (ctx.stream,)
    _check(getattr(_lib(), name)(ctx.h, lvl, dct.ptr, 2 * (lvl + 1) * N, *args, *tail))
    return rig.fetch(out, so, rows)


def _mono_ntt(rig, lvl):
    mono = np.zeros(rig.N, dtype=np.uint64)
    mono[rig.N // 2] = 1
    return [rig.o.ntt(j, mono) for j in range(lvl + 1)]


def _oracle_times(rig, lvl, ct, re, im, cs, scale=D40):
    """ct (at `scale`) x (re + i im) at const_scale cs with the oracle: mul_const(re) + mul_by_i(mul_const(im))"""
    ev = rig.ev
    x = rig.ct(ct, lvl, scale)
    if im == 0:
        return ev.mul_const(x, re, cs)
    return ev.add(ev.mul_const(x, re, cs), ev.mul_by_i(ev.mul_const(x, im, cs)))


def _oracle_plus(rig, lvl, x, re, im):
    """x + (re + i im) at x's scale: add_const for the real part, c0 + kim NTT(X^(N/2)) for the imaginary one"""
    y = rig.ev.add_const(x, re)
    kim = int(round(im * x.scale))
    if kim == 0:
        return y
    d = y.data.copy()
    mono = _mono_ntt(rig, lvl)
    for j in range(lvl + 1):
        d[0, j] = rig.o.vec("add", j, d[0, j], rig.o.vec("mul", j, mono[j], rig.ev._const(kim, j)))
    return rig.ct(d, lvl, x.scale)


def test_mult_const(rig):
    ctx, N, ev = rig.ctx, rig.N, rig.ev
    for lvl in rig.levels:
        L = lvl + 1
        ct, dct = rig.cts[lvl][0], rig.dcts[lvl][0]
        # real constants: small, negative, a tie (0.5 rounds to even), and one whose integer has 62 bits
        for re, cs in ((0.731, float(2 ** 30)), (-1.25, float(2 ** 33)), (2.5, 1.0), (1.7, float(2 ** 61)), (-1.9, float(2 ** 61))):
            got = _raw_const(rig, "lsa_ckks_mult_const", lvl, dct, (re, 0.0, cs), L, rescale=0)
            for b in range(BATCH):
                assert np.array_equal(got[b], ev.mul_const(rig.ct(ct[b], lvl), re, cs).data), (lvl, re, b)
        for sign in (1, -1):                                          # times +-i, exact
            got = _raw_const(rig, "lsa_ckks_mult_const", lvl, dct, (0.0, float(sign), 1.0), L, rescale=0)
            for b in range(BATCH):
                assert np.array_equal(got[b], ev.mul_by_i(rig.ct(ct[b], lvl), sign).data), (lvl, sign, b)
        for re, im, cs in ((0.37, -0.81, float(2 ** 35)), (-1.5, 1.9, float(2 ** 61))):
            for rescale in (0, 1):
                got = _raw_const(rig, "lsa_ckks_mult_const", lvl, dct, (re, im, cs), lvl if rescale else L, rescale=rescale)
                for b in range(BATCH):
                    want = _oracle_times(rig, lvl, ct[b], re, im, cs)
                    assert np.array_equal(got[b], (ev.rescale(want) if rescale else want).data), (lvl, re, im, rescale, b)
        mine = ctx.upload(ct)                                         # out == ct
        ctx.ckks_mult_const(lvl, mine, 0.37 - 0.81j, float(2 ** 35), BATCH, out=mine)
        want = np.stack([_oracle_times(rig, lvl, ct[b], 0.37, -0.81, float(2 ** 35)).data for b in range(BATCH)])
        assert np.array_equal(ctx.download(mine, (BATCH, 2, L, N)), want)


def test_add_const(rig):
    ctx, N = rig.ctx, rig.N
    for lvl in rig.levels:
        L = lvl + 1
        ct, dct = rig.cts[lvl][1], rig.dcts[lvl][1]
        for re, im in ((0.625, 0.0), (-3.0, 0.0), (0.0, 0.4375), (0.0, -2.0), (1.25, -0.75)):
            got = _raw_const(rig, "lsa_ckks_add_const", lvl, dct, (re, im, D40), L)
            for b in range(BATCH):
                assert np.array_equal(got[b], _oracle_plus(rig, lvl, rig.ct(ct[b], lvl), re, im).data), (lvl, re, im, b)
        mine = ctx.upload(ct)                                         # in place: c1 is left alone
        ctx.ckks_add_const(lvl, mine, 1.25 - 0.75j, D40, BATCH, out=mine)
        want = np.stack([_oracle_plus(rig, lvl, rig.ct(ct[b], lvl), 1.25, -0.75).data for b in range(BATCH)])
        assert np.array_equal(ctx.download(mine, (BATCH, 2, L, N)), want)


@pytest.mark.parametrize("rescale", [0, 1])
def test_affine_const(rig, rescale):
    ctx, N, ev = rig.ctx, rig.N, rig.ev
    cs, s_ct = float(2 ** 31), float(2 ** 25)                         # beta is encoded at 2^56
    for lvl in rig.levels:
        L = lvl + 1
        rows = lvl if rescale else L
        ct, dct = rig.cts[lvl][2], rig.dcts[lvl][2]
        for alpha, beta in ((0.37 - 0.81j, -0.25 + 0.5j), (1.5 + 0j, 0.125 + 0j), (-1j, 0.75j)):
            got = _raw_const(rig, "lsa_ckks_affine_const", lvl, dct, (alpha.real, alpha.imag, cs, beta.real, beta.imag, s_ct), rows,
                             rescale=rescale)
            two = ctx.ckks_mult_const(lvl, dct, alpha, cs, BATCH)     # the two-call composition on the device
            two = ctx.ckks_add_const(lvl, two, beta, s_ct * cs, BATCH, out=two)
            if rescale:
                two = ctx.ckks_rescale(lvl, 2, two, BATCH)
            assert np.array_equal(got, ctx.download(two, (BATCH, 2, rows, N))), (lvl, alpha, beta)
            for b in range(BATCH):
                want = _oracle_plus(rig, lvl, _oracle_times(rig, lvl, ct[b], alpha.real, alpha.imag, cs, s_ct), beta.real, beta.imag)
                assert want.scale == s_ct * cs
                assert np.array_equal(got[b], (ev.rescale(want) if rescale else want).data), (lvl, alpha, beta, b)


# ------------------------------------------------------------------------------------------------ arguments
def test_overlap_and_argument_refusals(rig):
    from lattisense_amd import params
    from lattisense_amd.device import ALGO_BFV, DeviceContext
    ctx, N, lvl = rig.ctx, rig.N, rig.top
    L = lvl + 1
    w = 2 * L * N
    lib = _lib()
    ct, pt = ctx.upload(rig.cts[lvl][0]), rig.dpts[lvl][0]
    big = ctx.alloc(BATCH * w + w)
    S = ctx.stream
    # out shifted into ct by half a ciphertext; a rescaled result on top of ct; out on top of the plaintexts
    _fails(lambda: _check(lib.lsa_ckks_mult_plain(ctx.h, lvl, ct.ptr, w, pt.ptr, L * N, _ptr(ct, L * N), w, BATCH - 1, 0, S)),
           "lsa_ckks_mult_plain: out must be ct or not overlap it")
    _fails(lambda: _check(lib.lsa_ckks_mult_plain(ctx.h, lvl, ct.ptr, w, pt.ptr, L * N, ct.ptr, w, BATCH, 1, S)),
           "lsa_ckks_mult_plain: out overlaps the ciphertexts")
    _fails(lambda: _check(lib.lsa_ckks_mult_plain(ctx.h, lvl, ct.ptr, w, big.ptr, 0, _ptr(big, N), w, BATCH, 0, S)),
           "lsa_ckks_mult_plain: out overlaps the plaintexts")
    _fails(lambda: _check(lib.lsa_ckks_addsub_plain(ctx.h, 0, lvl, ct.ptr, w, pt.ptr, L * N, _ptr(ct, 2 * N), w, BATCH - 1, S)),
           "lsa_ckks_addsub_plain: out must be ct or not overlap it")
    _fails(lambda: _check(lib.lsa_ckks_addsub_plain(ctx.h, 2, lvl, ct.ptr, w, pt.ptr, L * N, big.ptr, w, BATCH, S)), "lsa_ckks_addsub_plain: op")
    _fails(lambda: ctx.ckks_mac_plain(lvl, [rig.dcts[lvl][1], ct], [pt, pt], BATCH, out=ct), "lsa_ckks_mac_plain: out overlaps a ciphertext")
    _fails(lambda: ctx.ckks_mac_plain(lvl, [ct], [big], BATCH, out=big), "lsa_ckks_mac_plain: out overlaps a plaintext")
    _fails(lambda: ctx.ckks_mac_plain(lvl, [ct], [pt], BATCH, addend=big, out=big), "lsa_ckks_mac_plain: out overlaps the addend")
    _fails(lambda: ctx.ckks_mac_plain(lvl, [], [], BATCH, out=big), "lsa_ckks_mac_plain: needs at least one term")
    _fails(lambda: ctx.ckks_mult_const(lvl, ct, 1j, 1.0, BATCH, rescale=True, out=ct), "lsa_ckks_mult_const: out overlaps")
    _fails(lambda: _check(lib.lsa_ckks_add_const(ctx.h, lvl, ct.ptr, w, 1.0, 0.0, D40, _ptr(ct, 2 * N), w, BATCH - 1, S)),
           "lsa_ckks_add_const: out must be ct or not overlap it")
    _fails(lambda: ctx.ckks_affine_const(lvl, ct, 1.0, D20, 1.0, D20, BATCH, rescale=True, out=ct), "lsa_ckks_affine_const: out overlaps")
    # levels, scales, constants beyond 2^62, strides
    _fails(lambda: ctx.ckks_mult_plain(lvl + 1, ct, pt, BATCH, out=big), "lsa_ckks_mult_plain: level out of range")
    _fails(lambda: ctx.ckks_mult_plain(0, ct, pt, BATCH, rescale=True, out=big), "lsa_ckks_mult_plain: rescale needs level >= 1")
    _fails(lambda: ctx.ckks_mult_const(lvl, ct, 3.0, float(2 ** 62), BATCH, out=big), "lsa_ckks_mult_const: encoded constant out of range")
    _fails(lambda: ctx.ckks_mult_const(lvl, ct, 3.0, 0.0, BATCH, out=big), "lsa_ckks_mult_const: scale")
    _fails(lambda: ctx.ckks_add_const(lvl, ct, float("nan"), D40, BATCH, out=big), "lsa_ckks_add_const: constant not finite")
    _fails(lambda: _check(lib.lsa_ckks_mult_const(ctx.h, lvl, ct.ptr, w - 2, 1.0, 0.0, 1.0, big.ptr, w, BATCH, 0, S)),
           "lsa_ckks_mult_const: batch stride")
    # 16 bytes per lane: an odd stride or a pointer off the 16-byte grid is refused, for inputs, plaintexts and outputs alike
    _fails(lambda: _check(lib.lsa_ckks_mult_const(ctx.h, lvl, ct.ptr, w, 1.0, 0.0, 1.0, big.ptr, w + 1, 1, 0, S)),
           "lsa_ckks_mult_const: out must be 16-byte aligned with an even batch stride")
    _fails(lambda: _check(lib.lsa_ckks_add_const(ctx.h, lvl, _ptr(ct, 1), w, 1.0, 0.0, D40, big.ptr, w, 1, S)),
           "lsa_ckks_add_const: ct must be 16-byte aligned with an even batch stride")
    _fails(lambda: _check(lib.lsa_ckks_mult_plain(ctx.h, lvl, ct.ptr, w, _ptr(pt, 1), 0, big.ptr, w, 1, 0, S)),
           "lsa_ckks_mult_plain: pt must be 16-byte aligned with an even batch stride")
    _fails(lambda: _check(lib.lsa_ckks_addsub_plain(ctx.h, 0, lvl, ct.ptr, w, pt.ptr, L * N + 1, big.ptr, w, 2, S)),
           "lsa_ckks_addsub_plain: pt must be 16-byte aligned with an even batch stride")
    half = np.full(8, 0.5 + 0j)
    _fails(lambda: _check(lib.lsa_ckks_encode(ctx.h, lvl, 3, half.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double)), D40,
                                              _ptr(big, 1), L * N, 1, S)), "lsa_ckks_encode: out must be 16-byte aligned")
    assert np.array_equal(ctx.download(ct, (BATCH, 2, L, N)), rig.cts[lvl][0]), "a refused call wrote to its input"
    # batch <= 0: a no-op
    sent, so = rig.out_buf(L)
    for b in (0, -1):
        ctx.ckks_mult_plain(lvl, ct, pt, b, out=sent)
        ctx.ckks_addsub_plain(1, lvl, ct, pt, b, out=sent)
        ctx.ckks_mac_plain(lvl, [ct], [pt], b, out=sent)
        ctx.ckks_mult_const(lvl, ct, 2.0, D40, b, out=sent)
        ctx.ckks_add_const(lvl, ct, 2.0, D40, b, out=sent)
        ctx.ckks_affine_const(lvl, ct, 2.0, D20, 1.0, D20, b, out=sent)
    assert np.all(ctx.download(sent, (BATCH * so,)) == SENT)
    if rig.name == "n13":                                             # a BFV context: once is enough
        B = params.BFV_DEFAULT[8192]
        bfv = DeviceContext(ALGO_BFV, 8192, B["q"], B["p"], B["t"])
        x, y = bfv.alloc(2 * 3 * 8192), bfv.alloc(2 * 3 * 8192)
        _fails(lambda: bfv.ckks_encode(0, np.full(8, 0.5 + 0j), D40), "lsa_ckks_encode: context is not CKKS")
        _fails(lambda: bfv.ckks_mult_plain(0, x, y, 1, out=y), "lsa_ckks_mult_plain: context is not CKKS")
        _fails(lambda: bfv.ckks_addsub_plain(0, 0, x, y, 1, out=y), "lsa_ckks_addsub_plain: context is not CKKS")
        _fails(lambda: bfv.ckks_mac_plain(0, [x], [y], 1, out=y), "lsa_ckks_mac_plain: context is not CKKS")
        _fails(lambda: bfv.ckks_mult_const(0, x, 1.0, D40, 1, out=y), "lsa_ckks_mult_const: context is not CKKS")
        _fails(lambda: bfv.ckks_add_const(0, x, 1.0, D40, 1, out=y), "lsa_ckks_add_const: context is not CKKS")
        _fails(lambda: bfv.ckks_affine_const(0, x, 1.0, D20, 1.0, D20, 1, out=y), "lsa_ckks_affine_const: context is not CKKS")
        bfv.close()


# ------------------------------------------------------------------------------------------------ end to end
def test_encrypt_affine_mult_plain_rescale_decrypt(rig):
    """z encrypted, times alpha plus beta, times an encoded weight vector, rescaled: the device's words are the oracle's, so the
    decrypted slots are the oracle's decryption of its own result exactly (scales chosen to fit the ring's modulus)"""
    ctx, N, ev, c = rig.ctx, rig.N, rig.ev, rig.c
    lvl = rig.top
    L = lvl + 1
    s_ct, s_k, s_pt = {"n12": (float(2 ** 20), float(2 ** 10), float(2 ** 20)), "n13": (float(2 ** 30), float(2 ** 20), float(2 ** 30)),
                       "n13c": (float(2 ** 40), float(2 ** 21), float(2 ** 40))}[rig.name]   # n13c: 2^101 / q_3 leaves 2^40
    rng = np.random.default_rng(N)
    z = rng.uniform(-1, 1, N // 2) + 1j * rng.uniform(-1, 1, N // 2)
    wts = rng.uniform(-1, 1, N // 2) + 1j * rng.uniform(-1, 1, N // 2)
    alpha, beta = 0.5 - 0.25j, 0.125 + 0.375j
    ct = c.ckks_encrypt(z, lvl, s_ct)
    dpt = ctx.ckks_encode(lvl, wts, s_pt)
    pt = ctx.download(dpt, (L, N))
    y = ctx.ckks_affine_const(lvl, ctx.upload(ct[None]), alpha, s_k, beta, s_ct, 1)
    got = ctx.download(ctx.ckks_mult_plain(lvl, y, dpt, 1, rescale=True), (1, 2, lvl, N))[0]
    x = _oracle_plus(rig, lvl, _oracle_times(rig, lvl, ct, alpha.real, alpha.imag, s_k, s_ct), beta.real, beta.imag)
    want = ev.rescale(ev.mul_plain(x, pt, s_pt))
    assert np.array_equal(got, want.data)
    out_scale = s_ct * s_k * s_pt / float(rig.q[lvl])
    assert np.array_equal(c.ckks_decrypt(got, out_scale), c.ckks_decrypt(want.data, out_scale))
