"""Layout, aliasing and argument contract of the first-generation entry points (include/lattisense_amd.h, "Layout and aliasing"):
lsa_poly_addsub, lsa_ckks_mult / _relin / _rescale / _rotate / _rotate_many / _mult_relin_rescale, lsa_drop_level and
lsa_bfv_mult / _relin / _rotate / _rescale / _mult_relin, through raw C calls.

The reference of every result is oracle.pyoracle.Oracle on the same words (vec, ckks_* / bfv_*; the row slice for drop_level) --
never a dense call of the same entry point -- and every comparison is word for word.

  padded layout   every operand and the output inside a larger sentinel-filled buffer, each with its own 16-byte aligned base
                  offset (no multiple of N) and its own padded stride, the output's the largest: payload == oracle at every batch
                  position, every word of padding and of the guard zones still the sentinel, every input unchanged
  shared / square stride 0 on an input where the contract accepts it, a == b
  in place        addsub out == a / out == b, rotate out == in (Galois elements 5, 5^-7, 2N-1), rotate_many with one output == in
  interleaved     outputs between the items of the input in one buffer: overlap is exact, padding belongs to nobody
  refusals        every refusal of the contract: return code, message prefix, nothing written, context still usable

CKKS: N = 2048, the first five primes of CKKS_DEFAULT[16384] with its two special primes, level 3, keys at level 4, uniform
words, batch 5 with tile batch 2 (tiles 2, 2, 1) under both dual-stream settings, tile batch 0 once; N = 8192 (two-pass
transforms, chain of test_hoisted_rotations_equal_stand_alone_rotations) for relin and rotate.  BFV: N = 1024 on the four-prime
chain of tests/test_gpu_bfv.py, level 3, batch 3, tile batch 2."""
import ctypes

import numpy as np
import pytest

from tests.gpu_util import need_gpu, rand_ct
from tests.layout_util import SENT, Field, invoke, last_error, padded_inputs, padded_output

pytestmark = pytest.mark.gpu

ARG = 1                                                    # LSA_ERR_ARG


def _lib():
    from lattisense_amd._native import lib
    return lib()


def _rand_key(rng, q, p, klvl, n):
    beta = (klvl + 1 + len(p) - 1) // len(p)
    key = np.empty((beta, 2, klvl + 1 + len(p), n), dtype=np.uint64)
    for j, m in enumerate(list(q[: klvl + 1]) + list(p)):
        key[:, :, j, :] = rng.integers(0, m, size=(beta, 2, n), dtype=np.uint64)
    return key


class Rig:
    """one context, its oracle, operands made once and never written, oracle results computed once"""

    def __init__(self, algo, n, q, p, t, lvl, klvl, batch, galois, seed):
        from lattisense_amd.device import DeviceContext
        from oracle.pyoracle import Oracle
        self.algo, self.n, self.q, self.p, self.lvl, self.klvl, self.batch = algo, n, q, p, lvl, klvl, batch
        self.L = lvl + 1
        self.ctx = DeviceContext(algo, n, q, p, t)
        self.o = Oracle(n, q, p, t)
        rng = np.random.default_rng(seed)
        ql = q[: lvl + 1]
        self.A, self.B = rand_ct(rng, ql, 2, n, batch), rand_ct(rng, ql, 2, n, batch)
        self.D3 = rand_ct(rng, ql, 3, n, batch)
        self.raw = {"rlk": _rand_key(rng, q, p, klvl, n)}
        for g in galois:
            self.raw[g] = _rand_key(rng, q, p, klvl, n)
        self.key = {k: self.ctx.upload_key(v, klvl) for k, v in self.raw.items()}
        self.galois = list(galois)
        self._want = {}

    def settings(self, dual, tile=2):
        lib = _lib()
        assert lib.lsa_set_dual_stream(self.ctx.h, dual) == 0 and lib.lsa_set_tile_batch(self.ctx.h, tile) == 0

    def want(self, tag, fn):
        """fn(i) -> the oracle's result for batch item i; stacked and cached under `tag`"""
        if tag not in self._want:
            self._want[tag] = np.stack([fn(i) for i in range(self.batch)])
        return self._want[tag]

    def vec(self, op, a, b):
        """limb-wise add / sub / neg of [polys][L][N] arrays by the oracle"""
        out = np.empty_like(a)
        for pl in range(a.shape[0]):
            for j in range(a.shape[1]):
                out[pl, j] = self.o.vec(op, j, a[pl, j], None if b is None else b[pl, j])
        return out


_RIGS = {}


def _rig(name):
    need_gpu()
    if name not in _RIGS:
        from lattisense_amd import params
        from lattisense_amd.device import ALGO_BFV, ALGO_CKKS
        if name == "ckks":
            P = params.CKKS_DEFAULT[16384]
            n = 2048
            _RIGS[name] = Rig(ALGO_CKKS, n, P["q"][:5], P["p"], 0, 3, 4, 5, (5, pow(5, -7, 2 * n), 2 * n - 1), 1)
        elif name == "ckks2":
            P = params.CKKS_DEFAULT[65536]
            n = 8192
            _RIGS[name] = Rig(ALGO_CKKS, n, P["q"][:6], P["p"][:2], 0, 3, 5, 3, (5, 2 * n - 1), 2)
        else:
            P = params.BFV_DEFAULT[16384]
            n = 1024
            _RIGS[name] = Rig(ALGO_BFV, n, P["q"][:4], P["p"], P["t"], 3, 3, 3, (5, 2 * n - 1), 3)
    return _RIGS[name]


# ------------------------------------------------------------------------------------------------ the entry points as cases
# name -> (inputs(r) -> list of [batch][...] arrays, extra arguments(r), words of one output item(r), want(r, inputs, shared)).
# `ins` are the host arrays actually passed, so the same function serves the shared-operand and squaring forms.
def _cases(r):
    o, lvl, klvl, L, N = r.o, r.lvl, r.klvl, r.L, r.n
    g0 = r.galois[0]
    c = {}
    if r.algo == 1:
        for op, nm in enumerate(("add", "sub", "neg")):
            c["lsa_poly_addsub:" + nm] = ([r.A, r.B], dict(op=op, polys=2), 2 * L * N,
                                          lambda x, y, nm=nm: r.vec(nm, x, None if nm == "neg" else y))
        c["lsa_poly_addsub:add3"] = ([r.D3, r.D3[::-1].copy()], dict(op=0, polys=3), 3 * L * N, lambda x, y: r.vec("add", x, y))
        c["lsa_ckks_mult"] = ([r.A, r.B], {}, 3 * L * N, lambda x, y: o.ckks_mult(lvl, x, y))
        c["lsa_ckks_relin"] = ([r.D3], dict(key=r.key["rlk"]), 2 * L * N, lambda d: o.ckks_relin(lvl, d, r.raw["rlk"], klvl))
        c["lsa_ckks_rescale"] = ([r.A], dict(polys=2), 2 * lvl * N, lambda x: o.ckks_rescale(lvl, x))
        c["lsa_ckks_rescale:3"] = ([r.D3], dict(polys=3), 3 * lvl * N, lambda x: o.ckks_rescale(lvl, x))
        c["lsa_ckks_rotate"] = ([r.A], dict(g=g0, key=r.key[g0]), 2 * L * N, lambda x: o.ckks_rotate(lvl, x, g0, r.raw[g0], klvl))
        c["lsa_drop_level"] = ([r.D3], dict(polys=3), 3 * lvl * N, lambda x: x[:, :lvl])
        c["lsa_ckks_mult_relin_rescale"] = ([r.A, r.B], dict(key=r.key["rlk"]), 2 * lvl * N,
                                            lambda x, y: o.ckks_mult_relin_rescale(lvl, x, y, r.raw["rlk"], klvl))
    else:
        c["lsa_bfv_mult"] = ([r.A, r.B], {}, 3 * L * N, lambda x, y: o.bfv_mult(lvl, x, y))
        c["lsa_bfv_relin"] = ([r.D3], dict(key=r.key["rlk"]), 2 * L * N, lambda d: o.bfv_relin(lvl, d, r.raw["rlk"], klvl))
        c["lsa_bfv_rotate"] = ([r.A], dict(g=g0, key=r.key[g0]), 2 * L * N, lambda x: o.bfv_rotate(lvl, x, g0, r.raw[g0], klvl))
        c["lsa_bfv_rescale"] = ([r.A], dict(polys=2), 2 * lvl * N, lambda x: o.bfv_rescale(lvl, x))
        c["lsa_bfv_mult_relin"] = ([r.A, r.B], dict(key=r.key["rlk"]), 2 * L * N,
                                   lambda x, y: o.bfv_mult_relin(lvl, x, y, r.raw["rlk"], klvl))
        c["lsa_drop_level"] = ([r.A], dict(polys=2), 2 * lvl * N, lambda x: x[:, :lvl])
        c["lsa_poly_addsub:sub"] = ([r.A, r.B], dict(op=1, polys=2), 2 * L * N, lambda x, y: r.vec("sub", x, y))
    return c


CKKS_CASES = ["lsa_poly_addsub:add", "lsa_poly_addsub:sub", "lsa_poly_addsub:neg", "lsa_poly_addsub:add3", "lsa_ckks_mult",
              "lsa_ckks_relin", "lsa_ckks_rescale", "lsa_ckks_rescale:3", "lsa_ckks_rotate", "lsa_drop_level",
              "lsa_ckks_mult_relin_rescale"]
BFV_CASES = ["lsa_bfv_mult", "lsa_bfv_relin", "lsa_bfv_rotate", "lsa_bfv_rescale", "lsa_bfv_mult_relin", "lsa_drop_level",
             "lsa_poly_addsub:sub"]


def _args(r, ins, out, extra):
    a = dict(ptrs=[f.ptr for f in ins] + [None], strides=[f.stride for f in ins] + [0], out=out.ptr, so=out.stride,
             batch=r.batch, level=r.lvl)
    a.update(extra)
    return a


def _ok(rc):
    assert rc == 0, last_error()


def _padded(r, case):
    _padded_call(r, case, *_cases(r)[case])


def _padded_call(r, case, arrays, extra, wout, fn):
    """one case of the shape _cases() returns, under the tag `case` (entry point, ':', variant); shared with
    tests/test_gpu_ntt_chunk.py"""
    name = case.split(":")[0]
    want = r.want(case, lambda i: fn(*[np.ascontiguousarray(a[i]) for a in arrays]))
    ins = padded_inputs(r.ctx, arrays, r.batch)
    out = padded_output(r.ctx, wout, r.batch, ins)
    assert out.stride > max(f.stride for f in ins) and all(f.base % r.n and f.base % 2 == 0 for f in ins + [out])
    _ok(invoke(name, r.ctx.h, _args(r, ins, out, extra), r.ctx.stream))
    out.expect(want)
    out.check(case + ": output")
    for i, f in enumerate(ins):
        f.check(case + ": input %d" % i)
    if case == "lsa_poly_addsub:neg":                      # b is ignored: null with stride 0 is the documented form
        out2 = padded_output(r.ctx, wout, r.batch, ins)
        a = _args(r, ins, out2, extra)
        a["ptrs"][1], a["strides"][1] = None, 0
        _ok(invoke(name, r.ctx.h, a, r.ctx.stream))
        out2.expect(want)
        out2.check(case + ": output with b == NULL")
        ins[0].check(case + ": input with b == NULL")


# ------------------------------------------------------------------------------------------------ padded layouts
@pytest.mark.parametrize("dual", [0, 1])
@pytest.mark.parametrize("case", CKKS_CASES)
def test_ckks_padded_layout(case, dual):
    r = _rig("ckks")
    r.settings(dual)
    _padded(r, case)


@pytest.mark.parametrize("case", ["lsa_ckks_relin", "lsa_ckks_rescale", "lsa_ckks_rotate", "lsa_ckks_mult_relin_rescale"])
def test_ckks_padded_layout_unfused_tails(case):
    """lsa_set_fuse_tails(0): the ModDown and rescale tails as kernels of their own, and the rotation in two steps (key switch
    into the workspace, then the permutation into an output whose stride differs from the input's)"""
    r = _rig("ckks")
    r.settings(1)
    assert _lib().lsa_set_fuse_tails(r.ctx.h, 0) == 0
    try:
        _padded(r, case)
    finally:
        assert _lib().lsa_set_fuse_tails(r.ctx.h, 1) == 0


def test_ckks_padded_layout_automatic_tile():
    r = _rig("ckks")
    r.settings(0, tile=0)
    for case in CKKS_CASES:
        _padded(r, case)


@pytest.mark.parametrize("dual", [0, 1])
@pytest.mark.parametrize("case", BFV_CASES)
def test_bfv_padded_layout(case, dual):
    r = _rig("bfv")
    r.settings(dual)
    _padded(r, case)


@pytest.mark.parametrize("dual", [0, 1])
@pytest.mark.parametrize("case", ["lsa_ckks_relin", "lsa_ckks_rotate"])
def test_ckks_two_pass_ring_padded_layout(case, dual):
    r = _rig("ckks2")
    r.settings(dual)
    _padded(r, case)


def _rotate_many(r, in_place):
    """three (two on the small rigs) hoisted rotations into padded outputs with one stride; in_place: the FIRST output is the
    input itself, so every later rotation must still see the intact ciphertext"""
    N, L, lvl, klvl = r.n, r.L, r.lvl, r.klvl
    w = 2 * L * N
    stride = w + 30
    src = Field(r.ctx, w, r.batch, 38, stride, r.A)
    outs = [src if (in_place and i == 0) else Field(r.ctx, w, r.batch, 74 + 36 * i, stride) for i in range(len(r.galois))]
    a = dict(ptrs=[src.ptr], strides=[src.stride], out=[f.ptr for f in outs], so=stride, batch=r.batch, level=lvl, g=r.galois,
             key=[r.key[g] for g in r.galois])
    _ok(invoke("lsa_ckks_rotate_many", r.ctx.h, a, r.ctx.stream))
    for g, f in zip(r.galois, outs):
        f.expect(r.want(("rot", g), lambda i, g=g: r.o.ckks_rotate(lvl, r.A[i], g, r.raw[g], klvl)))
        f.check("rotate_many g=%d" % g)
    if not in_place:
        src.check("rotate_many: input")


@pytest.mark.parametrize("dual", [0, 1])
def test_ckks_rotate_many_padded_layout(dual):
    r = _rig("ckks")
    r.settings(dual)
    _rotate_many(r, False)


@pytest.mark.parametrize("dual", [0, 1])
def test_ckks_interleaved_operands(dual):
    """Overlap is exact, padding belongs to nobody: the outputs live BETWEEN the items of the input, in the same buffer (what the
    task runtime does when a fresh output slab lies between inputs gathered with their natural stride)."""
    r = _rig("ckks")
    r.settings(dual)
    N, L, lvl, klvl = r.n, r.L, r.lvl, r.klvl
    gap = 30
    for case in ("lsa_ckks_relin", "lsa_ckks_rescale", "lsa_ckks_rotate"):
        arrays, extra, wout, fn = _cases(r)[case]
        w = arrays[0][0].size
        stride = w + gap + wout + gap                      # item b | gap | output b | gap | item b + 1 ...
        f = Field(r.ctx, w, r.batch, 38, stride, arrays[0], room=wout + gap)
        a = dict(ptrs=[f.ptr, None], strides=[stride, 0], out=f.ptr + 8 * (w + gap), so=stride, batch=r.batch, level=lvl)
        a.update(extra)
        _ok(invoke(case, r.ctx.h, a, r.ctx.stream))
        want = r.want(case, lambda i: fn(np.ascontiguousarray(arrays[0][i])))
        for b in range(r.batch):
            o = f.base + b * stride + w + gap
            f.image[o:o + wout] = want[b].ravel()
        f.check(case + ": interleaved")
    w = 2 * L * N                                          # rotate_many: item b | out0 b | out1 b | out2 b | ...
    slot = w + gap
    stride = (1 + len(r.galois)) * slot
    f = Field(r.ctx, w, r.batch, 38, stride, r.A, room=stride)
    a = dict(ptrs=[f.ptr], strides=[stride], out=[f.ptr + 8 * (i + 1) * slot for i in range(len(r.galois))], so=stride,
             batch=r.batch, level=lvl, g=r.galois, key=[r.key[g] for g in r.galois])
    _ok(invoke("lsa_ckks_rotate_many", r.ctx.h, a, r.ctx.stream))
    for i, g in enumerate(r.galois):
        want = r.want(("rot", g), lambda j, g=g: r.o.ckks_rotate(lvl, r.A[j], g, r.raw[g], klvl))
        for b in range(r.batch):
            o = f.base + b * stride + (i + 1) * slot
            f.image[o:o + w] = want[b].ravel()
    f.check("rotate_many: interleaved")


# ------------------------------------------------------------------------------------------------ shared operands, squaring
def _shared(r, case, which, fuse_tails=1):
    """which: 'a0' / 'b0' = stride 0 on that operand, 'sq' = a == b"""
    arrays, extra, wout, fn = _cases(r)[case]
    name = case.split(":")[0]
    A, B = arrays
    if which == "sq":
        fa = Field(r.ctx, A[0].size, r.batch, 38, A[0].size + 6, A)
        ins, item = [fa, fa], lambda i: (A[i], A[i])
    elif which == "b0":
        ins = [Field(r.ctx, A[0].size, r.batch, 38, A[0].size + 6, A), Field(r.ctx, B[0].size, r.batch, 74, 0, B[1])]
        item = lambda i: (A[i], B[1])
    else:
        ins = [Field(r.ctx, A[0].size, r.batch, 38, 0, A[2]), Field(r.ctx, B[0].size, r.batch, 74, B[0].size + 10, B)]
        item = lambda i: (A[2], B[i])
    out = padded_output(r.ctx, wout, r.batch, ins)
    want = r.want((case, which), lambda i: fn(*[np.ascontiguousarray(x) for x in item(i)]))
    assert _lib().lsa_set_fuse_tails(r.ctx.h, fuse_tails) == 0
    try:
        _ok(invoke(name, r.ctx.h, _args(r, ins, out, extra), r.ctx.stream))
        out.expect(want)
        out.check("%s %s" % (case, which))
        for f in ins:
            f.check("%s %s: input" % (case, which))
    finally:
        assert _lib().lsa_set_fuse_tails(r.ctx.h, 1) == 0


@pytest.mark.parametrize("dual", [0, 1])
@pytest.mark.parametrize("which", ["a0", "b0", "sq"])
def test_ckks_shared_operand_and_squaring(which, dual):
    r = _rig("ckks")
    r.settings(dual)
    for case in ("lsa_poly_addsub:sub", "lsa_ckks_mult", "lsa_ckks_mult_relin_rescale"):
        _shared(r, case, which)
    _shared(r, "lsa_ckks_mult_relin_rescale", which, fuse_tails=0)      # the unfolded path: k_tensor, key switch, rescale


@pytest.mark.parametrize("dual", [0, 1])
@pytest.mark.parametrize("which", ["a0", "b0", "sq"])
def test_bfv_shared_operand_and_squaring(which, dual):
    r = _rig("bfv")
    r.settings(dual)
    for case in ("lsa_bfv_mult", "lsa_bfv_mult_relin"):
        _shared(r, case, which)


# ------------------------------------------------------------------------------------------------ in place
@pytest.mark.parametrize("dual", [0, 1])
@pytest.mark.parametrize("op", ["add", "sub"])
def test_addsub_in_place(op, dual):
    r = _rig("ckks")
    r.settings(dual)
    arrays, extra, wout, fn = _cases(r)["lsa_poly_addsub:" + op]
    want = r.want("lsa_poly_addsub:" + op, lambda i: fn(r.A[i], r.B[i]))
    for target in (0, 1):                                  # out == a, out == b
        ins = padded_inputs(r.ctx, arrays, r.batch)
        _ok(invoke("lsa_poly_addsub", r.ctx.h, _args(r, ins, ins[target], extra), r.ctx.stream))
        ins[target].expect(want)
        ins[target].check("addsub in place over operand %d" % target)
        ins[1 - target].check("addsub in place: the other operand")
    fa = padded_inputs(r.ctx, [r.A], r.batch)[0]          # out == a == b
    _ok(invoke("lsa_poly_addsub", r.ctx.h, _args(r, [fa, fa], fa, extra), r.ctx.stream))
    fa.expect(r.want(("self", op), lambda i: r.vec(op, r.A[i], r.A[i])))
    fa.check("addsub out == a == b")


@pytest.mark.parametrize("dual", [0, 1])
def test_ckks_rotate_in_place(dual):
    r = _rig("ckks")
    r.settings(dual)
    for g in r.galois:                                     # 5, 5^-7, 2N - 1
        f = padded_inputs(r.ctx, [r.A], r.batch)[0]
        a = _args(r, [f], f, dict(g=g, key=r.key[g]))
        _ok(invoke("lsa_ckks_rotate", r.ctx.h, a, r.ctx.stream))
        f.expect(r.want(("rot", g), lambda i, g=g: r.o.ckks_rotate(r.lvl, r.A[i], g, r.raw[g], r.klvl)))
        f.check("rotate in place g=%d" % g)


@pytest.mark.parametrize("dual", [0, 1])
def test_ckks_rotate_many_one_output_is_the_input(dual):
    r = _rig("ckks")
    r.settings(dual)
    _rotate_many(r, True)


def test_ckks_two_pass_ring_rotate_in_place():
    r = _rig("ckks2")
    r.settings(1)
    g = r.galois[0]
    f = padded_inputs(r.ctx, [r.A], r.batch)[0]
    _ok(invoke("lsa_ckks_rotate", r.ctx.h, _args(r, [f], f, dict(g=g, key=r.key[g])), r.ctx.stream))
    f.expect(r.want(("rot", g), lambda i: r.o.ckks_rotate(r.lvl, r.A[i], g, r.raw[g], r.klvl)))
    f.check("rotate in place, N = 8192")


@pytest.mark.parametrize("dual", [0, 1])
def test_bfv_rotate_in_place(dual):
    r = _rig("bfv")
    r.settings(dual)
    for g in r.galois:
        f = padded_inputs(r.ctx, [r.A], r.batch)[0]
        _ok(invoke("lsa_bfv_rotate", r.ctx.h, _args(r, [f], f, dict(g=g, key=r.key[g])), r.ctx.stream))
        f.expect(r.want(("rot", g), lambda i, g=g: r.o.bfv_rotate(r.lvl, r.A[i], g, r.raw[g], r.klvl)))
        f.check("bfv rotate in place g=%d" % g)


# ------------------------------------------------------------------------------------------------ refusals
# What the contract accepts per entry point: inputs that may be shared (stride 0), inputs the output may BE, the lowest level,
# and whether the entry point is bound to one scheme.
SPEC = {
    "lsa_poly_addsub": dict(shared=(True, True), same=(True, True), min_level=0, bound=False),
    "lsa_ckks_mult": dict(shared=(True, True), same=(False, False), min_level=0, bound=True),
    "lsa_ckks_relin": dict(shared=(False,), same=(False,), min_level=0, bound=True),
    "lsa_ckks_rescale": dict(shared=(False,), same=(False,), min_level=1, bound=True),
    "lsa_ckks_rotate": dict(shared=(False,), same=(True,), min_level=0, bound=True),
    "lsa_drop_level": dict(shared=(False,), same=(False,), min_level=1, bound=False),
    "lsa_ckks_mult_relin_rescale": dict(shared=(True, True), same=(False, False), min_level=1, bound=True),
    "lsa_bfv_mult": dict(shared=(True, True), same=(False, False), min_level=0, bound=True),
    "lsa_bfv_relin": dict(shared=(False,), same=(False,), min_level=0, bound=True),
    "lsa_bfv_rotate": dict(shared=(False,), same=(True,), min_level=0, bound=True),
    "lsa_bfv_rescale": dict(shared=(False,), same=(False,), min_level=1, bound=True),
    "lsa_bfv_mult_relin": dict(shared=(True, True), same=(False, False), min_level=0, bound=True),
}


def _refusals(r, other, case, low_key):
    """every refusal of `case`'s entry point; other: a context of the other scheme; low_key: a key uploaded below the level"""
    arrays, extra, wout, fn = _cases(r)[case]
    name = case.split(":")[0]
    spec = SPEC[name]
    # room behind every input: the overlapping outputs below stay inside the input's own allocation
    ins = padded_inputs(r.ctx, arrays, r.batch, room=r.batch * (max(a[0].size for a in arrays) + 64))
    out = padded_output(r.ctx, wout, r.batch, ins)
    good = _args(r, ins, out, extra)
    bad = []                                               # (what, arguments, context handle)

    def mut(what, h=None, **kw):
        a = dict(good)
        a["ptrs"], a["strides"] = list(good["ptrs"]), list(good["strides"])
        for k, v in kw.items():
            if k in ("ptr", "stride"):
                a[k + "s"][v[0]] = v[1]
            else:
                a[k] = v
        bad.append((what, a, h if h is not None else r.ctx.h))

    for i, f in enumerate(ins):
        if not (name == "lsa_poly_addsub" and extra["op"] == 2 and i == 1):
            mut("input %d null" % i, ptr=(i, None))
            mut("input %d stride short" % i, stride=(i, f.words - 2))
            mut("input %d stride odd" % i, stride=(i, f.words + 1))
            mut("input %d stride negative" % i, stride=(i, -f.stride))
            mut("input %d misaligned" % i, ptr=(i, f.ptr + 8))
            if not spec["shared"][i]:
                mut("input %d shared" % i, stride=(i, 0))
            mut("out one item into input %d" % i, out=f.ptr + 8 * f.stride)
            mut("out starting in the padding of input %d, reaching its next item" % i, out=f.ptr + 8 * f.words, so=f.stride if wout <= f.words else out.stride)
            if spec["same"][i]:
                mut("out == input %d with another stride" % i, out=f.ptr, so=f.stride + 2)
            else:
                mut("out == input %d" % i, out=f.ptr, so=max(f.stride, wout + 2))
    mut("out null", out=None)
    mut("out stride 0", so=0)
    mut("out stride short", so=wout - 2)
    mut("out stride odd", so=out.stride + 1)
    mut("out misaligned", out=out.ptr + 8)
    mut("level -1", level=-1)
    mut("level past the chain", level=len(r.q))
    if spec["min_level"] == 1:
        mut("level 0", level=0)
    if "polys" in extra:
        mut("polys 0", polys=0)
        mut("polys 4", polys=4)
    if "op" in extra:
        mut("op 3", op=3)
    if "key" in extra:
        mut("key null", key=None)
        mut("key below the level", key=low_key)
    if spec["bound"]:
        mut("context of the other scheme", h=other.ctx.h)
    for what, a, h in bad:
        rc = invoke(name, h, a, r.ctx.stream)
        assert rc == ARG, (case, what, rc, last_error())
        assert last_error().startswith(name + ":"), (case, what, last_error())
    for nb in (0, -1):                                     # a no-op, whatever else is passed
        a = dict(good)
        a["batch"] = nb
        _ok(invoke(name, r.ctx.h, a, r.ctx.stream))
    out.check(case + ": a refused call or an empty batch wrote to the output")
    for f in ins:
        f.check(case + ": a refused call wrote to an input")
    _ok(invoke(name, r.ctx.h, good, r.ctx.stream))         # the context still works
    out.expect(r.want(case, lambda i: fn(*[np.ascontiguousarray(a[i]) for a in arrays])))
    out.check(case + ": the call after the refusals")


@pytest.mark.parametrize("case", ["lsa_poly_addsub:add", "lsa_poly_addsub:neg", "lsa_ckks_mult", "lsa_ckks_relin", "lsa_ckks_rescale",
                                  "lsa_ckks_rotate", "lsa_drop_level", "lsa_ckks_mult_relin_rescale"])
def test_ckks_refusals(case):
    r, other = _rig("ckks"), _rig("bfv")
    r.settings(1)
    if "low" not in r.key:
        r.key["low"] = r.ctx.upload_key(_rand_key(np.random.default_rng(9), r.q, r.p, r.lvl - 1, r.n), r.lvl - 1)
    _refusals(r, other, case, r.key["low"])


@pytest.mark.parametrize("case", ["lsa_bfv_mult", "lsa_bfv_relin", "lsa_bfv_rotate", "lsa_bfv_rescale", "lsa_bfv_mult_relin"])
def test_bfv_refusals(case):
    r, other = _rig("bfv"), _rig("ckks")
    r.settings(1)
    if "low" not in r.key:
        r.key["low"] = r.ctx.upload_key(_rand_key(np.random.default_rng(9), r.q, r.p, r.lvl - 1, r.n), r.lvl - 1)
    _refusals(r, other, case, r.key["low"])


def test_ckks_rotate_many_refusals():
    r, other = _rig("ckks"), _rig("bfv")
    r.settings(1)
    N, L, lvl = r.n, r.L, r.lvl
    w = 2 * L * N
    stride = w + 30
    src = Field(r.ctx, w, r.batch, 38, stride, r.A, room=r.batch * (stride + 64))
    outs = [Field(r.ctx, w, r.batch, 74 + 36 * i, stride, room=r.batch * (stride + 64)) for i in range(len(r.galois))]
    if "low" not in r.key:
        r.key["low"] = r.ctx.upload_key(_rand_key(np.random.default_rng(9), r.q, r.p, lvl - 1, N), lvl - 1)
    good = dict(ptrs=[src.ptr], strides=[stride], out=[f.ptr for f in outs], so=stride, batch=r.batch, level=lvl, g=r.galois,
                key=[r.key[g] for g in r.galois])
    o0, o1, o2 = good["out"]
    bad = [("two outputs equal", dict(out=[o0, o1, o1])),
           ("two outputs one item apart", dict(out=[o0, o1, o1 + 8 * stride])),
           ("an output starting in another's padding, reaching its next item", dict(out=[o0, o1, o1 + 8 * w])),
           ("two outputs are the input", dict(out=[src.ptr, src.ptr, o2])),
           ("an output one item into the input", dict(out=[o0, src.ptr + 8 * stride, o2])),
           ("an output starting in the input's padding, reaching its next item", dict(out=[o0, o1, src.ptr + 8 * w])),
           ("the input with another stride", dict(out=[src.ptr, o1, o2], strides=[stride + 2])),
           ("an output null", dict(out=[o0, None, o2])),
           ("an output misaligned", dict(out=[o0, o1 + 8, o2])),
           ("output stride 0", dict(so=0)), ("output stride short", dict(so=w - 2)), ("output stride odd", dict(so=stride + 1)),
           ("input null", dict(ptrs=[None])), ("input misaligned", dict(ptrs=[src.ptr + 8])),
           ("input shared", dict(strides=[0])), ("input stride short", dict(strides=[w - 2])),
           ("input stride odd", dict(strides=[stride + 1])),
           ("level -1", dict(level=-1)), ("level past the chain", dict(level=len(r.q))),
           ("a key null", dict(key=[r.key[r.galois[0]], None, r.key[r.galois[2]]])),
           ("a key below the level", dict(key=[r.key[r.galois[0]], r.key["low"], r.key[r.galois[2]]]))]
    for what, kw in bad:
        a = dict(good)
        a.update(kw)
        rc = invoke("lsa_ckks_rotate_many", r.ctx.h, a, r.ctx.stream)
        assert rc == ARG, (what, rc, last_error())
        assert last_error().startswith("lsa_ckks_rotate_many:"), (what, last_error())
    rc = invoke("lsa_ckks_rotate_many", other.ctx.h, good, r.ctx.stream)
    assert rc == ARG and last_error().startswith("lsa_ckks_rotate_many:"), last_error()
    for nb in (0, -1):
        a = dict(good)
        a["batch"] = nb
        _ok(invoke("lsa_ckks_rotate_many", r.ctx.h, a, r.ctx.stream))
    for f in outs + [src]:
        f.check("rotate_many: a refused call wrote")
    _ok(invoke("lsa_ckks_rotate_many", r.ctx.h, good, r.ctx.stream))
    for g, f in zip(r.galois, outs):
        f.expect(r.want(("rot", g), lambda i, g=g: r.o.ckks_rotate(lvl, r.A[i], g, r.raw[g], r.klvl)))
        f.check("rotate_many after the refusals g=%d" % g)
    assert SENT not in (int(x) for x in r.q + r.p)
