"""Helpers of tests/test_gpu_entry_layout.py: operands placed inside larger, sentinel-filled device buffers, and one function
that turns a dictionary of arguments into the raw C call of a first-generation entry point."""
import ctypes

import numpy as np

SENT = 0xABCDEF0123456789        # no residue: every modulus is below 2^62
GUARD = 70                       # sentinel words behind the last item (the words before `base` guard the front)
BASES = (38, 74, 110, 146, 182, 218)   # words: even (16-byte aligned), no multiple of any ring degree, one per operand
PADS = (6, 10, 18)               # words between the items of the inputs: even, no multiple of N, one per operand
OUT_PAD = 26                     # the output's stride exceeds every input's by this


class Field:
    """`batch` items of `words` words inside a device buffer pre-filled with SENT: item b at base + b * stride (stride 0: one
    item).  `image` is what the buffer must hold; expect() updates it, check() compares the whole buffer with it."""

    def __init__(self, ctx, words, batch, base, stride, data=None, room=0):
        self.ctx, self.words, self.batch, self.base, self.stride = ctx, int(words), batch, base, int(stride)
        self.items = 1 if stride == 0 else batch
        self.total = base + (self.items - 1) * self.stride + self.words + GUARD + room
        self.image = np.full(self.total, SENT, dtype=np.uint64)
        if data is not None:
            self.expect(data)
        self.buf = ctx.upload(self.image)

    @property
    def ptr(self):
        return self.buf.ptr + 8 * self.base

    def expect(self, data):
        data = np.ascontiguousarray(data, dtype=np.uint64).reshape(self.items, self.words)
        for b in range(self.items):
            o = self.base + b * self.stride
            self.image[o:o + self.words] = data[b]

    def check(self, what):
        got = self.ctx.download(self.buf, (self.total,))
        for b in range(self.items):                       # the payload first: the more telling message
            o = self.base + b * self.stride
            assert np.array_equal(got[o:o + self.words], self.image[o:o + self.words]), "%s: item %d differs" % (what, b)
        assert np.array_equal(got, self.image), "%s: padding or a guard zone was written" % what


def padded_inputs(ctx, arrays, batch, room=0):
    """every array [batch][...] in a buffer of its own, with its own base offset and its own padded stride"""
    out = []
    for i, a in enumerate(arrays):
        words = a[0].size
        out.append(Field(ctx, words, batch, BASES[i], words + PADS[i], a, room))
    return out


def padded_output(ctx, words, batch, inputs, slot=3):
    """a sentinel-filled output whose stride is larger than every input's"""
    stride = max([words] + [f.stride for f in inputs]) + OUT_PAD
    return Field(ctx, words, batch, BASES[slot], stride)


def invoke(name, h, a, stream=None):
    """the raw call of entry point `name` from a dictionary: ptrs / strides of the inputs, out / so, batch, level, and op, polys,
    g, key where the entry point has them; returns the C return code"""
    from lattisense_amd._native import lib
    L = lib()
    p, s, lvl, out, so, batch = a["ptrs"], a["strides"], a["level"], a["out"], a["so"], a["batch"]
    if name == "lsa_poly_addsub":
        return L.lsa_poly_addsub(h, a["op"], lvl, a["polys"], p[0], p[1], out, batch, s[0], s[1], so, stream)
    if name in ("lsa_ckks_mult", "lsa_bfv_mult"):
        return getattr(L, name)(h, lvl, p[0], p[1], out, batch, s[0], s[1], so, stream)
    if name in ("lsa_ckks_relin", "lsa_bfv_relin"):
        return getattr(L, name)(h, lvl, p[0], a["key"], out, batch, s[0], so, stream)
    if name in ("lsa_ckks_rescale", "lsa_bfv_rescale", "lsa_drop_level"):
        return getattr(L, name)(h, lvl, a["polys"], p[0], out, batch, s[0], so, stream)
    if name in ("lsa_ckks_rotate", "lsa_bfv_rotate"):
        return getattr(L, name)(h, lvl, p[0], a["g"], a["key"], out, batch, s[0], so, stream)
    if name in ("lsa_ckks_mult_relin_rescale", "lsa_bfv_mult_relin"):
        return getattr(L, name)(h, lvl, p[0], p[1], a["key"], out, batch, s[0], s[1], so, stream)
    if name == "lsa_ckks_rotate_many":                   # g, key, out: lists
        n = len(a["g"])
        els = (ctypes.c_uint64 * n)(*a["g"])
        keys = (ctypes.c_void_p * n)(*[k.value if hasattr(k, "value") else k for k in a["key"]])
        outs = (ctypes.c_void_p * n)(*out)
        return L.lsa_ckks_rotate_many(h, lvl, p[0], n, els, keys, outs, batch, s[0], so, stream)
    raise KeyError(name)


def last_error():
    from lattisense_amd._native import lib
    return lib().lsa_last_error().decode()
