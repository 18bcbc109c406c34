"""Helpers of tests/test_gpu_entry_layout.py and tests/test_gpu_operator_layout.py: operands placed inside larger, sentinel-filled
device buffers, and one function that turns a dictionary of arguments into the raw C call of an entry point."""
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


def padded_operands(ctx, arrays, batch, room=0):
    """padded_inputs for any number of operands (a multiply-accumulate has seven): operand i at its own base, 36 words after the
    one before, with its own pad -- PADS for the first three, then 22, 26, 30 ..."""
    out = []
    for i, a in enumerate(arrays):
        words = a[0].size
        base = BASES[i] if i < len(BASES) else BASES[-1] + 36 * (i - len(BASES) + 1)
        pad = PADS[i] if i < len(PADS) else PADS[-1] + 4 * (i - len(PADS) + 1)
        out.append(Field(ctx, words, batch, base, words + pad, a, room))
    return out


def padded_outputs(ctx, words, batch, inputs, count=1, room=0):
    """`count` sentinel-filled outputs with ONE stride, larger than every input's (the hoisted rotations take one stride for all
    their outputs), each in a buffer of its own at a base no input uses"""
    stride = max([words] + [f.stride for f in inputs]) + OUT_PAD
    first = max([BASES[3] - 36] + [f.base for f in inputs]) + 36
    return [Field(ctx, words, batch, first + 36 * j, stride, room=room) for j in range(count)]


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
    return _invoke_operator(name, L, h, a, stream)


def _vp(values):
    return (ctypes.c_void_p * max(len(values), 1))(*[v.value if hasattr(v, "value") else v for v in values])


def _ll(values):
    return (ctypes.c_longlong * max(len(values), 1))(*[int(v) for v in values])


def _u64(values):
    return (ctypes.c_uint64 * max(len(values), 1))(*[int(v) for v in values])


def _glk(glk):
    """{galois element: key handle} -> (count, elements, handles)"""
    return len(glk), _u64(list(glk)), _vp(list(glk.values()))


def _invoke_operator(name, L, h, a, stream):
    """the second-generation operators.  ptrs / strides list the inputs in the entry point's own order: the ciphertexts, then the
    plaintexts (or the b side), then the partial sum / addend where a["partial"] / a["addend"] says there is one.  Further keys:
    n (terms), g and key (lists: Galois elements and their keys), plan (handle), glk ({element: key}), rescale, k and c."""
    p, s, lvl, out, so, batch = a["ptrs"], a["strides"], a["level"], a["out"], a["so"], a["batch"]
    if name == "lsa_bfv_rotate_many":                    # g, key, out: lists
        n = len(a["g"])
        return L.lsa_bfv_rotate_many(h, lvl, p[0], n, _u64(a["g"]), _vp(a["key"]), _vp(out), batch, s[0], so, stream)
    if name == "lsa_bfv_mult_plain_mul":
        return L.lsa_bfv_mult_plain_mul(h, lvl, p[0], p[1], out, batch, s[0], s[1], so, stream)
    if name == "lsa_bfv_mac_plain_mul":
        n = a["n"]
        part = (p[2 * n], s[2 * n]) if a.get("partial") else (None, 0)
        return L.lsa_bfv_mac_plain_mul(h, lvl, n, _vp(p[:n]), _ll(s[:n]), _vp(p[n:2 * n]), _ll(s[n:2 * n]), part[0], part[1], out, batch, so,
                                       stream)
    if name == "lsa_bfv_rotate_mac_plain_mul":
        n = len(a["g"])
        part = (p[1 + n], s[1 + n]) if a.get("partial") else (None, 0)
        return L.lsa_bfv_rotate_mac_plain_mul(h, lvl, p[0], n, _u64(a["g"]), _vp(a["key"]), _vp(p[1:1 + n]), _ll(s[1:1 + n]), part[0], part[1],
                                              out, batch, s[0], so, stream)
    if name in ("lsa_ckks_slot_sum", "lsa_bfv_slot_sum", "lsa_bfv_linear_transform"):
        return getattr(L, name)(h, a["plan"], p[0], out, batch, s[0], so, *_glk(a["glk"]), stream)
    if name == "lsa_ckks_linear_transform":
        return L.lsa_ckks_linear_transform(h, a["plan"], p[0], out, batch, s[0], so, int(a["rescale"]), *_glk(a["glk"]), stream)
    if name in ("lsa_ckks_poly_eval", "lsa_bfv_poly_eval"):
        return getattr(L, name)(h, a["plan"], p[0], out, batch, s[0], so, a["key"], stream)
    if name == "lsa_bfv_affine_const":
        return L.lsa_bfv_affine_const(h, lvl, p[0], s[0], a["k"], a["c"], out, so, batch, stream)
    if name in ("lsa_ckks_mult_sum", "lsa_ckks_dot", "lsa_bfv_mult_sum", "lsa_bfv_dot"):
        n = a["n"]
        add = (p[2 * n], s[2 * n]) if a.get("addend") else (None, 0)
        terms = (_vp(p[:n]), _ll(s[:n])), (_vp(p[n:2 * n]), _ll(s[n:2 * n]))
        if name == "lsa_ckks_mult_sum":
            return L.lsa_ckks_mult_sum(h, lvl, n, *terms[0], None, *terms[1], None, add[0], add[1], out, batch, so, stream)
        if name == "lsa_ckks_dot":
            return L.lsa_ckks_dot(h, lvl, n, *terms[0], None, *terms[1], None, add[0], add[1], a["key"], out, batch, so, int(a["rescale"]),
                                  stream)
        if name == "lsa_bfv_mult_sum":
            return L.lsa_bfv_mult_sum(h, lvl, n, *terms[0], *terms[1], add[0], add[1], out, batch, so, stream)
        return L.lsa_bfv_dot(h, lvl, n, *terms[0], *terms[1], add[0], add[1], a["key"], out, batch, so, stream)
    raise KeyError(name)


def last_error():
    from lattisense_amd._native import lib
    return lib().lsa_last_error().decode()
