"""Host-side mirror of the operator surface the reference's GPU executors use (heongpu::HEContext +
HEArithmeticOperator as called from mega_ag_runners/gpu/mega_ag_executors_gpu.cu:71-426), over the C-ABI.

Buffers are device-resident u64 limb arrays laid out [batch][poly][limb][N]; NumPy is used only to move test data in
and out.  No arithmetic happens in Python.
"""
import ctypes

import numpy as np

from . import _native
from ._native import check, lib

ALGO_BFV, ALGO_CKKS = 0, 1


class DeviceBuffer:
    def __init__(self, ctx, nwords):
        self.ctx = ctx
        self.nwords = int(nwords)
        p = ctypes.c_void_p()
        check(lib().lsa_malloc(ctx.h, ctypes.byref(p), self.nwords * 8))
        self.ptr = p.value

    def free(self):
        if self.ptr:
            check(lib().lsa_free(self.ctx.h, self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceContext:
    """One parameter set on one GPU (replaces init_gpu_context, gpu_wrapper.cu:53-138; tables are cached)."""

    def __init__(self, algo, n, q, p, t=0, device=0):
        self.algo, self.n, self.q, self.p, self.t = algo, int(n), list(q), list(p), int(t)
        qa = (ctypes.c_uint64 * len(q))(*q)
        pa = (ctypes.c_uint64 * max(1, len(p)))(*p)
        h = ctypes.c_void_p()
        check(lib().lsa_context_create(algo, self.n, qa, len(q), pa, len(p), self.t, device, ctypes.byref(h)))
        self.h = h
        self.stream = None  # default (null) stream unless the caller sets one
        cnt = ctypes.c_int()
        out = (ctypes.c_uint64 * 256)()
        check(lib().lsa_context_moduli(self.h, out, 256, ctypes.byref(cnt)))
        self.moduli = [int(out[i]) for i in range(cnt.value)]

    def close(self):
        if self.h:
            check(lib().lsa_context_destroy(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- memory
    def alloc(self, nwords):
        return DeviceBuffer(self, nwords)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        buf = self.alloc(arr.size)
        check(lib().lsa_memcpy_h2d(self.h, buf.ptr, arr.ctypes.data, arr.nbytes, self.stream))
        self.sync()
        return buf

    def download(self, buf, shape):
        out = np.empty(shape, dtype=np.uint64)
        assert out.size <= buf.nwords
        check(lib().lsa_memcpy_d2h(self.h, out.ctypes.data, buf.ptr, out.nbytes, self.stream))
        return out

    def sync(self):
        check(lib().lsa_stream_synchronize(self.h, self.stream))

    def set_tile_batch(self, tb):
        check(lib().lsa_set_tile_batch(self.h, tb))

    def set_ntt_chunk_mib(self, mib):
        """> 0: two-pass transforms run both passes over chunks of at most `mib` MiB of the batch (identical results); 0: off"""
        check(lib().lsa_set_ntt_chunk_mib(self.h, int(mib)))

    def baseconv_plans(self):
        """the base-conversion plans built so far: a list of (source limbs, destination limbs, runs the 29-bit split)"""
        cnt = ctypes.c_int()
        check(lib().lsa_debug_baseconv_plans(self.h, 0, ctypes.byref(cnt), None, None, None))
        n = cnt.value
        ns, nd, sp = (ctypes.c_int * max(n, 1))(), (ctypes.c_int * max(n, 1))(), (ctypes.c_int * max(n, 1))()
        check(lib().lsa_debug_baseconv_plans(self.h, n, ctypes.byref(cnt), ns, nd, sp))
        return [(ns[i], nd[i], bool(sp[i])) for i in range(min(n, cnt.value))]

    def key_switch_fused(self, level, key):
        """whether a switch with this one key at this level runs the fused second pass + key MAC kernel"""
        out = ctypes.c_int()
        check(lib().lsa_debug_key_switch_fused(self.h, level, key, ctypes.byref(out)))
        return bool(out.value)

    def set_modup_lift(self, enable):
        """0: single-limb key-switch digits go through the base-conversion kernel like the others (A/B, identical results)"""
        check(lib().lsa_set_modup_lift(self.h, int(enable)))

    def set_ks_tail_in_mac(self, mode):
        """the merged rescale tail inside the fused key MAC: 0 never, 1 (default) at N = 2^16, 2 wherever the shape allows
        (identical results)"""
        check(lib().lsa_set_ks_tail_in_mac(self.h, int(mode)))

    def set_rescale_head_in_conv(self, mode):
        """the merged rescale head formed inside ModDown's base conversion: 0 never, 1 (default) at N >= 2^16, 2 every ring
        (identical results)"""
        check(lib().lsa_set_rescale_head_in_conv(self.h, int(mode)))

    def set_bfv_dot_chunk(self, pairs):
        """pairs that bfv_mult_sum / bfv_dot extend per tensor launch (0: the default); the same words for every value"""
        check(lib().lsa_set_bfv_dot_chunk(self.h, int(pairs)))

    def set_fp64_ntt(self, enable):
        check(lib().lsa_set_fp64_ntt(self.h, int(enable)))

    # ---- keys
    def upload_key(self, compact, key_level):
        compact = np.ascontiguousarray(compact, dtype=np.uint64)
        assert compact.nbytes == lib().lsa_key_bytes(self.h, key_level), "key shape does not match its level"
        k = ctypes.c_void_p()
        check(lib().lsa_key_upload(self.h, compact.ctypes.data, key_level, self.stream, ctypes.byref(k)))
        return k

    def adopt_key(self, dev_ptr, key_level):
        k = ctypes.c_void_p()
        check(lib().lsa_key_adopt_device(self.h, dev_ptr, key_level, self.stream, ctypes.byref(k)))
        return k

    def key_bytes(self, key_level):
        return lib().lsa_key_bytes(self.h, key_level)

    def destroy_key(self, k):
        check(lib().lsa_key_destroy(self.h, k))

    # ---- operators (all batched; strides in u64 elements)
    def ntt(self, buf, batch, rows, mod_of, inverse=False, batch_stride=None):
        mo = (ctypes.c_int * len(mod_of))(*mod_of)
        bs = rows * self.n if batch_stride is None else batch_stride
        check(lib().lsa_ntt(self.h, buf.ptr, batch, bs, rows, mo, len(mod_of), int(inverse), self.stream))

    def addsub(self, op, level, polys, a, b, batch):
        L = level + 1
        out = self.alloc(batch * polys * L * self.n)
        s = polys * L * self.n
        check(lib().lsa_poly_addsub(self.h, op, level, polys, a.ptr, b.ptr if b is not None else None, out.ptr,
                                    batch, s, s, s, self.stream))
        return out

    def ckks_mult(self, level, a, b, batch):
        L = level + 1
        out = self.alloc(batch * 3 * L * self.n)
        check(lib().lsa_ckks_mult(self.h, level, a.ptr, b.ptr, out.ptr, batch, 2 * L * self.n, 2 * L * self.n,
                                  3 * L * self.n, self.stream))
        return out

    def ckks_relin(self, level, d3, rlk, batch):
        L = level + 1
        out = self.alloc(batch * 2 * L * self.n)
        check(lib().lsa_ckks_relin(self.h, level, d3.ptr, rlk, out.ptr, batch, 3 * L * self.n, 2 * L * self.n,
                                   self.stream))
        return out

    def ckks_rescale(self, level, polys, ct, batch):
        L = level + 1
        out = self.alloc(batch * polys * level * self.n)
        check(lib().lsa_ckks_rescale(self.h, level, polys, ct.ptr, out.ptr, batch, polys * L * self.n,
                                     polys * level * self.n, self.stream))
        return out

    def ckks_rotate_many(self, level, ct, keys, batch):
        """keys: {galois element: key handle}; returns {element: device buffer}, one decomposition for all (hoisted)"""
        L = level + 1
        outs = {g: self.alloc(batch * 2 * L * self.n) for g in keys}
        els = (ctypes.c_uint64 * len(keys))(*keys.keys())
        hk = (ctypes.c_void_p * len(keys))(*[k.value for k in keys.values()])
        po = (ctypes.c_void_p * len(keys))(*[o.ptr for o in outs.values()])
        check(lib().lsa_ckks_rotate_many(self.h, level, ct.ptr, len(keys), els, hk, po, batch, 2 * L * self.n, 2 * L * self.n,
                                         self.stream))
        return outs

    def ckks_rotate(self, level, ct, g, glk, batch):
        L = level + 1
        out = self.alloc(batch * 2 * L * self.n)
        check(lib().lsa_ckks_rotate(self.h, level, ct.ptr, g, glk, out.ptr, batch, 2 * L * self.n, 2 * L * self.n,
                                    self.stream))
        return out

    def drop_level(self, level, polys, ct, batch):
        L = level + 1
        out = self.alloc(batch * polys * level * self.n)
        check(lib().lsa_drop_level(self.h, level, polys, ct.ptr, out.ptr, batch, polys * L * self.n,
                                   polys * level * self.n, self.stream))
        return out

    def ckks_mult_relin_rescale(self, level, a, b, rlk, batch, out=None):
        L = level + 1
        if out is None:
            out = self.alloc(batch * 2 * level * self.n)
        check(lib().lsa_ckks_mult_relin_rescale(self.h, level, a.ptr, b.ptr, rlk, out.ptr, batch, 2 * L * self.n,
                                                2 * L * self.n, 2 * level * self.n, self.stream))
        return out

    def _dot_terms(self, level, a_list, b_list, addend):
        n, w = len(a_list), 2 * (level + 1) * self.n
        assert n == len(b_list), "as many b operands as a operands"
        pa = (ctypes.c_void_p * max(n, 1))(*[a.ptr for a in a_list])
        pb = (ctypes.c_void_p * max(n, 1))(*[b.ptr for b in b_list])
        st = (ctypes.c_longlong * max(n, 1))(*([w] * n))
        return n, pa, st, None, pb, st, None, addend.ptr if addend is not None else None, w

    def ckks_mult_sum(self, level, a_list, b_list, batch, addend=None, out=None):
        """d3 = sum_i a_list[i] (x) b_list[i] (+ addend on polynomials 0 and 1): [batch][3][level+1][N]"""
        L = level + 1
        if out is None:
            out = self.alloc(batch * 3 * L * self.n)
        check(lib().lsa_ckks_mult_sum(self.h, level, *self._dot_terms(level, a_list, b_list, addend), out.ptr, batch,
                                      3 * L * self.n, self.stream))
        return out

    def ckks_dot(self, level, a_list, b_list, rlk, batch, rescale=True, addend=None, out=None):
        """sum_i a_list[i] x b_list[i] (+ addend) with one relinearisation (and one rescale): [batch][2][level | level+1][N]"""
        rows = level if rescale else level + 1
        if out is None:
            out = self.alloc(batch * 2 * rows * self.n)
        check(lib().lsa_ckks_dot(self.h, level, *self._dot_terms(level, a_list, b_list, addend), rlk, out.ptr, batch,
                                 2 * rows * self.n, int(bool(rescale)), self.stream))
        return out

    # ---- CKKS plaintext and constant operands (ct / out: [batch][2][level+1][N], pt: [batch][level+1][N], compact strides)
    def _plain_out(self, level, batch, rescale, out):
        rows = level if rescale else level + 1
        if out is None:
            out = self.alloc(max(batch, 1) * 2 * rows * self.n)
        return out, 2 * rows * self.n

    def ckks_encode(self, level, values, scale, batch=1, out=None):
        """values: [batch][2^log_slots] complex (tiled over the N/2 slots) -> device plaintexts [batch][level+1][N] at `scale`"""
        v = np.ascontiguousarray(np.asarray(values, dtype=np.complex128).reshape(max(batch, 1), -1))
        period = v.shape[1]
        assert period >= 1 and period & (period - 1) == 0, "2^log_slots values per plaintext"
        w = (level + 1) * self.n
        if out is None:
            out = self.alloc(max(batch, 1) * w)
        check(lib().lsa_ckks_encode(self.h, level, period.bit_length() - 1, v.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                    float(scale), out.ptr, w, batch, self.stream))
        return out

    def bfv_pt_rows(self, level, form):
        """rows of a BFV plaintext: form 0 ring-t coefficients (1), 1 pt_mul (level+1), 2 extended over Q_level u P (level+1+k)"""
        return {0: 1, 1: level + 1, 2: level + 1 + len(self.p)}[form]

    def bfv_encode(self, level, form, values, out=None, sout=None):
        """values: [batch][N] integers in [0, t), row 0 of the 2 x N/2 slot matrix then row 1 -> device plaintexts
        [batch][rows][N] (include/lattisense_amd.h: lsa_bfv_encode); sout: batch stride in words (default: compact)"""
        v = np.ascontiguousarray(np.asarray(values, dtype=np.uint64).reshape(-1, self.n))
        batch = v.shape[0]
        w = self.bfv_pt_rows(level, form) * self.n
        sout = w if sout is None else sout
        if out is None:
            out = self.alloc(max(batch, 1) * max(sout, w))
        check(lib().lsa_bfv_encode(self.h, level, form, v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), out.ptr, sout, batch, self.stream))
        return out

    def ckks_mult_plain(self, level, ct, pt, batch, rescale=False, out=None, spt=None):
        """ct x pt on both polynomials (then rescaled); spt: the plaintexts' batch stride in words (0: one for the whole batch)"""
        out, so = self._plain_out(level, batch, rescale, out)
        L = level + 1
        check(lib().lsa_ckks_mult_plain(self.h, level, ct.ptr, 2 * L * self.n, pt.ptr, L * self.n if spt is None else spt, out.ptr, so,
                                        batch, int(bool(rescale)), self.stream))
        return out

    def ckks_addsub_plain(self, op, level, ct, pt, batch, out=None, spt=None):
        """op 0: c0 + pt, 1: c0 - pt; c1 unchanged"""
        out, so = self._plain_out(level, batch, False, out)
        L = level + 1
        check(lib().lsa_ckks_addsub_plain(self.h, op, level, ct.ptr, 2 * L * self.n, pt.ptr, L * self.n if spt is None else spt, out.ptr,
                                          so, batch, self.stream))
        return out

    def ckks_mac_plain(self, level, cts, pts, batch, rescale=False, addend=None, out=None, spts=None):
        """sum_i cts[i] x pts[i] (+ addend); spts: per-term plaintext strides (0: shared by the batch), default compact"""
        out, so = self._plain_out(level, batch, rescale, out)
        L, n = level + 1, len(cts)
        assert n == len(pts), "as many plaintexts as ciphertexts"
        pc = (ctypes.c_void_p * max(n, 1))(*[c.ptr for c in cts])
        sc = (ctypes.c_longlong * max(n, 1))(*([2 * L * self.n] * n))
        pp = (ctypes.c_void_p * max(n, 1))(*[p.ptr for p in pts])
        sp = (ctypes.c_longlong * max(n, 1))(*([L * self.n] * n if spts is None else spts))
        check(lib().lsa_ckks_mac_plain(self.h, level, n, pc, sc, pp, sp, addend.ptr if addend is not None else None, 2 * L * self.n,
                                       out.ptr, so, batch, int(bool(rescale)), self.stream))
        return out

    def ckks_mult_const(self, level, ct, value, const_scale, batch, rescale=False, out=None):
        """ct x round(value * const_scale), value complex: slot-wise; const_scale = 1 and value = +-1j multiplies by +-i exactly"""
        out, so = self._plain_out(level, batch, rescale, out)
        v = complex(value)
        check(lib().lsa_ckks_mult_const(self.h, level, ct.ptr, 2 * (level + 1) * self.n, v.real, v.imag, float(const_scale), out.ptr, so,
                                        batch, int(bool(rescale)), self.stream))
        return out

    def ckks_add_const(self, level, ct, value, ct_scale, batch, out=None):
        """ct + value in every slot, value complex, ct at scale ct_scale"""
        out, so = self._plain_out(level, batch, False, out)
        v = complex(value)
        check(lib().lsa_ckks_add_const(self.h, level, ct.ptr, 2 * (level + 1) * self.n, v.real, v.imag, float(ct_scale), out.ptr, so,
                                       batch, self.stream))
        return out

    def ckks_affine_const(self, level, ct, alpha, const_scale, beta, ct_scale, batch, rescale=False, out=None):
        """ct x alpha + beta in one pass (alpha at const_scale, beta at ct_scale * const_scale; then rescaled)"""
        out, so = self._plain_out(level, batch, rescale, out)
        a, b = complex(alpha), complex(beta)
        check(lib().lsa_ckks_affine_const(self.h, level, ct.ptr, 2 * (level + 1) * self.n, a.real, a.imag, float(const_scale), b.real,
                                          b.imag, float(ct_scale), out.ptr, so, batch, int(bool(rescale)), self.stream))
        return out

    def bfv_mult(self, level, a, b, batch):
        L = level + 1
        out = self.alloc(batch * 3 * L * self.n)
        check(lib().lsa_bfv_mult(self.h, level, a.ptr, b.ptr, out.ptr, batch, 2 * L * self.n, 2 * L * self.n,
                                 3 * L * self.n, self.stream))
        return out

    def bfv_relin(self, level, d3, rlk, batch):
        L = level + 1
        out = self.alloc(batch * 2 * L * self.n)
        check(lib().lsa_bfv_relin(self.h, level, d3.ptr, rlk, out.ptr, batch, 3 * L * self.n, 2 * L * self.n,
                                  self.stream))
        return out

    def bfv_rotate(self, level, ct, g, glk, batch):
        L = level + 1
        out = self.alloc(batch * 2 * L * self.n)
        check(lib().lsa_bfv_rotate(self.h, level, ct.ptr, g, glk, out.ptr, batch, 2 * L * self.n, 2 * L * self.n,
                                   self.stream))
        return out

    def bfv_mul_monomial(self, level, ct, exponent, batch, polys=2, out=None):
        """X^exponent * ct on `polys` coefficient-domain polynomials (the negacyclic shift); any exponent"""
        words = polys * (level + 1) * self.n
        if out is None:
            out = self.alloc(max(batch, 1) * words)
        check(lib().lsa_bfv_mul_monomial(self.h, level, polys, int(exponent), ct.ptr, out.ptr, batch, words, words, self.stream))
        return out

    def set_rgsw_pair_mac(self, enable):
        """0: an external product's two gadget products run as two key MAC launches instead of one k_ks_mac_pair (A/B, identical
        results)"""
        check(lib().lsa_set_rgsw_pair_mac(self.h, int(enable)))

    def bfv_external_product(self, level, ct, rgsw, batch, base=None, out=None):
        """ct [.] rgsw (+ base) on coefficient-domain ciphertexts [batch][2][level+1][N]; rgsw: the key handles (r0, r1) of an RGSW
        ciphertext (include/lattisense_amd.h: lsa_bfv_external_product).  out may be ct or base."""
        words = 2 * (level + 1) * self.n
        if out is None:
            out = self.alloc(max(batch, 1) * words)
        check(lib().lsa_bfv_external_product(self.h, level, ct.ptr, words, rgsw[0], rgsw[1], base.ptr if base is not None else None, words,
                                             out.ptr, words, batch, self.stream))
        return out

    def bfv_cmux(self, level, c0, c1, rgsw, batch, out=None):
        """c0 + rgsw [.] (c1 - c0): c1 where rgsw encrypts 1, c0 where it encrypts 0.  out may be c0 or c1."""
        words = 2 * (level + 1) * self.n
        if out is None:
            out = self.alloc(max(batch, 1) * words)
        check(lib().lsa_bfv_cmux(self.h, level, c0.ptr, words, c1.ptr, words, rgsw[0], rgsw[1], out.ptr, words, batch, self.stream))
        return out

    def bfv_rotate_many(self, level, ct, keys, batch):
        """keys: {galois element: key handle}; returns {element: device buffer}, one decomposition for all (hoisted), each
        output bit-identical to bfv_rotate's"""
        L = level + 1
        outs = {g: self.alloc(batch * 2 * L * self.n) for g in keys}
        els = (ctypes.c_uint64 * len(keys))(*keys.keys())
        hk = (ctypes.c_void_p * len(keys))(*[k.value for k in keys.values()])
        po = (ctypes.c_void_p * len(keys))(*[o.ptr for o in outs.values()])
        check(lib().lsa_bfv_rotate_many(self.h, level, ct.ptr, len(keys), els, hk, po, batch, 2 * L * self.n, 2 * L * self.n,
                                        self.stream))
        return outs

    def bfv_mult_plain_mul(self, level, ct, pt, batch, out=None, spt=None):
        """ct [batch][2][L][N] x pt_mul plaintexts [batch][L][N] (NTT domain, Montgomery form); out=ct multiplies in place;
        spt: the plaintexts' batch stride in words (0: one plaintext for the whole batch)"""
        L = level + 1
        if out is None:
            out = self.alloc(batch * 2 * L * self.n)
        check(lib().lsa_bfv_mult_plain_mul(self.h, level, ct.ptr, pt.ptr, out.ptr, batch, 2 * L * self.n,
                                           L * self.n if spt is None else spt, 2 * L * self.n, self.stream))
        return out

    # ---- BFV ring-t plaintext operands (ct / out: [batch][2][level+1][N], pt: [batch][N] ring-t coefficients, lsa_bfv_encode form 0)
    def bfv_addsub_plain(self, op, level, ct, pt, batch, out=None, spt=None, sct=None, sout=None):
        """op 0: ct + pt, 1: ct - pt, 2: pt - ct; out=ct works in place; spt: the plaintexts' batch stride in words (0: one
        plaintext for the whole batch); sct / sout: the ciphertexts' strides (default compact)"""
        w = 2 * (level + 1) * self.n
        sct = w if sct is None else sct
        sout = (sct if out is ct else w) if sout is None else sout
        if out is None:
            out = self.alloc(max(batch, 1) * sout)
        check(lib().lsa_bfv_addsub_plain(self.h, op, level, ct.ptr, sct, pt.ptr, self.n if spt is None else spt, out.ptr, sout, batch,
                                         self.stream))
        return out

    def bfv_plain_lift(self, level, form, pt, batch, out=None, spt=None, sout=None):
        """device ring-t plaintexts -> form 1 (pt_mul) or 2 (extended): [batch][rows][N], the words of bfv_encode; asynchronous"""
        w = self.bfv_pt_rows(level, form) * self.n
        sout = w if sout is None else sout
        if out is None:
            out = self.alloc(max(batch, 1) * sout)
        check(lib().lsa_bfv_plain_lift(self.h, level, form, pt.ptr, self.n if spt is None else spt, out.ptr, sout, batch, self.stream))
        return out

    def bfv_mult_plain(self, level, ct, pt, batch, out=None, spt=None):
        """ct x pt slot-wise, pt ring-t coefficients; out=ct multiplies in place; spt = 0: one plaintext for the whole batch"""
        w = 2 * (level + 1) * self.n
        if out is None:
            out = self.alloc(max(batch, 1) * w)
        check(lib().lsa_bfv_mult_plain(self.h, level, ct.ptr, w, pt.ptr, self.n if spt is None else spt, out.ptr, w, batch, self.stream))
        return out

    def bfv_mac_plain_mul(self, level, cts, pts, batch, partial=None):
        """sum_i cts[i] x pts[i] (+ partial): lists of device buffers, [batch][2][L][N] / [batch][L][N]"""
        L = level + 1
        n = len(cts)
        assert n == len(pts) and n >= 1
        out = self.alloc(batch * 2 * L * self.n)
        pc = (ctypes.c_void_p * n)(*[c.ptr for c in cts])
        sc = (ctypes.c_longlong * n)(*([2 * L * self.n] * n))
        pp = (ctypes.c_void_p * n)(*[p.ptr for p in pts])
        sp = (ctypes.c_longlong * n)(*([L * self.n] * n))
        check(lib().lsa_bfv_mac_plain_mul(self.h, level, n, pc, sc, pp, sp, partial.ptr if partial is not None else None,
                                          2 * L * self.n, out.ptr, batch, 2 * L * self.n, self.stream))
        return out

    def set_bfv_matvec_block(self, row_block=0, col_block=0):
        """forces the blocks of bfv_matvec_plain_mul: row_block in 0 (the default), 1, 2, 4, 8 output rows per workgroup, col_block
        columns per launch (0: all that fit the workspace).  A/B and parity; identical results"""
        check(lib().lsa_set_bfv_matvec_block(self.h, int(row_block), int(col_block)))

    def bfv_matvec_plain_mul(self, level, cts, pts, rows, cols, batch, partial=None, out=None, shared=True):
        """out[r] = sum_c cts[c] x pts[r][c] (+ partial[r]), the words of bfv_mac_plain_mul on row r's terms with every ciphertext
        transformed once (include/lattisense_amd.h: lsa_bfv_matvec_plain_mul).  cts: one device buffer [cols][batch][2][L][N], what
        BfvExpandPlan.run returns; pts: one device buffer of pt_mul plaintexts, [rows][cols][L][N] shared by the batch or, with
        shared=False, [batch][rows][cols][L][N]; partial and the result: [rows][batch][2][L][N], what BfvSelectPlan.run takes."""
        L = level + 1
        wct, wpt = 2 * L * self.n, L * self.n
        nb = max(batch, 1)
        per_item = not shared
        if out is None:
            out = self.alloc(rows * nb * wct)
        check(lib().lsa_bfv_matvec_plain_mul(self.h, level, rows, cols, cts.ptr, nb * wct, wct, pts.ptr, cols * wpt, wpt,
                                             rows * cols * wpt if per_item else 0, partial.ptr if partial is not None else None, nb * wct,
                                             wct, out.ptr, nb * wct, wct, batch, self.stream))
        return out

    def bfv_rotate_mac_plain_mul(self, level, ct, terms, batch, partial=None):
        """sum_i rotate(ct, g_i) x pt_i (+ partial), hoisted, the rotations kept in the NTT domain; terms: a list of
        (galois element, key handle or None for g = 1, pt_mul plaintexts [batch][L][N]); bit-identical to bfv_rotate_many
        followed by bfv_mac_plain_mul"""
        L = level + 1
        n = len(terms)
        assert n >= 1
        out = self.alloc(batch * 2 * L * self.n)
        els = (ctypes.c_uint64 * n)(*[g for g, _, _ in terms])
        hk = (ctypes.c_void_p * n)(*[k.value if k is not None else None for _, k, _ in terms])
        pp = (ctypes.c_void_p * n)(*[p.ptr for _, _, p in terms])
        sp = (ctypes.c_longlong * n)(*([L * self.n] * n))
        check(lib().lsa_bfv_rotate_mac_plain_mul(self.h, level, ct.ptr, n, els, hk, pp, sp,
                                                 partial.ptr if partial is not None else None, 2 * L * self.n, out.ptr, batch,
                                                 2 * L * self.n, 2 * L * self.n, self.stream))
        return out

    def bfv_rescale(self, level, polys, ct, batch):
        L = level + 1
        out = self.alloc(batch * polys * level * self.n)
        check(lib().lsa_bfv_rescale(self.h, level, polys, ct.ptr, out.ptr, batch, polys * L * self.n,
                                    polys * level * self.n, self.stream))
        return out

    def bfv_mult_relin(self, level, a, b, rlk, batch, out=None):
        L = level + 1
        if out is None:
            out = self.alloc(batch * 2 * L * self.n)
        check(lib().lsa_bfv_mult_relin(self.h, level, a.ptr, b.ptr, rlk, out.ptr, batch, 2 * L * self.n,
                                       2 * L * self.n, 2 * L * self.n, self.stream))
        return out

    def _bfv_dot_terms(self, level, a_list, b_list, addend, sas=None, sbs=None):
        n, w = len(a_list), 2 * (level + 1) * self.n
        assert n == len(b_list), "as many b operands as a operands"
        pa = (ctypes.c_void_p * max(n, 1))(*[a.ptr for a in a_list])
        pb = (ctypes.c_void_p * max(n, 1))(*[b.ptr for b in b_list])
        sa = (ctypes.c_longlong * max(n, 1))(*([w] * n if sas is None else sas))
        sb = (ctypes.c_longlong * max(n, 1))(*([w] * n if sbs is None else sbs))
        return n, pa, sa, pb, sb, addend.ptr if addend is not None else None, w

    def bfv_mult_sum(self, level, a_list, b_list, batch, addend=None, out=None, sas=None, sbs=None):
        """d3 = t * round(sum_i a_list[i] (x) b_list[i] / Q) (+ addend on polynomials 0 and 1): [batch][3][level+1][N]; sas / sbs:
        per-term batch strides in words (0: one ciphertext shared by the batch), default compact"""
        L = level + 1
        if out is None:
            out = self.alloc(max(batch, 1) * 3 * L * self.n)
        check(lib().lsa_bfv_mult_sum(self.h, level, *self._bfv_dot_terms(level, a_list, b_list, addend, sas, sbs), out.ptr, batch,
                                     3 * L * self.n, self.stream))
        return out

    def bfv_dot(self, level, a_list, b_list, rlk, batch, addend=None, out=None, sas=None, sbs=None):
        """sum_i a_list[i] x b_list[i] (+ addend) with one scale-down and one relinearisation: [batch][2][level+1][N]"""
        L = level + 1
        if out is None:
            out = self.alloc(max(batch, 1) * 2 * L * self.n)
        check(lib().lsa_bfv_dot(self.h, level, *self._bfv_dot_terms(level, a_list, b_list, addend, sas, sbs), rlk, out.ptr, batch,
                                2 * L * self.n, self.stream))
        return out

    def bfv_affine_const(self, level, ct, k, c, batch, out=None):
        """k * ct + c in every slot, k and c in [0, t): [batch][2][level+1][N], coefficient domain; out=ct works in place"""
        w = 2 * (level + 1) * self.n
        if out is None:
            out = self.alloc(max(batch, 1) * w)
        check(lib().lsa_bfv_affine_const(self.h, level, ct.ptr, w, int(k), int(c), out.ptr, w, batch, self.stream))
        return out


def bfv_dot_plan(n, q, level, terms):
    """{max_terms, groups, aux_limbs} of the BFV inner product of `terms` pairs at `level` of the chain q at ring degree n -- host
    only (include/lattisense_amd.h: lsa_bfv_dot_plan, with the headroom rule)"""
    qa = (ctypes.c_uint64 * max(len(q), 1))(*[int(x) for x in q])
    mt, ng, al = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(lib().lsa_bfv_dot_plan(int(n), qa, len(q), int(level), int(terms), ctypes.byref(mt), ctypes.byref(ng), ctypes.byref(al)))
    return {"max_terms": mt.value, "groups": ng.value, "aux_limbs": al.value}


def _key_arrays(glk):
    """{galois element: key handle} -> (count, elements, handles) as an operator's three key arguments"""
    n = len(glk)
    return n, (ctypes.c_uint64 * max(n, 1))(*glk.keys()), (ctypes.c_void_p * max(n, 1))(*[k.value for k in glk.values()])


def _fetch(ctype, count, fill):
    """the list an entry point writes into a caller's array of `count` elements: fill(array, count)"""
    a = (ctype * max(count, 1))()
    check(fill(a, count))
    return [int(x) for x in a[:count]]


class _Plan:
    """The handle of a device plan: `h` (None until the plan exists), released by close() or with the object.  A subclass
    names its destroy entry point; one that plans on the host makes the handle in _handle(), on first use."""
    _destroy = None

    def _adopt(self, create):
        """create(byref(handle)) -> status: the handle becomes self.h"""
        h = ctypes.c_void_p()
        check(create(ctypes.byref(h)))
        self.h = h
        return h

    def close(self):
        if getattr(self, "h", None):
            getattr(lib(), self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BootstrapPlan(_Plan):
    """Device-side CKKS bootstrapping plan (include/lattisense_amd.h: lsa_bootstrap_*)."""
    _destroy = "lsa_bootstrap_destroy"

    def __init__(self, ctx, cts_depth=4, stc_depth=3, k=16, double_angle=3, message_ratio=256.0, in_scale=2.0 ** 40,
                 out_scale=0.0, log_slots=0, sine_deg=30, arcsine_deg=0):
        self.ctx = ctx
        self._adopt(lambda h: lib().lsa_bootstrap_create_ex(ctx.h, cts_depth, stc_depth, k, double_angle, message_ratio, in_scale,
                                                            out_scale, log_slots, sine_deg, arcsine_deg, ctx.stream, h))
        lv, sc, ng, nm, nc, sp = ctypes.c_int(), ctypes.c_double(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib().lsa_bootstrap_info(self.h, ctypes.byref(lv), ctypes.byref(sc), ctypes.byref(ng), ctypes.byref(nm),
                                       ctypes.byref(nc), ctypes.byref(sp)))
        self.out_level, self.out_scale, self.n_matrices = lv.value, sc.value, nm.value
        self.sparse, self.n_cts = bool(sp.value), nc.value
        self.galois_elements = _fetch(ctypes.c_uint64, ng.value, lambda a, n: lib().lsa_bootstrap_galois_elements(self.h, a, n))
        # double hoisting (the default): baby-step / giant-step matrices carry plaintext rows for the special primes too
        self.double_hoist = False
        for i in range(self.n_matrices):
            lvl, rows = ctypes.c_int(), ctypes.c_int()
            check(lib().lsa_bootstrap_matrix_info(self.h, i, ctypes.byref(lvl), None, None, None, 0))
            check(lib().lsa_bootstrap_plaintext_rows(self.h, i, ctypes.byref(rows)))
            self.double_hoist = self.double_hoist or rows.value > lvl.value + 1

    def __del__(self):   # a bootstrap plan is released by close() alone, as it has always been
        pass

    def chebyshev(self):
        return self.evalmod_constants()[0]

    def evalmod_constants(self):
        """(Chebyshev coefficients of the cosine interpolant, monomial coefficients of the arcsine correction or None)"""
        nc, na = ctypes.c_int(), ctypes.c_int()
        check(lib().lsa_bootstrap_evalmod_constants(self.h, ctypes.byref(nc), None, ctypes.byref(na), None))
        c = (ctypes.c_double * nc.value)()
        a = (ctypes.c_double * max(na.value, 1))()
        check(lib().lsa_bootstrap_evalmod_constants(self.h, None, c, None, a))
        return np.array(c[:], dtype=np.float64), (np.array(a[: na.value], dtype=np.float64) if na.value else None)

    def matrix(self, index):
        """(level, n1 (0: no baby-step/giant-step), diagonal indices, {k: plaintext [rows][N]}); rows = level+1, or level+1+k
        (residues at the special primes too) for a baby-step / giant-step matrix of a double-hoisting plan"""
        lv, n1, nd = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib().lsa_bootstrap_matrix_info(self.h, index, ctypes.byref(lv), ctypes.byref(n1), ctypes.byref(nd), None, 0))
        ks = _fetch(ctypes.c_int, nd.value, lambda a, n: lib().lsa_bootstrap_matrix_info(self.h, index, None, None, None, a, n))
        plains = {}
        rows = ctypes.c_int()
        check(lib().lsa_bootstrap_plaintext_rows(self.h, index, ctypes.byref(rows)))
        for i, k in enumerate(ks):
            pt = np.empty((rows.value, self.ctx.n), dtype=np.uint64)
            check(lib().lsa_bootstrap_plaintext_ext(self.h, index, i, pt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), pt.size))
            plains[k] = pt
        return lv.value, n1.value, ks, plains

    def run(self, in_buf, batch, rlk, glk, swk_dts=None, swk_std=None):
        """in_buf: device [batch][2][1][N]; glk: {galois element: key handle}; returns device [batch][2][out_level+1][N]"""
        n = self.ctx.n
        out = self.ctx.alloc(batch * 2 * (self.out_level + 1) * n)
        check(lib().lsa_ckks_bootstrap(self.ctx.h, self.h, in_buf.ptr, out.ptr, batch, 2 * n, 2 * (self.out_level + 1) * n, rlk,
                                       *_key_arrays(glk), swk_dts, swk_std, self.ctx.stream))
        return out

    def oracle_plains(self):
        """the plan's encoded diagonals keyed as oracle/ckks_bootstrap.py expects them"""
        keys = [("cts", i) for i in range(self.n_cts)] + ([("p1",), ("p2",)] if self.sparse else [])
        keys += [("stc", i) for i in range(self.n_matrices - len(keys))]
        return {k: self.matrix(i)[3] for i, k in enumerate(keys)}

    def oracle_levels(self):
        """level of every matrix, keyed like oracle_plains()"""
        keys = [("cts", i) for i in range(self.n_cts)] + ([("p1",), ("p2",)] if self.sparse else [])
        keys += [("stc", i) for i in range(self.n_matrices - len(keys))]
        out = {}
        for i, k in enumerate(keys):
            lv = ctypes.c_int()
            check(lib().lsa_bootstrap_matrix_info(self.h, i, ctypes.byref(lv), None, None, None, 0))
            out[k] = lv.value
        return out


def plan_rotations(period, diag_index, ratio=0.0):
    """(n1, rotations): the baby-step count (0: no split) and the non-zero rotations a diagonal index set gets -- host only"""
    idx = (ctypes.c_int * len(diag_index))(*[int(k) for k in diag_index])
    n1, cnt = ctypes.c_int(), ctypes.c_int()
    check(lib().lsa_lt_plan_rotations(period, len(diag_index), idx, ratio, ctypes.byref(n1), None, 0, ctypes.byref(cnt)))
    rot = _fetch(ctypes.c_int, cnt.value, lambda a, n: lib().lsa_lt_plan_rotations(period, len(diag_index), idx, ratio, ctypes.byref(n1), a, n, None))
    return n1.value, rot


class LinearTransformPlan(_Plan):
    """A plaintext matrix in diagonal form, encoded for ciphertexts at `level` (include/lattisense_amd.h: lsa_lt_*).
    diags: {k: complex array of length period}, d_k[t] multiplies x[(t + k) mod period], period = 2^log_slots (default: the
    arrays' length)."""
    _destroy = "lsa_lt_destroy"

    def __init__(self, ctx, level, diags, log_slots=None, pt_scale=0, ratio=0, double_hoist=True):
        self.ctx = ctx
        self.h = None
        ks = list(diags)
        assert ks, "at least one diagonal"
        period = len(diags[ks[0]]) if log_slots is None else 1 << log_slots
        assert period & (period - 1) == 0 and all(len(diags[k]) == period for k in ks), "diagonals must have 2^log_slots entries"
        vals = np.empty((len(ks), period, 2), dtype=np.float64)
        for i, k in enumerate(ks):
            d = np.asarray(diags[k], dtype=np.complex128)
            vals[i, :, 0], vals[i, :, 1] = d.real, d.imag
        idx = (ctypes.c_int * len(ks))(*[int(k) for k in ks])
        self._adopt(lambda h: lib().lsa_lt_create(ctx.h, level, period.bit_length() - 1, len(ks), idx,
                                                  vals.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), float(pt_scale), float(ratio),
                                                  int(bool(double_hoist)), ctx.stream, h))
        lv, pe, nd, n1, rows, ng, dh, sc = (ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(),
                                            ctypes.c_int(), ctypes.c_int(), ctypes.c_double())
        check(lib().lsa_lt_info(self.h, ctypes.byref(lv), ctypes.byref(pe), ctypes.byref(nd), ctypes.byref(n1), ctypes.byref(rows),
                                ctypes.byref(ng), ctypes.byref(dh), ctypes.byref(sc)))
        self.level, self.period, self.n1, self.rows = lv.value, pe.value, n1.value, rows.value
        self.double_hoist, self.pt_scale = bool(dh.value), sc.value
        self.diagonals = _fetch(ctypes.c_int, nd.value, lambda a, n: lib().lsa_lt_diagonals(self.h, a, n))
        self.galois_elements = _fetch(ctypes.c_uint64, ng.value, lambda a, n: lib().lsa_lt_galois_elements(self.h, a, n))

    def oracle_plains(self):
        """{k (reduced mod period): plaintext [rows][N]}: what oracle/ckks_bootstrap.py linear_transform takes as `plains`"""
        out = {}
        for i, k in enumerate(self.diagonals):
            pt = np.empty((self.rows, self.ctx.n), dtype=np.uint64)
            check(lib().lsa_lt_plaintext(self.h, i, pt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), pt.size))
            out[k] = pt
        return out

    def run(self, in_buf, batch, glk, rescale=True, out=None):
        """in_buf: device [batch][2][level+1][N]; glk: {galois element: key handle}; returns device
        [batch][2][level (rescale) | level+1][N]"""
        n = self.ctx.n
        lo = self.level if rescale else self.level + 1
        if out is None:
            out = self.ctx.alloc(max(batch, 1) * 2 * lo * n)
        check(lib().lsa_ckks_linear_transform(self.ctx.h, self.h, in_buf.ptr, out.ptr, batch, 2 * (self.level + 1) * n, 2 * lo * n,
                                              int(bool(rescale)), *_key_arrays(glk), self.ctx.stream))
        return out


def bfv_lt_plan(n, period, diag_index, ratio=0.0):
    """{n1, rotations, galois_elements, babies, giants, moddowns} of the BFV linear transform over these diagonals at ring degree
    n -- host only: the split of plan_rotations (lsa_lt_plan_rotations), n1 = 0 meaning every diagonal is a baby step of giant 0"""
    assert period >= 1 and period & (period - 1) == 0 and (n // 2) % period == 0, "period: a power of two that divides N/2"
    n1, rot = plan_rotations(period, diag_index, ratio)
    ks = sorted({int(k) % period for k in diag_index})
    split = n1 if n1 else period
    giants = sorted({(k // split) * split for k in ks})
    babies = sorted({k % split for k in ks})
    return {"n1": n1, "rotations": rot, "galois_elements": sorted(pow(5, r, 2 * n) for r in rot), "babies": babies, "giants": giants,
            "moddowns": len([g for g in giants if g]) + 1}


class BfvLinearTransformPlan(_Plan):
    """A plaintext matrix in diagonal form over both rows of the BFV slot matrix, encoded for ciphertexts at `level`
    (include/lattisense_amd.h: lsa_bfv_lt_*).  diags: {k: integer array [2][period] (one vector per slot row) or [period] (the
    same vector on both rows)}, values in [0, t): out_row[c] = sum_k d_k,row[c mod period] * x_row[(c + k) mod N/2] mod t.
    Planning needs no GPU (`.n1`, `.rotations`, `.galois_elements`); the device plan is created on first use."""
    _destroy = "lsa_bfv_lt_destroy"

    def __init__(self, ctx, level, diags, period=None, ratio=0.0):
        self.ctx, self.level, self.ratio = ctx, level, ratio
        self.h = None
        ks = list(diags)
        assert ks, "at least one diagonal"
        first = np.asarray(diags[ks[0]])
        self.period = int(first.shape[-1]) if period is None else int(period)
        vals = np.empty((len(ks), 2, self.period), dtype=np.uint64)
        for i, k in enumerate(ks):
            d = np.asarray(diags[k], dtype=np.uint64)
            assert d.shape in ((self.period,), (2, self.period)), "a diagonal is [period] or [2][period]"
            vals[i] = d
        self._index, self._values = [int(k) for k in ks], vals
        info = bfv_lt_plan(ctx.n, self.period, self._index, ratio)
        self.n1, self.rotations, self.galois_elements = info["n1"], info["rotations"], info["galois_elements"]
        self.babies, self.giants, self.moddowns = info["babies"], info["giants"], info["moddowns"]
        self.diagonals = sorted(k % self.period for k in self._index)

    def _handle(self):
        if self.h is None:
            idx = (ctypes.c_int * len(self._index))(*self._index)
            self._adopt(lambda h: lib().lsa_bfv_lt_create(self.ctx.h, self.level, self.period, len(self._index), idx,
                                                          self._values.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), float(self.ratio),
                                                          self.ctx.stream, h))
            rows = ctypes.c_int()
            check(lib().lsa_bfv_lt_info(self.h, None, None, None, None, None, None, ctypes.byref(rows), None, None))
            self.rows = rows.value
        return self.h

    def info(self):
        """the device plan's own counts (lsa_bfv_lt_info) and lists"""
        h = self._handle()
        v = [ctypes.c_int() for _ in range(9)]
        check(lib().lsa_bfv_lt_info(h, *[ctypes.byref(x) for x in v]))
        names = ("level", "period", "n_diag", "n1", "n_baby", "n_giant", "rows", "n_galois", "n_moddown")
        out = {k: x.value for k, x in zip(names, v)}
        out["diagonals"] = _fetch(ctypes.c_int, out["n_diag"], lambda a, n: lib().lsa_bfv_lt_diagonals(h, a, n))
        out["galois_elements"] = _fetch(ctypes.c_uint64, out["n_galois"], lambda a, n: lib().lsa_bfv_lt_galois_elements(h, a, n))
        return out

    def oracle_plains(self):
        """{k (reduced mod period): extended plaintext [rows][N]}: what tests/bfv_lt_model.py linear_transform takes as `plains`"""
        h = self._handle()
        out = {}
        for i, k in enumerate(self.diagonals):
            pt = np.empty((self.rows, self.ctx.n), dtype=np.uint64)
            check(lib().lsa_bfv_lt_plaintext(h, i, pt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), pt.size))
            out[k] = pt
        return out

    def run(self, in_buf, batch, glk, out=None, sin=None, sout=None):
        """in_buf: device [batch][2][level+1][N], coefficient domain; glk: {galois element: key handle}; returns the device
        output, the same shape (sin / sout: batch strides in words, default compact)"""
        w = 2 * (self.level + 1) * self.ctx.n
        sin, sout = (w if sin is None else sin), (w if sout is None else sout)
        h = self._handle()
        if out is None:
            out = self.ctx.alloc(max(batch, 1) * max(sout, w))
        check(lib().lsa_bfv_linear_transform(self.ctx.h, h, in_buf.ptr, out.ptr, batch, sin, sout, *_key_arrays(glk), self.ctx.stream))
        return out


def plan_slot_sum(n, step, count, radix=0):
    """{steps, keyswitches, moddowns, rotations} of the slot sum sum_{i<count} rot(ct, i*step) at ring degree n -- host only
    (include/lattisense_amd.h: lsa_slot_sum_plan).  radix: 2, 4 or 0 = the default; rotations ascending, reduced mod n/2."""
    ns, nk, nm, cnt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    args = (int(n), int(step), int(count), int(radix), ctypes.byref(ns), ctypes.byref(nk), ctypes.byref(nm))
    check(lib().lsa_slot_sum_plan(*args, None, 0, ctypes.byref(cnt)))
    rot = _fetch(ctypes.c_int, cnt.value, lambda a, n: lib().lsa_slot_sum_plan(*args, a, n, None))
    return {"steps": ns.value, "keyswitches": nk.value, "moddowns": nm.value, "rotations": rot}


class SlotSumPlan(_Plan):
    """out = sum_{i<count} rot(ct, i*step) on ciphertexts at `level` (include/lattisense_amd.h: lsa_slot_sum_*); Replicate is
    step = -batch_size.  Planning needs no GPU (`.rotations`, `.galois_elements`, the counts); the device plan is made by the
    first run."""
    _destroy = "lsa_slot_sum_destroy"

    def __init__(self, ctx, level, step, count, radix=0):
        self.ctx, self.level, self.step, self.count = ctx, int(level), int(step), int(count)
        self.h = None
        self.multi_mac = False   # True: steps with several keys in one k_ks_mac_multi launch (A/B; the same words)
        n = ctx.n
        info = plan_slot_sum(n, step, count, radix)
        self.steps, self.keyswitches, self.moddowns, self.rotations = info["steps"], info["keyswitches"], info["moddowns"], info["rotations"]
        self.radix = int(radix)
        self.galois_elements = sorted(pow(5, r, 2 * n) for r in self.rotations)

    def _handle(self):
        if self.h is None:
            # (a context without a device has no handle: the library refuses, there is no CPU path)
            self._adopt(lambda h: lib().lsa_slot_sum_create(self.ctx.h, self.level, self.step, self.count, self.radix, h))
            rx, ng = ctypes.c_int(), ctypes.c_int()
            check(lib().lsa_slot_sum_info(self.h, None, None, ctypes.byref(rx), None, None, None, ctypes.byref(ng)))
            assert _fetch(ctypes.c_uint64, ng.value, lambda a, n: lib().lsa_slot_sum_galois_elements(self.h, a, n)) == self.galois_elements
            self.radix = rx.value
        return self.h

    def run(self, in_buf, batch, glk, out=None):
        """in_buf: device [batch][2][level+1][N]; glk: {galois element: key handle}; returns device [batch][2][level+1][N]
        (out may be in_buf)"""
        h = self._handle()
        n = self.ctx.n
        words = 2 * (self.level + 1) * n
        if out is None:
            out = self.ctx.alloc(max(batch, 1) * words)
        check(lib().lsa_slot_sum_set_multi_mac(h, int(bool(self.multi_mac))))
        check(lib().lsa_ckks_slot_sum(self.ctx.h, h, in_buf.ptr, out.ptr, batch, words, words, *_key_arrays(glk), self.ctx.stream))
        return out


def bfv_slot_sum_plan(n, step, count, radix=0, rows=0):
    """{steps, keyswitches, moddowns, galois_elements} of the BFV slot sum sum_{i<count} rot_cols(y, i*step), y = ct + rot_rows(ct)
    if rows -- host only (include/lattisense_amd.h: lsa_bfv_slot_sum_plan).  radix: 2, 4 or 0 = the default; elements ascending."""
    ns, nk, nm, cnt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    args = (int(n), int(step), int(count), int(radix), int(bool(rows)), ctypes.byref(ns), ctypes.byref(nk), ctypes.byref(nm))
    check(lib().lsa_bfv_slot_sum_plan(*args, None, 0, ctypes.byref(cnt)))
    g = _fetch(ctypes.c_uint64, cnt.value, lambda a, n: lib().lsa_bfv_slot_sum_plan(*args, a, n, None))
    return {"steps": ns.value, "keyswitches": nk.value, "moddowns": nm.value, "galois_elements": g}


class BfvSlotSumPlan(_Plan):
    """out = sum_{i<count} rot_cols(y, i*step), y = ct + rot_rows(ct) if rows, on coefficient-domain BFV ciphertexts at `level`
    (include/lattisense_amd.h: lsa_bfv_slot_sum_*).  Planning needs no GPU (`.galois_elements`, the counts); the device plan is
    made by the first run.  gather: None = the library's default, else the tail to run (False: the plain form)."""
    _destroy = "lsa_bfv_slot_sum_destroy"

    def __init__(self, ctx, level, step, count, radix=0, rows=0):
        self.ctx, self.level, self.step, self.count, self.rows = ctx, int(level), int(step), int(count), int(bool(rows))
        self.h = None
        self.gather = None
        info = bfv_slot_sum_plan(ctx.n, step, count, radix, rows)
        self.steps, self.keyswitches, self.moddowns = info["steps"], info["keyswitches"], info["moddowns"]
        self.galois_elements = info["galois_elements"]
        self.radix = int(radix)

    def _handle(self):
        if self.h is None:
            # (a context without a device has no handle: the library refuses, there is no CPU path)
            self._adopt(lambda h: lib().lsa_bfv_slot_sum_create(self.ctx.h, self.level, self.step, self.count, self.radix, self.rows, h))
            rx, ng = ctypes.c_int(), ctypes.c_int()
            check(lib().lsa_bfv_slot_sum_info(self.h, None, None, ctypes.byref(rx), None, None, None, None, ctypes.byref(ng), None))
            assert _fetch(ctypes.c_uint64, ng.value, lambda a, n: lib().lsa_bfv_slot_sum_galois_elements(self.h, a, n)) == self.galois_elements
            self.radix = rx.value
        return self.h

    def gather_in_force(self):
        ga = ctypes.c_int()
        check(lib().lsa_bfv_slot_sum_info(self._handle(), None, None, None, None, None, None, None, None, ctypes.byref(ga)))
        return bool(ga.value)

    def run(self, in_buf, batch, glk, out=None):
        """in_buf: device [batch][2][level+1][N], coefficient domain; glk: {galois element: key handle}; returns device
        [batch][2][level+1][N] (out may be in_buf)"""
        h = self._handle()
        words = 2 * (self.level + 1) * self.ctx.n
        if self.gather is not None:
            check(lib().lsa_bfv_slot_sum_set_gather(h, int(bool(self.gather))))
        if out is None:
            out = self.ctx.alloc(max(batch, 1) * words)
        check(lib().lsa_bfv_slot_sum(self.ctx.h, h, in_buf.ptr, out.ptr, batch, words, words, *_key_arrays(glk), self.ctx.stream))
        return out


def bfv_expand_plan(n, count):
    """{levels, keyswitches, galois_elements} of the BFV oblivious expansion of one ciphertext into `count` -- host only
    (include/lattisense_amd.h: lsa_bfv_expand_plan); elements ascending."""
    nl, nk, cnt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    args = (int(n), int(count), ctypes.byref(nl), ctypes.byref(nk))
    check(lib().lsa_bfv_expand_plan(*args, None, 0, ctypes.byref(cnt)))
    g = _fetch(ctypes.c_uint64, cnt.value, lambda a, m: lib().lsa_bfv_expand_plan(*args, a, m, None))
    return {"levels": nl.value, "keyswitches": nk.value, "galois_elements": g}


class BfvExpandPlan(_Plan):
    """One coefficient-domain BFV ciphertext at `level` expanded into `count`: output i holds 2^levels * m_i in its low
    coefficients (include/lattisense_amd.h: lsa_bfv_expand_*).  Planning needs no GPU (`.galois_elements`, `.levels`,
    `.keyswitches`); the device plan is made by the first run.  gather: None = the library's default, else the tail to run."""
    _destroy = "lsa_bfv_expand_destroy"

    def __init__(self, ctx, level, count):
        self.ctx, self.level, self.count = ctx, int(level), int(count)
        self.h = None
        self.gather = None
        info = bfv_expand_plan(ctx.n, count)
        self.levels, self.keyswitches, self.galois_elements = info["levels"], info["keyswitches"], info["galois_elements"]

    def _handle(self):
        if self.h is None:
            self._adopt(lambda h: lib().lsa_bfv_expand_create(self.ctx.h, self.level, self.count, h))
            ng = ctypes.c_int()
            check(lib().lsa_bfv_expand_info(self.h, None, None, None, None, ctypes.byref(ng), None))
            assert _fetch(ctypes.c_uint64, ng.value, lambda a, n: lib().lsa_bfv_expand_galois_elements(self.h, a, n)) == self.galois_elements
        return self.h

    def gather_in_force(self):
        ga = ctypes.c_int()
        check(lib().lsa_bfv_expand_info(self._handle(), None, None, None, None, None, ctypes.byref(ga)))
        return bool(ga.value)

    def set_gather(self, enable):
        check(lib().lsa_bfv_expand_set_gather(self._handle(), int(bool(enable))))
        self.gather = bool(enable)

    def run(self, in_buf, batch, glk, out=None, s_index=None):
        """in_buf: device [batch][2][level+1][N], coefficient domain; glk: {galois element: key handle}; returns the device
        outputs, output i of item b at i * s_index + b * words (s_index: None = dense, batch * words).  out may start with
        in_buf's words (in is output 0)."""
        h = self._handle()
        words = 2 * (self.level + 1) * self.ctx.n
        if s_index is None:
            s_index = max(batch, 1) * words
        if self.gather is not None:
            check(lib().lsa_bfv_expand_set_gather(h, int(bool(self.gather))))
        if out is None:
            out = self.ctx.alloc((self.count - 1) * s_index + max(batch, 1) * words)
        check(lib().lsa_bfv_expand(self.ctx.h, h, in_buf.ptr, words, out.ptr, words, int(s_index), batch, *_key_arrays(glk),
                                   self.ctx.stream))
        return out


def bfv_pack_plan(n, count, trace=False):
    """{levels, trace_levels, keyswitches, galois_elements} of the BFV coefficient packing of `count` ciphertexts into one -- host
    only (include/lattisense_amd.h: lsa_bfv_pack_plan); elements ascending."""
    nl, nt, nk, cnt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    args = (int(n), int(count), int(bool(trace)), ctypes.byref(nl), ctypes.byref(nt), ctypes.byref(nk))
    check(lib().lsa_bfv_pack_plan(*args, None, 0, ctypes.byref(cnt)))
    g = _fetch(ctypes.c_uint64, cnt.value, lambda a, m: lib().lsa_bfv_pack_plan(*args, a, m, None))
    return {"levels": nl.value, "trace_levels": nt.value, "keyswitches": nk.value, "galois_elements": g}


class BfvPackPlan(_Plan):
    """`count` coefficient-domain BFV ciphertexts at `level` packed into one: coefficient i * N / 2^levels of the result holds
    F * (coefficient 0 of input i), F = 2^levels, or N with the trace, which also clears every other coefficient
    (include/lattisense_amd.h: lsa_bfv_pack_*).  Planning needs no GPU (`.galois_elements`, `.levels`, `.trace_levels`,
    `.keyswitches`); the device plan is made by the first run.  gather: None = the library's default, else the tail to run."""
    _destroy = "lsa_bfv_pack_destroy"

    def __init__(self, ctx, level, count, trace=False):
        self.ctx, self.level, self.count, self.trace = ctx, int(level), int(count), bool(trace)
        self.h = None
        self.gather = None
        info = bfv_pack_plan(ctx.n, count, trace)
        self.levels, self.trace_levels = info["levels"], info["trace_levels"]
        self.keyswitches, self.galois_elements = info["keyswitches"], info["galois_elements"]

    def _handle(self):
        if self.h is None:
            self._adopt(lambda h: lib().lsa_bfv_pack_create(self.ctx.h, self.level, self.count, int(self.trace), h))
            ng = ctypes.c_int()
            check(lib().lsa_bfv_pack_info(self.h, None, None, None, None, None, None, ctypes.byref(ng), None))
            assert _fetch(ctypes.c_uint64, ng.value, lambda a, n: lib().lsa_bfv_pack_galois_elements(self.h, a, n)) == self.galois_elements
        return self.h

    def gather_in_force(self):
        ga = ctypes.c_int()
        check(lib().lsa_bfv_pack_info(self._handle(), None, None, None, None, None, None, None, ctypes.byref(ga)))
        return bool(ga.value)

    def set_gather(self, enable):
        check(lib().lsa_bfv_pack_set_gather(self._handle(), int(bool(enable))))
        self.gather = bool(enable)

    def run(self, in_buf, batch, glk, out=None, s_index=None):
        """in_buf: the device inputs, input i of item b at i * s_index + b * words, each [2][level+1][N] in the coefficient domain
        (s_index: None = dense, batch * words); they are consumed.  glk: {galois element: key handle}.  Returns the device result
        [batch][2][level+1][N]; out may be in_buf (the result takes the place of input 0)."""
        h = self._handle()
        words = 2 * (self.level + 1) * self.ctx.n
        if s_index is None:
            s_index = max(batch, 1) * words
        if self.gather is not None:
            check(lib().lsa_bfv_pack_set_gather(h, int(bool(self.gather))))
        if out is None:
            out = self.ctx.alloc(max(batch, 1) * words)
        check(lib().lsa_bfv_pack(self.ctx.h, h, in_buf.ptr, words, int(s_index), out.ptr, words, batch, *_key_arrays(glk), self.ctx.stream))
        return out


def bfv_select_plan(count):
    """{levels, products} of the select of one of `count` ciphertexts by an encrypted index -- host only
    (include/lattisense_amd.h: lsa_bfv_select_plan)"""
    nl, npr = ctypes.c_int(), ctypes.c_int()
    check(lib().lsa_bfv_select_plan(int(count), ctypes.byref(nl), ctypes.byref(npr)))
    return {"levels": nl.value, "products": npr.value}


def bfv_matvec_plan(n_ring, level_limbs, rows, cols, batch, workspace_bytes=8 << 30):
    """{row_block, col_block, launches, workspace_rows} of a plaintext matrix x ciphertext vector product -- host only
    (include/lattisense_amd.h: lsa_bfv_matvec_plan)"""
    rb, cb, nl, wr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    check(lib().lsa_bfv_matvec_plan(int(n_ring), int(level_limbs), int(rows), int(cols), int(batch), int(workspace_bytes), ctypes.byref(rb),
                                    ctypes.byref(cb), ctypes.byref(nl), ctypes.byref(wr)))
    return {"row_block": rb.value, "col_block": cb.value, "launches": nl.value, "workspace_rows": wr.value}


class BfvSelectPlan(_Plan):
    """One of `count` coefficient-domain BFV ciphertexts at `level` selected by an encrypted index: a CMux tree whose selectors are
    RGSW ciphertexts of the index bits (include/lattisense_amd.h: lsa_bfv_select_*).  Planning needs no GPU (`.levels`, `.products`);
    the device plan is made by the first run."""
    _destroy = "lsa_bfv_select_destroy"

    def __init__(self, ctx, level, count):
        self.ctx, self.level, self.count = ctx, int(level), int(count)
        self.h = None
        info = bfv_select_plan(count)
        self.levels, self.products = info["levels"], info["products"]

    def _handle(self):
        if self.h is None:
            self._adopt(lambda h: lib().lsa_bfv_select_create(self.ctx.h, self.level, self.count, h))
            nl, npr = ctypes.c_int(), ctypes.c_int()
            check(lib().lsa_bfv_select_info(self.h, None, None, ctypes.byref(nl), ctypes.byref(npr)))
            assert (nl.value, npr.value) == (self.levels, self.products)
        return self.h

    def run(self, in_buf, batch, selectors, out=None, s_index=None):
        """in_buf: the device inputs, input i of item b at i * s_index + b * words, each [2][level+1][N] in the coefficient domain
        (s_index: None = dense, batch * words); the inputs below max(1, 2^(levels-1)) are consumed.  selectors: [(r0, r1)] key handles,
        entry j the RGSW ciphertext of index bit j.  Returns the device result [batch][2][level+1][N]; out may be in_buf (the result
        takes the place of input 0)."""
        h = self._handle()
        words = 2 * (self.level + 1) * self.ctx.n
        if s_index is None:
            s_index = max(batch, 1) * words
        if out is None:
            out = self.ctx.alloc(max(batch, 1) * words)
        n = len(selectors)
        r0s = (ctypes.c_void_p * max(n, 1))(*[s[0].value if hasattr(s[0], "value") else s[0] for s in selectors])
        r1s = (ctypes.c_void_p * max(n, 1))(*[s[1].value if hasattr(s[1], "value") else s[1] for s in selectors])
        check(lib().lsa_bfv_select(self.ctx.h, h, in_buf.ptr, words, int(s_index), out.ptr, words, batch, n, r0s, r1s, self.ctx.stream))
        return out


BASES = {"chebyshev": 0, "monomial": 1}


def plan_polynomial(coeffs, level, basis="chebyshev", log_baby=0, interval=False):
    """{depth, log_baby, mults, leaves, leaf_launches} of the evaluation plan a coefficient list gets -- host only"""
    cf = (ctypes.c_double * len(coeffs))(*[float(x) for x in coeffs])
    d, b, mu, lv, la = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(lib().lsa_poly_plan(BASES[basis], len(coeffs), cf, int(log_baby), int(level), int(bool(interval)), ctypes.byref(d),
                              ctypes.byref(b), ctypes.byref(mu), ctypes.byref(lv), ctypes.byref(la)))
    return {"depth": d.value, "log_baby": b.value, "mults": mu.value, "leaves": lv.value, "leaf_launches": la.value}


class PolynomialPlan(_Plan):
    """sum_k coeffs[k] T_k(u) (basis "chebyshev") or sum_k coeffs[k] u^k ("monomial") on ciphertexts at `level` and scale
    `scale_in`, u = x mapped from `interval` to [-1, 1] (include/lattisense_amd.h: lsa_poly_*)."""
    _destroy = "lsa_poly_destroy"

    def __init__(self, ctx, coeffs, level, scale_in, basis="chebyshev", interval=(-1, 1), scale_out=None, log_baby=0):
        self.ctx = ctx
        self.h = None
        cf = (ctypes.c_double * len(coeffs))(*[float(x) for x in coeffs])
        self._adopt(lambda h: lib().lsa_poly_create(ctx.h, BASES[basis], len(coeffs), cf, float(interval[0]), float(interval[1]), int(level),
                                                    float(scale_in), float(scale_out or 0.0), int(log_baby), h))
        li, lo, d, b, mu, lv, la, nc = (ctypes.c_int() for _ in range(8))
        sc = ctypes.c_double()
        check(lib().lsa_poly_info(self.h, ctypes.byref(li), ctypes.byref(lo), ctypes.byref(sc), ctypes.byref(d), ctypes.byref(b),
                                  ctypes.byref(mu), ctypes.byref(lv), ctypes.byref(la), ctypes.byref(nc)))
        self.level_in, self.level_out, self.scale_out, self.depth, self.log_baby = li.value, lo.value, sc.value, d.value, b.value
        self.mults, self.leaves, self.leaf_launches, self.n_constants = mu.value, lv.value, la.value, nc.value
        self.basis, self.scale_in = basis, float(scale_in)

    def constants(self):
        """every integer constant of the plan, in the planner's order (what tests/poly_model.py consumes)"""
        return _fetch(ctypes.c_longlong, self.n_constants, lambda a, n: lib().lsa_poly_constants(self.h, a, n))

    def run(self, in_buf, batch, rlk, out=None):
        """in_buf: device [batch][2][level_in+1][N]; rlk: relinearisation key handle; returns device [batch][2][level_out+1][N]"""
        n = self.ctx.n
        if out is None:
            out = self.ctx.alloc(max(batch, 1) * 2 * (self.level_out + 1) * n)
        check(lib().lsa_ckks_poly_eval(self.ctx.h, self.h, in_buf.ptr, out.ptr, batch, 2 * (self.level_in + 1) * n,
                                       2 * (self.level_out + 1) * n, rlk, self.ctx.stream))
        return out


_BFV_POLY_COUNTS = ("log_baby", "depth", "n_mult", "n_leaves", "n_leaf_launches", "n_pairs")


def _u64_array(values):
    return (ctypes.c_uint64 * max(len(values), 1))(*[int(x) for x in values])


def bfv_poly_plan(t, coeffs, log_baby=0):
    """{log_baby, depth, n_mult, n_leaves, n_leaf_launches, n_pairs} of the flat baby-step / giant-step plan that
    sum_k coeffs[k] x^k mod t gets -- host only (include/lattisense_amd.h: lsa_bfv_poly_plan); log_baby 0 = the planner's choice"""
    v = [ctypes.c_int() for _ in _BFV_POLY_COUNTS]
    check(lib().lsa_bfv_poly_plan(int(t), len(coeffs), _u64_array(coeffs), int(log_baby), *[ctypes.byref(x) for x in v]))
    return {k: x.value for k, x in zip(_BFV_POLY_COUNTS, v)}


class BfvPolynomialPlan(_Plan):
    """sum_k coeffs[k] x^k mod t, slot-wise on coefficient-domain BFV ciphertexts at `level`, coeffs in [0, t)
    (include/lattisense_amd.h: lsa_bfv_poly_*).  The only key is the relinearisation key."""
    _destroy = "lsa_bfv_poly_destroy"

    def __init__(self, ctx, coeffs, level, log_baby=0):
        self.ctx, self.level = ctx, int(level)
        self.h = None
        self._adopt(lambda h: lib().lsa_bfv_poly_create(ctx.h, self.level, len(coeffs), _u64_array(coeffs), int(log_baby), ctx.stream, h))
        for k, x in self.info().items():
            setattr(self, k, x)

    def info(self):
        """the device plan's own counts (lsa_bfv_poly_info)"""
        v = [ctypes.c_int() for _ in range(8)]
        check(lib().lsa_bfv_poly_info(self.h, *[ctypes.byref(x) for x in v]))
        return {k: x.value for k, x in zip(("level", "n_coef") + _BFV_POLY_COUNTS, v)}

    def run(self, in_buf, batch, rlk, out=None):
        """in_buf: device [batch][2][level+1][N]; rlk: relinearisation key handle; returns device [batch][2][level+1][N]
        (out overlaps no word of in_buf)"""
        w = 2 * (self.level + 1) * self.ctx.n
        if out is None:
            out = self.ctx.alloc(max(batch, 1) * w)
        check(lib().lsa_bfv_poly_eval(self.ctx.h, self.h, in_buf.ptr, out.ptr, batch, w, w, rlk, self.ctx.stream))
        return out
