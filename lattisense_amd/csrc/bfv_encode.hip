// bfv_encode.hip — the BFV slot encoder (bfv_encode.h): k_bfv_encode_t, the inverse negacyclic transform mod t of a whole
// plaintext in LDS, and the host side that lifts its coefficient row into the three plaintext forms.
#include "bfv_encode.h"

namespace lsa {

// ------------------------------------------------------------------------------------------------ kernel
// Gentleman-Sande, bit-reversed in, natural out -- the stage order of oracle/ls_oracle.c ora_intt, so the butterfly distance
// grows 1, 2, 4, ... N/2.  LDS addressing (MI355X: 32 banks of 4 bytes for 32-bit accesses, served per 32-lane half; 64 banks
// for the 16-byte reads, served per 16 lanes):
//   image    word w lives at w + 4 (w >> 5): four words of padding after every 32
//   scatter  slot i goes to index[i], a bit-reversed position: conflicts as they fall, once per word
//   pass 1   distances 1..16 never leave a 32-word chunk: one thread takes a chunk into registers (eight 16-byte reads; chunk
//            bases are 36 words apart, so 16 lanes start on 16 different 4-bank slots: no conflict, where the unpadded image would
//            put every other lane on the same slot), runs the five stages there -- distances 1..8 on each 16-word half, then 16
//            across the halves -- and writes it back.  N/32 threads work, all 1024 at N = 2^15
//   pass 2   distances 32..N/2, one stage per barrier, N/2 butterflies over the block: a 32-lane half reads 32 consecutive words
//            of one chunk (U) and of another (V): no conflict; its twiddle is one word, broadcast
//   store    pairs of words, N^-1 applied, 16 bytes per lane to global memory
// Words stay below t < 2^32; a product is x * w - floor(x * w' / 2^32) * t with w' = floor(w 2^32 / t) (Shoup), in [0, 2t).
struct BfvEncodeArgs {
    const u64* values;   // [batch][N], words < t
    u64* out;            // [batch] rows of N words
    long long so;
    const u32* index;    // [N]
    const uint2* tw;     // [N] {w, w'}, w = psi^-brv(x)
    u32 t, ninv, ninv_s;
    int logn;
};

__device__ __forceinline__ u32 enc_pad(u32 w) { return w + ((w >> 5) << 2); }
__device__ __forceinline__ u32 enc_add(u32 a, u32 b, u32 t) {
    const u64 s = (u64)a + b;
    return (u32)(s >= t ? s - t : s);
}
__device__ __forceinline__ u32 enc_sub(u32 a, u32 b, u32 t) { return a >= b ? a - b : a + (t - b); }
__device__ __forceinline__ u32 enc_mul(u32 x, uint2 w, u32 t) {
    const u64 r = (u64)x * w.x - (u64)__umulhi(x, w.y) * t;
    return (u32)(r >= t ? r - t : r);
}

__global__ void __launch_bounds__(LSA_BFV_ENC_THREADS) k_bfv_encode_t(BfvEncodeArgs g) {
    extern __shared__ __align__(16) u32 enc_img[];
    const u32 n = 1u << g.logn, tid = threadIdx.x, t = g.t;
    const u64* v = g.values + ((long long)blockIdx.x << g.logn);
    for (u32 i = tid; i < n; i += LSA_BFV_ENC_THREADS) enc_img[enc_pad(g.index[i])] = (u32)v[i];
    __syncthreads();
    if (tid < (n >> 5)) {   // (N <= 2^15: at most one chunk per thread)
        const u32 chunk = tid;
        uint4* p = reinterpret_cast<uint4*>(enc_img + chunk * 36);
        u32 a[32];
        // stages 1..8 on each 16-word half, then distance 16 across the halves.  (The twiddle loads stay with their stage: hoisted
        // together, the 31 of them spill the 32 words.)
#pragma unroll
        for (int half = 0; half < 2; half++) {
#pragma unroll
            for (int i = 4 * half; i < 4 * half + 4; i++) {
                const uint4 q = p[i];
                a[4 * i] = q.x;
                a[4 * i + 1] = q.y;
                a[4 * i + 2] = q.z;
                a[4 * i + 3] = q.w;
            }
#pragma unroll
            for (int s = 0; s < 4; s++) {
                __asm__ volatile("" ::: "memory");
                const uint2* tw = g.tw + (n >> (s + 1)) + (2 * chunk + half) * (8u >> s);   // this half's 8 >> s groups of the stage
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int grp = k >> s, j = 16 * half + ((grp << (s + 1)) | (k & ((1 << s) - 1)));
                    const u32 x = a[j], y = a[j + (1 << s)];
                    a[j] = enc_add(x, y, t);
                    a[j + (1 << s)] = enc_mul(enc_sub(x, y, t), tw[grp], t);
                }
            }
        }
        __asm__ volatile("" ::: "memory");
        {
            const uint2 w = g.tw[(n >> 5) + chunk];
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const u32 x = a[k], y = a[k + 16];
                a[k] = enc_add(x, y, t);
                a[k + 16] = enc_mul(enc_sub(x, y, t), w, t);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; i++) p[i] = make_uint4(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]);
    }
    __syncthreads();
    for (int s = 5; s < g.logn; s++) {
        const uint2* tw = g.tw + (n >> (s + 1));
        for (u32 b = tid; b < (n >> 1); b += LSA_BFV_ENC_THREADS) {
            const u32 grp = b >> s, j = (grp << (s + 1)) | (b & ((1u << s) - 1));
            const u32 pj = enc_pad(j), pk = enc_pad(j + (1u << s));
            const u32 x = enc_img[pj], y = enc_img[pk];
            enc_img[pj] = enc_add(x, y, t);
            enc_img[pk] = enc_mul(enc_sub(x, y, t), tw[grp], t);
        }
        __syncthreads();
    }
    u64* o = g.out + (long long)blockIdx.x * g.so;
    const uint2 ni = make_uint2(g.ninv, g.ninv_s);
    for (u32 x = 2 * tid; x < n; x += 2 * LSA_BFV_ENC_THREADS) {
        const uint2 w = *reinterpret_cast<const uint2*>(enc_img + enc_pad(x));   // (x even: both words in one chunk, 8-byte aligned)
        ulonglong2 r;
        r.x = enc_mul(w.x, ni, t);
        r.y = enc_mul(w.y, ni, t);
        *reinterpret_cast<ulonglong2*>(o + x) = r;
    }
}

static void launch_bfv_encode_t(Context& c, const BfvEncodeTables& T, const u64* d_values, u64* out, long long so, int batch,
                                hipStream_t s) {
    if (batch <= 0) return;
    LSA_REQUIRE(c.logn >= LSA_BFV_ENC_MIN_LOGN && c.logn <= LSA_BFV_ENC_MAX_LOGN, "BFV encode kernel: ring degree outside 2^6..2^15");
    LSA_REQUIRE(T.n == c.n && so >= (long long)c.n && (so & 1) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0,
                "BFV encode kernel: short, odd or misaligned output");
    std::vector<u64> idx((size_t)c.n / 2), tw((size_t)c.n);
    for (size_t i = 0; i < idx.size(); i++) idx[i] = (u64)T.index[2 * i] | ((u64)T.index[2 * i + 1] << 32);
    for (size_t i = 0; i < tw.size(); i++) tw[i] = (u64)T.psiinv[2 * i] | ((u64)T.psiinv[2 * i + 1] << 32);
    BfvEncodeArgs g{};
    g.values = d_values;
    g.out = out;
    g.so = so;
    g.index = reinterpret_cast<const u32*>(c.raw_vec("bfv_encode_index", idx));
    g.tw = reinterpret_cast<const uint2*>(c.raw_vec("bfv_encode_psiinv", tw));
    g.t = (u32)T.t;
    g.ninv = T.ninv;
    g.ninv_s = T.ninv_shoup;
    g.logn = c.logn;
    const size_t lds_bytes = ((size_t)c.n + (size_t)c.n / 8) * sizeof(u32);
    raise_dynamic_lds<&k_bfv_encode_t>(lds_bytes, 160 * 1024);
    ProfScope ps(c, PROF_ELEMWISE, 16.0 * c.n * batch, s);
    hipLaunchKernelGGL(k_bfv_encode_t, dim3((unsigned)batch), dim3(LSA_BFV_ENC_THREADS), lds_bytes, s, g);
    LSA_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ host side
const BfvEncodeTables& bfv_encode_tables(Context& c, const char* who) {
    std::lock_guard<std::mutex> lk(c.mu);
    if (!c.bfv_enc) {
        auto t = std::make_shared<BfvEncodeTables>();
        try {
            t->build(c.n, c.t);
        } catch (const std::invalid_argument& e) {
            throw Error(LSA_ERR_ARG, std::string(who) + ": " + e.what());
        }
        c.bfv_enc = t;
    }
    return *c.bfv_enc;
}

void bfv_lift_rows(Context& c, int level, int form, const u64* coef, long long scoef, u64* out, long long sout, int batch,
                   hipStream_t s) {
    if (batch <= 0) return;
    const long long N = c.n;
    const int rows = bfv_pt_rows(c, level, form);
    LSA_REQUIRE((form == BFV_PT_MUL || form == BFV_PT_EXT) && rows <= LSA_MAX_PERIOD, "bfv_lift_rows: internal: form or row count");
    RowMap rm;
    rm.period = rows;
    for (int j = 0; j < rows; j++) rm.mod_of[j] = (unsigned char)c.qp_mod(level + 1, j);
    NttFusion lf;   // every row of a plaintext reads the one coefficient row (x < t < q: the lift is the identity)
    lf.pro = 4;
    lf.limbs = rows;
    lf.last = coef;
    lf.last_stride = scoef;
    lf.last_rpp = 1;
    lf.ql_mod = 0;
    launch_ntt(c, out, out, batch, sout, sout, rows, rm, false, s, &lf);
    if (form == BFV_PT_MUL) {
        if (sout == (long long)rows * N) {
            launch_to_mont(c, out, batch * rows, rm, s);
        } else {
            for (int b = 0; b < batch; b++) launch_to_mont(c, out + (size_t)b * sout, rows, rm, s);
        }
    }
}

void bfv_encode_rows(Context& c, int level, int form, const u64* values, u64* out, long long sout, int batch, hipStream_t s) {
    if (batch <= 0) return;
    const char* who = "lsa_bfv_encode";
    const BfvEncodeTables& T = bfv_encode_tables(c, who);
    const long long N = c.n;
    const int rows = bfv_pt_rows(c, level, form);
    LSA_REQUIRE(rows <= LSA_MAX_PERIOD, std::string(who) + ": more rows than a transform launch takes");
    for (int j = 0; j < rows; j++)   // the lift: a coefficient in [0, t) is its own residue
        LSA_REQUIRE(form == BFV_PT_RINGT || c.t < c.T.mod[c.qp_mod(level + 1, j)], std::string(who) + ": t must be below every modulus of the chain");
    const bool on_device = c.logn <= LSA_BFV_ENC_MAX_LOGN && c.logn >= LSA_BFV_ENC_MIN_LOGN;
    const size_t words = (size_t)batch * N;
    u64* stage = c.workspace(2 * words, s);   // the uploaded words | the coefficient rows (forms 1 and 2, the host transform)
    u64* coef = stage + words;
    std::vector<u64> host;
    if (on_device) {
        LSA_HIP(hipMemcpyAsync(stage, values, words * sizeof(u64), hipMemcpyHostToDevice, s));
        if (form == BFV_PT_RINGT) launch_bfv_encode_t(c, T, stage, out, sout, batch, s);
        else launch_bfv_encode_t(c, T, stage, coef, N, batch, s);
    } else {
        host.resize(words);
        for (int b = 0; b < batch; b++) T.encode(values + (size_t)b * N, host.data() + (size_t)b * N);
        LSA_HIP(hipMemcpyAsync(coef, host.data(), words * sizeof(u64), hipMemcpyHostToDevice, s));
        if (form == BFV_PT_RINGT) {
            const int row0 = 0;
            launch_copy_rows(c, coef, N, out, sout, 1, &row0, batch, s);
        }
    }
    if (form != BFV_PT_RINGT) bfv_lift_rows(c, level, form, coef, N, out, sout, batch, s);
    LSA_HIP(hipStreamSynchronize(s));   // `values` and `host` have been read; the plaintexts are complete
}

void bfv_encode(Context& c, int level, int form, const u64* values, u64* out, long long sout, int batch, hipStream_t s) {
    const std::string who = "lsa_bfv_encode";
    LSA_REQUIRE(c.algo == LSA_ALGO_BFV, who + ": context is not BFV");
    LSA_REQUIRE(level >= 0 && level < c.nq, who + ": level out of range (0.." + std::to_string(c.nq - 1) + ")");
    LSA_REQUIRE(form >= BFV_PT_RINGT && form <= BFV_PT_EXT, who + ": form must be 0 (ring-t), 1 (pt_mul) or 2 (extended)");
    if (batch <= 0) return;
    LSA_REQUIRE(values && out, who + ": null argument");
    const long long N = c.n;
    LSA_REQUIRE(sout >= (long long)bfv_pt_rows(c, level, form) * N, who + ": output stride below one plaintext");
    LSA_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0 && (sout & 1) == 0,
                who + ": out must be 16-byte aligned with an even batch stride");
    (void)bfv_encode_tables(c, who.c_str());   // refuses a t that has no slots
    for (size_t i = 0; i < (size_t)batch * N; i++)
        LSA_REQUIRE(values[i] < c.t, who + ": value " + std::to_string(values[i]) + " at word " + std::to_string(i) + " is not below t");
    bfv_encode_rows(c, level, form, values, out, sout, batch, s);
}

}  // namespace lsa
