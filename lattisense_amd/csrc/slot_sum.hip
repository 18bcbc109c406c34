// slot_sum.hip — the device kernels of the CKKS slot sum (ops.hip slot_sum_run; plan: slot_sum.h):
//   k_ks_mac_multi<KB, K>  the gadget inner product of ONE decomposition with K = 2..4 keys ("a MAC kernel that reads the
//                          decomposed digits once for all keys of a hoisted group"), each key's product leaving
//                          as that key's rotated extended ciphertext in that key's own buffer;
//   k_ext_sum              out (+)= sum of up to three extended ciphertexts: joins the per-key buffers.
// The per-point arithmetic is ks_mac_multi.h's, which the host compiles too (tests/cpp/test_ks_mac_multi.cpp).  k_ks_mac
// (kernels.hip) stays the single-key kernel: SlotSum::multi_mac = false runs it once per key, each launch adding to its
// destination, and that form measured faster at every bench shape, so it is the default.
#include "ks_mac_multi.h"
#include "lsa_internal.h"

namespace lsa {

namespace {

constexpr int TPB = 256;

__device__ __forceinline__ ulonglong2 ld2(const u64* p) { return *reinterpret_cast<const ulonglong2*>(p); }
__device__ __forceinline__ void st2(u64* p, u64 x, u64 y) {
    ulonglong2 v;
    v.x = x;
    v.y = y;
    *reinterpret_cast<ulonglong2*>(p) = v;
}

struct KsMacMultiArgs {
    const u64* cx;
    const u64* ext;
    const u64* key[LSA_KSM_MAX_KEYS];            // compact order [beta][2][kcomp][N], Montgomery form
    u64* out[LSA_KSM_MAX_KEYS];                  // [batch][2][T][N] each, batch stride sout
    const unsigned* scatter[LSA_KSM_MAX_KEYS];   // out[k][h][tl][scatter[k][x]] = value_k(x)
    int kcomp[LSA_KSM_MAX_KEYS], klvl[LSA_KSM_MAX_KEYS];
    long long scx, sext, sout, sbase;
    const u64* base;   // the ciphertext whose c0 enters times P on the Q rows of polynomial 0
    const u64* pm;     // [L] P mod q_j, Montgomery form
    const ModDev* mods;
    int logn, L, np, nq, beta, batch, bpt;
};

// grid: x = T * (N/2/TPB), y = groups of `bpt` batch items (the walk of k_ks_mac).  A thread owns target limb tl and the point
// pair (x, x+1): it loads each digit value once per batch item and multiplies it into the 2K sums of its K keys.
// KB > 0: beta <= KB digits, the next item's digit values fetched before the current one is multiplied (k_ks_mac's prefetch); the
// key words stay in registers where K * KB <= 8 (64 VGPRs) and are re-read per item otherwise -- K times fewer bytes of them
// than digit values of the batch group, and they stay in the caches across the group (resident up to K * KB = 16 was tried: the
// compiler parks 37 to 125 values in AGPRs and one wave per SIMD is left).  KB = 0: digits and keys streamed, folded every
// eighth digit.
template <int KB, int K>
__global__ __launch_bounds__(TPB) void k_ks_mac_multi(KsMacMultiArgs g) {
    constexpr bool in_regs = KB > 0;
    constexpr bool key_regs = in_regs && K * KB <= 8;
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int tl = blockIdx.x / chunks;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const int T = g.L + g.np;
    const int mi = tl < g.L ? tl : g.nq + (tl - g.L);
    const ModDev m = g.mods[mi];
    const long long N = 1LL << g.logn;
    const int own_d = tl < g.L ? tl / g.np : -1;   // the digit that contains this limb reads cx directly
    const u64* pk[K];                              // key k, digit 0, first half, this limb and point pair
    long long kstep[K];                            // words from one half to the next (two halves per digit)
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int kj = tl < g.L ? tl : g.klvl[k] + 1 + (tl - g.L);
        pk[k] = g.key[k] + kj * N + x;
        kstep[k] = (long long)g.kcomp[k] * N;
    }
    ulonglong2 k0[key_regs ? KB : 1][K], k1[key_regs ? KB : 1][K];
    if constexpr (key_regs) {
#pragma unroll
        for (int d = 0; d < KB; d++)
            if (d < g.beta) {
#pragma unroll
                for (int k = 0; k < K; k++) {
                    k0[d][k] = ld2(pk[k] + 2 * d * kstep[k]);
                    k1[d][k] = ld2(pk[k] + (2 * d + 1) * kstep[k]);
                }
            }
    }
    auto digit = [&](long long b, int d) {
        return d == own_d ? g.cx + b * g.scx + tl * N + x : g.ext + b * g.sext + ((long long)d * T + tl) * N + x;
    };
    const int b_begin = blockIdx.y * g.bpt;
    const int b_end = min(g.batch, b_begin + g.bpt);
    ulonglong2 en[in_regs ? KB : 1];
    auto fetch = [&](long long b) {
        if constexpr (in_regs) {
#pragma unroll
            for (int d = 0; d < KB; d++)
                if (d < g.beta) en[d] = ld2(digit(b, d));
        }
    };
    if (b_begin < b_end) fetch(b_begin);
    for (long long b = b_begin; b < b_end; b++) {
        KsmAcc<K> ax, ay;   // the sums of point x and of point x + 1
        ksm_init(ax);
        ksm_init(ay);
        auto term = [&](int d, const ulonglong2& e, const ulonglong2* w0, const ulonglong2* w1) {
            u64 x0[K], x1[K], y0[K], y1[K];
#pragma unroll
            for (int k = 0; k < K; k++) {
                x0[k] = w0[k].x;
                y0[k] = w0[k].y;
                x1[k] = w1[k].x;
                y1[k] = w1[k].y;
            }
            ksm_term(ax, d, e.x, x0, x1, m);
            ksm_term(ay, d, e.y, y0, y1, m);
        };
        if constexpr (in_regs) {
            ulonglong2 ec[KB];
#pragma unroll
            for (int d = 0; d < KB; d++) ec[d] = en[d];
            if (b + 1 < b_end) fetch(b + 1);
#pragma unroll
            for (int d = 0; d < KB; d++)
                if (d < g.beta) {
                    if constexpr (key_regs) {
                        term(d, ec[d], k0[d], k1[d]);
                    } else {
                        ulonglong2 w0[K], w1[K];
#pragma unroll
                        for (int k = 0; k < K; k++) {
                            w0[k] = ld2(pk[k] + 2 * d * kstep[k]);
                            w1[k] = ld2(pk[k] + (2 * d + 1) * kstep[k]);
                        }
                        term(d, ec[d], w0, w1);
                    }
                }
        } else {
            for (int d = 0; d < g.beta; d++) {
                const ulonglong2 e = ld2(digit(b, d));
                ulonglong2 w0[K], w1[K];
#pragma unroll
                for (int k = 0; k < K; k++) {
                    w0[k] = ld2(pk[k] + 2 * d * kstep[k]);
                    w1[k] = ld2(pk[k] + (2 * d + 1) * kstep[k]);
                }
                term(d, e, w0, w1);
            }
        }
        ksm_finish(ax, g.beta, m);
        ksm_finish(ay, g.beta, m);
        if (tl < g.L) {
            const ulonglong2 c0 = ld2(g.base + b * g.sbase + tl * N + x);
            const u64 pm = g.pm[tl];
            ksm_add_base(ax, c0.x, pm, m);
            ksm_add_base(ay, c0.y, pm, m);
        }
        // key k's own permutation into key k's own buffer: scatter[k] is a permutation of the row and the thread owns its two
        // points, so no word of any buffer is touched by two threads
#pragma unroll
        for (int k = 0; k < K; k++) {
            const uint2 sx = *reinterpret_cast<const uint2*>(g.scatter[k] + x);
            u64* po = g.out[k] + b * g.sout + tl * N;
            po[sx.x] = ax.r[2 * k];
            po[sx.y] = ay.r[2 * k];
            po[(long long)T * N + sx.x] = ax.r[2 * k + 1];
            po[(long long)T * N + sx.y] = ay.r[2 * k + 1];
        }
    }
}

template <int K>
void launch_ksm_kb(int beta, dim3 grid, hipStream_t s, const KsMacMultiArgs& g) {
    if (beta <= 2) hipLaunchKernelGGL((k_ks_mac_multi<2, K>), grid, dim3(TPB), 0, s, g);
    else if (beta <= 4) hipLaunchKernelGGL((k_ks_mac_multi<4, K>), grid, dim3(TPB), 0, s, g);
    else if constexpr (K == 2) {
        if (beta <= 8) hipLaunchKernelGGL((k_ks_mac_multi<8, K>), grid, dim3(TPB), 0, s, g);
        else hipLaunchKernelGGL((k_ks_mac_multi<0, K>), grid, dim3(TPB), 0, s, g);
    } else {
        // 5 to 8 prefetched digits next to the 4K sums of three or four keys do not fit 256 VGPRs: streamed from 5 digits on
        hipLaunchKernelGGL((k_ks_mac_multi<0, K>), grid, dim3(TPB), 0, s, g);
    }
}

struct ExtSumArgs {
    const u64* in[LSA_KSM_MAX_KEYS - 1];
    u64* out;
    long long sin, sout;
    const ModDev* mods;
    int n_in, accumulate, T, logn;
    unsigned char mod_of[LSA_MAX_PERIOD];   // [T]
};

// grid: x = 2T * (N/2/TPB), y = batch.  out[b][row][x] (+)= sum_k in_k[b][row][x] mod q_row
__global__ __launch_bounds__(TPB) void k_ext_sum(ExtSumArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int row = blockIdx.x / chunks;
    const int tl = row >= g.T ? row - g.T : row;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const long long b = blockIdx.y;
    const u64 q = g.mods[g.mod_of[tl]].q;
    const long long off = ((long long)row << g.logn) + x;
    u64 vx[LSA_KSM_MAX_KEYS - 1], vy[LSA_KSM_MAX_KEYS - 1];
#pragma unroll
    for (int k = 0; k < LSA_KSM_MAX_KEYS - 1; k++) {
        vx[k] = vy[k] = 0;
        if (k < g.n_in) {
            const ulonglong2 v = ld2(g.in[k] + b * g.sin + off);
            vx[k] = v.x;
            vy[k] = v.y;
        }
    }
    u64* po = g.out + b * g.sout + off;
    ulonglong2 r{0, 0};
    if (g.accumulate) r = ld2(po);
    st2(po, ext_sum_point(r.x, vx, LSA_KSM_MAX_KEYS - 1, q), ext_sum_point(r.y, vy, LSA_KSM_MAX_KEYS - 1, q));
}

}  // namespace

void launch_ks_mac_multi(Context& c, int level, const u64* cx, long long scx, const u64* ext, long long sext, int n_keys,
                         const KsMacMultiKey* keys, long long sout, const u64* base, long long sbase, int batch, hipStream_t s) {
    if (batch <= 0) return;
    LSA_REQUIRE(n_keys >= 2 && n_keys <= LSA_KSM_MAX_KEYS, "multi-key MAC: 2 to 4 keys per launch");
    LSA_REQUIRE(cx && ext && base && keys, "multi-key MAC: null argument");
    LSA_REQUIRE(c.n >= 2 * TPB, "ring degree too small for the multi-key MAC (need N >= 512)");
    KsMacMultiArgs g{};
    g.cx = cx;
    g.ext = ext;
    g.scx = scx;
    g.sext = sext;
    g.sout = sout;
    g.base = base;
    g.sbase = sbase;
    g.pm = c.pmodq_vec(level);
    g.mods = c.d_mods;
    g.logn = c.logn;
    g.L = level + 1;
    g.np = c.np;
    g.nq = c.nq;
    g.beta = (g.L + c.np - 1) / c.np;
    const int T = g.L + c.np;
    LSA_REQUIRE(sout >= 2LL * T * c.n, "multi-key MAC: output stride below one extended ciphertext");
    for (int k = 0; k < n_keys; k++) {
        LSA_REQUIRE(keys[k].key && keys[k].key->data && keys[k].scatter && keys[k].out, "multi-key MAC: null key, index map or output");
        LSA_REQUIRE(keys[k].key->level >= level, "key-switch key exported at a lower level than the ciphertext");
        for (int j = 0; j < k; j++) LSA_REQUIRE(keys[j].out != keys[k].out, "multi-key MAC: two keys share an output buffer");
        g.key[k] = keys[k].key->data;
        g.klvl[k] = keys[k].key->level;
        g.kcomp[k] = keys[k].key->level + 1 + c.np;
        g.scatter[k] = keys[k].scatter;
        g.out[k] = keys[k].out;
    }
    ProfScope ps(c, PROF_KSMAC, 8.0 * c.n * (batch * ((double)g.beta * T + 2.0 * T * n_keys + g.L) + 2.0 * g.beta * T * n_keys), s);
    // enough workgroups to fill the chip, as few key re-reads as possible (launch_ks_mac's grouping)
    const unsigned gx = (unsigned)(T * (c.n / (2 * TPB)));
    const int groups = std::max(1, std::min(batch, (int)((2048 + gx - 1) / gx)));
    g.batch = batch;
    g.bpt = (batch + groups - 1) / groups;
    const dim3 grid(gx, (unsigned)((batch + g.bpt - 1) / g.bpt));
    if (n_keys == 2) launch_ksm_kb<2>(g.beta, grid, s, g);
    else if (n_keys == 3) launch_ksm_kb<3>(g.beta, grid, s, g);
    else launch_ksm_kb<4>(g.beta, grid, s, g);
    LSA_HIP(hipGetLastError());
}

void launch_ext_sum(Context& c, int level, int n_in, const u64* const* in, long long sin, u64* out, long long sout, bool accumulate,
                    int batch, hipStream_t s) {
    if (batch <= 0) return;
    const int L = level + 1, T = L + c.np;
    LSA_REQUIRE(n_in >= 1 && n_in <= LSA_KSM_MAX_KEYS - 1 && in && out, "extended sum: 1 to 3 addends");
    LSA_REQUIRE(T <= LSA_MAX_PERIOD, "extended ciphertext: too many limbs");
    LSA_REQUIRE(c.n >= 2 * TPB, "ring degree too small for the extended sum (need N >= 512)");
    LSA_REQUIRE(sin >= 2LL * T * c.n && sout >= 2LL * T * c.n, "extended sum: stride below one extended ciphertext");
    ExtSumArgs g{};
    for (int k = 0; k < n_in; k++) {
        LSA_REQUIRE(in[k] != nullptr && in[k] != out, "extended sum: an addend is null or the output itself");
        g.in[k] = in[k];
    }
    g.out = out;
    g.sin = sin;
    g.sout = sout;
    g.mods = c.d_mods;
    g.n_in = n_in;
    g.accumulate = accumulate ? 1 : 0;
    g.T = T;
    g.logn = c.logn;
    for (int tl = 0; tl < T; tl++) g.mod_of[tl] = (unsigned char)c.qp_mod(L, tl);
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * 2.0 * T * (n_in + (accumulate ? 2.0 : 1.0)) * batch, s);
    hipLaunchKernelGGL(k_ext_sum, dim3((unsigned)(2 * T * (c.n / (2 * TPB))), (unsigned)batch), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

}  // namespace lsa
