// slot_sum.hip — the device kernels of the slot sums (ops.hip slot_sum_run, bfv_slot_sum_run; plan: slot_sum.h).  CKKS:
//   k_ks_mac_multi<KB, K>  the gadget inner product of ONE decomposition with K = 2..4 keys ("a MAC kernel that reads the
//                          decomposed digits once for all keys of a hoisted group"), each key's product leaving
//                          as that key's rotated extended ciphertext in that key's own buffer;
//   k_ext_sum              out (+)= sum of up to three extended ciphertexts: joins the per-key buffers.
// The per-point arithmetic is ks_mac_multi.h's, which the host compiles too (tests/cpp/test_ks_mac_multi.cpp).  k_ks_mac
// (kernels.hip) stays the single-key kernel: SlotSum::multi_mac = false runs it once per key, each launch adding to its
// destination, and that form measured faster at every bench shape, so it is the default.  BFV:
//   k_bfv_slot_tail        the coefficient-domain ModDown tail of one step: x + (acc - conv) / P plus the step's rotated c0 terms,
//                          gathered from the c0 row staged in LDS.
#include <atomic>

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

struct BfvSlotTailArgs {
    const u64* x;             // [2][L][N], coefficient domain
    const u64* acc;           // [2][acc_rpp][N], out of the NTT domain
    const u64* conv;          // [2][L][N]
    const u64* addend;        // [L][N] or null: one more addend of polynomial 0
    u64* out;                 // [2][L][N]; may be x
    u64* tail_c0;             // [L][N] or null
    const u32* next[LSA_KSM_MAX_KEYS - 1];   // coeff_perm tables of the NEXT rotations
    const u32* tail;          // coeff_perm table of the TAIL rotation (with tail_c0)
    const u64* kvec;          // [L] P^-1 mod q_j, Montgomery form
    const ModDev* mods;
    long long sx, sacc, sconv, sadd, so, stail;
    int n_next, tail_acc, acc_rpp, limbs, logn;
};

#define LSA_SLOT_TAIL_THREADS 1024
// grid: x = 2*limbs, y = batch; dynamic LDS: 8N bytes when the launch gathers, else none.  One workgroup per row: a c0 row is
// loaded once (coalesced, into LDS) and serves the row's own term, up to three NEXT gathers and the TAIL gather; every word of x is
// read before the barrier and every word of out is stored after it by the same workgroup, so out == x is safe.  The c1 rows are
// plain element-wise work.
__global__ __launch_bounds__(LSA_SLOT_TAIL_THREADS) void k_bfv_slot_tail(BfvSlotTailArgs g) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    const int n = 1 << g.logn;
    const int row = blockIdx.x;
    const int poly = row / g.limbs, limb = row % g.limbs;
    const ModDev m = g.mods[limb];
    const u64 k = g.kvec[limb];
    const long long b = blockIdx.y;
    const long long ro = ((long long)poly * g.limbs + limb) << g.logn;
    const u64* xr = g.x + b * g.sx + ro;
    const u64* a = g.acc + b * g.sacc + (((long long)poly * g.acc_rpp + limb) << g.logn);
    const u64* v = g.conv + b * g.sconv + ro;
    u64* o = g.out + b * g.so + ro;
    const bool gather = poly == 0 && (g.n_next > 0 || g.tail != nullptr);   // uniform over the workgroup
    if (gather) {
        for (int x = threadIdx.x * 2; x < n; x += 2 * LSA_SLOT_TAIL_THREADS) *reinterpret_cast<ulonglong2*>(lds + x) = ld2(xr + x);
        __syncthreads();
    }
    const u64* ad = poly == 0 && g.addend ? g.addend + b * g.sadd + ((long long)limb << g.logn) : nullptr;
    u64* tc = gather && g.tail ? g.tail_c0 + b * g.stail + ((long long)limb << g.logn) : nullptr;
    for (int x = threadIdx.x * 2; x < n; x += 2 * LSA_SLOT_TAIL_THREADS) {
        const ulonglong2 va = ld2(a + x), vv = ld2(v + x);
        const ulonglong2 c = gather ? *reinterpret_cast<const ulonglong2*>(lds + x) : ld2(xr + x);
        u64 r0 = add_mod(mont_mul(sub_mod(va.x, vv.x, m.q), k, m.q, m.qinv), c.x, m.q);
        u64 r1 = add_mod(mont_mul(sub_mod(va.y, vv.y, m.q), k, m.q, m.qinv), c.y, m.q);
        if (ad) {
            const ulonglong2 w = ld2(ad + x);
            r0 = add_mod(r0, w.x, m.q);
            r1 = add_mod(r1, w.y, m.q);
        }
        if (gather) {
            auto rotated = [&](const u32* perm, u64& t0, u64& t1) {
                const uint2 p = *reinterpret_cast<const uint2*>(perm + x);
                t0 = lds[p.x & 0x7fffffffu];
                t1 = lds[p.y & 0x7fffffffu];
                if (p.x >> 31) t0 = neg_mod(t0, m.q);
                if (p.y >> 31) t1 = neg_mod(t1, m.q);
            };
#pragma unroll
            for (int i = 0; i < LSA_KSM_MAX_KEYS - 1; i++)
                if (i < g.n_next) {
                    u64 t0, t1;
                    rotated(g.next[i], t0, t1);
                    r0 = add_mod(r0, t0, m.q);
                    r1 = add_mod(r1, t1, m.q);
                }
            if (tc) {
                u64 t0, t1;
                rotated(g.tail, t0, t1);
                if (g.tail_acc) {
                    const ulonglong2 w = ld2(tc + x);
                    t0 = add_mod(t0, w.x, m.q);
                    t1 = add_mod(t1, w.y, m.q);
                }
                st2(tc + x, t0, t1);
            }
        }
        st2(o + x, r0, r1);
    }
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

void launch_bfv_slot_tail(Context& c, int level, const BfvSlotTail& t, const u64* acc, long long sacc, int acc_rpp, const u64* conv,
                          long long sconv, const u64* x, long long sx, u64* out, long long sout, int batch, hipStream_t s) {
    if (batch <= 0) return;
    const int L = level + 1;
    LSA_REQUIRE(level >= 0 && L <= c.nq, "BFV slot tail: level out of range");
    LSA_REQUIRE(acc && conv && x && out && acc_rpp >= L, "BFV slot tail: null or short operand");
    LSA_REQUIRE(t.n_next >= 0 && t.n_next <= LSA_KSM_MAX_KEYS - 1, "BFV slot tail: at most three NEXT rotations");
    LSA_REQUIRE((t.tail != nullptr) == (t.tail_c0 != nullptr), "BFV slot tail: the TAIL rotation and its accumulator come together");
    const bool gathers = t.n_next > 0 || t.tail;
    LSA_REQUIRE(!gathers || c.logn <= LSA_PERM_LDS_MAX_LOGN, "BFV slot tail: the ring's limbs do not fit in LDS");
    LSA_REQUIRE(c.n >= 2, "BFV slot tail: ring degree too small");
    BfvSlotTailArgs g{};
    g.x = x;
    g.acc = acc;
    g.conv = conv;
    g.addend = t.addend;
    g.out = out;
    g.tail_c0 = t.tail_c0;
    for (int i = 0; i < t.n_next; i++) {
        LSA_REQUIRE(t.next[i] != nullptr, "BFV slot tail: permutation missing");
        g.next[i] = t.next[i];
    }
    g.tail = t.tail;
    g.kvec = c.pinv_vec(level);
    g.mods = c.d_mods;
    g.sx = sx;
    g.sacc = sacc;
    g.sconv = sconv;
    g.sadd = t.s_addend;
    g.so = sout;
    g.stail = t.s_tail;
    g.n_next = t.n_next;
    g.tail_acc = t.tail_accumulate ? 1 : 0;
    g.acc_rpp = acc_rpp;
    g.limbs = L;
    g.logn = c.logn;
    // x, acc, conv and out for both polynomials; per c0 row the addend, the tail (read if it accumulates) and 4 bytes per point and table
    ProfScope ps(c, PROF_ELEMWISE,
                 8.0 * c.n * batch * L * (8.0 + (t.addend ? 1 : 0) + (t.tail ? (t.tail_accumulate ? 2 : 1) : 0)) +
                     4.0 * c.n * batch * L * (t.n_next + (t.tail ? 1 : 0)),
                 s);
    const size_t lds_bytes = gathers ? (size_t)c.n * sizeof(u64) : 0;
    if (lds_bytes > 65536) {   // opt in to more than 64 KiB of dynamic LDS, once per device (the attribute is per device)
        static std::atomic<unsigned long long> raised{0};
        int dev = 0;
        LSA_HIP(hipGetDevice(&dev));
        const unsigned long long bit = 1ull << (dev & 63);
        if (!(raised.load(std::memory_order_acquire) & bit)) {
            LSA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bfv_slot_tail), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        160 * 1024));
            raised.fetch_or(bit, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL(k_bfv_slot_tail, dim3((unsigned)(2 * L), (unsigned)batch), dim3(LSA_SLOT_TAIL_THREADS), lds_bytes, s, g);
    LSA_HIP(hipGetLastError());
}

}  // namespace lsa
