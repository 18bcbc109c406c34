// slot_sum.hip — the slot sums: their device kernels and, below them, their runners on the key-switch tile of key_switch.h
// (slot_sum_run, bfv_slot_sum_run; plan: slot_sum.h).  CKKS:
//   k_ks_mac_multi<KB, K>  the gadget inner product of ONE decomposition with K = 2..4 keys ("a MAC kernel that reads the
//                          decomposed digits once for all keys of a hoisted group"), each key's product leaving
//                          as that key's rotated extended ciphertext in that key's own buffer;
//   k_ext_sum              out (+)= sum of up to three extended ciphertexts: joins the per-key buffers.
// The per-point arithmetic is ks_mac_multi.h's, which the host compiles too (tests/cpp/test_ks_mac_multi.cpp).  k_ks_mac
// (kernels.hip) stays the single-key kernel: SlotSum::multi_mac = false runs it once per key, each launch adding to its
// destination, and that form measured faster at every bench shape, so it is the default.  BFV:
//   k_bfv_slot_tail        the coefficient-domain ModDown tail of one step, the key switch's tail hook (BfvSlotTail): x + (acc - conv) / P
//                          plus the step's rotated c0 terms, gathered from the c0 row staged in LDS.  Its own kernel, on
//                          the helpers of moddown_gather.h.
#include "entry_check.h"
#include "moddown_gather.h"
#include "ks_mac_groups.h"
#include "ks_mac_multi.h"

namespace lsa {

namespace {

constexpr int TPB = 256;

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

// the coefficient-domain ModDown tail of one step of the BFV slot sum, the key switch's tail hook (k_bfv_slot_tail), x = KsOut::base
// and out = KsOut::p [2][L][N]:
//   out[0][j][y] = x0[j][y] + sum_{r<n_next} sign_r(y) x0[j][pi_r(y)] + (addend ? addend[j][y] : 0) + (acc[0][j][y] - conv[0][j][y]) Pinv_j
//   out[1][j][y] = x1[j][y] + (acc[1][j][y] - conv[1][j][y]) Pinv_j
//   tail_c0[j][y] (+)= sign_t(y) x0[j][pi_t(y)]                       when `tail` is given
// next / tail: Context::coeff_perm tables.  out may be x itself: a row is read and written by one workgroup, reads first.
struct BfvSlotTail final : KsCoeffTail {
    int n_next = 0;
    const u32* next[3] = {nullptr, nullptr, nullptr};
    const u32* tail = nullptr;
    u64* tail_c0 = nullptr;   // [L][N] per batch item
    long long s_tail = 0;
    bool tail_accumulate = false;
    const u64* addend = nullptr;   // [L][N] per batch item
    long long s_addend = 0;
    BfvSlotTail() : KsCoeffTail(2) {}
    void launch(Context& c, int level, const u64* acc, long long s_acc, int acc_rpp, const u64* conv, long long s_conv, const KsOut& o,
                int nb, hipStream_t s) const override;
};

struct BfvSlotTailArgs {
    RowTailArgs t;            // base: x, [2][L][N], coefficient domain; out may be x; perm unused
    const u64* addend;        // [L][N] or null: one more addend of polynomial 0
    u64* tail_c0;             // [L][N] or null
    const u32* next[LSA_KSM_MAX_KEYS - 1];   // coeff_perm tables of the NEXT rotations
    const u32* tail;          // coeff_perm table of the TAIL rotation (with tail_c0)
    long long sadd, stail;
    int n_next, tail_acc;
};

// grid: x = 2*limbs, y = batch; dynamic LDS: 8N bytes when the launch gathers, else none.  One workgroup per row: a c0 row is
// loaded once (coalesced, into LDS) and serves the row's own term, up to three NEXT gathers and the TAIL gather; every word of x is
// read before the barrier and every word of out is stored after it by the same workgroup, so out == x is safe.  The c1 rows are
// plain element-wise work.  (Not the skeleton of moddown_gather.h: it stages x, not the ModDown result, and gathers up to four tables.)
__global__ __launch_bounds__(LSA_LDS_ROW_THREADS) void k_bfv_slot_tail(BfvSlotTailArgs g) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    const int n = 1 << g.t.logn;
    const int row = blockIdx.x;
    const int poly = row / g.t.limbs, limb = row % g.t.limbs;
    const ModDev m = g.t.mods[limb];
    const u64 k = g.t.kvec[limb];
    const long long b = blockIdx.y;
    const long long ro = ((long long)poly * g.t.limbs + limb) << g.t.logn;
    const u64* xr = g.t.base + b * g.t.sbase + ro;
    const u64* a = g.t.acc + b * g.t.sacc + (((long long)poly * g.t.acc_rpp + limb) << g.t.logn);
    const u64* v = g.t.conv + b * g.t.sconv + ro;
    u64* o = g.t.out + b * g.t.sout + ro;
    const bool gather = poly == 0 && (g.n_next > 0 || g.tail != nullptr);   // uniform over the workgroup
    if (gather) {
        for (int x = threadIdx.x * 2; x < n; x += 2 * LSA_LDS_ROW_THREADS) *reinterpret_cast<ulonglong2*>(lds + x) = ld2(xr + x);
        __syncthreads();
    }
    const u64* ad = poly == 0 && g.addend ? g.addend + b * g.sadd + ((long long)limb << g.t.logn) : nullptr;
    u64* tc = gather && g.tail ? g.tail_c0 + b * g.stail + ((long long)limb << g.t.logn) : nullptr;
    for (int x = threadIdx.x * 2; x < n; x += 2 * LSA_LDS_ROW_THREADS) {
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
#pragma unroll
            for (int i = 0; i < LSA_KSM_MAX_KEYS - 1; i++)
                if (i < g.n_next) {
                    const ulonglong2 t = lds_gather_pair(lds, g.next[i], x, m.q);
                    r0 = add_mod(r0, t.x, m.q);
                    r1 = add_mod(r1, t.y, m.q);
                }
            if (tc) {
                ulonglong2 t = lds_gather_pair(lds, g.tail, x, m.q);
                if (g.tail_acc) {
                    const ulonglong2 w = ld2(tc + x);
                    t.x = add_mod(t.x, w.x, m.q);
                    t.y = add_mod(t.y, w.y, m.q);
                }
                st2(tc + x, t.x, t.y);
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
    const KsMacGroups gr = ks_mac_groups(gx, batch);
    g.batch = batch;
    g.bpt = gr.bpt;
    const dim3 grid(gx, (unsigned)gr.gy);
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

void BfvSlotTail::launch(Context& c, int level, const u64* acc, long long s_acc, int acc_rpp, const u64* conv, long long s_conv,
                         const KsOut& o, int nb, hipStream_t s) const {
    if (nb <= 0) return;
    const int L = level + 1;
    LSA_REQUIRE(n_next >= 0 && n_next <= LSA_KSM_MAX_KEYS - 1, "BFV slot tail: at most three NEXT rotations");
    LSA_REQUIRE((tail != nullptr) == (tail_c0 != nullptr), "BFV slot tail: the TAIL rotation and its accumulator come together");
    BfvSlotTailArgs g{};
    g.addend = addend;
    g.tail_c0 = tail_c0;
    for (int i = 0; i < n_next; i++) {
        LSA_REQUIRE(next[i] != nullptr, "BFV slot tail: permutation missing");
        g.next[i] = next[i];
    }
    g.tail = tail;
    g.sadd = s_addend;
    g.stail = s_tail;
    g.n_next = n_next;
    g.tail_acc = tail_accumulate ? 1 : 0;
    // x, acc, conv and out for both polynomials; per c0 row the addend, the tail (read if it accumulates) and 4 bytes per point and table
    launch_lds_row_tail<&k_bfv_slot_tail>(c, level, "BFV slot tail", g, acc, s_acc, acc_rpp, conv, s_conv, o, nb,
                                          8.0 * c.n * nb * L * (8.0 + (addend ? 1 : 0) + (tail ? (tail_accumulate ? 2 : 1) : 0)) +
                                              4.0 * c.n * nb * L * (n_next + (tail ? 1 : 0)),
                                          s, n_next > 0 || tail);
}

// ------------------------------------------------------------------------------------------------ CKKS slot sum
// out = sum_{i<count} rot(in, i*step) by the plan of slot_sum.h.  Per tile the steps run back to back: one decomposition of x's c1,
// the gadget products of the step's 1..4 keys written as rotated extended ciphertexts (KsTile::mac_ext: the words of
// ckks_rotate_ext) -- several keys in ONE k_ks_mac_multi launch, each into its own buffer, k_ext_sum joining them -- then
// x <- x + ModDown(NEXT sum) with x riding on the ModDown tail's base (base_polys = 2).  That store is index for index, so from
// the second step on x lives in `out` and is updated in place, and out == in is allowed.  The TAIL rotations gather in an extended
// accumulator that is divided once, after the last step.  All temporaries are the tile's workspace: the KsTile rows, up to three more
// extended ciphertexts for the keys of a multi-key launch beyond the first, and one for the tail.
SlotSumPlanHost slot_sum_plan_checked(int n_ring, long long step, int count, int radix) {
    try {
        return slot_sum_plan(n_ring, step, count, radix, LSA_SLOTSUM_DEFAULT_RADIX);
    } catch (const std::invalid_argument& e) {
        throw Error(LSA_ERR_ARG, e.what());
    }
}

SlotSum* slot_sum_create(Context& c, int level, long long step, int count, int radix) {
    LSA_REQUIRE(c.algo == LSA_ALGO_CKKS, "slot sum: context is not CKKS");
    LSA_REQUIRE(level >= 0 && level < c.nq, "slot sum: level out of range");
    auto p = std::make_unique<SlotSum>(c, level);
    p->plan = slot_sum_plan_checked(c.n, step, count, radix);
    LSA_REQUIRE(p->plan.steps.empty() || c.np >= 1, "slot sum: key switching needs at least one special prime");
    return p.release();
}

// What both slot-sum runners do before their tiles.  Every key of `elements` (the plan's, in the order a missing one is reported)
// is looked up and checked before anything is queued; then the operands; a plan without steps (count == 1, no row fold) is a
// copy; last the rotations' tables, element by element (table look-ups upload on first use: only after every argument is
// accepted): the NTT-domain scatter and, for the BFV gathering tail, the coefficient-domain permutation.
// run == false: nothing is left to do.
struct SlotSumCall {
    bool run = false;
    GaloisKeys key_of;   // the plan's keys alone, all present
    std::map<u64, const u32*> scatter_of, perm_of;
};
static SlotSumCall slot_sum_prologue(Context& c, const EntryCheck& ck, const SlotSumPlanHost& plan, const std::vector<u64>& elements,
                                     const GaloisKeys& glk, const u64* in, long long sin, u64* out, long long sout, int batch,
                                     bool gather, hipStream_t s) {
    SlotSumCall call;
    const std::vector<const Key*> keys = glk.resolve(elements, ck.who, [&](u64, const Key& k) { ck.key(k, "a Galois key"); });
    for (size_t i = 0; i < elements.size(); i++) call.key_of.insert(elements[i], keys[i]);
    if (batch <= 0) return call;
    const int L = ck.level + 1;
    const size_t w = 2 * (size_t)L * c.n;
    const layout::Span sp_in = ck.operand(in, sin, w, "in", false), sp_out = ck.output(out, sout, w);
    ck.same_or_apart(sp_out, sp_in, "in");
    if (plan.steps.empty()) {
        if (layout::same(sp_out, sp_in)) return call;
        std::vector<int> rows(2 * L);
        for (int i = 0; i < 2 * L; i++) rows[i] = i;
        launch_copy_rows(c, in, sin, out, sout, 2 * L, rows.data(), batch, s);
        return call;
    }
    LSA_REQUIRE(!gather || c.logn <= LSA_PERM_LDS_MAX_LOGN, ck.who + ": the gathering tail needs N <= 2^14");
    for (u64 e : elements) {
        call.scatter_of[e] = inverse_perm(c, e);
        if (gather) call.perm_of[e] = c.coeff_perm(e);
    }
    call.run = true;
    return call;
}

void slot_sum_run(SlotSum& p, const u64* in, long long sin, u64* out, long long sout, int batch,
                  const GaloisKeys& glk, hipStream_t s) {
    Context& c = p.c;
    const int level = p.level;
    const EntryCheck ck(c, "lsa_ckks_slot_sum", LSA_ALGO_CKKS, level, 0, batch);
    std::vector<u64> by_rotation;   // a missing key is reported in the order of the plan's rotations
    for (int r : p.plan.rotations) by_rotation.push_back(galois_of_rotation(r, c.n));
    const SlotSumCall call = slot_sum_prologue(c, ck, p.plan, by_rotation, glk, in, sin, out, sout, batch, false, s);
    if (!call.run) return;
    const auto& key_of = call.key_of;
    const auto& scatter_of = call.scatter_of;
    const long long N = c.n;
    const int L = level + 1, T = L + c.np;
    const size_t ks_rows = KsTile::rows(c, level);
    const bool multi = p.multi_mac;
    // extended buffers beyond KsTile's acc: one per key of a multi-key launch that is neither the first NEXT key nor the first
    // TAIL key of the plan (the most any step needs), and the tail accumulator
    int n_more = 0;
    {
        bool live = false;
        for (const SlotSumStep& step : p.plan.steps) {
            int more = 0, next = 0;
            for (const SlotSumKey& k : step.keys) more += k.tail ? (live ? 1 : 0) : (next++ ? 1 : 0);
            for (const SlotSumKey& k : step.keys) live = live || k.tail;
            if (multi && step.keys.size() >= 2) n_more = std::max(n_more, more);
        }
    }
    const int n_extra = n_more + (p.plan.has_tail ? 1 : 0);
    for_tiles(c, ks_rows + (size_t)n_extra * 2 * T, batch, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t st) {
        KsTile t(c, level, nb, ws, st);
        const long long s_ext2 = t.s_acc;   // [2][T][N] per batch item, like t.acc
        u64* extra[LSA_SLOTSUM_MAX_KEYS];
        for (int i = 0; i < n_extra; i++) extra[i] = ws + (ks_rows * tb + (size_t)i * 2 * T * tb) * N;
        u64* tail = p.plan.has_tail ? extra[n_more] : nullptr;
        const u64* x = in + (size_t)b0 * sin;
        long long sx = sin;
        u64* o = out + (size_t)b0 * sout;
        bool tail_live = false;
        for (const SlotSumStep& step : p.plan.steps) {
            t.decompose(KsSource::of_ntt(x + (long long)L * N, sx));
            const int nk = (int)step.keys.size();
            const bool one_launch = multi && nk >= 2;
            KsMacMultiKey mk[LSA_SLOTSUM_MAX_KEYS];
            bool add_to[LSA_SLOTSUM_MAX_KEYS];   // sequential form: the key's product is added to its destination
            const u64* next_more[LSA_SLOTSUM_MAX_KEYS];
            const u64* tail_more = nullptr;
            int n_next = 0, n_sum = 0, used = 0;
            for (int i = 0; i < nk; i++) {
                const SlotSumKey& k = step.keys[i];
                u64* dst;
                if (k.tail) {
                    add_to[i] = tail_live;
                    dst = !tail_live || !one_launch ? tail : extra[used++];
                    if (dst != tail) tail_more = dst;
                } else {
                    add_to[i] = n_next > 0;
                    dst = n_next == 0 || !one_launch ? t.acc : extra[used++];
                    if (dst != t.acc) next_more[n_sum++] = dst;
                    n_next++;
                }
                mk[i] = {key_of.at(k.g), scatter_of.at(k.g), dst};
            }
            if (one_launch) {
                t.mac_ext_multi(nk, mk, s_ext2, x, sx);
                if (n_sum) launch_ext_sum(c, level, n_sum, next_more, s_ext2, t.acc, s_ext2, true, nb, st);
                if (tail_more) launch_ext_sum(c, level, 1, &tail_more, s_ext2, tail, s_ext2, true, nb, st);
            } else {
                for (int i = 0; i < nk; i++)
                    t.mac_ext(*mk[i].key, {.out = mk[i].out, .sout = s_ext2, .scatter = mk[i].scatter, .base = x, .sbase = sx, .accumulate = add_to[i]});
            }
            for (int i = 0; i < nk; i++) tail_live = tail_live || step.keys[i].tail;
            t.moddown(ks_onto_ct(o, sout, x, sx, L));
            x = o;
            sx = sout;
        }
        if (tail_live) t.moddown_of(tail, s_ext2, ks_onto_ct(o, sout, x, sx, L));
    });
}

// ------------------------------------------------------------------------------------------------ BFV slot sum
// out = sum_{i<count} rot_cols(y, i*step), y = in + rot_rows(in) if rows, by the plan of slot_sum.h on coefficient-domain
// ciphertexts.  Per tile and step, as bfv_rotate_many: c1 of x into the NTT domain once (the MAC's own-digit operand, a COEFF
// source of the tile), the decomposition from the coefficients, one extended MAC per key with the rotation's NTT-domain scatter
// -- the first NEXT key writes the tile's acc, later ones add to it, the TAIL key writes or adds to the extended tail accumulator
// -- then the coefficient-domain ModDown of the NEXT sum.  gather: the MACs add no P * c0; the tail (k_bfv_slot_tail) adds x and
// the rotated c0 terms, gathered from the c0 row in LDS, and collects the TAIL rotation's c0 term in tail_c0 [L][N]; after the
// last step out = x + (tail_c0, 0) + ModDown(tail).  plain: c0 is transformed too and enters the MACs as `base` (the CKKS form), the
// tails are launch_moddown_final with base = x.  ModDown(P z + a) = z + ModDown(a) residue for residue, so both give the same
// words.  x lives in `out` from the second step on and is updated in place.
SlotSumPlanHost bfv_slot_sum_plan_checked(int n_ring, long long step, int count, int radix, int rows) {
    try {
        return bfv_slot_sum_plan(n_ring, step, count, radix, rows, LSA_BFV_SLOTSUM_DEFAULT_RADIX);
    } catch (const std::invalid_argument& e) {
        throw Error(LSA_ERR_ARG, e.what());
    }
}

BfvSlotSum* bfv_slot_sum_create(Context& c, int level, long long step, int count, int radix, int rows) {
    LSA_REQUIRE(c.algo == LSA_ALGO_BFV, "lsa_bfv_slot_sum_create: context is not BFV");
    LSA_REQUIRE(level >= 0 && level < c.nq, "lsa_bfv_slot_sum_create: level out of range (0.." + std::to_string(c.nq - 1) + ")");
    auto p = std::make_unique<BfvSlotSum>(c, level);
    p->plan = bfv_slot_sum_plan_checked(c.n, step, count, radix, rows);
    LSA_REQUIRE(p->plan.steps.empty() || c.np >= 1, "lsa_bfv_slot_sum_create: key switching needs at least one special prime");
    return p.release();
}

void bfv_slot_sum_run(BfvSlotSum& p, const u64* in, long long sin, u64* out, long long sout, int batch,
                      const GaloisKeys& glk, hipStream_t s) {
    Context& c = p.c;
    const int level = p.level;
    const EntryCheck ck(c, "lsa_bfv_slot_sum", LSA_ALGO_BFV, level, 0, batch);
    const bool gather = p.gather;
    const SlotSumCall call = slot_sum_prologue(c, ck, p.plan, p.plan.galois, glk, in, sin, out, sout, batch, gather, s);
    if (!call.run) return;
    const auto& key_of = call.key_of;
    const auto& scatter_of = call.scatter_of;
    const auto& perm_of = call.perm_of;
    const long long N = c.n;
    const int L = level + 1, T = L + c.np;
    const bool has_tail = p.plan.has_tail;
    const size_t ks_rows = KsTile::rows(c, level, KsSource::COEFF);   // NTT(c1) in front of the tile's own rows
    // per batch item: the KsTile rows | the extended tail accumulator | tail_c0 (gather) or NTT(c0) (plain)
    const size_t r_tail = has_tail ? 2 * (size_t)T : 0, r_last = gather ? (has_tail ? (size_t)L : 0) : (size_t)L;
    const long long sL = (long long)L * N;
    for_tiles(c, ks_rows + r_tail + r_last, batch, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t st) {
        u64* tail = ws + ks_rows * N * tb;
        u64* last = tail + r_tail * N * tb;   // tail_c0 or NTT(c0)
        // (tb: tail and last follow the tile's rows at offsets counted in tiles of tb items, so the tile's NTT(c1) block in front
        // of its own rows spans tb items as well, a ragged last tile included)
        KsTile t(c, level, nb, ws, st, nullptr, KsSource::COEFF, tb);
        const long long s_ext2 = t.s_acc;   // [2][T][N] per batch item, like t.acc
        const u64* x = in + (size_t)b0 * sin;
        long long sx = sin;
        u64* o = out + (size_t)b0 * sout;
        bool tail_live = false;
        for (const SlotSumStep& step : p.plan.steps) {
            if (!gather) launch_ntt(c, x, last, nb, sx, sL, L, rm_seq(L), false, st);
            t.decompose(KsSource::of_coeff(x + sL, sx));
            BfvSlotTail bt;
            bool next_live = false;
            for (const SlotSumKey& k : step.keys) {
                const bool add_to = k.tail ? tail_live : next_live;
                t.mac_ext(*key_of.at(k.g), {.out = k.tail ? tail : t.acc, .sout = s_ext2, .scatter = scatter_of.at(k.g),
                                            .base = gather ? nullptr : last, .sbase = sL, .accumulate = add_to});
                if (k.tail) {
                    if (gather) {
                        bt.tail = perm_of.at(k.g);
                        bt.tail_c0 = last;
                        bt.s_tail = sL;
                        bt.tail_accumulate = tail_live;
                    }
                    tail_live = true;
                } else {
                    if (gather) bt.next[bt.n_next++] = perm_of.at(k.g);
                    next_live = true;
                }
            }
            t.moddown(ks_onto_ct(o, sout, x, sx, L, {.form = KsOut::COEFF, .tail = gather ? &bt : nullptr}));
            x = o;
            sx = sout;
        }
        if (tail_live) {
            BfvSlotTail bt;
            bt.addend = last;
            bt.s_addend = sL;
            t.moddown_of(tail, s_ext2, ks_onto_ct(o, sout, x, sx, L, {.form = KsOut::COEFF, .tail = gather ? &bt : nullptr}));
        }
    });
}

}  // namespace lsa
