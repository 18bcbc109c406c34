// kernels.hip — hand-written gfx950 kernels for the RNS hot path and their launchers.
// HBM-bound integer work: 16 B/lane coalesced accesses, LDS-staged butterflies, no MFMA (no dense FP contraction here).
#include <cstdlib>

#include "build_flags.h"
#include "ks_mac_groups.h"
#include "lsa_internal.h"
#include "moddown_gather.h"
#include "ntt_r16.h"
#include "plain_ops.h"
#include "poly_lincomb.h"
#include "tensor_sum.h"

namespace lsa {

const char* kernels_build_flags() { return LSA_BUILD_FLAGS_TEXT; }

static constexpr int TPB = 256;

// ------------------------------------------------------------------------------------------------ K1/K2 NTT pass
#ifndef LSA_NTT_WAVES
#define LSA_NTT_WAVES 4   // min waves/SIMD the register allocator must allow (= co-resident 256-thread workgroups per CU):
                          // 4 = at most 128 VGPRs; the plain and epilogue-only variants fit without spilling
#endif

#if defined(LSA_NTT_DIAG_STAMPS)   // diagnostic build: shader-clock stamp k of this workgroup (first 8192 workgroups)
#define LSA_STAMP(k)                                                                               \
    do {                                                                                           \
        if (a.diag && threadIdx.x == 0 && blockIdx.x < 8192) a.diag[blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define LSA_STAMP(k) do { } while (0)
#endif

template <int NT, bool TWL = false>
__device__ __forceinline__ void ntt_butterfly_phases(const NttPassArgs& a, const NttBlockCtx& bc, int tid, u64* lds) {
    int rho[4];
    const int np = ntt_split(a.mu, rho);
    if (!a.inverse) {
        int sig = 0;
        for (int i = 0; i < np; i++) {
            ntt_phase_sub_dyn<NT, TWL>(a, bc, tid, lds, sig, rho[i]);
            LSA_STAMP(3 + 2 * i);
            __syncthreads();
            LSA_STAMP(4 + 2 * i);
            sig += rho[i];
        }
    } else {
        int sig = a.mu;
        for (int i = np - 1; i >= 0; i--) {
            sig -= rho[i];
            ntt_phase_sub_dyn<NT, TWL>(a, bc, tid, lds, sig, rho[i]);
            __syncthreads();
        }
    }
}

// FZ: the launch carries a fused prologue/epilogue (NttPassArgs::fz_*)
#ifndef LSA_NTT_WAVES_FUSED
#define LSA_NTT_WAVES_FUSED 3   // variants with the two-operand prologue (FZ & 1): 3 workgroups per CU, up to 168 VGPRs
#endif
// NT: workgroup size = tile points / 16.  256 threads (4096-point tiles, 3-4 workgroups per CU) is the two-pass shape;
// 512 / 1024 threads hold a whole N = 2^13 / 2^14 limb in LDS (69 / 136 KiB) and transform it in ONE pass: half the HBM
// traffic of the two-pass plan, at one or two workgroups per CU.
// TWL: the pass holds global stage 0 (strided first pass of a two-pass plan): its 2^mu twiddles are the same for every tile
// of the limb and go through LDS -- one fetch per workgroup, issued with the tile loads, instead of one per sub-pass.
// FZ: 0 plain, 1 fused prologue only (first pass of a two-pass fused transform), 2 fused epilogue only (its last pass), 3 both
// (single-pass transforms), 4 the pt_mul epilogue (fz_epi == 3) only, 8 the rotate-and-MAC epilogue (fz_epi == 4) only, 16 the
// product prologue (fz_pro == 3, the first executed pass of an inverse transform) only, 32 (k_ntt_r16 first passes) the single-source
// lift prologue (fz_pro == 4) only; on k_ntt_pass the lift rides on FZ bit 1.  Split so that a pass carries only the tail code and
// registers it can execute.
template <int FZ, int NT, bool TWL = false>
__global__ __launch_bounds__(NT, NT > 512 ? 1 : NT > 256 ? 2 : (FZ & 1) ? LSA_NTT_WAVES_FUSED : LSA_NTT_WAVES) void k_ntt_pass(NttPassArgs a) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    const int tid = threadIdx.x;
    NttBlockCtx bc = ntt_decode_block(a, (long long)blockIdx.x);
    if (bc.mod == LSA_ROW_SKIP) return;  // uniform per block, before any barrier
    ulonglong2 twp = {0, 0};
    if (TWL) {
        bc.tw_l = lds + lds_words(a.tau);
        if (tid < (1 << a.mu)) {
            if (bc.fp) twp.x = d_to_bits(a.twd[((long long)bc.mod << a.logn) + tid]);
            else twp = *reinterpret_cast<const ulonglong2*>(a.tw + (((long long)bc.mod << a.logn) << 1) + 2 * tid);
        }
    }
#if defined(LSA_NTT_STAGGER)
    // Workgroups of one launch have identical phase lengths and start together, so the 3-4 co-resident ones run their
    // HBM phase and their butterfly phase in lockstep (measured: kernel time == copy-only time + compute-only time).
    // Delay the workgroups that share a CU (blockIdx 256 apart in the first dispatch wave) by thirds of a tile period once.
    {
        const int phase = blockIdx.x < 768 ? (int)(blockIdx.x >> 8) : 0;   // first dispatch wave only
        for (int i = 0; i < phase * LSA_NTT_STAGGER; i++) __builtin_amdgcn_s_sleep(100);
    }
#endif
#if defined(LSA_NTT_DIAG_COMPUTE_ONLY)   // diagnostic build: butterflies on synthetic LDS contents, no global traffic
    for (int i = tid; i < (1 << a.tau); i += NT)
        lds[lds_addr(i)] = bc.fp ? d_to_bits((double)(i * 7 + 1)) : (u64)(i * 7 + 1);
    __syncthreads();
    ntt_butterfly_phases<NT>(a, bc, tid, lds);
    if (lds[lds_addr(tid)] == 0x123456789abcull) a.dst[bc.base_dst + tid] = 1;   // keeps the work alive
    return;
#endif
    LSA_STAMP(0);
    ntt_phase_load<(FZ & 1) != 0, NT, (FZ & 16) != 0>(a, bc, tid, lds);
    if (TWL && tid < (1 << a.mu)) {
        u64* tw_l = lds + lds_words(a.tau);
        if (bc.fp) tw_l[tid] = twp.x;
        else {
            tw_l[2 * tid] = twp.x;
            tw_l[2 * tid + 1] = twp.y;
        }
    }
    LSA_STAMP(1);
    __syncthreads();
    LSA_STAMP(2);
#if defined(LSA_NTT_DIAG_COPY_ONLY)   // diagnostic build: data movement of the pass structure without butterflies
    ntt_phase_store<(FZ & 2) != 0, NT, (FZ & 4) != 0, (FZ & 8) != 0>(a, bc, tid, lds);
    return;
#endif
    ntt_butterfly_phases<NT, TWL>(a, bc, tid, lds);
    ntt_phase_store<(FZ & 2) != 0, NT, (FZ & 4) != 0, (FZ & 8) != 0>(a, bc, tid, lds);
    LSA_STAMP(7);
}

// ---- the 8-stage passes of two-pass plans: 16 x 16 register butterflies, one LDS exchange (ntt_r16.h)
// PASS 0 (first pass): the exchange crosses wavefronts -> one workgroup barrier.  PASS 1 (second pass): a 256-point transform
// lives in 16 lanes of one wavefront, LDS instructions of a wavefront execute in order: the exchanges need no barrier, only
// that the compiler keeps the LDS accesses in program order (wavefront-scope fences).
template <int PASS>
__device__ __forceinline__ void r16_sync() {
#if defined(LSA_R16_BARRIERS)   // A/B: workgroup barriers in the second pass too
    __syncthreads();
#else
    if (PASS == 0) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
#endif
}
#ifndef LSA_R16_WAVES
#define LSA_R16_WAVES 4
#endif
template <int PASS, int FZ, int MU>
__global__ __launch_bounds__(LSA_R16_THREADS, (FZ & 1) ? LSA_NTT_WAVES_FUSED : LSA_R16_WAVES) void k_ntt_r16(NttPassArgs a) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    const int tid = threadIdx.x;
    const NttBlockCtx bc = ntt_decode_block(a, (long long)blockIdx.x);
    if (bc.mod == LSA_ROW_SKIP) return;  // uniform per block, before any barrier
    u64 v[16];
    r16_phase<PASS, FZ, MU>(a, bc, tid, lds, 0, v);
    if (!(PASS == 0 && a.inverse)) r16_sync<PASS>();   // (first pass, inverse: phase 0 only filled registers)
    r16_phase<PASS, FZ, MU>(a, bc, tid, lds, 1, v);
    if (PASS == 0 && !a.inverse) return;                // (first pass, forward: phase 1 stored the results)
    r16_sync<PASS>();
    r16_phase<PASS, FZ, MU>(a, bc, tid, lds, 2, v);
}
// the nine-stage second pass (N = 2^17 / 2^18): three radix-8 groups per point, two wave-local LDS exchanges (ntt_r16.h)
template <int FZ>
__global__ __launch_bounds__(LSA_R16_THREADS, LSA_R16_WAVES) void k_ntt_r8x3(NttPassArgs a) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    const int tid = threadIdx.x;
    const NttBlockCtx bc = ntt_decode_block(a, (long long)blockIdx.x);
    if (bc.mod == LSA_ROW_SKIP) return;
    u64 v[16];
    r8x3_phase<FZ>(a, bc, tid, lds, 0, v);
    r16_sync<1>();
    r8x3_phase<FZ>(a, bc, tid, lds, 1, v);
    r16_sync<1>();
    r8x3_phase<FZ>(a, bc, tid, lds, 2, v);
    r16_sync<1>();
    r8x3_phase<FZ>(a, bc, tid, lds, 3, v);
}
// The FZ variant of a pass (k_ntt_pass): which fused tail it can execute.  The prologue lives in the pass that holds stage 0,
// the epilogue in the pass that reduces and stores the final values; the product prologue and the pt_mul / rotate-and-MAC
// epilogues come alone.
static int ntt_pass_fz(const NttPassArgs& a, bool fused) {
    const bool pro = fused && a.fz_pro && a.fz_first, epi = fused && a.fz_epi && a.final_reduce;
    if (pro && a.fz_pro == 3) return 16;
    if (epi && a.fz_epi == 3) return 4;
    if (epi && a.fz_epi == 4) return 8;
    return (pro ? 1 : 0) | (epi ? 2 : 0);
}
template <int FZ>
static auto ntt_r16_second_pass(int mu) {
    return mu == 9 ? &k_ntt_r8x3<FZ> : mu == 8 ? &k_ntt_r16<1, FZ, 8> : &k_ntt_r16<1, FZ, 7>;
}
// false: this pass is not covered, the caller takes the staged kernel
static bool ntt_launch_r16(const NttPassArgs& a, int npass, bool fused, long long nblocks, hipStream_t s) {
    if (!sw::ntt_r16() || !ntt_r16_shape_ok(a, npass)) return false;
    const int fz = ntt_pass_fz(a, fused);
    void (*k)(NttPassArgs) = nullptr;
    if (a.lambda) {   // a first pass (seven or eight stages): plain, or the two-operand prologue at eight stages; it is never the
                      // last pass of a two-pass plan, and the product prologue's first executed pass is a second pass
        // the two-operand prologue: 394 us per headline launch here against 450 on the staged kernel once the lift's block-uniform
        // cases became branches (628 before: both lifts were evaluated per element, profiles/r03/ab_r16_prologue_epilogue_branches.log);
        // LSA_R16_PRO=0 keeps it on the staged kernel (A/B)
        // the single-source lift (fz_pro == 4) has a variant of its own, FZ bit 32: one operand, the plain kernel's occupancy
        if (fz == 1 && a.fz_pro == 4 && sw::r16_pro()) k = a.mu == 8 ? &k_ntt_r16<0, 32, 8> : &k_ntt_r16<0, 32, 7>;
        else if (fz == 1 && a.fz_pro != 4 && a.mu == 8 && sw::r16_pro()) k = &k_ntt_r16<0, 1, 8>;
        else if (fz == 0) k = a.mu == 8 ? &k_ntt_r16<0, 0, 8> : &k_ntt_r16<0, 0, 7>;
    } else if (a.mu != 9 || sw::ntt_r8x3()) {   // a second pass; LSA_NTT_R8X3=0: the nine-stage one on the staged kernel (A/B)
        switch (fz) {   // it has no two-operand prologue (FZ 1, 3), and the product prologue belongs to inverse transforms
            case 0: k = ntt_r16_second_pass<0>(a.mu); break;
            case 2: k = ntt_r16_second_pass<2>(a.mu); break;
            case 4: k = ntt_r16_second_pass<4>(a.mu); break;
            case 8: k = ntt_r16_second_pass<8>(a.mu); break;
            case 16: k = a.inverse ? ntt_r16_second_pass<16>(a.mu) : nullptr; break;
        }
    }
    if (!k) return false;
    hipLaunchKernelGGL(k, dim3((unsigned)nblocks), dim3(LSA_R16_THREADS), (size_t)LSA_R16_LDS_WORDS * sizeof(u64), s, a);
    LSA_HIP(hipGetLastError());
    return true;
}

// ---- second pass of the extension transform + key MAC in one launch (ntt_r16.h, "second pass + key MAC")
// grid: (tile, tl, b) with b fastest: consecutive workgroups are consecutive ciphertexts at one (limb, tile) -- they read the
// same key tile within microseconds of each other -- and a CU's resident workgroups mix integer- and FP64-engine limbs
#ifndef LSA_KSMAC_WAVES
#define LSA_KSMAC_WAVES 2   // 32 running sums (64 VGPRs) stay live across the transform phases: at 3 workgroups per CU (168 VGPRs) 76 registers spill
#endif
#ifndef LSA_KSMAC_WAVES_FP
#define LSA_KSMAC_WAVES_FP LSA_KSMAC_WAVES
#endif
// TAIL (FP64-engine Q limbs of a merged ModDown + rescale): after the digits the workgroup transforms the hand-off of in_j for
// both polynomials the same way and stores the rescaled limb from the running sums (KsFusedArgs::tconv, r16_mac_tail) -- two more
// iterations of the digit loop's shape, no register a digit iteration does not hold
template <int MU, bool FP, bool TAIL = false>
__global__ __launch_bounds__(LSA_R16_THREADS, FP ? LSA_KSMAC_WAVES_FP : LSA_KSMAC_WAVES) void k_ntt_r16_ksmac(KsFusedArgs g) {
    static_assert(!TAIL || (FP && MU <= 8), "the tail runs on the FP64 engine's eight- and seven-stage passes");
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    const int tid = threadIdx.x;
    const int T = g.L + g.np;
    long long bid = blockIdx.x;
    long long b;
    if (g.xcd_deal) {   // consecutive workgroup ids go round-robin over the 8 XCDs: the batch of one key tile stays on one
        const long long slot = bid >> 3;
        b = slot % g.batch;
        bid = (slot / g.batch) * 8 + (bid & 7);
    } else {
        b = bid % g.batch;
        bid /= g.batch;
    }
    const int tl = g.tl_list[bid % g.n_tl], tile = (int)(bid / g.n_tl);
    NttPassArgs a;   // only the scalar fields the pass functions read are set (the row tables are never indexed here)
    a.logn = g.logn;
    a.s_lo = g.logn - MU;
    a.mu = MU;
    a.lambda = 0;
    a.tau = 12;
    a.inverse = 0;
    a.apply_scale = 0;
    a.final_reduce = 1;
    a.fp_raw_in = g.fp_raw_in;
    a.fp_raw_out = 0;
    a.mods = g.mods;
    a.tw = g.tw;
    a.twd = g.twd;
    a.scale = nullptr;
    a.scaled = nullptr;
    a.src = g.ext;
    a.fz_pro = a.fz_epi = 0;
    a.fz_first = 0;
    NttBlockCtx bc;
    bc.tile = tile;
    bc.mod = tl < g.L ? tl : g.nq + (tl - g.L);
    bc.fp = FP;   // (the launcher put this limb on the launch of its engine)
    bc.b = (int)b;
    bc.row = 0;
    bc.tw_l = nullptr;
    bc.base_dst = 0;
    const R16Limb L = r16_limb(a, bc);
    const int kj = tl < g.L ? tl : g.klvl + 1 + (tl - g.L);
    const int own_d = tl < g.L ? tl / g.np : -1;
    int k, i;
    r16_lane<1, MU>(tid, k, i);
    const unsigned G1 = r16_G1<1, MU>(bc, k), G2 = (G1 << 4) + ((unsigned)i << (MU <= 8 ? 8 - MU : 0));   // (G2: 8- and 7-stage passes only)
    u64 acc0[16], acc1[16];
#pragma unroll
    for (int e = 0; e < 16; e++) acc0[e] = acc1[e] = 0;   // (0 is also +0.0)
    // FP64 engine, eight- and seven-stage passes: the transforms' twiddles come from the workgroup's LDS copy behind the tile image
    // (ntt_r16.h, "twiddles once per workgroup"); the other instantiations fetch them per transform as they did
    constexpr bool TWC = ks_fused_twc(MU, FP);
    double* const twc = reinterpret_cast<double*>(lds + LSA_R16_LDS_WORDS);
    if constexpr (TWC) {
        r16_twc_fill<MU>(twc, tid, L, G1, G2);
        r16_sync<1>();   // (a wave reads only what it wrote)
    }
    for (int d = 0; d < g.beta; d++) {
        const bool own = d == own_d;
        if (!own) {
            bc.base_src = b * g.sext + ((long long)(d * T + tl) << g.logn);
            bc.row = d * T + tl;
            u64 v[16];
            r16_load_direct<1, false, 0, MU>(a, bc, tid, v);
            if constexpr (MU == 9) {   // nine stages: three radix-8 groups per point, two exchanges (ntt_r16.h)
                r8x3_group<0>(v, a, bc, L, G1, i);
                r8x3_put<0>(k, i, lds, v);
                r16_sync<1>();
                r8x3_get<1>(k, i, lds, v);
                r8x3_group<1>(v, a, bc, L, G1, i);
                r8x3_put<1>(k, i, lds, v);
                r16_sync<1>();
                r8x3_get<2>(k, i, lds, v);
                r8x3_group<2>(v, a, bc, L, G1, i);
                r8x3_put<2>(k, i, lds, v);
            } else if constexpr (TWC) {
                double w[15];
                r16_twc_get<MU, 0>(twc, tid, w);
                r16_group_twc<0, MU>(v, false, L, w);
                r16_lds_put<1, 0, MU>(tid, lds, v);
                r16_sync<1>();
                r16_twc_get<MU, 1>(twc, tid, w);
                r16_lds_get<1, 1, MU>(tid, lds, v);
                r16_group_twc<1, MU>(v, false, L, w);
                r16_lds_put<1, 1, MU>(tid, lds, v);
            } else {
                r16_group<1, 0, MU>(v, a, bc, L, G1);
                r16_lds_put<1, 0, MU>(tid, lds, v);
                r16_sync<1>();
                r16_lds_get<1, 1, MU>(tid, lds, v);
                r16_group<1, 1, MU>(v, a, bc, L, G2);
                r16_lds_put<1, 1, MU>(tid, lds, v);
            }
            r16_sync<1>();
        }
        r16_mac_digit<MU, FP>(g, a, bc, L, tid, d, kj, own, b, tl, lds, acc0, acc1);
        r16_sync<1>();   // the next digit's first exchange overwrites the tile image these lanes just read
    }
    if constexpr (TAIL) {
        a.src = g.tconv;
        // the tail's addresses are derived from copies of the lane, limb and batch indices that the compiler cannot see through:
        // from the originals it forms them ahead of the digit loop, next to the loop's own, and carries them through it in
        // registers the loop needs (MU = 8: 14 VGPRs spilled around the whole loop, MU = 7: 34; none this way)
        int tt = tid, ttl = tl;
        long long tb = b;
        asm volatile("" : "+v"(tt), "+s"(ttl), "+s"(tb));
        int tk, ti;   // (the twiddle groups too: the per-lane table addresses formed from them are 64-bit values)
        r16_lane<1, MU>(tt, tk, ti);
        const unsigned T1 = r16_G1<1, MU>(bc, tk), T2 = (T1 << 4) + ((unsigned)ti << (8 - MU));
        const double kd = g.tkd[ttl], k2d = g.tkd[g.L - 1 + ttl];   // P^-1 and q_l^-1 of this limb, the values the epilogue pass takes
        // (a loop that is not unrolled, the second polynomial's sums moved into the first's registers for its turn: unrolled, the
        // compiler starts the second polynomial's loads under the first one's tail and the kernel spills)
#pragma unroll 1
        for (int h = 0; h < 2; h++) {
            bc.row = h * g.L + ttl;
            bc.base_src = tb * g.stconv + ((long long)bc.row << g.logn);
            u64 v[16];
            r16_load_direct<1, false, 0, MU>(a, bc, tt, v);
            if constexpr (TWC) {
                double w[15];
                r16_twc_get<MU, 0>(twc, tt, w);
                r16_group_twc<0, MU>(v, false, L, w);
                r16_lds_put<1, 0, MU>(tt, lds, v);
                r16_sync<1>();
                r16_twc_get<MU, 1>(twc, tt, w);
                r16_lds_get<1, 1, MU>(tt, lds, v);
                r16_group_twc<1, MU>(v, false, L, w);
                r16_lds_put<1, 1, MU>(tt, lds, v);
            } else {
                r16_group<1, 0, MU>(v, a, bc, L, T1);
                r16_lds_put<1, 0, MU>(tt, lds, v);
                r16_sync<1>();
                r16_lds_get<1, 1, MU>(tt, lds, v);
                r16_group<1, 1, MU>(v, a, bc, L, T2);
                r16_lds_put<1, 1, MU>(tt, lds, v);
            }
            r16_sync<1>();
            r16_mac_tail<MU>(g, a, bc, L, tt, tb, ttl, h, kd, k2d, lds, acc0);
            r16_sync<1>();
#pragma unroll
            for (int e = 0; e < 16; e++) acc0[e] = acc1[e];
        }
        return;
    }
    r16_mac_store<MU, FP>(g, a, bc, L, tid, b, tl, acc0, acc1);
}

// image + twiddle cache: above 64 KiB of dynamic LDS the kernel instance opts in, once per instance AND device (as ntt_launch_variant)
template <int MU, bool FP, bool TAIL = false>
static void ks_fused_launch(dim3 grid, dim3 block, hipStream_t s, const KsFusedArgs& g) {
    constexpr size_t lds_bytes = ks_fused_lds_bytes(MU, FP);
    raise_dynamic_lds<&k_ntt_r16_ksmac<MU, FP, TAIL>>(lds_bytes, (int)lds_bytes);
    hipLaunchKernelGGL((k_ntt_r16_ksmac<MU, FP, TAIL>), grid, block, lds_bytes, s, g);
}

bool ks_fused_enabled(const Context& c) {
    // (a key uploaded under either setting works with both: the fused path needs key.fp and is skipped without it)
    if (!sw::ks_fused() || c.plan.npass != 2 || !c.fp_raw) return false;
    const NttPassShape& p = c.plan.pass[1];
    return p.tau == 12 && p.lambda == 0 && (p.mu == 7 || p.mu == 8 || p.mu == 9) && p.s_lo == c.logn - p.mu;
}

int ks_fused_engines(const Context& c) {
    // integer-engine target limbs measured slower fused than apart (two lazy REDCs per product and digit, 256 VGPRs and still
    // spilling: 593 us against ~500 for pass + MAC on the headline's 5 integer limbs), FP64-engine limbs faster (643 us for 36
    // transforms + their MAC against ~1050): profiles/r03/ab_ks_fused_kernel_stats.log
    return c.fp64_ntt ? sw::ks_fused_engines() : 0;
}

bool ks_fused_limb(const Context& c, int L, int tl) { return (ks_fused_engines(c) >> (c.fp_engine(c.qp_mod(L, tl)) ? 1 : 0)) & 1; }

bool launch_ntt_ksmac(Context& c, int level, const u64* cx, long long scx, u64* ext, long long sext, const Key& key, u64* acc,
                      long long sacc, int batch, hipStream_t s, const TensorFold* fold, KsFusedLimbs limbs, const KsTailOperands* tail) {
    if (batch <= 0) return true;
    if (!ks_fused_enabled(c) || (c.fp64_ntt && !key.fp)) return false;
    LSA_REQUIRE(key.level >= level, "key-switch key exported at a lower level than the ciphertext");
    LSA_REQUIRE((limbs == KS_FUSED_Q_TAIL) == (tail != nullptr), "fused key MAC: the tail launch and its operands go together");
    if (tail && (level < 1 || ks_fused_engines(c) != 2 || c.plan.pass[1].mu > 8)) return false;
    KsFusedArgs g{};
    if (tail) {
        g.tconv = tail->conv;
        g.stconv = tail->sconv;
        g.tout = tail->out;
        g.stout = tail->sout;
        g.tkd = reinterpret_cast<const double*>(c.tail_fp_vec(level));
    }
    g.ext = ext;
    g.cx = cx;
    g.key = key.data;
    g.keyd = key.fp;
    g.acc = acc;
    g.sext = sext;
    g.scx = scx;
    g.sacc = sacc;
    g.mods = c.d_mods;
    g.tw = c.d_psi;
    g.twd = c.d_psi_d;
    g.logn = c.logn;
    g.L = level + 1;
    g.np = c.np;
    g.nq = c.nq;
    g.beta = (g.L + c.np - 1) / c.np;
    g.klvl = key.level;
    g.kcomp = key.level + 1 + c.np;
    g.batch = batch;
    g.allow_fp64 = c.fp64_ntt;
    g.fp_raw_in = c.fp_raw;
    if (fold) {
        g.fa = fold->a;
        g.fb = fold->b;
        g.sfa = fold->sa;
        g.sfb = fold->sb;
        g.pfa = fold->pa;
        g.pfb = fold->pb;
        g.pf = c.pfold_vec(level);
    }
    const int T = g.L + c.np, mu = c.plan.pass[1].mu;
    LSA_REQUIRE(T <= 64, "fused key MAC: too many target limbs");
    // one launch per butterfly engine (own register budget each); bytes: one pass of the launch's extension transforms
    // (16 N / 2 per limb) + its share of the gadget inner product as launch_ks_mac counts it
    for (int eng = 0; eng < 2; eng++) {
        g.n_tl = 0;
        int transforms = 0, q_targets = 0;
        for (int tl = 0; tl < T; tl++) {
            if (!ks_fused_limb(c, g.L, tl) || (int)c.fp_engine(c.qp_mod(g.L, tl)) != eng) continue;
            if (limbs == KS_FUSED_P && tl < g.L) continue;
            if (limbs == KS_FUSED_Q_TAIL && tl >= level) continue;
            g.tl_list[g.n_tl++] = (unsigned char)tl;
            transforms += g.beta - (tl < g.L ? 1 : 0);
            q_targets += tl < g.L;
        }
        if (!g.n_tl) continue;
        const long long nblocks = (long long)batch * g.n_tl * (1 << (c.logn - 12));
        LSA_REQUIRE(nblocks < (1LL << 31), "ntt: grid too large");
        // LSA_KSMAC_XCD=0: plain batch-fastest order (A/B: +0.45 % headline with the deal, ab_ksmac_xcd_deal.log)
        g.xcd_deal = sw::ksmac_xcd() && ((g.n_tl << (c.logn - 12)) % 8 == 0) ? 1 : 0;
        // (the tail launch: the second pass of two more transforms per limb, as the epilogue pass it replaces counted them, and no
        // accumulator rows: the MAC's two writes per limb are gone, and the epilogue never counted its reads of them)
        if (tail) transforms += 2 * g.n_tl;
        const double ntt_bytes = 16.0 * c.n * transforms * batch / 2;
        // (tensor fold: the own digit of a Q target reads a0, a1, b0, b1 instead of cx)
        const double fold_bytes = fold ? 3.0 * 8 * c.n * q_targets * batch : 0.0;
        ProfScope ps(c, PROF_NTT, ntt_bytes + fold_bytes + 8.0 * c.n * g.n_tl * (batch * ((double)g.beta + (tail ? 0.0 : 2.0)) + 2.0 * g.beta), s,
                     ntt_bytes);
        const dim3 grid((unsigned)nblocks), block(LSA_R16_THREADS);
        if (tail) {
            LSA_REQUIRE(eng == 1 && (mu == 8 || mu == 7), "fused key MAC: the tail runs on the FP64 engine's eight- and seven-stage passes");
            if (mu == 8) ks_fused_launch<8, true, true>(grid, block, s, g);
            else ks_fused_launch<7, true, true>(grid, block, s, g);
        } else if (mu == 9 && eng) ks_fused_launch<9, true>(grid, block, s, g);
        else if (mu == 9) ks_fused_launch<9, false>(grid, block, s, g);
        else if (mu == 8 && eng) ks_fused_launch<8, true>(grid, block, s, g);
        else if (mu == 8) ks_fused_launch<8, false>(grid, block, s, g);
        else if (eng) ks_fused_launch<7, true>(grid, block, s, g);
        else ks_fused_launch<7, false>(grid, block, s, g);
    }
    LSA_HIP(hipGetLastError());
    return true;
}

template <int FZ, int NT>
static void ntt_launch_variant(const NttPassArgs& a, long long nblocks, size_t lds_bytes, hipStream_t s) {
    raise_dynamic_lds<&k_ntt_pass<FZ, NT>>(lds_bytes, 160 * 1024);   // whole-limb tiles
    hipLaunchKernelGGL((k_ntt_pass<FZ, NT>), dim3((unsigned)nblocks), dim3(NT), lds_bytes, s, a);
    LSA_HIP(hipGetLastError());
}

template <int NT>
static void ntt_launch_pass(const NttPassArgs& a, bool fused, long long nblocks, size_t lds_bytes, hipStream_t s) {
    LSA_REQUIRE((1 << a.tau) <= 2 * LSA_NTT_STAGE_PAIRS * NT, "ntt: tile larger than the staging registers");
    switch (ntt_pass_fz(a, fused)) {
        case 0: ntt_launch_variant<0, NT>(a, nblocks, lds_bytes, s); break;
        case 1: ntt_launch_variant<1, NT>(a, nblocks, lds_bytes, s); break;
        case 2: ntt_launch_variant<2, NT>(a, nblocks, lds_bytes, s); break;
        case 3: ntt_launch_variant<3, NT>(a, nblocks, lds_bytes, s); break;
        case 4: ntt_launch_variant<4, NT>(a, nblocks, lds_bytes, s); break;
        case 8: ntt_launch_variant<8, NT>(a, nblocks, lds_bytes, s); break;
        default:   // 16, the product prologue: only tiles of the two-pass shape take it
            if constexpr (NT == LSA_NTT_THREADS) ntt_launch_variant<16, NT>(a, nblocks, lds_bytes, s);
            else LSA_REQUIRE(false, "ntt: the product prologue needs a tile of at most 4096 points");
    }
}

void launch_ntt(Context& c, const u64* src, u64* dst, int batch, long long batch_stride, int rows, const RowMap& rm,
                bool inverse, hipStream_t s) {
    launch_ntt(c, src, dst, batch, batch_stride, batch_stride, rows, rm, inverse, s);
}

void launch_ntt(Context& c, const u64* src, u64* dst, int batch, long long src_stride, long long dst_stride, int rows,
                const RowMap& rm, bool inverse, hipStream_t s, const NttFusion* fz, int passes) {
    if (batch <= 0 || rows <= 0) return;
    LSA_REQUIRE(rm.period >= 1 && rm.period <= LSA_MAX_PERIOD, "ntt: bad row-map period");
    NttPassArgs a{};
    a.batch = batch;
    a.rows = rows;
    a.mods = c.d_mods;
    a.scale = c.d_scale;
    a.diag = c.ntt_diag;
    a.scaled = c.d_scale_d;
    a.allow_fp64 = c.fp64_ntt;
    if (fz) {
        // inverse transforms take the product prologue and nothing else; it forms its input in the first executed pass
        LSA_REQUIRE(!inverse || (fz->pro == 3 && !fz->epi), "inverse transforms take the product prologue only");
        LSA_REQUIRE(fz->pro != 3 || (inverse && !fz->epi && fz->a && fz->b && fz->limbs >= 1 && (passes & 1)),
                    "product prologue: an inverse transform from its first pass, two operands, no epilogue");
        LSA_REQUIRE(fz->pro != 4 || (!inverse && !fz->epi && fz->last && fz->limbs >= 1 && (passes & 1)),
                    "lift prologue: a forward transform from its first pass, one source row per polynomial, no epilogue");
        a.fz_epi = fz->epi;
        a.fz_pro = fz->pro;
        a.fz_limbs = fz->limbs;
        a.fz_base_polys = fz->base_polys;
        a.fz_ql_mod = fz->ql_mod;
        a.fz_a = fz->a;
        a.fz_a_stride = fz->a_stride;
        a.fz_a_rpp = fz->a_rpp;
        a.fz_base = fz->base;
        a.fz_base_stride = fz->base_stride;
        a.fz_base_rpp = fz->base_rpp;
        a.fz_k = fz->k;
        a.fz_out = fz->out;
        a.fz_out_stride = fz->out_stride;
        a.fz_out_rpp = fz->out_rpp;
        a.fz_last = fz->last;
        a.fz_last_stride = fz->last_stride;
        a.fz_last_rpp = fz->last_rpp;
        a.fz_k2 = fz->k2;
        a.fz_scatter = fz->scatter;
        LSA_REQUIRE(fz->epi != 2 || fz->k2, "merged tail needs its second factor");
        LSA_REQUIRE(!fz->scatter || fz->epi, "a scattered store needs an epilogue");
        LSA_REQUIRE(fz->epi != 3 || (!fz->pro && !fz->scatter && fz->a && fz->out), "pt_mul epilogue: plaintext and output, nothing else");
        LSA_REQUIRE(fz->epi != 4 || (!fz->pro && !fz->k2 && fz->scatter && fz->a && fz->k && fz->out && fz->pt),
                    "rotate-and-MAC epilogue: ModDown operands, index map, plaintext and output");
        LSA_REQUIRE(fz->epi != 4 || (fz->base_polys <= 1 && fz->limbs == rm.period), "rotate-and-MAC epilogue: base on poly 0, one row per limb");
        a.fz_pt = fz->pt;
        a.fz_pt_stride = fz->pt_stride;
        a.fz_accum = fz->accumulate ? 1 : 0;
        a.fz_b = fz->b;
        a.fz_b_stride = fz->b_stride;
        a.fz_b_rpp = fz->b_rpp;
    }
    a.period = rm.period;
    a.row0 = rm.row0;
    a.row_step = rm.row_step;
    for (int i = 0; i < rm.period; i++) {
        LSA_REQUIRE(rm.mod_of[i] == LSA_ROW_SKIP || rm.mod_of[i] < c.nmod, "ntt: modulus index out of range");
        a.mod_of[i] = rm.mod_of[i];
    }
    int active_rows = 0;
    for (int r = 0; r < rows; r++) active_rows += rm.mod_of[(rm.row0 + r * rm.row_step) % rm.period] != LSA_ROW_SKIP;
    if (active_rows == 0) return;
    // the grid covers the active rows only
    int launch_rows = rows;
    a.compact = 0;
    if (active_rows <= LSA_MAX_PERIOD && rm.row0 + (rows - 1) * rm.row_step < 65536) {
        a.compact = 1;
        int k = 0;
        for (int r = 0; r < rows; r++) {
            const int row = rm.row0 + r * rm.row_step;
            if (rm.mod_of[row % rm.period] != LSA_ROW_SKIP) a.row_tbl[k++] = (unsigned short)row;
        }
        launch_rows = active_rows;
    }
    a.rows = launch_rows;
    // Two-pass transforms: run both passes on a chunk of the batch that fits the 256 MiB Infinity Cache before moving
    // on, so the second pass reads what the first just wrote from the memory-side cache instead of HBM.
    // whole-limb single pass (N = 2^13 / 2^14) where it measured faster: launches that fill the chip at one (2^14) or two
    // (2^13) workgroups per CU, without fused tails (at 1024 threads their registers spill); at 2^14 only limbs of the
    // FP64 engine -- the integer engine is bound by its multiplies there, not by traffic (tools/probe_wide.py)
    bool wide = c.plan_wide.npass < c.plan.npass && c.wide_mode != 0;
    if (wide && c.wide_mode == 2) {
        bool all_fp = c.fp64_ntt != 0;
        for (int r = 0; r < rows && all_fp; r++) {
            const unsigned char m = rm.mod_of[(rm.row0 + r * rm.row_step) % rm.period];
            if (m != LSA_ROW_SKIP && (c.T.mods[m].q >> LSA_FP64_MAX_BITS) != 0) all_fp = false;
        }
        const long long limbs = (long long)active_rows * batch;
        wide = !fz && (c.logn == 13 ? limbs >= 1024 : (all_fp && limbs >= 512));
    }
    if (passes != 3) wide = false;   // a caller that runs the passes separately means the two-pass plan
    if (fz && fz->pro == 3) wide = false;   // (the product prologue has no whole-limb kernel)
    const NttPlan& plan = wide ? c.plan_wide : c.plan;
    a.tw = wide ? (inverse ? c.d_psiinv_w : c.d_psi_w) : (inverse ? c.d_psiinv : c.d_psi);
    a.twd = wide ? (inverse ? c.d_psiinv_d_w : c.d_psi_d_w) : (inverse ? c.d_psiinv_d : c.d_psi_d);
    {   // launches that mix both butterfly engines interleave their limbs (+1.4 % hmult / +2.2 % rotate NTT rate, profiles/r01/ab_row_inner.log)
        bool any_fp = false, any_int = false;
        for (int r = 0; r < rows; r++) {
            const unsigned char m = rm.mod_of[(rm.row0 + r * rm.row_step) % rm.period];
            if (m == LSA_ROW_SKIP) continue;
            const bool fp = c.fp_engine(m);
            any_fp |= fp;
            any_int |= !fp;
        }
        a.row_inner = any_fp && any_int;
        // the lift prologue: every row of a (polynomial, tile) reads the same source tile -- they run next to each other
        // (-DLSA_LIFT_ROW_OUTER: the (row, tile, batch) order for A/B, profiles/r09/ab_lift_row_order.log)
#if defined(LSA_LIFT_ROW_OUTER)
        if (fz && fz->pro == 4) a.row_inner = 0;
#else
        if (fz && fz->pro == 4) a.row_inner = 1;
#endif
    }
    // (every fused operand follows its chunk -- block batch indices restart at 0 -- through the one function of ntt_chunk.h)
    const int chunk = plan.npass > 1 ? ntt_chunk_items(c.n, active_rows, batch, c.ntt_chunk_mib) : batch;
    const NttPassArgs whole = a;
    for (int b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = std::min(chunk, batch - b0);
        a = ntt_chunk_rebase(whole, b0);
        a.batch = nb;
        bool first = true;
        for (int step = 0; step < plan.npass; step++) {
            if (plan.npass == 2 && !((passes >> step) & 1)) continue;
            a.fz_first = first ? 1 : 0;   // the prologue's pass: the transform's first EXECUTED pass, forward or inverse
            first = false;
            const int k = inverse ? plan.npass - 1 - step : step;
            ntt_fill_pass(a, plan, c.logn, k, inverse ? 1 : 0);
            a.fp_raw_out = plan.npass == 2 && step == 0 && c.fp_raw;
            a.fp_raw_in = plan.npass == 2 && step == 1 && c.fp_raw;
            LSA_REQUIRE(!(a.fz_first && a.fz_pro && a.fp_raw_in), "ntt: a fused prologue reads canonical inputs, never a raw hand-off");
            a.src = (step == 0 ? src + (long long)b0 * src_stride : dst + (long long)b0 * dst_stride);
            a.src_stride = step == 0 ? src_stride : dst_stride;
            a.dst = dst + (long long)b0 * dst_stride;
            a.dst_stride = dst_stride;
            a.total_tiles = (long long)nb * launch_rows * (1 << (a.logn - a.tau));
            const long long nblocks = a.total_tiles;
            LSA_REQUIRE(nblocks < (1LL << 31), "ntt: grid too large");
            const size_t lds_bytes = (size_t)lds_words(a.tau) * sizeof(u64);
            // one launch = one pass = 1/npass of the limb transforms it touches (algorithmic 16*N bytes per transform)
            // (+ the product prologue's second operand: two 8 N reads in place of one)
            const double pro_bytes = fz && fz->pro == 3 && a.fz_first ? 8.0 * c.n * active_rows * nb : 0.0;
            ProfScope ps(c, PROF_NTT, 16.0 * c.n * active_rows * nb / plan.npass + pro_bytes, s);
            if (ntt_launch_r16(a, plan.npass, fz != nullptr, nblocks, s)) continue;
            if (a.tau <= 12) ntt_launch_pass<LSA_NTT_THREADS>(a, fz != nullptr, nblocks, lds_bytes, s);
            else if (a.tau == 13) ntt_launch_pass<512>(a, fz != nullptr, nblocks, lds_bytes, s);
            else ntt_launch_pass<1024>(a, fz != nullptr, nblocks, lds_bytes, s);
        }
    }
}

// ------------------------------------------------------------------------------------------------ elementwise (K3/K4)
struct EwArgs {
    const u64* a;
    const u64* b;
    const u64* acc;   // EW_MUL only: optional accumulator operand
    u64* out;
    long long sa, sb, so, sacc;
    const ModDev* mods;
    int rows, logn, op, period;
    unsigned char mod_of[LSA_MAX_PERIOD];
};

// grid: x = rows * (N/2/TPB), y = batch
__global__ __launch_bounds__(TPB) void k_elementwise(EwArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int row = blockIdx.x / chunks;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const int mi = g.mod_of[row % g.period];
    if (mi == LSA_ROW_SKIP) return;
    const ModDev m = g.mods[mi];
    const long long off = ((long long)row << g.logn) + x;
    const long long b = blockIdx.y;
    const ulonglong2 va = ld2(g.a + b * g.sa + off);
    u64 r0, r1;
    if (g.op == EW_NEG) {
        r0 = neg_mod(va.x, m.q);
        r1 = neg_mod(va.y, m.q);
    } else {
        const ulonglong2 vb = ld2(g.b + b * g.sb + off);
        if (g.op == EW_ADD) {
            r0 = add_mod(va.x, vb.x, m.q);
            r1 = add_mod(va.y, vb.y, m.q);
        } else if (g.op == EW_SUB) {
            r0 = sub_mod(va.x, vb.x, m.q);
            r1 = sub_mod(va.y, vb.y, m.q);
        } else {
            r0 = mul_mod(va.x, vb.x, m);
            r1 = mul_mod(va.y, vb.y, m);
            if (g.acc) {   // multiply-accumulate: out = acc + a*b
                const ulonglong2 vc = ld2(g.acc + b * g.sacc + off);
                r0 = add_mod(r0, vc.x, m.q);
                r1 = add_mod(r1, vc.y, m.q);
            }
        }
    }
    st2(g.out + b * g.so + off, r0, r1);
}

static void fill_rowmap(unsigned char* dst, int& period, const RowMap& rm, int nmod) {
    LSA_REQUIRE(rm.period >= 1 && rm.period <= LSA_MAX_PERIOD, "bad row-map period");
    period = rm.period;
    for (int i = 0; i < rm.period; i++) {
        LSA_REQUIRE(rm.mod_of[i] == LSA_ROW_SKIP || rm.mod_of[i] < nmod, "modulus index out of range");
        dst[i] = rm.mod_of[i];
    }
}

static dim3 ew_grid(const Context& c, int rows, int batch) {
    LSA_REQUIRE(c.n >= 2 * TPB, "ring degree too small for the elementwise kernels (need N >= 512)");
    return dim3((unsigned)(rows * (c.n / (2 * TPB))), (unsigned)batch);
}

void launch_elementwise(Context& c, EwOp op, const u64* a, const u64* b, u64* out, int batch, long long sa, long long sb,
                        long long so, int rows, const RowMap& rm, hipStream_t s) {
    launch_muladd(c, op, a, b, nullptr, 0, out, batch, sa, sb, so, rows, rm, s);
}

// out = op(a, b) (+ acc for EW_MUL when acc != nullptr)
void launch_muladd(Context& c, EwOp op, const u64* a, const u64* b, const u64* acc, long long sacc, u64* out, int batch,
                   long long sa, long long sb, long long so, int rows, const RowMap& rm, hipStream_t s) {
    if (batch <= 0 || rows <= 0) return;
    EwArgs g{};
    g.acc = acc;
    g.sacc = sacc;
    g.a = a;
    g.b = b;
    g.out = out;
    g.sa = sa;
    g.sb = sb;
    g.so = so;
    g.mods = c.d_mods;
    g.rows = rows;
    g.logn = c.logn;
    g.op = op;
    fill_rowmap(g.mod_of, g.period, rm, c.nmod);
    ProfScope ps(c, PROF_ELEMWISE, 24.0 * c.n * rows * batch, s);
    hipLaunchKernelGGL(k_elementwise, ew_grid(c, rows, batch), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

// out[b][row] = a[b][row] * mvec[row] + kvec[row]: a real constant added to every slot is the same residue in every NTT
// coefficient of c0 (kvec: plain residues, one per row; mvec: optional Montgomery-form factors, null = 1)
struct AddConstArgs {
    const u64* a;
    u64* out;
    const u64* kvec;
    const u64* mvec;
    long long sa, so;
    const ModDev* mods;
    int logn;
    unsigned char mod_of[LSA_MAX_PERIOD];
};
__global__ __launch_bounds__(TPB) void k_add_const(AddConstArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int row = blockIdx.x / chunks;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const ModDev m = g.mods[g.mod_of[row]];
    const u64 k = g.kvec[row];
    const long long b = blockIdx.y, off = ((long long)row << g.logn) + x;
    ulonglong2 v = ld2(g.a + b * g.sa + off);
    if (g.mvec) {
        const u64 f = g.mvec[row];
        v.x = mont_mul(v.x, f, m.q, m.qinv);
        v.y = mont_mul(v.y, f, m.q, m.qinv);
    }
    st2(g.out + b * g.so + off, add_mod(v.x, k, m.q), add_mod(v.y, k, m.q));
}
void launch_add_const(Context& c, const u64* a, long long sa, const u64* kvec, u64* out, long long so, int rows,
                      const RowMap& rm, int batch, hipStream_t s, const u64* mvec) {
    if (batch <= 0 || rows <= 0) return;
    LSA_REQUIRE(rm.period == rows && rows <= LSA_MAX_PERIOD, "add_const: row map must cover the rows");
    AddConstArgs g{};
    g.a = a;
    g.out = out;
    g.kvec = kvec;
    g.mvec = mvec;
    g.sa = sa;
    g.so = so;
    g.mods = c.d_mods;
    g.logn = c.logn;
    int period;
    fill_rowmap(g.mod_of, period, rm, c.nmod);
    ProfScope ps(c, PROF_ELEMWISE, 16.0 * c.n * rows * batch, s);
    hipLaunchKernelGGL(k_add_const, ew_grid(c, rows, batch), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

// ciphertext x plaintext multiply-accumulate over up to LSA_MAC_MAX_TERMS terms in ONE launch (cmp_sum / cmpac_sum nodes,
// mega_ag_executors_gpu.cu:294-408 does multiply_plain + add_inplace per term):
//   out[p][j] = (partial[p][j]) + sum_i ct_i[p][j] * pt_i[j]
// The products are summed as 128-bit integers and reduced once (REDC, then * R^2), folded every 8 terms.
struct MacPlainArgs {
    const u64* ct[LSA_MAC_MAX_TERMS];
    const u64* pt[LSA_MAC_MAX_TERMS];
    long long sct[LSA_MAC_MAX_TERMS], spt[LSA_MAC_MAX_TERMS];
    const u64* partial;
    u64* out;
    long long spartial, so;
    const ModDev* mods;
    int terms, polys, limbs, logn;
    unsigned char mod_of[LSA_MAX_PERIOD];
};

// grid: x = polys*limbs*(N/2/TPB), y = batch
__global__ __launch_bounds__(TPB) void k_mac_plain(MacPlainArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int row = blockIdx.x / chunks;             // poly * limbs + limb
    const int limb = row % g.limbs;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const ModDev m = g.mods[g.mod_of[limb]];
    const long long b = blockIdx.y;
    const long long coff = ((long long)row << g.logn) + x, poff = ((long long)limb << g.logn) + x;
    u64 h0 = 0, l0 = 0, h1 = 0, l1 = 0, r0 = 0, r1 = 0;
    for (int i = 0; i < g.terms; i++) {
        const ulonglong2 c = ld2(g.ct[i] + b * g.sct[i] + coff);
        const ulonglong2 w = ld2(g.pt[i] + b * g.spt[i] + poff);
        mac128(h0, l0, c.x, w.x);
        mac128(h1, l1, c.y, w.y);
        if ((i & 7) == 7) {   // keep the 128-bit sum below q*2^64 (8 products of < q^2, q < 2^61)
            r0 = add_mod(r0, csub(mont_redc_lazy(h0, l0, m.q, m.qinv), m.q), m.q);
            r1 = add_mod(r1, csub(mont_redc_lazy(h1, l1, m.q, m.qinv), m.q), m.q);
            h0 = l0 = h1 = l1 = 0;
        }
    }
    r0 = add_mod(r0, csub(mont_redc_lazy(h0, l0, m.q, m.qinv), m.q), m.q);
    r1 = add_mod(r1, csub(mont_redc_lazy(h1, l1, m.q, m.qinv), m.q), m.q);
    r0 = mont_mul(r0, m.r2, m.q, m.qinv);            // sum * R^-1 -> sum
    r1 = mont_mul(r1, m.r2, m.q, m.qinv);
    if (g.partial) {
        const ulonglong2 v = ld2(g.partial + b * g.spartial + coff);
        r0 = add_mod(r0, v.x, m.q);
        r1 = add_mod(r1, v.y, m.q);
    }
    st2(g.out + b * g.so + coff, r0, r1);
}

void launch_mac_plain(Context& c, int terms, const u64* const* ct, const long long* sct, const u64* const* pt,
                      const long long* spt, const u64* partial, long long spartial, u64* out, long long so, int batch,
                      int polys, int limbs, const RowMap& rm, hipStream_t s) {
    if (batch <= 0 || terms <= 0) return;
    LSA_REQUIRE(terms <= LSA_MAC_MAX_TERMS, "too many terms for one multiply-accumulate launch");
    LSA_REQUIRE(rm.period == limbs && limbs <= LSA_MAX_PERIOD, "mac: row map must cover the limbs");
    MacPlainArgs g{};
    for (int i = 0; i < terms; i++) {
        g.ct[i] = ct[i];
        g.sct[i] = sct[i];
        g.pt[i] = pt[i];
        g.spt[i] = spt[i];
    }
    g.partial = partial;
    g.spartial = spartial;
    g.out = out;
    g.so = so;
    g.mods = c.d_mods;
    g.terms = terms;
    g.polys = polys;
    g.limbs = limbs;
    g.logn = c.logn;
    int period;
    fill_rowmap(g.mod_of, period, rm, c.nmod);
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * limbs * batch * ((double)terms * (polys + 1) + polys * (partial ? 2 : 1)), s);
    hipLaunchKernelGGL(k_mac_plain, ew_grid(c, polys * limbs, batch), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

// BFV ct x pt_mul, unfused form (the fused one is the forward transform's fz_epi == 3 epilogue):
// out[p][j] = a[p][j] * pt[j] * 2^-64 mod q (+ acc[p][j]) for every poly p of [batch][polys][limbs][N]; the pt_mul plaintext
// is in Montgomery form, so one Montgomery product is the whole multiply.  acc and a may be out.
struct MontMulArgs {
    const u64* a;
    const u64* pt;
    const u64* acc;
    u64* out;
    long long sa, spt, sacc, so;
    const ModDev* mods;
    int limbs, logn;
    unsigned char mod_of[LSA_MAX_PERIOD];
};
__global__ __launch_bounds__(TPB) void k_mont_muladd(MontMulArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int row = blockIdx.x / chunks;             // poly * limbs + limb
    const int limb = row % g.limbs;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const ModDev m = g.mods[g.mod_of[limb]];
    const long long b = blockIdx.y;
    const long long off = ((long long)row << g.logn) + x;
    const ulonglong2 va = ld2(g.a + b * g.sa + off);
    const ulonglong2 w = ld2(g.pt + b * g.spt + ((long long)limb << g.logn) + x);
    u64 r0 = mont_mul(va.x, w.x, m.q, m.qinv), r1 = mont_mul(va.y, w.y, m.q, m.qinv);
    if (g.acc) {
        const ulonglong2 vc = ld2(g.acc + b * g.sacc + off);
        r0 = add_mod(r0, vc.x, m.q);
        r1 = add_mod(r1, vc.y, m.q);
    }
    st2(g.out + b * g.so + off, r0, r1);
}

void launch_mont_muladd(Context& c, const u64* a, long long sa, const u64* pt, long long spt, const u64* acc, long long sacc,
                        u64* out, long long so, int batch, int polys, int limbs, const RowMap& rm, hipStream_t s) {
    if (batch <= 0) return;
    LSA_REQUIRE(rm.period == limbs && limbs <= LSA_MAX_PERIOD, "mont_muladd: row map must cover the limbs");
    MontMulArgs g{};
    g.a = a;
    g.pt = pt;
    g.acc = acc;
    g.out = out;
    g.sa = sa;
    g.spt = spt;
    g.sacc = sacc;
    g.so = so;
    g.mods = c.d_mods;
    g.limbs = limbs;
    g.logn = c.logn;
    int period;
    fill_rowmap(g.mod_of, period, rm, c.nmod);
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * limbs * batch * (polys * (acc ? 3.0 : 2.0) + 1.0), s);
    hipLaunchKernelGGL(k_mont_muladd, ew_grid(c, polys * limbs, batch), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

// The inner sums of a baby-step / giant-step linear transform in ONE launch: out[g] = sum_b ct[b] * pt[g][b] for every giant
// step g.  Each baby-step ciphertext is read once for all giant steps (k_mac_plain, one launch per giant step, re-reads all of
// them every time): nb*polys + terms + ng*polys limb streams instead of terms*(polys + 1) + ng*polys.
// ACC (k_mac_plain_multi<POLYS, true>): out[g] += the same sums -- the launch is one 8 x 8 block of a wider matrix and adds to
// what the previous baby-step block left (LtEval::inner_sums): nb baby and ng giant steps then cost ceil(nb/8) * ceil(ng/8)
// launches, every baby-step ciphertext read ceil(ng/8) times instead of ng times, every plaintext once.
struct MacPlainMultiArgs {
    const u64* ct[LSA_MACM_MAX];
    long long sct[LSA_MACM_MAX];
    const u64* pt[LSA_MACM_MAX][LSA_MACM_MAX];   // [giant][baby], null = no such diagonal; shared by the batch
    u64* out[LSA_MACM_MAX];
    long long so;
    const ModDev* mods;
    int nb, ng, polys, limbs, logn, batch, xcd_map;
    unsigned char mod_of[LSA_MAX_PERIOD];
};

// One workgroup = one 512-coefficient piece of one limb of one batch item, BOTH polynomials (they meet the same plaintext
// words).  The plaintext pieces are the larger half of a workgroup's reads (nb*ng of them against 2*nb ciphertext pieces) and are
// shared by the whole batch: the batch index varies fastest and, where the piece count allows, the workgroups of one piece
// are dealt to ONE XCD (consecutive workgroup ids go round-robin over the 8 XCDs, each with its own L2), so a piece is
// fetched from HBM once instead of once per batch item (LSA_MACM_NO_XCD=1: batch-fastest order only).
template <int POLYS, bool ACC>
__global__ __launch_bounds__(TPB) void k_mac_plain_multi(MacPlainMultiArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    int piece, b;
    if (g.xcd_map) {
        const int w = (int)blockIdx.x, slot = w >> 3;
        b = slot % g.batch;
        piece = (slot / g.batch) * 8 + (w & 7);
    } else {
        b = (int)blockIdx.x % g.batch;
        piece = (int)blockIdx.x / g.batch;
    }
    const int limb = piece / chunks;
    const int x = ((piece % chunks) * TPB + threadIdx.x) * 2;
    const ModDev m = g.mods[g.mod_of[limb]];
    const long long poff = ((long long)limb << g.logn) + x, pstep = (long long)g.limbs << g.logn;
    ulonglong2 c[POLYS][LSA_MACM_MAX];
#pragma unroll
    for (int i = 0; i < LSA_MACM_MAX; i++)
        if (i < g.nb) {
#pragma unroll
            for (int p = 0; p < POLYS; p++) c[p][i] = ld2(g.ct[i] + (long long)b * g.sct[i] + p * pstep + poff);
        }
    for (int gi = 0; gi < g.ng; gi++) {
        // at most 8 products of < q^2, q < 2^61: the 128-bit sum stays below q * 2^64, which is what the lazy REDC takes.  The
        // running sum of an ACC launch does not enter it: it is a fully reduced residue, added (mod q) to the reduced block sum
        // after the reduction, so the bound is the same 8 products with or without it and the stored sum is again < q.
        u64 h[POLYS][2], l[POLYS][2];
#pragma unroll
        for (int p = 0; p < POLYS; p++) h[p][0] = h[p][1] = l[p][0] = l[p][1] = 0;
#pragma unroll
        for (int i = 0; i < LSA_MACM_MAX; i++) {
            if (i < g.nb && g.pt[gi][i]) {
                const ulonglong2 w = ld2(g.pt[gi][i] + poff);
#pragma unroll
                for (int p = 0; p < POLYS; p++) {
                    mac128(h[p][0], l[p][0], c[p][i].x, w.x);
                    mac128(h[p][1], l[p][1], c[p][i].y, w.y);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < POLYS; p++) {
            u64 r0 = csub(mont_redc_lazy(h[p][0], l[p][0], m.q, m.qinv), m.q), r1 = csub(mont_redc_lazy(h[p][1], l[p][1], m.q, m.qinv), m.q);
            r0 = mont_mul(r0, m.r2, m.q, m.qinv);            // sum * R^-1 -> sum
            r1 = mont_mul(r1, m.r2, m.q, m.qinv);
            u64* po = g.out[gi] + (long long)b * g.so + p * pstep + poff;
            if constexpr (ACC) {
                const ulonglong2 v = ld2(po);
                r0 = add_mod(r0, v.x, m.q);
                r1 = add_mod(r1, v.y, m.q);
            }
            st2(po, r0, r1);
        }
    }
}

void launch_mac_plain_multi(Context& c, int nb, const u64* const* ct, const long long* sct, int ng, const u64* const* pt /*[ng*nb]*/,
                            u64* const* out, long long so, int batch, int polys, int limbs, const RowMap& rm, hipStream_t s,
                            bool accumulate) {
    if (batch <= 0 || nb <= 0 || ng <= 0) return;
    LSA_REQUIRE(nb <= LSA_MACM_MAX && ng <= LSA_MACM_MAX, "too many baby or giant steps for one multiply-accumulate launch");
    LSA_REQUIRE(rm.period == limbs && limbs <= LSA_MAX_PERIOD, "mac: row map must cover the limbs");
    MacPlainMultiArgs g{};
    int terms = 0;
    for (int i = 0; i < nb; i++) {
        g.ct[i] = ct[i];
        g.sct[i] = sct[i];
    }
    for (int gi = 0; gi < ng; gi++) {
        g.out[gi] = out[gi];
        for (int i = 0; i < nb; i++) {
            g.pt[gi][i] = pt[gi * nb + i];
            terms += pt[gi * nb + i] != nullptr;
        }
    }
    g.so = so;
    g.mods = c.d_mods;
    g.nb = nb;
    g.ng = ng;
    g.polys = polys;
    g.limbs = limbs;
    g.logn = c.logn;
    int period;
    fill_rowmap(g.mod_of, period, rm, c.nmod);
    // algorithmic bytes: every ciphertext piece read once, every plaintext ONCE per launch (shared by the batch), the sums written
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * limbs * ((double)batch * polys * (nb + ng * (accumulate ? 2 : 1)) + (double)terms), s);
    LSA_REQUIRE(polys == 1 || polys == 2, "mac: one or two polynomials per ciphertext");
    const int pieces = limbs * (c.n / (2 * TPB));
    g.batch = batch;
    g.xcd_map = (pieces % 8 == 0 && !sw::macm_no_xcd()) ? 1 : 0;
    LSA_REQUIRE(c.n >= 2 * TPB, "ring degree too small for the elementwise kernels (need N >= 512)");
    const dim3 grid((unsigned)(pieces * batch));
    if (polys == 2 && accumulate) hipLaunchKernelGGL((k_mac_plain_multi<2, true>), grid, dim3(TPB), 0, s, g);
    else if (polys == 2) hipLaunchKernelGGL((k_mac_plain_multi<2, false>), grid, dim3(TPB), 0, s, g);
    else if (accumulate) hipLaunchKernelGGL((k_mac_plain_multi<1, true>), grid, dim3(TPB), 0, s, g);
    else hipLaunchKernelGGL((k_mac_plain_multi<1, false>), grid, dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

// Leaves of a polynomial evaluation (poly_eval.hip): n_out linear combinations of the same nsrc ciphertexts by per-limb integer
// constants, out[g] = sum_i K[g][i] * src_i (+ A[g] on polynomial 0), one launch.  Every source element is read once for all
// outputs; the sources sit at different levels and only their leading `rows` rows per polynomial are read (own batch stride and
// rows per polynomial each, no copy to drop levels).  The constants are uniform per workgroup (one row): scalar loads.  The
// products are summed in 128 bits and reduced once per output (poly_lincomb.h).
struct PolyLincombArgs {
    const u64* src[LSA_PLC_MAX_SRC];
    long long ss[LSA_PLC_MAX_SRC];
    int rpp[LSA_PLC_MAX_SRC];
    u64* out;          // [n_out][batch][2][rows][N]
    const u64* ktab;   // [n_out][nsrc][rows], Montgomery form
    const u64* atab;   // [n_out][rows] plain residues added to polynomial 0, or null
    const ModDev* mods;
    int nsrc, n_out, rows, logn, batch;
};

// One workgroup = one 512-coefficient piece of one row of one polynomial of one batch item, batch index fastest (the batch
// items of a piece share its constants); 16 B per lane.
template <int GMAX>
__global__ __launch_bounds__(TPB) void k_poly_lincomb(PolyLincombArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int b = (int)blockIdx.x % g.batch, piece = (int)blockIdx.x / g.batch;
    const int prow = piece / chunks;   // poly * rows + row
    const int poly = prow / g.rows, row = prow % g.rows;
    const int x = ((piece % chunks) * TPB + threadIdx.x) * 2;
    const ModDev m = g.mods[row];
    PlcAcc a0[GMAX], a1[GMAX];
#pragma unroll
    for (int gi = 0; gi < GMAX; gi++) {
        plc_init(a0[gi]);
        plc_init(a1[gi]);
    }
    for (int i = 0; i < g.nsrc; i++) {
        const ulonglong2 v = ld2(g.src[i] + (long long)b * g.ss[i] + (((long long)poly * g.rpp[i] + row) << g.logn) + x);
#pragma unroll
        for (int gi = 0; gi < GMAX; gi++)
            if (gi < g.n_out) {
                const u64 k = g.ktab[((long long)gi * g.nsrc + i) * g.rows + row];
                if (k) {   // uniform: a power this output does not use
                    plc_term(a0[gi], i, v.x, k, m.q, m.qinv);
                    plc_term(a1[gi], i, v.y, k, m.q, m.qinv);
                } else if (i == 8) {
                    plc_fold(a0[gi], m.q, m.qinv);
                    plc_fold(a1[gi], m.q, m.qinv);
                }
            }
    }
#pragma unroll
    for (int gi = 0; gi < GMAX; gi++)
        if (gi < g.n_out) {
            u64 r0 = plc_finish(a0[gi], m.q, m.qinv), r1 = plc_finish(a1[gi], m.q, m.qinv);
            if (g.atab && poly == 0) {
                const u64 add = g.atab[(long long)gi * g.rows + row];
                r0 = add_mod(r0, add, m.q);
                r1 = add_mod(r1, add, m.q);
            }
            st2(g.out + ((((long long)gi * g.batch + b) * 2 * g.rows + prow) << g.logn) + x, r0, r1);
        }
}

void launch_poly_lincomb(Context& c, int nsrc, const u64* const* src, const long long* ss, const int* rpp, int n_out,
                         const u64* d_k, const u64* d_a, u64* out, int rows, int batch, hipStream_t s) {
    if (batch <= 0) return;
    LSA_REQUIRE(nsrc >= 1 && nsrc <= LSA_PLC_MAX_SRC && n_out >= 1 && n_out <= LSA_PLC_MAX_OUT, "poly: too many sources or outputs for one launch");
    LSA_REQUIRE(rows >= 1 && rows <= c.nq, "poly: rows beyond the modulus chain");
    LSA_REQUIRE(c.n >= 2 * TPB, "ring degree too small for the elementwise kernels (need N >= 512)");
    PolyLincombArgs g{};
    for (int i = 0; i < nsrc; i++) {
        LSA_REQUIRE(rpp[i] >= rows && ss[i] >= 2LL * rpp[i] * c.n, "poly: a source with fewer rows than the launch reads");
        g.src[i] = src[i];
        g.ss[i] = ss[i];
        g.rpp[i] = rpp[i];
    }
    g.out = out;
    g.ktab = d_k;
    g.atab = d_a;
    g.mods = c.d_mods;
    g.nsrc = nsrc;
    g.n_out = n_out;
    g.rows = rows;
    g.logn = c.logn;
    g.batch = batch;
    const long long blocks = 2LL * rows * (c.n / (2 * TPB)) * batch;
    LSA_REQUIRE(blocks < (1LL << 31), "poly: grid too large");
    // algorithmic bytes: every source row read once, every output row written once
    ProfScope ps(c, PROF_ELEMWISE, 16.0 * c.n * rows * batch * (nsrc + n_out), s);
    const dim3 grid((unsigned)blocks);
    if (n_out == 1) hipLaunchKernelGGL((k_poly_lincomb<1>), grid, dim3(TPB), 0, s, g);
    else if (n_out == 2) hipLaunchKernelGGL((k_poly_lincomb<2>), grid, dim3(TPB), 0, s, g);
    else if (n_out <= 4) hipLaunchKernelGGL((k_poly_lincomb<4>), grid, dim3(TPB), 0, s, g);
    else hipLaunchKernelGGL((k_poly_lincomb<8>), grid, dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

// tensor product of two degree-1 ciphertexts: d0=a0*b0, d1=a0*b1+a1*b0, d2=a1*b1 (mega_ag_executors_gpu.cu:185,223)
struct TensorArgs {
    const u64* a;
    const u64* b;
    u64* d;
    long long sa, sb, sd;
    long long pa, pb;   // elements between the two polynomials of a / b (operands kept at a higher level: more rows per polynomial)
    const ModDev* mods;
    int limbs, logn;
    unsigned char mod_of[LSA_MAX_PERIOD];
};

__global__ __launch_bounds__(TPB) void k_tensor(TensorArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int limb = blockIdx.x / chunks;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const ModDev m = g.mods[g.mod_of[limb]];
    const long long b = blockIdx.y;
    const long long poly = (long long)g.limbs << g.logn;
    const long long off = ((long long)limb << g.logn) + x;
    const u64* pa = g.a + b * g.sa + off;
    const u64* pb = g.b + b * g.sb + off;
    u64* pd = g.d + b * g.sd + off;
    const ulonglong2 a0 = ld2(pa), a1 = ld2(pa + g.pa), b0 = ld2(pb), b1 = ld2(pb + g.pb);
    u64 r[3][2];
    const u64 a0v[2] = {a0.x, a0.y}, a1v[2] = {a1.x, a1.y}, b0v[2] = {b0.x, b0.y}, b1v[2] = {b1.x, b1.y};
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const u64 b0m = mont_mul_lazy(b0v[e], m.r2, m.q, m.qinv);  // to Montgomery form, [0,2q)
        const u64 b1m = mont_mul_lazy(b1v[e], m.r2, m.q, m.qinv);
        r[0][e] = mont_mul(a0v[e], b0m, m.q, m.qinv);
        r[2][e] = mont_mul(a1v[e], b1m, m.q, m.qinv);
        r[1][e] = add_mod(mont_mul(a0v[e], b1m, m.q, m.qinv), mont_mul(a1v[e], b0m, m.q, m.qinv), m.q);
    }
    st2(pd, r[0][0], r[0][1]);
    st2(pd + poly, r[1][0], r[1][1]);
    st2(pd + 2 * poly, r[2][0], r[2][1]);
}

void launch_tensor(Context& c, const u64* a, const u64* b, u64* d, int batch, long long sa, long long sb, long long sd,
                   int limbs, const RowMap& rm, hipStream_t s, int a_rpp, int b_rpp) {
    if (batch <= 0) return;
    TensorArgs g{};
    LSA_REQUIRE((a_rpp == 0 || a_rpp >= limbs) && (b_rpp == 0 || b_rpp >= limbs), "tensor: rows per polynomial below the limb count");
    g.pa = (long long)(a_rpp ? a_rpp : limbs) << c.logn;
    g.pb = (long long)(b_rpp ? b_rpp : limbs) << c.logn;
    g.a = a;
    g.b = b;
    g.d = d;
    g.sa = sa;
    g.sb = sb;
    g.sd = sd;
    g.mods = c.d_mods;
    g.limbs = limbs;
    g.logn = c.logn;
    LSA_REQUIRE(rm.period == limbs && limbs <= LSA_MAX_PERIOD, "tensor: row map must cover the limbs");
    int period;
    fill_rowmap(g.mod_of, period, rm, c.nmod);
    ProfScope ps(c, PROF_TENSOR, 7.0 * 8 * c.n * limbs * batch, s);
    hipLaunchKernelGGL(k_tensor, ew_grid(c, limbs, batch), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

// Sum of tensor products (ckks_mult_sum / ckks_dot): d = sum_i a_i (x) b_i (+ (addend_0, addend_1, 0)) (+ d, ACC), up to
// LSA_DOT_MAX_TERMS pairs per launch.  Every operand row is read once and the three output rows are written once per launch; the
// products are summed in 128 bits per coefficient and reduced once per output (tensor_sum.h).  Each pair has its own batch stride
// (0: one ciphertext for the whole batch) and rows per polynomial (an operand kept at a higher level is read through its leading
// rows).  The term loop is uniform: pointers, strides and offsets are read from the argument struct by the scalar unit.
struct TensorSumArgs {
    const u64* a[LSA_DOT_MAX_TERMS];
    const u64* b[LSA_DOT_MAX_TERMS];
    long long sa[LSA_DOT_MAX_TERMS], sb[LSA_DOT_MAX_TERMS];   // batch strides
    long long pa[LSA_DOT_MAX_TERMS], pb[LSA_DOT_MAX_TERMS];   // elements between the two polynomials
    const u64* addend;   // [2][limbs][N] per batch item, or null
    u64* d;              // [3][limbs][N] per batch item
    long long s_addend, sd;
    const ModDev* mods;
    int terms, limbs, logn;
    unsigned char mod_of[LSA_MAX_PERIOD];
};

// grid as k_tensor: x = limbs * (N/2/TPB), y = batch; 16 B per lane
template <bool ACC>
__global__ __launch_bounds__(TPB) void k_tensor_sum(TensorSumArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int limb = blockIdx.x / chunks;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const ModDev m = g.mods[g.mod_of[limb]];
    const long long b = blockIdx.y;
    const long long poly = (long long)g.limbs << g.logn;
    const long long off = ((long long)limb << g.logn) + x;
    u64* pd = g.d + b * g.sd + off;
    TsAcc t0, t1;   // the two coefficients of this lane
    ts_init(t0);
    ts_init(t1);
    if (ACC) {
        const ulonglong2 v0 = ld2(pd), v1 = ld2(pd + poly), v2 = ld2(pd + 2 * poly);
        ts_seed(t0.l0, v0.x);
        ts_seed(t1.l0, v0.y);
        ts_seed(t0.l1, v1.x);
        ts_seed(t1.l1, v1.y);
        ts_seed(t0.l2, v2.x);
        ts_seed(t1.l2, v2.y);
    }
    if (g.addend) {
        const u64* pe = g.addend + b * g.s_addend + off;
        const ulonglong2 v0 = ld2(pe), v1 = ld2(pe + poly);
        ts_seed(t0.l0, v0.x);
        ts_seed(t1.l0, v0.y);
        ts_seed(t0.l1, v1.x);
        ts_seed(t1.l1, v1.y);
    }
    for (int i = 0; i < g.terms; i++) {
        const u64* pa = g.a[i] + b * g.sa[i] + off;
        const u64* pb = g.b[i] + b * g.sb[i] + off;
        const ulonglong2 a0 = ld2(pa), a1 = ld2(pa + g.pa[i]), b0 = ld2(pb), b1 = ld2(pb + g.pb[i]);
        ts_term(t0, i, a0.x, a1.x, b0.x, b1.x, m);
        ts_term(t1, i, a0.y, a1.y, b0.y, b1.y, m);
    }
    st2(pd, ts_finish(t0.h0, t0.l0, m), ts_finish(t1.h0, t1.l0, m));
    st2(pd + poly, ts_finish(t0.h1, t0.l1, m), ts_finish(t1.h1, t1.l1, m));
    st2(pd + 2 * poly, ts_finish(t0.h2, t0.l2, m), ts_finish(t1.h2, t1.l2, m));
}

void launch_tensor_sum(Context& c, int terms, const u64* const* a, const long long* sa, const int* a_rpp, const u64* const* b,
                       const long long* sb, const int* b_rpp, const u64* addend, long long s_addend, bool accumulate, u64* d,
                       long long sd, int batch, int limbs, const RowMap& rm, hipStream_t s) {
    if (batch <= 0) return;
    LSA_REQUIRE(terms >= 1 && terms <= LSA_DOT_MAX_TERMS, "dot: too many terms for one launch");
    LSA_REQUIRE(rm.period == limbs && limbs <= LSA_MAX_PERIOD, "dot: row map must cover the limbs");
    LSA_REQUIRE(sd >= 3LL * limbs * c.n, "dot: output stride below three polynomials");
    TensorSumArgs g{};
    for (int i = 0; i < terms; i++) {
        const int ra = a_rpp && a_rpp[i] ? a_rpp[i] : limbs, rb = b_rpp && b_rpp[i] ? b_rpp[i] : limbs;
        LSA_REQUIRE(a[i] && b[i], "dot: null operand");
        LSA_REQUIRE(ra >= limbs && rb >= limbs, "dot: rows per polynomial below the limb count");
        LSA_REQUIRE((sa[i] == 0 || sa[i] >= 2LL * ra * c.n) && (sb[i] == 0 || sb[i] >= 2LL * rb * c.n), "dot: batch stride below one ciphertext");
        g.a[i] = a[i];
        g.b[i] = b[i];
        g.sa[i] = sa[i];
        g.sb[i] = sb[i];
        g.pa[i] = (long long)ra << c.logn;
        g.pb[i] = (long long)rb << c.logn;
    }
    LSA_REQUIRE(!addend || s_addend == 0 || s_addend >= 2LL * limbs * c.n, "dot: addend stride below one ciphertext");
    g.addend = addend;
    g.s_addend = s_addend;
    g.d = d;
    g.sd = sd;
    g.mods = c.d_mods;
    g.terms = terms;
    g.limbs = limbs;
    g.logn = c.logn;
    int period;
    fill_rowmap(g.mod_of, period, rm, c.nmod);
    for (int i = 0; i < limbs; i++) LSA_REQUIRE(g.mod_of[i] != LSA_ROW_SKIP, "dot: every limb needs a modulus");
    // algorithmic bytes: four operand rows per term, three output rows (+ two addend rows) (+ the three rows read back)
    ProfScope ps(c, PROF_TENSOR, 8.0 * c.n * limbs * batch * (4 * terms + 3 + (addend ? 2 : 0) + (accumulate ? 3 : 0)), s);
    if (accumulate) hipLaunchKernelGGL((k_tensor_sum<true>), ew_grid(c, limbs, batch), dim3(TPB), 0, s, g);
    else hipLaunchKernelGGL((k_tensor_sum<false>), ew_grid(c, limbs, batch), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ exact base conversion
//  y_i = x_i*(S/q_i)^-1 mod q_i ; v = floor(sum double(y_i)/double(q_i)) ;
// out_j = sum_i y_i*(S/q_i) - v*S mod p_j   [centered: x+floor(S/2) in, -floor(S/2) out]
struct BaseConvArgs {
    const BaseConvConsts* k;
    const ModDev* mods;
    const u64* src;
    u64* dst;
    long long ssrc, sdst;
    int logn;
    BaseConvRows rows;
    const u64* sub;   // optional: the converted value is src - sub (limb i of sub at row sub_row[i], batch stride ssub)
    long long ssub;
    int sub_row[LSA_BC_MAX_SRC];
};
// the rescale-head form (k_baseconv<.., HEAD>) takes these after the plain arguments, whose layout stays as it is
struct BaseConvHeadArgs : BaseConvArgs {
    const u64* head_a;      // INTT(acc[h][l]), one row per batch item
    const u64* head_b;      // optional: INTT(base[h][l])
    const u64* head_pinv;   // -> P^-1 mod q_l, Montgomery form (Context::pinv_vec(level) + l)
    long long s_head_a, s_head_b;
};

// NSMAX = compile-time bound of the source-limb loops (registers for y[] scale with it; dispatched from ns); EXACT: ns ==
// NSMAX, so the source loads carry no guard and are all in flight before the first is consumed.  The target loop has a
// fixed trip count (the tail group repeats its last target: same value stored twice by the same thread), so the per-target
// constants are fetched up front instead of one scalar-load latency chain per target.
// SPLIT (every modulus of the conversion below 2^58, BaseConvConsts::split29): the products y_i * shat_ij are accumulated on
// 29-bit halves -- y = y1 * 2^29 + y0, shat = w1 * 2^29 + w0, three 64-bit column sums y0 w0, y0 w1 + y1 w0, y1 w1 that
// cannot overflow for up to 16 terms -- so every partial product is ONE v_mad_u64_u32 into its own accumulator pair: no
// carries, no 64-bit addend built from register moves (the 128-bit form spends 14 instructions per term, 4 of them moves).
// The columns are recombined into the 128-bit sum once per target; same sum, same REDC, same residues.
// The conversion plan and the modulus table are read through the CONSTANT address space: they are never written while a
// kernel runs, and only then may the compiler keep their (wave-uniform) loads on the scalar unit after the kernel's first
// store -- as plain global loads 86 of a thread's 103 vector-memory instructions were broadcast reads of these constants,
// queued in front of its 13 stores.
#define LSA_CONST_AS __attribute__((address_space(4)))
__device__ __forceinline__ ModDev ld_mod(const LSA_CONST_AS ModDev* t, int i) {
    ModDev m;
    m.q = t[i].q;
    m.qinv = t[i].qinv;
    m.r2 = t[i].r2;
    m.r1 = t[i].r1;
    return m;
}
// HEAD (the merged ModDown + rescale, key_switch.hip ks_moddown_head): the plan is a pinv_scaled ModDown plan in its rescale-head
// flavour (Context::baseconv: the output correction of every target but the last also subtracts h = (q_l - 1) / 2), whose last
// target l = nd - 1 is unscaled.  Every block converts target l for itself first, reads A_l = INTT(acc_l) (and B_l =
// INTT(base_l)) at its two points and forms t = (A_l - conv_l) * P^-1 (+ B_l) and c = t + h mod q_l in registers (ntt_core.h
// rescale_head_t, rescale_head_centre).  The centred remainder of t IS the integer c - h, so
//   in_j = conv_j * P^-1 + lift_j(t) = conv_j * P^-1 + c - h  (mod q_j):
// c enters every other target's sum as one more term with weight 1 (2^64 mod q_j in the sum's Montgomery form) ahead of the
// single REDC, the plan's correction takes h off, and the stored word is in_j, canonical -- for any ratio q_l / q_j, without a
// second conditional subtraction (rescale_head_in states the same residue; tests/test_gpu_rescale_head_conv.py holds the kernel
// to it through the transform's prologue, word for word).  Nothing is stored for l.  The blocks of blockIdx.z split the nd - 1
// stored targets; y_i, v and every conv_j are computed exactly as in the plain form.
// Bounds with the extra term: c < q_l.  128-bit form: the term follows at most 7 products since the last reduction (8 products of
// < 2^61 * p_j stay below p_j * 2^64).  SPLIT: q_l < 2^58, so c splits like a y_i; the three-product columns take up to 8 terms
// (NSMAX + 1 <= 8, else the four-product form), whose columns hold 17 terms: 17 * 2 * 2^58 < 2^64, and 17 * 2^58 * p_j plus the
// correction stays below p_j * 2^64.
template <int NSMAX, bool EXACT, int TGT, bool SPLIT = false, bool HEAD = false>
__global__ __launch_bounds__(TPB) void k_baseconv(std::conditional_t<HEAD, BaseConvHeadArgs, BaseConvArgs> g) {
    const LSA_CONST_AS BaseConvConsts& K = *(const LSA_CONST_AS BaseConvConsts*)g.k;
    const LSA_CONST_AS ModDev* const mods_c = (const LSA_CONST_AS ModDev*)g.mods;
    const int x = (blockIdx.x * TPB + threadIdx.x) * 2;
    const long long b = blockIdx.y;
    const u64* src = g.src + b * g.ssrc + x;
    u64* dst = g.dst + b * g.sdst + x;
    const int ns = EXACT ? NSMAX : K.ns, nd = K.nd;
    ulonglong2 xin[NSMAX];
#pragma unroll
    for (int i = 0; i < NSMAX; i++)
        if (EXACT || i < ns) xin[i] = ld2(src + ((long long)g.rows.src_row[i] << g.logn));
    ulonglong2 head_a = {0, 0}, head_b = {0, 0};   // (HEAD: in flight with the source rows)
    u64 head_c0 = 0, head_c1 = 0;
    if constexpr (HEAD) {
        head_a = ld2(g.head_a + b * g.s_head_a + x);
        if (g.head_b) head_b = ld2(g.head_b + b * g.s_head_b + x);
    }
    // HEAD, target l (jj < 0): conv_l -> t -> c, kept in registers
    auto head_step = [&](const ModDev& m, u64 r0, u64 r1) {
        if constexpr (HEAD) {
            const u64 pinv = *(const LSA_CONST_AS u64*)g.head_pinv;
            u64 t0 = rescale_head_t(head_a.x, r0, pinv, m), t1 = rescale_head_t(head_a.y, r1, pinv, m);
            if (g.head_b) {
                t0 = add_mod(t0, head_b.x, m.q);
                t1 = add_mod(t1, head_b.y, m.q);
            }
            const u64 h = (m.q - 1) >> 1;
            head_c0 = rescale_head_centre(t0, h, m.q);
            head_c1 = rescale_head_centre(t1, h, m.q);
        }
    };
    if (g.sub) {   // block-uniform: a branch around the loop, only the launches that fold a subtraction take it
        const u64* sub = g.sub + b * g.ssub + x;
#pragma unroll
        for (int i = 0; i < NSMAX; i++)
            if (EXACT || i < ns) {
                const u64 q = mods_c[K.src_mod[i]].q;
                const ulonglong2 w = ld2(sub + ((long long)g.sub_row[i] << g.logn));
                xin[i].x = sub_mod(xin[i].x, w.x, q);
                xin[i].y = sub_mod(xin[i].y, w.y, q);
            }
    }
    u64 y[NSMAX][2];
    double vf0 = 0.0, vf1 = 0.0;
#pragma unroll
    for (int i = 0; i < NSMAX; i++) {
        if (EXACT || i < ns) {
            const ModDev m = ld_mod(mods_c, K.src_mod[i]);
            ulonglong2 v = xin[i];
            if (K.centered) {
                v.x = add_mod(v.x, K.half_src[i], m.q);
                v.y = add_mod(v.y, K.half_src[i], m.q);
            }
            y[i][0] = mont_mul(v.x, K.shat_inv_m[i], m.q, m.qinv);
            y[i][1] = mont_mul(v.y, K.shat_inv_m[i], m.q, m.qinv);
            // y/q correctly rounded == the oracle's IEEE division, in 3 operations (Markstein: with r = RN(1/q) and
            // q0 = RN(y*r), RN(q0 + (y - q0*q)*r) is the correctly rounded quotient; q's significand is not all ones),
            // then sequential adds: same float sequence as the oracle
            const double qf = K.qf[i], rf = K.rf[i];
            const double a0 = (double)y[i][0], a1 = (double)y[i][1];
            const double e0 = a0 * rf, e1 = a1 * rf;
            vf0 += __builtin_fma(__builtin_fma(-e0, qf, a0), rf, e0);
            vf1 += __builtin_fma(__builtin_fma(-e1, qf, a1), rf, e1);
        }
    }
    const int v0 = (int)(u64)vf0, v1 = (int)(u64)vf1;
    // targets are split over blockIdx.z (each block recomputes y_i/v and converts TGT targets)
    const int j0 = blockIdx.z * TGT;
    u32 ylo[SPLIT ? NSMAX : 1][2], yhi[SPLIT ? NSMAX : 1][2], ysum[SPLIT ? NSMAX : 1][2];
    if (SPLIT) {
#pragma unroll
        for (int i = 0; i < NSMAX; i++)
#pragma unroll
            for (int e = 0; e < 2; e++) {
                ylo[i][e] = (u32)y[i][e] & ((1u << 29) - 1);
                yhi[i][e] = (u32)(y[i][e] >> 29);
                ysum[i][e] = ylo[i][e] + yhi[i][e];
            }
    }
#pragma unroll
    for (int jj = HEAD ? -1 : 0; jj < TGT; jj++) {
        const int j = HEAD ? (jj < 0 ? nd - 1 : min(j0 + jj, nd - 2)) : min(j0 + jj, nd - 1);
        const ModDev m = ld_mod(mods_c, K.dst_mod[j]);
        u64 h0 = 0, l0 = 0, h1 = 0, l1 = 0, r0 = 0, r1 = 0;
#if defined(LSA_BC_DIAG_NO_MATH)       // diagnostic build: the loads and the stores, no conversion arithmetic
        if (SPLIT) {
            st2(dst + ((long long)g.rows.dst_row[j] << g.logn), xin[jj % NSMAX].x + v0, xin[jj % NSMAX].y + v1);
            continue;
        }
#endif
        if (SPLIT) {
            // columns y0 w0, (y0 + y1)(w0 + w1), y1 w1: three multiply-accumulates per term (the middle column is recovered as
            // cm - c0 - c2); 30-bit factors: up to 8 terms stay below 2^63, more take the four-product form
            constexpr bool KARA = NSMAX + (HEAD ? 1 : 0) <= 8;
            u64 c0[2] = {0, 0}, c1[2] = {0, 0}, c2[2] = {0, 0};
#pragma unroll
            for (int i = 0; i < NSMAX; i++) {
                if (EXACT || i < ns) {
                    const u32 w0 = K.shat_lo[j][i], w1 = K.shat_hi[j][i], ws = K.shat_sum[j][i];
#pragma unroll
                    for (int e = 0; e < 2; e++) {
                        c0[e] += (u64)ylo[i][e] * w0;
                        c2[e] += (u64)yhi[i][e] * w1;
                        if (KARA) {
                            c1[e] += (u64)ysum[i][e] * ws;
                        } else {
                            c1[e] += (u64)ylo[i][e] * w1;
                            c1[e] += (u64)yhi[i][e] * w0;
                        }
                    }
                }
            }
            if (HEAD && jj >= 0) {   // c as one more term, weight 2^64 mod p_j
                const u32 w0 = (u32)m.r1 & ((1u << 29) - 1), w1 = (u32)(m.r1 >> 29), ws = w0 + w1;
                const u64 hc[2] = {head_c0, head_c1};
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const u32 lo = (u32)hc[e] & ((1u << 29) - 1), hi = (u32)(hc[e] >> 29);
                    c0[e] += (u64)lo * w0;
                    c2[e] += (u64)hi * w1;
                    if (KARA) {
                        c1[e] += (u64)(lo + hi) * ws;
                    } else {
                        c1[e] += (u64)lo * w1;
                        c1[e] += (u64)hi * w0;
                    }
                }
            }
            // sum = c0 + c1 * 2^29 + c2 * 2^58 (+ the output corrections, Montgomery form) as (hi, lo) below p_j * 2^64
            u64 hs[2], ls[2];
            const u64 cr[2] = {(u64)(u32)v0 * K.corr_a[j] + K.corr_b[j], (u64)(u32)v1 * K.corr_a[j] + K.corr_b[j]};
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const u64 mid = KARA ? c1[e] - c0[e] - c2[e] : c1[e];
#if defined(LSA_BC_CARRY_COMPARES)   // A/B: carries recovered by 64-bit compares (18 cycles each on gfx950, tools/probe_issue.hip)
                const u64 a = c0[e] + (mid << 29);
                const u64 b = a + (c2[e] << 58);
                const u64 d = b + cr[e];
                ls[e] = d;
                hs[e] = (mid >> 35) + (c2[e] >> 6) + (a < c0[e] ? 1 : 0) + (b < a ? 1 : 0) + (d < b ? 1 : 0);
#else                                // one 128-bit sum: the carries ride the v_addc chain
                const unsigned __int128 sum = (unsigned __int128)c0[e] + ((unsigned __int128)mid << 29) + ((unsigned __int128)c2[e] << 58) + cr[e];
                ls[e] = (u64)sum;
                hs[e] = (u64)(sum >> 64);
#endif
            }
            r0 = csub(mont_redc_lazy(hs[0], ls[0], m.q, m.qinv), m.q);
            r1 = csub(mont_redc_lazy(hs[1], ls[1], m.q, m.qinv), m.q);
            if (HEAD && jj < 0) {
                head_step(m, r0, r1);
                continue;
            }
#if defined(LSA_BC_DIAG_NO_STORE)      // diagnostic build: all the arithmetic, (almost) no store traffic
            if (r0 == 0x123456789abcdefull) st2(dst + ((long long)g.rows.dst_row[j] << g.logn), r0, r1);
#else
            st2(dst + ((long long)g.rows.dst_row[j] << g.logn), r0, r1);
#endif
            continue;
        } else {
#pragma unroll
        for (int i = 0; i < NSMAX; i++) {
            if (EXACT || i < ns) {
                const u64 w = K.shat_m[j][i];
                mac128(h0, l0, y[i][0], w);
                mac128(h1, l1, y[i][1], w);
                if ((i & 7) == 7) {  // keep the 128-bit sum below p_j*2^64 (8 products of < 2^61 * p_j)
                    r0 = add_mod(r0, csub(mont_redc_lazy(h0, l0, m.q, m.qinv), m.q), m.q);
                    r1 = add_mod(r1, csub(mont_redc_lazy(h1, l1, m.q, m.qinv), m.q), m.q);
                    h0 = l0 = h1 = l1 = 0;
                }
            }
        }
        if (HEAD && jj >= 0) {   // c as one more term, weight 2^64 mod p_j
            mac128(h0, l0, head_c0, m.r1);
            mac128(h1, l1, head_c1, m.r1);
        }
        r0 = add_mod(r0, csub(mont_redc_lazy(h0, l0, m.q, m.qinv), m.q), m.q);
        r1 = add_mod(r1, csub(mont_redc_lazy(h1, l1, m.q, m.qinv), m.q), m.q);
        }
        r0 = sub_mod(r0, K.vs[j][v0], m.q);
        r1 = sub_mod(r1, K.vs[j][v1], m.q);
        if (K.centered) {
            r0 = sub_mod(r0, K.half_dst[j], m.q);
            r1 = sub_mod(r1, K.half_dst[j], m.q);
        }
        if (HEAD && jj < 0) {
            head_step(m, r0, r1);
            continue;
        }
        st2(dst + ((long long)g.rows.dst_row[j] << g.logn), r0, r1);
    }
}

// nd: the targets the launch stores (HEAD: without l)
template <int NSMAX, int TGT, bool HEAD = false, class Args = BaseConvArgs>
static void launch_baseconv_nt(int ns, int nd, bool split, dim3 grid, hipStream_t s, const Args& g) {
    grid.z = (unsigned)((nd + TGT - 1) / TGT);
    if (split) {
        if (ns == NSMAX) hipLaunchKernelGGL((k_baseconv<NSMAX, true, TGT, true, HEAD>), grid, dim3(TPB), 0, s, g);
        else hipLaunchKernelGGL((k_baseconv<NSMAX, false, TGT, true, HEAD>), grid, dim3(TPB), 0, s, g);
        return;
    }
    if (ns == NSMAX) hipLaunchKernelGGL((k_baseconv<NSMAX, true, TGT, false, HEAD>), grid, dim3(TPB), 0, s, g);
    else hipLaunchKernelGGL((k_baseconv<NSMAX, false, TGT, false, HEAD>), grid, dim3(TPB), 0, s, g);
}
// targets per block: the candidate with the least total work ceil(nd/T) * (Y + T*C), Y = y/v phase ~ 2.5 target conversions
static int baseconv_targets_per_block(int nd) {
    const int cand[3] = {4, 7, 13};
    int best = 4;
    double best_cost = 1e30;
    for (int T : cand) {
        const double cost = (double)((nd + T - 1) / T) * (2.5 + T);
        if (cost < best_cost) {
            best_cost = cost;
            best = T;
        }
    }
    return best;
}
template <int NSMAX, bool HEAD = false, class Args = BaseConvArgs>
static void launch_baseconv_ns(int ns, int nd, bool split, dim3 grid, hipStream_t s, const Args& g) {
    const int best = baseconv_targets_per_block(nd);
    if (best == 4) launch_baseconv_nt<NSMAX, 4, HEAD>(ns, nd, split, grid, s, g);
    else if (best == 7) launch_baseconv_nt<NSMAX, 7, HEAD>(ns, nd, split, grid, s, g);
    else launch_baseconv_nt<NSMAX, 13, HEAD>(ns, nd, split, grid, s, g);
}

// ------------------------------------------------------------------------- wide exact base conversion (17..32 sources)
// The BFV multiply at N = 2^16 converts 24 Q limbs to 24 auxiliary limbs and back.  k_baseconv keeps two points per thread
// (xin[NSMAX] and y[NSMAX][2]: 4 * NSMAX VGPRs, 128 at 32 sources before any accumulator), so the wide shapes have their own
// kernel with ONE point per thread: y[NSMAX] is 2 * NSMAX VGPRs.  Same formula, same residues: the loads (and the optional
// subtrahend) as in k_baseconv, the same y_i and the same float sequence for v, the output correction by the table vs[j][v]
// (v = 0..ns, ns + 1 entries).  The accumulate is the 128-bit form only, reduced every 8 terms as in k_baseconv (8 products
// of y_i < 2^61 and shat < p_j stay below p_j * 2^64, the bound of the REDC), which holds for any ns; the 29-bit SPLIT form
// is proved for at most 16 terms and is never taken here (Context::baseconv clears split29 above 16 sources; every BFV
// auxiliary prime is 61 bits wide, so the BFV conversions would not qualify anyway).  The 8-term blocks are reduced to
// [0, p_j) and added mod p_j, so the result is the exact residue whatever the block count.
template <int NSMAX, bool EXACT, int TGT>
__global__ __launch_bounds__(TPB) void k_baseconv_wide(BaseConvArgs g) {
    const LSA_CONST_AS BaseConvConsts& K = *(const LSA_CONST_AS BaseConvConsts*)g.k;
    const LSA_CONST_AS ModDev* const mods_c = (const LSA_CONST_AS ModDev*)g.mods;
    const int x = blockIdx.x * TPB + threadIdx.x;
    const long long b = blockIdx.y;
    const u64* src = g.src + b * g.ssrc + x;
    u64* dst = g.dst + b * g.sdst + x;
    const int ns = EXACT ? NSMAX : K.ns, nd = K.nd;
    u64 y[NSMAX];
#pragma unroll
    for (int i = 0; i < NSMAX; i++)
        if (EXACT || i < ns) y[i] = src[(long long)g.rows.src_row[i] << g.logn];
    if (g.sub) {   // block-uniform
        const u64* sub = g.sub + b * g.ssub + x;
#pragma unroll
        for (int i = 0; i < NSMAX; i++)
            if (EXACT || i < ns) y[i] = sub_mod(y[i], sub[(long long)g.sub_row[i] << g.logn], mods_c[K.src_mod[i]].q);
    }
    double vf = 0.0;
#pragma unroll
    for (int i = 0; i < NSMAX; i++) {
        if (EXACT || i < ns) {
            const ModDev m = ld_mod(mods_c, K.src_mod[i]);
            u64 v = y[i];
            if (K.centered) v = add_mod(v, K.half_src[i], m.q);
            y[i] = mont_mul(v, K.shat_inv_m[i], m.q, m.qinv);
            const double qf = K.qf[i], rf = K.rf[i];   // the correctly rounded y/q of k_baseconv, summed in source order
            const double a = (double)y[i];
            const double e = a * rf;
            vf += __builtin_fma(__builtin_fma(-e, qf, a), rf, e);
        }
    }
    const int v = (int)(u64)vf;
    const int j0 = blockIdx.z * TGT;
#pragma unroll
    for (int jj = 0; jj < TGT; jj++) {
        const int j = min(j0 + jj, nd - 1);
        const ModDev m = ld_mod(mods_c, K.dst_mod[j]);
        u64 h = 0, l = 0, r = 0;
#pragma unroll
        for (int i = 0; i < NSMAX; i++) {
            if (EXACT || i < ns) {
                mac128(h, l, y[i], K.shat_m[j][i]);
                if ((i & 7) == 7) {
                    r = add_mod(r, csub(mont_redc_lazy(h, l, m.q, m.qinv), m.q), m.q);
                    h = l = 0;
                }
            }
        }
        r = add_mod(r, csub(mont_redc_lazy(h, l, m.q, m.qinv), m.q), m.q);
        r = sub_mod(r, K.vs[j][v], m.q);
        if (K.centered) r = sub_mod(r, K.half_dst[j], m.q);
        dst[(long long)g.rows.dst_row[j] << g.logn] = r;
    }
}

template <int NSMAX, int TGT>
static void launch_baseconv_wide_nt(int ns, int nd, dim3 grid, hipStream_t s, const BaseConvArgs& g) {
    grid.z = (unsigned)((nd + TGT - 1) / TGT);
    if (ns == NSMAX) hipLaunchKernelGGL((k_baseconv_wide<NSMAX, true, TGT>), grid, dim3(TPB), 0, s, g);
    else hipLaunchKernelGGL((k_baseconv_wide<NSMAX, false, TGT>), grid, dim3(TPB), 0, s, g);
}
template <int NSMAX>
static void launch_baseconv_wide_ns(int ns, int nd, dim3 grid, hipStream_t s, const BaseConvArgs& g) {
    const int best = baseconv_targets_per_block(nd);
    if (best == 4) launch_baseconv_wide_nt<NSMAX, 4>(ns, nd, grid, s, g);
    else if (best == 7) launch_baseconv_wide_nt<NSMAX, 7>(ns, nd, grid, s, g);
    else launch_baseconv_wide_nt<NSMAX, 13>(ns, nd, grid, s, g);
}

void launch_baseconv(Context& c, const BaseConvPlan* k, const BaseConvRows& rows, const u64* src, u64* dst, int batch,
                     long long ssrc, long long sdst, hipStream_t s, const u64* sub, long long ssub, const int* sub_row,
                     const BaseConvHead* head) {
    if (batch <= 0) return;
    BaseConvHeadArgs g{};
    g.sub = sub;
    g.ssub = ssub;
    LSA_REQUIRE(!sub || sub_row, "base conversion: subtrahend rows missing");
    if (sub)
        for (int i = 0; i < k->ns; i++) g.sub_row[i] = sub_row[i];
    g.k = k->dev;
    g.mods = c.d_mods;
    g.src = src;
    g.dst = dst;
    g.ssrc = ssrc;
    g.sdst = sdst;
    g.logn = c.logn;
    g.rows = rows;
    const int ns = k->ns, nd = k->nd;
    if (head) {
        LSA_REQUIRE(ns <= LSA_BC_NARROW_SRC && nd >= 2 && !sub && head->a && head->pinv, "base conversion: rescale-head form on an unsupported shape");
        g.head_a = head->a;
        g.head_b = head->b;
        g.head_pinv = head->pinv;
        g.s_head_a = head->sa;
        g.s_head_b = head->sb;
    }
    // algorithmic bytes: the source rows (twice with a subtrahend) and one row per target;
    // rescale-head form: the source rows, the row A_l (and B_l), one row per target but l, which is not stored
    ProfScope ps(c, PROF_BASECONV, 8.0 * c.n * batch * (head ? (double)(ns + 1 + (head->b ? 1 : 0) + nd - 1)
                                                                  : (double)(ns * (sub ? 2 : 1) + nd)), s);
    if (head) {
        const dim3 grid((unsigned)(c.n / (2 * TPB)), (unsigned)batch, 1);
        const int st = nd - 1;   // stored targets
        if (ns <= 1) launch_baseconv_ns<1, true>(ns, st, k->split29, grid, s, g);
        else if (ns <= 2) launch_baseconv_ns<2, true>(ns, st, k->split29, grid, s, g);
        else if (ns <= 3) launch_baseconv_ns<3, true>(ns, st, k->split29, grid, s, g);
        else if (ns <= 4) launch_baseconv_ns<4, true>(ns, st, k->split29, grid, s, g);
        else if (ns <= 5) launch_baseconv_ns<5, true>(ns, st, k->split29, grid, s, g);
        else if (ns <= 8) launch_baseconv_ns<8, true>(ns, st, k->split29, grid, s, g);
        else if (ns <= 12) launch_baseconv_ns<12, true>(ns, st, k->split29, grid, s, g);
        else launch_baseconv_ns<LSA_BC_NARROW_SRC, true>(ns, st, k->split29, grid, s, g);
        LSA_HIP(hipGetLastError());
        return;
    }
    const BaseConvArgs& gp = g;   // the plain forms take the plain arguments
    if (ns > LSA_BC_NARROW_SRC) {
        const dim3 grid((unsigned)(c.n / TPB), (unsigned)batch, 1);   // one point per thread
        if (ns <= 24) launch_baseconv_wide_ns<24>(ns, nd, grid, s, gp);
        else launch_baseconv_wide_ns<LSA_BC_MAX_SRC>(ns, nd, grid, s, gp);
        LSA_HIP(hipGetLastError());
        return;
    }
    const dim3 grid((unsigned)(c.n / (2 * TPB)), (unsigned)batch, 1);
    if (ns <= 1) launch_baseconv_ns<1>(ns, nd, k->split29, grid, s, gp);
    else if (ns <= 2) launch_baseconv_ns<2>(ns, nd, k->split29, grid, s, gp);
    else if (ns <= 3) launch_baseconv_ns<3>(ns, nd, k->split29, grid, s, gp);
    else if (ns <= 4) launch_baseconv_ns<4>(ns, nd, k->split29, grid, s, gp);
    else if (ns <= 5) launch_baseconv_ns<5>(ns, nd, k->split29, grid, s, gp);
    else if (ns <= 8) launch_baseconv_ns<8>(ns, nd, k->split29, grid, s, gp);
    else if (ns <= 12) launch_baseconv_ns<12>(ns, nd, k->split29, grid, s, gp);
    else launch_baseconv_ns<LSA_BC_NARROW_SRC>(ns, nd, k->split29, grid, s, gp);
    LSA_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ key-switch MAC (K7)
struct KsMacArgs {
    const u64* cx;
    const u64* ext;
    const u64* key;
    u64* acc;
    long long scx, sext, sacc;
    const ModDev* mods;
    int logn, L, np, nq, beta, kcomp, klvl, batch, bpt;
    int n_tl;                      // 0: every target limb; else the launch covers tl_list[0..n_tl)
    unsigned char tl_list[64];
    // EXT (k_ks_mac<KB, true>): the product leaves as a ROTATED EXTENDED ciphertext instead of the plain accumulator --
    // acc[b][h][tl][scatter[x]] = sum(x) + (h == 0 and tl < L ? P * base[b][tl][x] : 0): the gadget product, the c0 * P term and
    // the automorphism of a baby-step rotation in one pass (otherwise k_permute_ext re-reads and re-writes 2(L+k) limbs)
    // EXT_ACC (k_ks_mac<KB, true, false, true>): the same values are ADDED to what acc holds at the scattered positions -- a
    // giant-step rotation joining the running sum of a double-hoisted linear transform without a permutation kernel.  scatter
    // is a permutation of the row and every thread owns its two points, so each word is read and written by one thread only.
    const unsigned* scatter;
    const u64* base;
    const u64* pm;                 // [L] P mod q_j, Montgomery form
    long long sbase;
    // FOLD (k_ks_mac<KB, false, true>, TensorFold): the own digit of a Q target limb is a1 * b1, and P * a0 b0 / P * (a0 b1 +
    // a1 b0) join the two sums; pf = Context::pfold_vec (its first L entries: mont_mul(x, pf[j]) = x * P in Montgomery form)
    const u64* fa;
    const u64* fb;
    long long sfa, sfb, pfa, pfb;
    const u64* pf;
};

// grid: x = T * (N/2/TPB), y = groups of `bpt` batch items.  The key is in Montgomery form, so sum_d ext_d*key_d needs
// ONE REDC per output.  A thread keeps its 2*beta key words in registers and walks `bpt` ciphertexts with them: the key
// (68 MiB at the headline shape) is then streamed once per group instead of once per ciphertext.
// KB = number of digits whose key words are register-resident (0: stream the key per ciphertext)
template <int KB, bool EXT = false, bool FOLD = false, bool EXT_ACC = false>
__global__ __launch_bounds__(TPB) void k_ks_mac(KsMacArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int tl = g.n_tl ? g.tl_list[blockIdx.x / chunks] : blockIdx.x / chunks;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const int T = g.L + g.np;
    const int mi = tl < g.L ? tl : g.nq + (tl - g.L);
    const int kj = tl < g.L ? tl : g.klvl + 1 + (tl - g.L);
    const ModDev m = g.mods[mi];
    const long long N = 1LL << g.logn;
    const int own_d = tl < g.L ? tl / g.np : -1;   // the digit that contains this limb reads cx directly
    ulonglong2 k0[KB > 0 ? KB : 1], k1[KB > 0 ? KB : 1];
    constexpr bool in_regs = KB > 0;
    if constexpr (in_regs) {
#pragma unroll
        for (int d = 0; d < KB; d++) {
            if (d < g.beta) {
                const u64* pk = g.key + ((long long)(d * 2) * g.kcomp + kj) * N + x;
                k0[d] = ld2(pk);
                k1[d] = ld2(pk + (long long)g.kcomp * N);
            }
        }
    }
    const int b_begin = blockIdx.y * g.bpt;
    const int b_end = min(g.batch, b_begin + g.bpt);
    // register-resident key: the NEXT ciphertext's digit values are fetched before the current one is multiplied, so a wave
    // always has one ciphertext's loads in flight behind its arithmetic and its stores (the kernel is traffic-bound: with the
    // loads issued and consumed in the same iteration it ran at 4.5 TB/s, no faster without its arithmetic)
    ulonglong2 en[KB > 0 ? KB : 1];
    ulonglong2 fn[FOLD ? 4 : 1];   // FOLD: the next ciphertext's a0, a1, b0, b1 (Q targets)
    auto fetch = [&](long long b) {
        if constexpr (in_regs) {
#pragma unroll
            for (int d = 0; d < KB; d++)
                if (d < g.beta && !(FOLD && d == own_d))
                    en[d] = ld2(d == own_d ? g.cx + b * g.scx + tl * N + x : g.ext + b * g.sext + ((long long)d * T + tl) * N + x);
        }
        if constexpr (FOLD) {
            if (own_d >= 0) {
                const u64* pa = g.fa + b * g.sfa + tl * N + x;
                const u64* pb = g.fb + b * g.sfb + tl * N + x;
                fn[0] = ld2(pa);
                fn[1] = ld2(pa + g.pfa);
                fn[2] = ld2(pb);
                fn[3] = ld2(pb + g.pfb);
            }
        }
    };
    // FOLD: the own digit's value d2 = a1 * b1, canonical (k_tensor's residues)
    auto own_d2 = [&](const ulonglong2& a1, const ulonglong2& b1) {
        return ulonglong2{mont_mul(a1.x, mont_mul_lazy(b1.x, m.r2, m.q, m.qinv), m.q, m.qinv),
                          mont_mul(a1.y, mont_mul_lazy(b1.y, m.r2, m.q, m.qinv), m.q, m.qinv)};
    };
    if (b_begin < b_end) fetch(b_begin);
    for (long long b = b_begin; b < b_end; b++) {
        u64 h00 = 0, l00 = 0, h01 = 0, l01 = 0, h10 = 0, l10 = 0, h11 = 0, l11 = 0;
        u64 r00 = 0, r01 = 0, r10 = 0, r11 = 0;
        ulonglong2 fc[FOLD ? 4 : 1];
        if constexpr (FOLD) {
            if constexpr (in_regs) {
#pragma unroll
                for (int i = 0; i < 4; i++) fc[i] = fn[i];
            } else if (own_d >= 0) {
                const u64* pa = g.fa + b * g.sfa + tl * N + x;
                const u64* pb = g.fb + b * g.sfb + tl * N + x;
                fc[0] = ld2(pa);
                fc[1] = ld2(pa + g.pfa);
                fc[2] = ld2(pb);
                fc[3] = ld2(pb + g.pfb);
            }
        }
        if constexpr (in_regs) {
            ulonglong2 ec[KB > 0 ? KB : 1];
#pragma unroll
            for (int d = 0; d < KB; d++) ec[d] = en[d];
            if (b + 1 < b_end) fetch(b + 1);
            if constexpr (FOLD) {
                if (own_d >= 0) {
#pragma unroll
                    for (int d = 0; d < KB; d++)
                        if (d == own_d) ec[d] = own_d2(fc[1], fc[3]);
                }
            }
#pragma unroll
            for (int d = 0; d < KB; d++) {
                if (d < g.beta) {
                    const ulonglong2 e = ec[d];
#if defined(LSA_KS_DIAG_NO_MATH)
                    l00 += e.x ^ k0[d].x; l01 += e.y ^ k0[d].y; l10 += e.x ^ k1[d].x; l11 += e.y ^ k1[d].y;
#else
                    mac128(h00, l00, e.x, k0[d].x);
                    mac128(h01, l01, e.y, k0[d].y);
                    mac128(h10, l10, e.x, k1[d].x);
                    mac128(h11, l11, e.y, k1[d].y);
#endif
                }
            }
        } else {
            for (int d = 0; d < g.beta; d++) {
                const u64* pe = d == own_d ? g.cx + b * g.scx + tl * N + x : g.ext + b * g.sext + ((long long)d * T + tl) * N + x;
                const ulonglong2 e = FOLD && d == own_d ? own_d2(fc[1], fc[3]) : ld2(pe);
                const u64* pk = g.key + ((long long)(d * 2) * g.kcomp + kj) * N + x;
                const ulonglong2 kk0 = ld2(pk), kk1 = ld2(pk + (long long)g.kcomp * N);
                mac128(h00, l00, e.x, kk0.x);
                mac128(h01, l01, e.y, kk0.y);
                mac128(h10, l10, e.x, kk1.x);
                mac128(h11, l11, e.y, kk1.y);
                if ((d & 7) == 7) {  // fold so the 128-bit sum stays below q*2^64 (8 products of < q^2, q < 2^61)
                    r00 = add_mod(r00, csub(mont_redc_lazy(h00, l00, m.q, m.qinv), m.q), m.q);
                    r01 = add_mod(r01, csub(mont_redc_lazy(h01, l01, m.q, m.qinv), m.q), m.q);
                    r10 = add_mod(r10, csub(mont_redc_lazy(h10, l10, m.q, m.qinv), m.q), m.q);
                    r11 = add_mod(r11, csub(mont_redc_lazy(h11, l11, m.q, m.qinv), m.q), m.q);
                    h00 = l00 = h01 = l01 = h10 = l10 = h11 = l11 = 0;
                }
            }
        }
#if defined(LSA_KS_DIAG_NO_MATH)
        r00 = l00; r01 = l01; r10 = l10; r11 = l11;
#else
        r00 = add_mod(r00, csub(mont_redc_lazy(h00, l00, m.q, m.qinv), m.q), m.q);
        r01 = add_mod(r01, csub(mont_redc_lazy(h01, l01, m.q, m.qinv), m.q), m.q);
        r10 = add_mod(r10, csub(mont_redc_lazy(h10, l10, m.q, m.qinv), m.q), m.q);
        r11 = add_mod(r11, csub(mont_redc_lazy(h11, l11, m.q, m.qinv), m.q), m.q);
#endif
        if constexpr (FOLD) {   // + P * d0, + P * d1 (canonical, like the EXT path's P * c0)
            if (own_d >= 0) {
                const u64 pm = g.pf[tl];
                const u64 p0x = mont_mul(fc[2].x, pm, m.q, m.qinv), p0y = mont_mul(fc[2].y, pm, m.q, m.qinv);   // b0 * P * 2^64
                const u64 p1x = mont_mul(fc[3].x, pm, m.q, m.qinv), p1y = mont_mul(fc[3].y, pm, m.q, m.qinv);   // b1 * P * 2^64
                r00 = add_mod(r00, mont_mul(fc[0].x, p0x, m.q, m.qinv), m.q);
                r01 = add_mod(r01, mont_mul(fc[0].y, p0y, m.q, m.qinv), m.q);
                r10 = add_mod(r10, add_mod(mont_mul(fc[0].x, p1x, m.q, m.qinv), mont_mul(fc[1].x, p0x, m.q, m.qinv), m.q), m.q);
                r11 = add_mod(r11, add_mod(mont_mul(fc[0].y, p1y, m.q, m.qinv), mont_mul(fc[1].y, p0y, m.q, m.qinv), m.q), m.q);
            }
        }
        if constexpr (EXT) {
            if (g.base && tl < g.L) {   // (no base: the caller adds the rotated c0 itself, the BFV slot sum's gathering tail)
                const ulonglong2 c0 = ld2(g.base + b * g.sbase + tl * N + x);
                const u64 k = g.pm[tl];
                r00 = add_mod(r00, mont_mul(c0.x, k, m.q, m.qinv), m.q);
                r01 = add_mod(r01, mont_mul(c0.y, k, m.q, m.qinv), m.q);
            }
            const uint2 sx = *reinterpret_cast<const uint2*>(g.scatter + x);
            u64* po = g.acc + b * g.sacc + tl * N;
            if constexpr (EXT_ACC) {
                r00 = add_mod(r00, po[sx.x], m.q);
                r01 = add_mod(r01, po[sx.y], m.q);
                r10 = add_mod(r10, po[(long long)T * N + sx.x], m.q);
                r11 = add_mod(r11, po[(long long)T * N + sx.y], m.q);
            }
            po[sx.x] = r00;
            po[sx.y] = r01;
            po[(long long)T * N + sx.x] = r10;
            po[(long long)T * N + sx.y] = r11;
            continue;
        }
        u64* pa = g.acc + b * g.sacc + tl * N + x;
#if defined(LSA_KS_DIAG_NO_STORE)
        if (r00 == 0x123456789abcdefull) st2(pa, r00, r01);
        if (r10 == 0x123456789abcdefull) st2(pa + (long long)T * N, r10, r11);
#else
        st2(pa, r00, r01);
        st2(pa + (long long)T * N, r10, r11);
#endif
    }
}

template <bool EXT, bool FOLD = false, bool EXT_ACC = false>
static void launch_ks_mac_kb(int beta, dim3 grid, hipStream_t s, const KsMacArgs& g) {
    // the register-resident key costs 8 VGPRs per digit slot: 5 and 6 digits (the 25Q+5P chains) get their own instantiations
    // instead of the 8-slot one (182 VGPRs, 2 waves per SIMD)
    if (beta <= 2) hipLaunchKernelGGL((k_ks_mac<2, EXT, FOLD, EXT_ACC>), grid, dim3(TPB), 0, s, g);   // low levels: 86 VGPRs, 5 waves per SIMD
    else if (beta <= 4) hipLaunchKernelGGL((k_ks_mac<4, EXT, FOLD, EXT_ACC>), grid, dim3(TPB), 0, s, g);
    else if (beta <= 5) hipLaunchKernelGGL((k_ks_mac<5, EXT, FOLD, EXT_ACC>), grid, dim3(TPB), 0, s, g);
    else if (beta <= 6) hipLaunchKernelGGL((k_ks_mac<6, EXT, FOLD, EXT_ACC>), grid, dim3(TPB), 0, s, g);
    else if (beta <= 8) hipLaunchKernelGGL((k_ks_mac<8, EXT, FOLD, EXT_ACC>), grid, dim3(TPB), 0, s, g);
    else hipLaunchKernelGGL((k_ks_mac<0, EXT, FOLD, EXT_ACC>), grid, dim3(TPB), 0, s, g);
}

// scatter (with engine < 0): the result is written as the rotated extended ciphertext perm(acc + P * c0) -- scatter = the index
// map of the rotation's inverse element, base = the ciphertext whose c0 enters (see KsMacArgs); base == nullptr: no P * c0 is
// added, the result is perm(acc)
void launch_ks_mac(Context& c, int level, const u64* cx, long long scx, const u64* ext, long long sext, const Key& key,
                   const KsMacDst& dst, int batch, hipStream_t s, bool unfused_only, const TensorFold* fold, int extra_tl) {
    if (batch <= 0) return;
    const u32* scatter = dst.scatter;
    const u64* base = dst.base;
    const bool accumulate = dst.accumulate;
    KsMacArgs g{};
    LSA_REQUIRE(!accumulate || scatter, "key MAC: only the extended output accumulates");
    LSA_REQUIRE(!scatter || !unfused_only, "key MAC: the extended output covers every target limb");
    LSA_REQUIRE(!(scatter && fold), "key MAC: the tensor fold has no extended output");
    if (fold) {
        g.fa = fold->a;
        g.fb = fold->b;
        g.sfa = fold->sa;
        g.sfb = fold->sb;
        g.pfa = fold->pa;
        g.pfb = fold->pb;
        g.pf = c.pfold_vec(level);
    }
    if (scatter) {
        g.pm = c.pmodq_vec(level);
        g.scatter = scatter;
        g.base = base;
        g.sbase = dst.sbase;
    }
    g.cx = cx;
    g.ext = ext;
    g.key = key.data;
    g.acc = dst.out;
    g.scx = scx;
    g.sext = sext;
    g.sacc = dst.sout;
    g.mods = c.d_mods;
    g.logn = c.logn;
    g.L = level + 1;
    g.np = c.np;
    g.nq = c.nq;
    g.beta = (g.L + c.np - 1) / c.np;
    g.klvl = key.level;
    g.kcomp = key.level + 1 + c.np;
    LSA_REQUIRE(key.level >= level, "key-switch key exported at a lower level than the ciphertext");
    int targets = g.L + c.np;
    if (unfused_only) {   // the others went through the fused kernel
        LSA_REQUIRE(targets <= 64, "key MAC: too many target limbs for a subset launch");
        for (int tl = 0; tl < targets; tl++)
            if (!ks_fused_limb(c, g.L, tl) || tl == extra_tl) g.tl_list[g.n_tl++] = (unsigned char)tl;
        if (!g.n_tl) return;
        targets = g.n_tl;
    }
    const double T = targets;
    int q_targets = 0;   // (tensor fold: the own digit of a Q target reads a0, a1, b0, b1 instead of cx)
    for (int i = 0; i < targets; i++) q_targets += (g.n_tl ? g.tl_list[i] : i) < g.L;
    ProfScope ps(c, PROF_KSMAC, 8.0 * c.n * (batch * (g.beta * T + 2 * T * (accumulate ? 2 : 1) + (scatter && base ? g.L : 0) + (fold ? 3.0 * q_targets : 0.0)) +
                                             2.0 * g.beta * T), s);
    // enough workgroups to fill the chip, as few key re-reads as possible
    const dim3 grid1 = ew_grid(c, targets, 1);
    const KsMacGroups gr = ks_mac_groups(grid1.x, batch);
    g.batch = batch;
    g.bpt = gr.bpt;
    const dim3 grid(grid1.x, (unsigned)gr.gy);
    if (scatter && accumulate) launch_ks_mac_kb<true, false, true>(g.beta, grid, s, g);
    else if (scatter) launch_ks_mac_kb<true>(g.beta, grid, s, g);
    else if (fold) launch_ks_mac_kb<false, true>(g.beta, grid, s, g);
    else launch_ks_mac_kb<false>(g.beta, grid, s, g);
    LSA_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ (a-b)*k, a*k, ModDown tail
struct SubMulArgs {
    const u64* a;
    const u64* b;     // may be null: out = a*k
    const u64* base;  // may be null: else out += base
    const u64* kvec;  // per row-class constant, Montgomery form, indexed like mod_of
    u64* out;
    long long sa, sb, sbase, so;
    int a_rpp, b_rpp, base_rpp, out_rpp;  // rows per polynomial of each operand (row = poly*rpp + limb)
    int base_polys;                       // base is added to polynomials [0, base_polys)
    int limbs, logn;
    const ModDev* mods;
    unsigned char mod_of[LSA_MAX_PERIOD];  // per limb
};

// grid: x = polys*limbs*(N/2/TPB), y = batch
__global__ __launch_bounds__(TPB) void k_sub_mul(SubMulArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int pl = blockIdx.x / chunks;
    const int poly = pl / g.limbs, limb = pl % g.limbs;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const ModDev m = g.mods[g.mod_of[limb]];
    const u64 k = g.kvec[limb];
    const long long b = blockIdx.y;
    ulonglong2 va = ld2(g.a + b * g.sa + (((long long)poly * g.a_rpp + limb) << g.logn) + x);
    if (g.b) {
        const ulonglong2 vb = ld2(g.b + b * g.sb + (((long long)poly * g.b_rpp + limb) << g.logn) + x);
        va.x = sub_mod(va.x, vb.x, m.q);
        va.y = sub_mod(va.y, vb.y, m.q);
    }
    u64 r0 = mont_mul(va.x, k, m.q, m.qinv), r1 = mont_mul(va.y, k, m.q, m.qinv);
    if (g.base && poly < g.base_polys) {
        const ulonglong2 vc = ld2(g.base + b * g.sbase + (((long long)poly * g.base_rpp + limb) << g.logn) + x);
        r0 = add_mod(r0, vc.x, m.q);
        r1 = add_mod(r1, vc.y, m.q);
    }
    st2(g.out + b * g.so + (((long long)poly * g.out_rpp + limb) << g.logn) + x, r0, r1);
}

void launch_sub_mul_general(Context& c, int polys, int limbs, const unsigned char* limb_mod, const u64* kvec,
                                   const u64* a, long long sa, int a_rpp, const u64* b, long long sb, int b_rpp,
                                   const u64* base, long long sbase, int base_rpp, int base_polys, u64* out,
                                   long long so, int out_rpp, int batch, hipStream_t s) {
    if (batch <= 0) return;
    SubMulArgs g{};
    g.a = a;
    g.b = b;
    g.base = base;
    g.kvec = kvec;
    g.out = out;
    g.sa = sa;
    g.sb = sb;
    g.sbase = sbase;
    g.so = so;
    g.a_rpp = a_rpp;
    g.b_rpp = b_rpp;
    g.base_rpp = base_rpp;
    g.base_polys = base_polys;
    g.out_rpp = out_rpp;
    g.limbs = limbs;
    g.logn = c.logn;
    g.mods = c.d_mods;
    LSA_REQUIRE(limbs <= LSA_MAX_PERIOD, "too many limbs");
    for (int i = 0; i < limbs; i++) g.mod_of[i] = limb_mod[i];
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * polys * limbs * batch * (2 + (b != nullptr) + (base != nullptr)), s);
    hipLaunchKernelGGL(k_sub_mul, ew_grid(c, polys * limbs, batch), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

void launch_moddown_final(Context& c, int level, const u64* acc, long long sacc, int acc_rpp, const u64* conv,
                          long long sconv, const u64* base, long long sbase, int base_rpp, int base_polys, u64* out,
                          long long sout, int batch, hipStream_t s) {
    const int L = level + 1;
    std::vector<int> mods(L);
    std::vector<u64> pinv(L);
    unsigned char lm[LSA_MAX_PERIOD];
    for (int i = 0; i < L; i++) {
        mods[i] = i;
        lm[i] = (unsigned char)i;
        u64 q = c.T.mod[i], pr = 1;
        for (int l = 0; l < c.np; l++) pr = mul_mod_host(pr, c.T.mod[c.p_mod(l)] % q, q);
        pinv[i] = inv_mod(pr, q);
    }
    const u64* kv = c.const_vec("pinv" + std::to_string(L), mods, pinv);
    launch_sub_mul_general(c, 2, L, lm, kv, acc, sacc, acc_rpp, conv, sconv, L, base, sbase, base_rpp, base_polys, out,
                           sout, L, batch, s);
}

// The coefficient-domain ModDown tail followed by the automorphism of a rotation, in one pass (hoisted BFV rotations):
//   out[h][j][i] = s_i * ((acc[h][j][pi_i] - conv[h][j][pi_i]) * P^-1 + (h < base_polys ? base[h][j][pi_i] : 0))
// pi_i = perm[i] & 0x7fffffff, s_i = -1 where bit 31 is set (Context::coeff_perm, the table of k_permute): residue for residue
// launch_permute_coeff(launch_moddown_final(...)) without the intermediate.  The row skeleton of moddown_gather.h with the plainest
// policy: one workgroup per (row, batch item), the row computed with coalesced loads into LDS (8N bytes: N <= 2^14,
// LSA_PERM_LDS_MAX_LOGN), then gathered from LDS and stored coalesced, two words per lane.  The key switch reaches it through its
// tail hook (KsPermTail, key_switch.h).  Gathering from global memory instead (three gathered 8-byte streams per output through L2)
// measured slower than the two-step form at N = 2^14 and 2^16: larger rings keep the two steps.
struct SubMulPermArgs {
    RowTailArgs t;
    int base_rpp, base_polys;
};

struct SubMulPermOp {   // out = sign * (value + base): the base joins the staged row, nothing crosses the barrier
    struct Keep {};
    static constexpr bool KEEPS = false;
    const u64* c;   // the row of base, or null
    u64* o;
    u64 q;
    __device__ __forceinline__ void stage(int x, int, ulonglong2& r, Keep&) const {
        if (!c) return;
        const ulonglong2 vc = ld2(c + x);
        r.x = add_mod(r.x, vc.x, q);
        r.y = add_mod(r.y, vc.y, q);
    }
    __device__ __forceinline__ void finish(int y, const Keep&, ulonglong2 s) const { st2(o + y, s.x, s.y); }
};

__global__ __launch_bounds__(LSA_LDS_ROW_THREADS) void k_sub_mul_perm(SubMulPermArgs g) {
    const int poly = blockIdx.x / g.t.limbs, limb = blockIdx.x % g.t.limbs;
    const long long b = blockIdx.y;
    const u64* c = g.t.base && poly < g.base_polys ? g.t.base + b * g.t.sbase + (((long long)poly * g.base_rpp + limb) << g.t.logn) : nullptr;
    u64* o = g.t.out + b * g.t.sout + (((long long)poly * g.t.limbs + limb) << g.t.logn);
    gathered_tail_row(g.t, SubMulPermOp{c, o, g.t.mods[limb].q});
}

void KsPermTail::launch(Context& c, int level, const u64* acc, long long s_acc, int acc_rpp, const u64* conv, long long s_conv,
                        const KsOut& o, int nb, hipStream_t s) const {
    if (nb <= 0) return;
    const int L = level + 1;
    LSA_REQUIRE(perm != nullptr, "gathered ModDown tail: permutation missing");
    LSA_REQUIRE(o.base_polys == 0 || o.base, "gathered ModDown tail: base polynomial missing");
    SubMulPermArgs g{};
    g.t.perm = perm;
    g.base_rpp = o.base_rpp;
    g.base_polys = o.base ? o.base_polys : 0;
    // acc, conv and out for both polynomials, base for base_polys of them, the permutation table (4 bytes per point) per row
    launch_lds_row_tail<&k_sub_mul_perm>(c, level, "gathered ModDown tail", g, acc, s_acc, acc_rpp, conv, s_conv, o, nb,
                                         8.0 * c.n * nb * (3.0 * 2 * L + (double)g.base_polys * L) + 4.0 * c.n * 2 * L * nb, s);
}

void launch_sub_mul_const(Context& c, const u64* a, long long sa, const u64* b, long long sb, const u64* kvec, u64* out,
                          long long so, int rows, const RowMap& rm, int batch, hipStream_t s) {
    launch_sub_mul_general(c, 1, rows, rm.mod_of, kvec, a, sa, rows, b, sb, rows, nullptr, 0, 0, 0, out, so, rows, batch,
                           s);
}

void launch_mul_const(Context& c, const u64* a, long long sa, const u64* kvec, u64* out, long long so, int rows,
                      const RowMap& rm, int batch, hipStream_t s) {
    launch_sub_mul_general(c, 1, rows, rm.mod_of, kvec, a, sa, rows, nullptr, 0, 0, nullptr, 0, 0, 0, out, so, rows,
                           batch, s);
}

// ------------------------------------------------------------------------------------------------ rescale (K9)
struct RescaleArgs {
    const u64* last;  // [batch][polys][N] coefficient-domain last limb
    u64* tmp;         // [batch][polys][level][N]
    long long slast, stmp;
    const ModDev* mods;
    int level, polys, logn;
};

// tmp[p][i] = ((last + h) mod q_l) mod q_i - (h mod q_i),  h = (q_l-1)/2     (divide-and-round, centred remainder)
__global__ __launch_bounds__(TPB) void k_rescale_prep(RescaleArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int pl = blockIdx.x / chunks;
    const int poly = pl / g.level, limb = pl % g.level;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const long long b = blockIdx.y;
    const ModDev ml = g.mods[g.level], mi = g.mods[limb];
    const u64 h = (ml.q - 1) >> 1;
    const u64 hq = reduce_u64(h, mi);
    const ulonglong2 v = ld2(g.last + b * g.slast + ((long long)poly << g.logn) + x);
    const u64 r0 = sub_mod(reduce_u64(add_mod(v.x, h, ml.q), mi), hq, mi.q);
    const u64 r1 = sub_mod(reduce_u64(add_mod(v.y, h, ml.q), mi), hq, mi.q);
    st2(g.tmp + b * g.stmp + (((long long)poly * g.level + limb) << g.logn) + x, r0, r1);
}

void launch_rescale_prep(Context& c, int level, int polys, const u64* last, long long slast, u64* tmp, long long stmp,
                         int batch, hipStream_t s) {
    if (batch <= 0) return;
    RescaleArgs g{};
    g.last = last;
    g.tmp = tmp;
    g.slast = slast;
    g.stmp = stmp;
    g.mods = c.d_mods;
    g.level = level;
    g.polys = polys;
    g.logn = c.logn;
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * polys * (level + 1) * batch, s);
    hipLaunchKernelGGL(k_rescale_prep, ew_grid(c, polys * level, batch), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

void launch_rescale_final(Context& c, int level, int polys, const u64* in, long long sin, const u64* tmp, long long stmp,
                          u64* out, long long sout, int batch, hipStream_t s) {
    std::vector<int> mods(level);
    std::vector<u64> qlinv(level);
    unsigned char lm[LSA_MAX_PERIOD];
    const u64 ql = c.T.mod[level];
    for (int i = 0; i < level; i++) {
        mods[i] = i;
        lm[i] = (unsigned char)i;
        qlinv[i] = inv_mod(ql % c.T.mod[i], c.T.mod[i]);
    }
    const u64* kv = c.const_vec("qlinv" + std::to_string(level), mods, qlinv);
    launch_sub_mul_general(c, polys, level, lm, kv, in, sin, level + 1, tmp, stmp, level, nullptr, 0, 0, 0, out, sout,
                           level, batch, s);
}

// ------------------------------------------------------------------------------------------------ automorphisms (K10)
struct PermArgs {
    const u32* perm;
    const u64* in;
    u64* out;
    long long sin, sout;
    const ModDev* mods;
    int rows, logn, with_sign, period;
    unsigned char mod_of[LSA_MAX_PERIOD];
};

// out[row][i] = (+/-) in[row][perm[i] & 0x7fffffff]; sign bit 31 negates (coefficient-domain automorphism)
__global__ __launch_bounds__(TPB) void k_permute(PermArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int row = blockIdx.x / chunks;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const long long b = blockIdx.y;
    const u64* in = g.in + b * g.sin + ((long long)row << g.logn);
    const uint2 p = *reinterpret_cast<const uint2*>(g.perm + x);
    u64 r0 = in[p.x & 0x7fffffffu], r1 = in[p.y & 0x7fffffffu];
    if (g.with_sign) {
        const u64 q = g.mods[g.mod_of[row % g.period]].q;
        if (p.x >> 31) r0 = neg_mod(r0, q);
        if (p.y >> 31) r1 = neg_mod(r1, q);
    }
    st2(g.out + b * g.sout + ((long long)row << g.logn) + x, r0, r1);
}

void launch_permute_ntt(Context& c, const u32* perm, const u64* in, long long sin, u64* out, long long sout, int rows,
                        int batch, hipStream_t s) {
    if (batch <= 0) return;
    PermArgs g{};
    g.perm = perm;
    g.in = in;
    g.out = out;
    g.sin = sin;
    g.sout = sout;
    g.mods = c.d_mods;
    g.rows = rows;
    g.logn = c.logn;
    g.with_sign = 0;
    g.period = 1;
    ProfScope ps(c, PROF_ELEMWISE, 16.0 * c.n * rows * batch, s);
    hipLaunchKernelGGL(k_permute, ew_grid(c, rows, batch), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

// Extended (Q_level u P) ciphertexts, the operands of double-hoisted linear transforms: a rotation WITHOUT its division by P.
//   out[h][tl][i] (+)= acc[h][tl][perm[i]] + (tl < L and h < base_polys ? P * base[h][tl][perm[i]] mod q_tl : 0)
// acc = the gadget product [2][T][N] (null: zero), base = the ciphertext [2][L][N] whose c0 (base_polys = 1) or both
// polynomials (2: the plain lift of a ciphertext) enter times P; perm null = identity.
struct PermExtArgs {
    const u32* perm;
    const u64* acc;
    const u64* base;
    const u64* pm;   // [L] P mod q_j, Montgomery form
    u64* out;
    long long sacc, sbase, sout;
    const ModDev* mods;
    int L, T, logn, accumulate, base_polys;
    unsigned char mod_of[LSA_MAX_PERIOD];   // [T]
};

__global__ __launch_bounds__(TPB) void k_permute_ext(PermExtArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int row = blockIdx.x / chunks;
    const int h = row / g.T, tl = row - h * g.T;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const long long b = blockIdx.y;
    const ModDev m = g.mods[g.mod_of[tl]];
    unsigned i0 = (unsigned)x, i1 = (unsigned)x + 1;
    if (g.perm) {
        const uint2 p = *reinterpret_cast<const uint2*>(g.perm + x);
        i0 = p.x;
        i1 = p.y;
    }
    u64 r0 = 0, r1 = 0;
    if (g.acc) {
        const u64* in = g.acc + b * g.sacc + ((long long)row << g.logn);
        r0 = in[i0];
        r1 = in[i1];
    }
    if (tl < g.L && h < g.base_polys) {
        const u64* bs = g.base + b * g.sbase + ((long long)(h * g.L + tl) << g.logn);
        const u64 k = g.pm[tl];
        r0 = add_mod(r0, mont_mul(bs[i0], k, m.q, m.qinv), m.q);
        r1 = add_mod(r1, mont_mul(bs[i1], k, m.q, m.qinv), m.q);
    }
    u64* o = g.out + b * g.sout + ((long long)row << g.logn) + x;
    if (g.accumulate) {
        const ulonglong2 v = ld2(o);
        r0 = add_mod(r0, v.x, m.q);
        r1 = add_mod(r1, v.y, m.q);
    }
    st2(o, r0, r1);
}

void launch_permute_ext(Context& c, int level, const u32* perm, const u64* acc, long long sacc, const u64* base, long long sbase,
                        int base_polys, u64* out, long long sout, bool accumulate, int batch, hipStream_t s) {
    if (batch <= 0) return;
    const int L = level + 1, T = L + c.np;
    LSA_REQUIRE(T <= LSA_MAX_PERIOD, "extended ciphertext: too many limbs");
    LSA_REQUIRE(base_polys == 0 || base, "extended ciphertext: base polynomial missing");
    PermExtArgs g{};
    g.perm = perm;
    g.acc = acc;
    g.base = base;
    g.out = out;
    g.sacc = sacc;
    g.sbase = sbase;
    g.sout = sout;
    g.mods = c.d_mods;
    g.L = L;
    g.T = T;
    g.logn = c.logn;
    g.accumulate = accumulate ? 1 : 0;
    g.base_polys = base_polys;
    g.pm = c.pmodq_vec(level);
    for (int tl = 0; tl < T; tl++) g.mod_of[tl] = (unsigned char)c.qp_mod(L, tl);
    const double streams = (acc ? 1.0 : 0.0) * 2 * T + (double)base_polys * L + (accumulate ? 2.0 : 1.0) * 2 * T;
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * streams * batch, s);
    hipLaunchKernelGGL(k_permute_ext, ew_grid(c, 2 * T, batch), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

void launch_permute_coeff(Context& c, const u32* perm, const u64* in, long long sin, u64* out, long long sout, int rows,
                          const RowMap& rm, int batch, hipStream_t s) {
    if (batch <= 0) return;
    PermArgs g{};
    g.perm = perm;
    g.in = in;
    g.out = out;
    g.sin = sin;
    g.sout = sout;
    g.mods = c.d_mods;
    g.rows = rows;
    g.logn = c.logn;
    g.with_sign = 1;
    fill_rowmap(g.mod_of, g.period, rm, c.nmod);
    ProfScope ps(c, PROF_ELEMWISE, 16.0 * c.n * rows * batch, s);
    hipLaunchKernelGGL(k_permute, ew_grid(c, rows, batch), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ row copy (K12) / to-Montgomery
struct CopyRowsArgs {
    const u64* in;
    u64* out;
    long long sin, sout;
    int rows, logn;
    short src_row[LSA_MAX_PERIOD];
};

__global__ __launch_bounds__(TPB) void k_copy_rows(CopyRowsArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int row = blockIdx.x / chunks;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const long long b = blockIdx.y;
    const ulonglong2 v = ld2(g.in + b * g.sin + ((long long)g.src_row[row] << g.logn) + x);
    st2(g.out + b * g.sout + ((long long)row << g.logn) + x, v.x, v.y);
}

void launch_copy_rows(Context& c, const u64* in, long long sin, u64* out, long long sout, int rows, const int* src_row,
                      int batch, hipStream_t s) {
    if (batch <= 0 || rows <= 0) return;
    LSA_REQUIRE(rows <= LSA_MAX_PERIOD, "copy_rows: too many rows");
    CopyRowsArgs g{};
    g.in = in;
    g.out = out;
    g.sin = sin;
    g.sout = sout;
    g.rows = rows;
    g.logn = c.logn;
    for (int i = 0; i < rows; i++) g.src_row[i] = (short)src_row[i];
    ProfScope ps(c, PROF_ELEMWISE, 16.0 * c.n * rows * batch, s);
    hipLaunchKernelGGL(k_copy_rows, ew_grid(c, rows, batch), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

struct ToMontArgs {
    u64* data;
    const ModDev* mods;
    int logn, period;
    unsigned char mod_of[LSA_MAX_PERIOD];
};

__global__ __launch_bounds__(TPB) void k_to_mont(ToMontArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int row = blockIdx.x / chunks;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const ModDev m = g.mods[g.mod_of[row % g.period]];
    u64* p = g.data + ((long long)row << g.logn) + x;
    const ulonglong2 v = ld2(p);
    st2(p, mont_mul(v.x, m.r2, m.q, m.qinv), mont_mul(v.y, m.r2, m.q, m.qinv));
}

void launch_to_mont(Context& c, u64* data, int rows, const RowMap& rm, hipStream_t s) {
    if (rows <= 0) return;
    ToMontArgs g{};
    g.data = data;
    g.mods = c.d_mods;
    g.logn = c.logn;
    fill_rowmap(g.mod_of, g.period, rm, c.nmod);
    hipLaunchKernelGGL(k_to_mont, ew_grid(c, rows, 1), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

// a freshly loaded key: plain residues -> Montgomery form in place, and (fp != null) the same values as doubles for the limbs
// the FP64 engine can serve -- whether it is switched on or not (lsa_set_fp64_ntt may turn it on after the upload)
struct KeyPrepArgs {
    u64* data;
    double* fp;
    const ModDev* mods;
    int logn, period;
    unsigned char mod_of[LSA_MAX_PERIOD];
};
__global__ __launch_bounds__(TPB) void k_key_prepare(KeyPrepArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int row = blockIdx.x / chunks;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const ModDev m = g.mods[g.mod_of[row % g.period]];
    const long long off = ((long long)row << g.logn) + x;
    const ulonglong2 v = ld2(g.data + off);
    st2(g.data + off, mont_mul(v.x, m.r2, m.q, m.qinv), mont_mul(v.y, m.r2, m.q, m.qinv));
    if (g.fp) {
        const bool fp = (m.q >> LSA_FP64_MAX_BITS) == 0;
        double2 d;
        d.x = fp ? (double)v.x : 0.0;
        d.y = fp ? (double)v.y : 0.0;
        *reinterpret_cast<double2*>(g.fp + off) = d;
    }
}
KeyLayout key_layout(const Context& c, int key_level) {
    KeyLayout k;
    if (c.np < 1 || key_level < 0 || key_level >= c.nq) return k;
    const int comp = key_level + 1 + c.np, beta = (key_level + 1 + c.np - 1) / c.np;
    k.words = (size_t)beta * 2 * comp * c.n;
    k.fp = ks_fused_enabled(c);
    return k;
}
void key_prepare(Context& c, Key& key, u64* data, int key_level, double* fp, hipStream_t s) {
    const int comp = key_level + 1 + c.np;
    LSA_REQUIRE(comp <= LSA_MAX_PERIOD, "key has too many limbs");
    KeyPrepArgs g{};
    g.data = data;
    g.fp = fp;
    g.mods = c.d_mods;
    g.logn = c.logn;
    g.period = comp;
    for (int j = 0; j < comp; j++) g.mod_of[j] = (unsigned char)c.qp_mod(key_level + 1, j);
    hipLaunchKernelGGL(k_key_prepare, ew_grid(c, (int)(key_layout(c, key_level).words >> c.logn), 1), dim3(TPB), 0, s, g);   // [beta][2][comp] rows
    LSA_HIP(hipGetLastError());
    key.data = data;
    key.level = key_level;
    key.fp = fp;
}

// ------------------------------------------------------------------------------------------------ ring-t plaintext lifts (K11)
// A ring-t plaintext is one coefficient-domain limb (plug-in/lattigo/acc/c_struct_import_export.go:179-184).
//   mode 0 (CKKS): residues mod q_src as CENTRED integers -> every q_i
//   mode 1 (BFV multiply): message mod t used directly as residues mod q_i
//   mode 2 (BFV add/sub): scale up by Q/t with rounding: u = (m*[Q]_t + t/2) mod t, out_i = (u - t/2) * (-t^-1) mod q_i
struct LiftArgs {
    const u64* pt;
    u64* out;
    long long spt, sout;
    const ModDev* mods;
    const u64* neg_tinv;   // mode 2: -(t^-1) mod q_i, Montgomery form
    u64 t, qmodt;
    int mode, src_mod, logn, limbs;
};

__global__ __launch_bounds__(TPB) void k_lift_ringt(LiftArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int limb = blockIdx.x / chunks;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const long long b = blockIdx.y;
    const ModDev mi = g.mods[limb];
    const ulonglong2 v = ld2(g.pt + b * g.spt + x);
    u64 r[2] = {v.x, v.y};
#pragma unroll
    for (int e = 0; e < 2; e++) {
        if (g.mode == 0) {
            const u64 q0 = g.mods[g.src_mod].q;
            r[e] = r[e] > (q0 >> 1) ? neg_mod(reduce_u64(q0 - r[e], mi), mi.q) : reduce_u64(r[e], mi);
        } else if (g.mode == 1) {
            r[e] = reduce_u64(r[e], mi);
        } else {
            const u64 thalf = g.t >> 1;
            const u64 u = ((r[e] % g.t) * g.qmodt + thalf) % g.t;   // t < 2^32: the product fits 64 bits
            r[e] = mont_mul(sub_mod(reduce_u64(u, mi), reduce_u64(thalf, mi), mi.q), g.neg_tinv[limb], mi.q, mi.qinv);
        }
    }
    st2(g.out + b * g.sout + ((long long)limb << g.logn) + x, r[0], r[1]);
}

void launch_lift_ringt(Context& c, int mode, int level, const u64* pt, long long spt, u64* out, long long sout, int batch,
                       hipStream_t s) {
    if (batch <= 0) return;
    const int L = level + 1;
    LiftArgs g{};
    g.pt = pt;
    g.out = out;
    g.spt = spt;
    g.sout = sout;
    g.mods = c.d_mods;
    g.mode = mode;
    g.src_mod = 0;
    g.logn = c.logn;
    g.limbs = L;
    if (mode == 2) {
        LSA_REQUIRE(c.t > 1 && c.t < (1ull << 32), "ring-t scale-up needs a plaintext modulus below 2^32");
        g.t = c.t;
        u64 qm = 1 % c.t;
        for (int i = 0; i < L; i++) qm = mul_mod_host(qm, c.T.mod[i] % c.t, c.t);
        g.qmodt = qm;
        std::vector<int> mods(L);
        std::vector<u64> v(L);
        for (int i = 0; i < L; i++) {
            mods[i] = i;
            v[i] = c.T.mod[i] - inv_mod(c.t % c.T.mod[i], c.T.mod[i]);
        }
        g.neg_tinv = c.const_vec("neg_tinv" + std::to_string(L), mods, v);
    }
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * (1 + L) * batch, s);
    hipLaunchKernelGGL(k_lift_ringt, ew_grid(c, L, batch), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ CKKS plaintext / constant operands
// The encoder's device half: v [batch][N] rounded coefficients (signed 64-bit) -> out [batch][limbs][N], row j = v mod q_j in
// [0, q_j) (plain_ops.h lift_i64).  The host uploads 8N bytes per plaintext instead of 8 (level + 1) N; launch_ntt then
// transforms the rows in place.  grid: x = limbs * (N/2/TPB), y = batch
struct LiftI64Args {
    const long long* v;
    u64* out;
    long long sv, so;
    const ModDev* mods;
    int logn;
};
__global__ __launch_bounds__(TPB) void k_lift_i64(LiftI64Args g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int limb = blockIdx.x / chunks;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const long long b = blockIdx.y;
    const ModDev m = g.mods[limb];
    const longlong2 v = *reinterpret_cast<const longlong2*>(g.v + b * g.sv + x);
    st2(g.out + b * g.so + ((long long)limb << g.logn) + x, lift_i64(v.x, m), lift_i64(v.y, m));
}
void launch_lift_i64(Context& c, const long long* v, long long sv, u64* out, long long so, int limbs, int batch, hipStream_t s) {
    if (batch <= 0 || limbs <= 0) return;
    LSA_REQUIRE(limbs <= c.nq, "lift_i64: more rows than the Q chain has primes");
    LiftI64Args g{};
    g.v = v;
    g.out = out;
    g.sv = sv;
    g.so = so;
    g.mods = c.d_mods;
    g.logn = c.logn;
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * (1 + limbs) * batch, s);
    hipLaunchKernelGGL(k_lift_i64, ew_grid(c, limbs, batch), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

// Ciphertext times / plus a complex constant (plain_ops.h): out[p][j][x] = a[p][j][x] * k(j, x) (MUL) + beta(j, x) (ADD, on
// polynomial 0 only), k and beta one of two per-limb constants picked by bit `sel_bit` of the point's index (the sign of
// X^(N/2) there).  No plaintext is read: one read and one write per row.  An addition alone copies polynomial 1.
// grid: x = rows * (N/2/TPB), y = batch; rows = 2 * limbs, or limbs for an addition in place
struct CconstArgs {
    const u64* a;
    u64* out;
    long long sa, so;
    const ModDev* mods;
    int limbs, logn, sel_bit, sel_pol;   // point x takes the "minus" constants when ((x >> sel_bit) & 1) != sel_pol
    CconstLimb k[LSA_CCONST_MAX_LIMBS];
};
template <bool MUL, bool ADD>
__global__ __launch_bounds__(TPB) void k_cconst(CconstArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int row = blockIdx.x / chunks;             // poly * limbs + limb
    const int limb = row % g.limbs;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const long long b = blockIdx.y, off = ((long long)row << g.logn) + x;
    const ulonglong2 v = ld2(g.a + b * g.sa + off);
    const bool add = ADD && row < g.limbs;
    if (!MUL && !add) {
        st2(g.out + b * g.so + off, v.x, v.y);
        return;
    }
    const ModDev m = g.mods[limb];
    const CconstLimb k = g.k[limb];
    const bool m0 = ((x >> g.sel_bit) & 1) != g.sel_pol, m1 = (((x + 1) >> g.sel_bit) & 1) != g.sel_pol;
    u64 r0, r1;
    if (add) {
        r0 = cconst_word<MUL, true>(v.x, m0 ? k.k_minus : k.k_plus, m0 ? k.b_minus : k.b_plus, m);
        r1 = cconst_word<MUL, true>(v.y, m1 ? k.k_minus : k.k_plus, m1 ? k.b_minus : k.b_plus, m);
    } else {
        r0 = cconst_word<MUL, false>(v.x, m0 ? k.k_minus : k.k_plus, 0, m);
        r1 = cconst_word<MUL, false>(v.y, m1 ? k.k_minus : k.k_plus, 0, m);
    }
    st2(g.out + b * g.so + off, r0, r1);
}
void launch_cconst(Context& c, bool mul, bool add, const u64* a, long long sa, const CconstLimb* k, int sel_bit, int sel_pol,
                   u64* out, long long so, int limbs, int batch, hipStream_t s) {
    if (batch <= 0 || limbs <= 0) return;
    LSA_REQUIRE(mul || add, "cconst: nothing to do");
    LSA_REQUIRE(limbs <= c.nq && limbs <= LSA_CCONST_MAX_LIMBS, "cconst: too many limbs for one launch");
    LSA_REQUIRE(sel_bit >= 0 && sel_bit < c.logn && (sel_pol == 0 || sel_pol == 1), "cconst: bad selector");
    CconstArgs g{};
    g.a = a;
    g.out = out;
    g.sa = sa;
    g.so = so;
    g.mods = c.d_mods;
    g.limbs = limbs;
    g.logn = c.logn;
    g.sel_bit = sel_bit;
    g.sel_pol = sel_pol;
    for (int j = 0; j < limbs; j++) g.k[j] = k[j];
    const int rows = !mul && out == a && so == sa ? limbs : 2 * limbs;   // an addition in place leaves polynomial 1 alone
    ProfScope ps(c, PROF_ELEMWISE, 16.0 * c.n * rows * batch, s);
    const dim3 grid = ew_grid(c, rows, batch);
    if (mul && add) hipLaunchKernelGGL((k_cconst<true, true>), grid, dim3(TPB), 0, s, g);
    else if (mul) hipLaunchKernelGGL((k_cconst<true, false>), grid, dim3(TPB), 0, s, g);
    else hipLaunchKernelGGL((k_cconst<false, true>), grid, dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ probes (ceilings for DESIGN.md)
__global__ __launch_bounds__(TPB) void k_probe_copy(u64* dst, const u64* src, size_t n2) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n2; i += (size_t)gridDim.x * TPB) {
        const ulonglong2 v = ld2(src + 2 * i);
        st2(dst + 2 * i, v.x, v.y);
    }
}
void launch_probe_copy(u64* dst, const u64* src, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_probe_copy, dim3(256 * 8), dim3(TPB), 0, s, dst, src, n / 2);
    LSA_HIP(hipGetLastError());
}

// dependent chains of Montgomery multiplies, 4 independent chains per lane: measures the 64-bit modmul issue ceiling
__global__ __launch_bounds__(TPB) void k_probe_mulhi(u64* buf, size_t n, int iters) {
    const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i * 4 + 3 >= n) return;
    const u64 q = 0x1FFFFFFFFFE00001ull, qinv = 1;  // constants irrelevant for timing
    u64 a = buf[4 * i], b = buf[4 * i + 1], c = buf[4 * i + 2], d = buf[4 * i + 3];
    const u64 w = a | 1;
    for (int it = 0; it < iters; it++) {
        a = mont_mul_lazy(a, w, q, qinv + it);
        b = mont_mul_lazy(b, w, q, qinv + it);
        c = mont_mul_lazy(c, w, q, qinv + it);
        d = mont_mul_lazy(d, w, q, qinv + it);
    }
    buf[4 * i] = a;
    buf[4 * i + 1] = b;
    buf[4 * i + 2] = c;
    buf[4 * i + 3] = d;
}
// the same chains with Shoup/Harvey multiplication by a constant with precomputed quotient w' = floor(w*2^64/q):
// r = w*v - mulhi(w', v)*q  (mod 2^64), in [0, 2q)
__device__ __forceinline__ u64 shoup_mul_lazy(u64 v, u64 w, u64 wq, u64 q) {
    const u64 t = mulhi64(wq, v);
    return mul_lo64(w, v) - mul_lo64(t, q);
}
__global__ __launch_bounds__(TPB) void k_probe_shoup(u64* buf, size_t n, int iters) {
    const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i * 4 + 3 >= n) return;
    const u64 q = 0x1FFFFFFFFFE00001ull;
    u64 a = buf[4 * i], b = buf[4 * i + 1], c = buf[4 * i + 2], d = buf[4 * i + 3];
    const u64 w = a | 1, wq = b | 1;
    for (int it = 0; it < iters; it++) {
        a = shoup_mul_lazy(a, w, wq + it, q);
        b = shoup_mul_lazy(b, w, wq + it, q);
        c = shoup_mul_lazy(c, w, wq + it, q);
        d = shoup_mul_lazy(d, w, wq + it, q);
    }
    buf[4 * i] = a;
    buf[4 * i + 1] = b;
    buf[4 * i + 2] = c;
    buf[4 * i + 3] = d;
}
// the same chains on the FP64 engine's exact modular product (6 double operations: mul, fma, mul, rndne, fma, add)
__global__ __launch_bounds__(TPB) void k_probe_fp(u64* buf, size_t n, int iters) {
    const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i * 4 + 3 >= n) return;
    const double q = 70368744161281.0, qinv = 1.0 / q;   // a 46-bit modulus; values irrelevant for timing
    double a = (double)(buf[4 * i] & 0xFFFFFFFFFFull), b = (double)(buf[4 * i + 1] & 0xFFFFFFFFFFull);
    double c = (double)(buf[4 * i + 2] & 0xFFFFFFFFFFull), d = (double)(buf[4 * i + 3] & 0xFFFFFFFFFFull);
    const double w = a + 1.0;
    for (int it = 0; it < iters; it++) {
        a = fp_modmul(a, w + it, q, qinv);
        b = fp_modmul(b, w + it, q, qinv);
        c = fp_modmul(c, w + it, q, qinv);
        d = fp_modmul(d, w + it, q, qinv);
    }
    buf[4 * i] = (u64)(long long)a;
    buf[4 * i + 1] = (u64)(long long)b;
    buf[4 * i + 2] = (u64)(long long)c;
    buf[4 * i + 3] = (u64)(long long)d;
}
void launch_probe_mulhi(u64* buf, size_t n, int iters, hipStream_t s) {
    if (iters >= (1 << 20)) {   // offset by 2^20: the FP64 variant
        const size_t threads = n / 4;
        hipLaunchKernelGGL(k_probe_fp, dim3((unsigned)((threads + TPB - 1) / TPB)), dim3(TPB), 0, s, buf, n, iters - (1 << 20));
        LSA_HIP(hipGetLastError());
        return;
    }
    if (iters < 0) {   // negative: the Shoup variant
        const size_t threads = n / 4;
        hipLaunchKernelGGL(k_probe_shoup, dim3((unsigned)((threads + TPB - 1) / TPB)), dim3(TPB), 0, s, buf, n, -iters);
        LSA_HIP(hipGetLastError());
        return;
    }
    const size_t threads = n / 4;
    hipLaunchKernelGGL(k_probe_mulhi, dim3((unsigned)((threads + TPB - 1) / TPB)), dim3(TPB), 0, s, buf, n, iters);
    LSA_HIP(hipGetLastError());
}

}  // namespace lsa
