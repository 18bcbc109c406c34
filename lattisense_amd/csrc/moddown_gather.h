// moddown_gather.h — the coefficient-domain ModDown tail that applies a rotation by a signed gather, written once:
//   r[x]   = (acc[x] - conv[x]) * P^-1 (+ the operator's term on polynomial 0)     staged in an 8N-byte LDS row, coalesced
//   out    = finish(sign_y * r[pi_y])                                              gathered from LDS after one barrier
// One workgroup of LSA_LDS_ROW_THREADS per (row, batch item), N <= 2^LSA_PERM_LDS_MAX_LOGN.  The operator is a policy `Op`:
//   Op::Keep, Op::KEEPS   the registers a point pair carries across the barrier (KEEPS false: none, Keep is empty)
//   op.stage(x, poly, r, keep)   adds the operator's polynomial-0 term to r at the points (x, x + 1) and fills keep
//   op.finish(y, keep, s)        stores the operator's result at (y, y + 1) from the signed gathered pair s
// k_sub_mul_perm (kernels.hip), k_bfv_expand_tail (bfv_expand.hip) and k_bfv_pack_tail (bfv_pack.hip) are this skeleton with
// their policies; the two-step kernels of the last two call the same finish() with the pair gathered from global memory, so an
// operator's epilogue stands once.  k_bfv_slot_tail (slot_sum.hip) stages another row and gathers several tables: it shares
// ld2 / st2, lds_gather_pair and the host helpers, not the skeleton.  Device code and its launcher: HIP units only.
#pragma once
#include "key_switch.h"

namespace lsa {

// threads of a workgroup that owns one LDS row, and the point pairs a thread owns at the largest ring: 2^14 / (2 * 1024)
#define LSA_LDS_ROW_THREADS 1024
constexpr int LDS_ROW_PAIRS = (1 << LSA_PERM_LDS_MAX_LOGN) / (2 * LSA_LDS_ROW_THREADS);

__device__ __forceinline__ ulonglong2 ld2(const u64* p) { return *reinterpret_cast<const ulonglong2*>(p); }
__device__ __forceinline__ void st2(u64* p, u64 x, u64 y) {
    ulonglong2 v;
    v.x = x;
    v.y = y;
    *reinterpret_cast<ulonglong2*>(p) = v;
}

// sign_y * row[pi_y] at the points (y, y + 1), y even: perm = Context::coeff_perm(g), bit 31 negates.  row: LDS or global memory
__device__ __forceinline__ ulonglong2 lds_gather_pair(const u64* row, const u32* perm, int y, u64 q) {
    const uint2 p = *reinterpret_cast<const uint2*>(perm + y);
    ulonglong2 s;
    s.x = row[p.x & 0x7fffffffu];
    s.y = row[p.y & 0x7fffffffu];
    if (p.x >> 31) s.x = neg_mod(s.x, q);
    if (p.y >> 31) s.y = neg_mod(s.y, q);
    return s;
}

// what every row tail is given (launch_lds_row_tail fills all but perm).  A two-step kernel reads the rotation's source at acc.
struct RowTailArgs {
    const u32* perm;     // Context::coeff_perm(g)
    const u64* acc;      // [2][acc_rpp][N] out of the NTT domain
    const u64* conv;     // [2][L][N]
    const u64* base;     // KsOut::base
    u64* out;            // KsOut::p
    const u64* kvec;     // [L] P^-1 mod q_j, Montgomery form
    const ModDev* mods;
    long long sacc, sconv, sbase, sout;
    int acc_rpp, limbs, logn;
};

// f(i, x) for the point pairs (x, x + 1) of the row a thread owns, i the pair's register slot.  UNROLL: LDS_ROW_PAIRS guarded
// iterations, so that slot i names a register; else the strided loop (i = 0)
template <bool UNROLL, class F>
__device__ __forceinline__ void for_row_pairs(int n, F&& f) {
    if constexpr (UNROLL) {
#pragma unroll
        for (int i = 0; i < LDS_ROW_PAIRS; i++) {
            const int x = (i * LSA_LDS_ROW_THREADS + (int)threadIdx.x) * 2;
            if (x < n) f(i, x);
        }
    } else {
        for (int x = threadIdx.x * 2; x < n; x += 2 * LSA_LDS_ROW_THREADS) f(0, x);
    }
}

// grid: x = 2*limbs, y = items; dynamic LDS 8N bytes.  Nothing of the row is read from global memory after the barrier but what
// finish() reads at the points it writes, so an operator's output may lie over the operand it kept.
template <class Op>
__device__ __forceinline__ void gathered_tail_row(const RowTailArgs& g, const Op& op) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    const int n = 1 << g.logn;
    const int poly = blockIdx.x / g.limbs, limb = blockIdx.x % g.limbs;
    const ModDev m = g.mods[limb];
    const u64 k = g.kvec[limb];
    const long long b = blockIdx.y;
    const u64* a = g.acc + b * g.sacc + (((long long)poly * g.acc_rpp + limb) << g.logn);
    const u64* v = g.conv + b * g.sconv + (((long long)poly * g.limbs + limb) << g.logn);
    typename Op::Keep keep[Op::KEEPS ? LDS_ROW_PAIRS : 1];
    for_row_pairs<Op::KEEPS>(n, [&](int i, int x) {
        const ulonglong2 va = ld2(a + x), vv = ld2(v + x);
        ulonglong2 r;
        r.x = mont_mul(sub_mod(va.x, vv.x, m.q), k, m.q, m.qinv);
        r.y = mont_mul(sub_mod(va.y, vv.y, m.q), k, m.q, m.qinv);
        op.stage(x, poly, r, keep[i]);
        *reinterpret_cast<ulonglong2*>(lds + x) = r;
    });
    __syncthreads();
    for_row_pairs<Op::KEEPS>(n, [&](int i, int y) { op.finish(y, keep[i], lds_gather_pair(lds, g.perm, y, m.q)); });
}

// One workgroup of LSA_LDS_ROW_THREADS per (row, item) with an 8N-byte LDS row (lds false: without the row): the shared checks,
// the common fields of g.t, the launch.  who: the tail's name in its messages; bytes: what the launch moves (ProfScope)
template <auto Kernel, class Args>
void launch_lds_row_tail(Context& c, int level, const std::string& who, Args g, const u64* acc, long long sacc, int acc_rpp,
                         const u64* conv, long long sconv, const KsOut& o, int nb, double bytes, hipStream_t s, bool lds = true) {
    const int L = level + 1;
    LSA_REQUIRE(level >= 0 && L <= c.nq, who + ": level out of range");
    LSA_REQUIRE(acc && conv && o.p && acc_rpp >= L, who + ": null or short operand");
    LSA_REQUIRE(!lds || c.logn <= LSA_PERM_LDS_MAX_LOGN, who + ": the ring's limbs do not fit in LDS");
    LSA_REQUIRE(c.n >= 2, who + ": ring degree too small");
    g.t.acc = acc;
    g.t.conv = conv;
    g.t.base = o.base;
    g.t.out = o.p;
    g.t.kvec = c.pinv_vec(level);
    g.t.mods = c.d_mods;
    g.t.sacc = sacc;
    g.t.sconv = sconv;
    g.t.sbase = o.sbase;
    g.t.sout = o.sp;
    g.t.acc_rpp = acc_rpp;
    g.t.limbs = L;
    g.t.logn = c.logn;
    ProfScope ps(c, PROF_ELEMWISE, bytes, s);
    const size_t lds_bytes = lds ? (size_t)c.n * sizeof(u64) : 0;
    raise_dynamic_lds<Kernel>(lds_bytes, 160 * 1024);
    hipLaunchKernelGGL(Kernel, dim3((unsigned)(2 * L), (unsigned)nb), dim3(LSA_LDS_ROW_THREADS), lds_bytes, s, g);
    LSA_HIP(hipGetLastError());
}

}  // namespace lsa
