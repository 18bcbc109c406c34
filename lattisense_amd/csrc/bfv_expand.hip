// bfv_expand.hip — the BFV oblivious expansion (plan and point arithmetic: bfv_expand.h; semantics: include/lattisense_amd.h):
//   k_bfv_expand_tail     the coefficient-domain ModDown tail of one level: (acc - conv) / P (+ c0) staged in LDS, the rotation
//                         gathered from there, and BOTH children stored -- the even one over the parent, the odd one shifted
//   k_bfv_expand_combine  the two-step form: the key switch leaves (c0 + ks0, ks1) in the workspace and this kernel gathers the
//                         rotation from global memory (N > 2^14, unfused tails, the plan's gather switched off)
//   k_mul_monomial        X^e * in, the negacyclic shift (lsa_bfv_mul_monomial)
// and below them the runner on key_switch() (bfv_expand_run).  Every word equals the composition lsa_bfv_rotate, lsa_poly_addsub
// (add, sub), lsa_bfv_mul_monomial: canonical residues, add_mod / sub_mod / neg_mod.
#include <atomic>

#include "bfv_expand.h"
#include "entry_check.h"
#include "key_switch.h"

namespace lsa {

namespace {

constexpr int TPB = 256;
#define LSA_EXPAND_TAIL_THREADS 1024
// pairs of points a thread of the tail owns at the largest ring: 2^14 / (2 * 1024)
constexpr int EXPAND_TAIL_PAIRS = (1 << LSA_PERM_LDS_MAX_LOGN) / (2 * LSA_EXPAND_TAIL_THREADS);

__device__ __forceinline__ ulonglong2 ld2(const u64* p) { return *reinterpret_cast<const ulonglong2*>(p); }
__device__ __forceinline__ void st2(u64* p, u64 x, u64 y) {
    ulonglong2 v;
    v.x = x;
    v.y = y;
    *reinterpret_cast<ulonglong2*>(p) = v;
}

// the children of the point pair (y, y + 1), y even, of one row: even[y] = c + sigma in the parent's place, and where the node has
// an odd child +-(c - sigma) at (y - s) mod N.  s even: y - s is even and both points share the sign, one 16-byte store; s = 1: the
// shifted pair straddles the 16-byte grid (and the row's end at y = 0), so its words go singly.
__device__ __forceinline__ void expand_children(u64* even, u64* odd, unsigned y, unsigned s, int logn, ulonglong2 cv, u64 sg0, u64 sg1,
                                                u64 q) {
    st2(even + y, add_mod(cv.x, sg0, q), add_mod(cv.y, sg1, q));
    if (!odd) return;
    u64 d0 = sub_mod(cv.x, sg0, q), d1 = sub_mod(cv.y, sg1, q);
    const MonomialDest t0 = bfv_expand_odd_dest(y, s, logn), t1 = bfv_expand_odd_dest(y + 1, s, logn);
    if (t0.neg) d0 = neg_mod(d0, q);
    if (t1.neg) d1 = neg_mod(d1, q);
    if ((s & 1) == 0) {
        st2(odd + t0.idx, d0, d1);
    } else {
        odd[t0.idx] = d0;
        odd[t1.idx] = d1;
    }
}

struct ExpandArgs {
    const u32* perm;      // Context::coeff_perm(g)
    const u64* acc;       // tail: [2][acc_rpp][N] out of the NTT domain.  combine: the rotated pair's source (c0 + ks0, ks1), [2][L][N]
    const u64* conv;      // tail: [2][L][N]
    const u64* parent;    // [2][L][N], coefficient domain
    u64* even;            // [2][L][N]; may be parent
    const u64* kvec;      // [L] P^-1 mod q_j, Montgomery form
    const ModDev* mods;
    long long sacc, sconv, sparent, seven, odd_off;
    int acc_rpp, limbs, logn, shift;
    int item0, batch, n_odd;   // item item0 + blockIdx.y has an odd child iff its index coordinate, item / batch, is below n_odd
};

// grid: x = 2*limbs, y = items; dynamic LDS 8N bytes.  One workgroup per (row, item).  A thread keeps the parent's words of its own
// points from the staging loop on (read once), so the even child may be written over the parent: nothing else of the row is read
// from global memory after the barrier.
__global__ __launch_bounds__(LSA_EXPAND_TAIL_THREADS) void k_bfv_expand_tail(ExpandArgs g) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    const int n = 1 << g.logn;
    const int row = blockIdx.x;
    const int poly = row / g.limbs, limb = row % g.limbs;
    const ModDev m = g.mods[limb];
    const u64 k = g.kvec[limb];
    const long long b = blockIdx.y;
    const long long ro = ((long long)poly * g.limbs + limb) << g.logn;
    const u64* a = g.acc + b * g.sacc + (((long long)poly * g.acc_rpp + limb) << g.logn);
    const u64* v = g.conv + b * g.sconv + ro;
    const u64* c = g.parent + b * g.sparent + ro;
    u64* even = g.even + b * g.seven + ro;
    const bool has_odd = (g.item0 + (int)blockIdx.y) / g.batch < g.n_odd;   // uniform over the workgroup
    u64* odd = has_odd ? even + g.odd_off : nullptr;
    ulonglong2 cr[EXPAND_TAIL_PAIRS];
#pragma unroll
    for (int i = 0; i < EXPAND_TAIL_PAIRS; i++) {
        const int x = (i * LSA_EXPAND_TAIL_THREADS + (int)threadIdx.x) * 2;
        if (x < n) {
            const ulonglong2 va = ld2(a + x), vv = ld2(v + x);
            cr[i] = ld2(c + x);
            ulonglong2 r;
            r.x = mont_mul(sub_mod(va.x, vv.x, m.q), k, m.q, m.qinv);
            r.y = mont_mul(sub_mod(va.y, vv.y, m.q), k, m.q, m.qinv);
            if (poly == 0) {
                r.x = add_mod(r.x, cr[i].x, m.q);
                r.y = add_mod(r.y, cr[i].y, m.q);
            }
            *reinterpret_cast<ulonglong2*>(lds + x) = r;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < EXPAND_TAIL_PAIRS; i++) {
        const int y = (i * LSA_EXPAND_TAIL_THREADS + (int)threadIdx.x) * 2;
        if (y < n) {
            const uint2 p = *reinterpret_cast<const uint2*>(g.perm + y);
            u64 s0 = lds[p.x & 0x7fffffffu], s1 = lds[p.y & 0x7fffffffu];
            if (p.x >> 31) s0 = neg_mod(s0, m.q);
            if (p.y >> 31) s1 = neg_mod(s1, m.q);
            expand_children(even, odd, (unsigned)y, (unsigned)g.shift, g.logn, cr[i], s0, s1, m.q);
        }
    }
}

// grid: x = 2*limbs * (N/2/TPB), y = items.  acc: the rotation's source in the workspace.  A thread reads only the parent's words it
// writes over.
__global__ __launch_bounds__(TPB) void k_bfv_expand_combine(ExpandArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int row = blockIdx.x / chunks;
    const int limb = row % g.limbs;
    const unsigned y = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const long long b = blockIdx.y;
    const long long ro = (long long)row << g.logn;
    const u64 q = g.mods[limb].q;
    const u64* src = g.acc + b * g.sacc + ro;
    u64* even = g.even + b * g.seven + ro;
    const bool has_odd = (g.item0 + (int)blockIdx.y) / g.batch < g.n_odd;
    const uint2 p = *reinterpret_cast<const uint2*>(g.perm + y);
    u64 s0 = src[p.x & 0x7fffffffu], s1 = src[p.y & 0x7fffffffu];
    if (p.x >> 31) s0 = neg_mod(s0, q);
    if (p.y >> 31) s1 = neg_mod(s1, q);
    const ulonglong2 cv = ld2(g.parent + b * g.sparent + ro + y);
    expand_children(even, has_odd ? even + g.odd_off : nullptr, y, (unsigned)g.shift, g.logn, cv, s0, s1, q);
}

struct MonomialArgs {
    const u64* in;
    u64* out;
    long long sin, sout;
    const ModDev* mods;
    int limbs, logn;
    unsigned e;   // in [0, 2N)
};

// grid: x = rows * (N/2/TPB), y = batch.  out[(y + e) mod N] = +-in[y]; an even e keeps the pair (y, y + 1) together and aligned
__global__ __launch_bounds__(TPB) void k_mul_monomial(MonomialArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int row = blockIdx.x / chunks;
    const unsigned y = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const long long b = blockIdx.y;
    const u64 q = g.mods[row % g.limbs].q;
    const ulonglong2 v = ld2(g.in + b * g.sin + ((long long)row << g.logn) + y);
    u64* o = g.out + b * g.sout + ((long long)row << g.logn);
    const MonomialDest t0 = monomial_dest(y, g.e, g.logn), t1 = monomial_dest(y + 1, g.e, g.logn);
    const u64 d0 = t0.neg ? neg_mod(v.x, q) : v.x, d1 = t1.neg ? neg_mod(v.y, q) : v.y;
    if ((g.e & 1) == 0) {
        st2(o + t0.idx, d0, d1);
    } else {
        o[t0.idx] = d0;
        o[t1.idx] = d1;
    }
}

ExpandArgs expand_args(Context& c, int level, const BfvExpandTail& t, const u64* parent, long long sparent, u64* even, long long seven) {
    LSA_REQUIRE(level >= 0 && level < c.nq, "BFV expand tail: level out of range");
    LSA_REQUIRE(t.perm && parent && even, "BFV expand tail: null operand");
    LSA_REQUIRE(t.shift >= 1 && t.shift < c.n && t.batch >= 1 && t.item0 >= 0 && t.n_odd >= 0, "BFV expand tail: bad node geometry");
    LSA_REQUIRE(((t.odd_off | sparent | seven) & 1) == 0, "BFV expand tail: odd stride");
    ExpandArgs g{};
    g.perm = t.perm;
    g.parent = parent;
    g.even = even;
    g.kvec = c.pinv_vec(level);
    g.mods = c.d_mods;
    g.sparent = sparent;
    g.seven = seven;
    g.odd_off = t.odd_off;
    g.limbs = level + 1;
    g.logn = c.logn;
    g.shift = t.shift;
    g.item0 = t.item0;
    g.batch = t.batch;
    g.n_odd = t.n_odd;
    return g;
}

// the words the children's stores move per row, in rows of N: the even child for every item, the odd one for those that have it
double expand_child_rows(const BfvExpandTail& t, int nb) {
    double odd = 0;
    for (int i = 0; i < nb; i++) odd += (t.item0 + i) / t.batch < t.n_odd ? 1 : 0;
    return nb + odd;
}

}  // namespace

void launch_bfv_expand_tail(Context& c, int level, const BfvExpandTail& t, const u64* acc, long long sacc, int acc_rpp, const u64* conv,
                            long long sconv, const u64* parent, long long sparent, u64* even, long long seven, int nb, hipStream_t s) {
    if (nb <= 0) return;
    const int L = level + 1;
    LSA_REQUIRE(acc && conv && acc_rpp >= L, "BFV expand tail: null or short operand");
    LSA_REQUIRE(c.logn <= LSA_PERM_LDS_MAX_LOGN, "BFV expand tail: the ring's limbs do not fit in LDS");
    LSA_REQUIRE(c.n >= 2, "BFV expand tail: ring degree too small");
    ExpandArgs g = expand_args(c, level, t, parent, sparent, even, seven);
    g.acc = acc;
    g.conv = conv;
    g.sacc = sacc;
    g.sconv = sconv;
    g.acc_rpp = acc_rpp;
    // per row: acc, conv and the parent read, the children written, 4 bytes per point of the table
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * 2 * L * (3.0 * nb + expand_child_rows(t, nb)) + 4.0 * c.n * 2 * L * nb, s);
    const size_t lds_bytes = (size_t)c.n * sizeof(u64);
    if (lds_bytes > 65536) {   // opt in to more than 64 KiB of dynamic LDS, once per device (the attribute is per device)
        static std::atomic<unsigned long long> raised{0};
        int dev = 0;
        LSA_HIP(hipGetDevice(&dev));
        const unsigned long long bit = 1ull << (dev & 63);
        if (!(raised.load(std::memory_order_acquire) & bit)) {
            LSA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bfv_expand_tail), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        160 * 1024));
            raised.fetch_or(bit, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL(k_bfv_expand_tail, dim3((unsigned)(2 * L), (unsigned)nb), dim3(LSA_EXPAND_TAIL_THREADS), lds_bytes, s, g);
    LSA_HIP(hipGetLastError());
}

// sigma: (c0 + ks0, ks1), [2][L][N] per item, not yet rotated
void launch_bfv_expand_combine(Context& c, int level, const BfvExpandTail& t, const u64* sigma, long long ssigma, const u64* parent,
                               long long sparent, u64* even, long long seven, int nb, hipStream_t s) {
    if (nb <= 0) return;
    const int L = level + 1;
    LSA_REQUIRE(sigma != nullptr, "BFV expand combine: null operand");
    LSA_REQUIRE(c.n >= 2 * TPB, "ring degree too small for the BFV expand combine (need N >= 512)");
    ExpandArgs g = expand_args(c, level, t, parent, sparent, even, seven);
    g.acc = sigma;
    g.sacc = ssigma;
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * 2 * L * (2.0 * nb + expand_child_rows(t, nb)) + 4.0 * c.n * 2 * L * nb, s);
    hipLaunchKernelGGL(k_bfv_expand_combine, dim3((unsigned)(2 * L * (c.n / (2 * TPB))), (unsigned)nb), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

void bfv_mul_monomial(Context& c, int level, int polys, long long exponent, const u64* in, u64* out, int batch, long long sin,
                      long long sout, hipStream_t s) {
    const EntryCheck ck(c, "lsa_bfv_mul_monomial", LSA_ALGO_BFV, level, 0, batch);
    ck.polys(polys);
    if (batch <= 0) return;
    const int L = level + 1;
    const size_t w = (size_t)polys * L * ck.N;
    ck.apart(ck.output(out, sout, w), ck.operand(in, sin, w, "in", false), "in");
    LSA_REQUIRE(c.n >= 2 * TPB, ck.who + ": ring degree too small (need N >= 512)");
    MonomialArgs g{};
    g.in = in;
    g.out = out;
    g.sin = sin;
    g.sout = sout;
    g.mods = c.d_mods;
    g.limbs = L;
    g.logn = c.logn;
    g.e = monomial_exponent(exponent, c.logn);
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * polys * L * 2.0 * batch, s);
    hipLaunchKernelGGL(k_mul_monomial, dim3((unsigned)(polys * L * (c.n / (2 * TPB))), (unsigned)batch), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ the operator
BfvExpandPlanHost bfv_expand_plan_checked(int n_ring, int count) {
    try {
        return bfv_expand_plan(n_ring, count);
    } catch (const std::invalid_argument& e) {
        throw Error(LSA_ERR_ARG, e.what());
    }
}

BfvExpand* bfv_expand_create(Context& c, int level, int count) {
    LSA_REQUIRE(c.algo == LSA_ALGO_BFV, "lsa_bfv_expand_create: context is not BFV");
    LSA_REQUIRE(level >= 0 && level < c.nq, "lsa_bfv_expand_create: level out of range (0.." + std::to_string(c.nq - 1) + ")");
    auto p = std::make_unique<BfvExpand>(c, level);
    p->plan = bfv_expand_plan_checked(c.n, count);
    LSA_REQUIRE(p->plan.levels.empty() || c.np >= 1, "lsa_bfv_expand_create: count: key switching needs at least one special prime");
    return p.release();
}

// All levels work inside the output array: level j reads the parents c[a], a < min(2^j, count) (level 0: `in`), writes the even
// child over the parent (level 0: output 0) and the odd child 2^j outputs further on, which no key switch of this level reads.  A
// level is one key switch with one key.  Dense layout (s_index == batch * sout): the nodes x batch items of a level are one
// strided batch -- one tiled key switch and one tail launch per tile, the tail telling from its item index whether the node has an odd
// child.  Otherwise one tiled key switch per node.
void bfv_expand_run(BfvExpand& p, const u64* in, long long sin, u64* out, long long sout, long long s_index, int batch,
                    const GaloisKeys& glk, hipStream_t s) {
    Context& c = p.c;
    const int level = p.level, count = p.plan.count;
    const EntryCheck ck(c, "lsa_bfv_expand", LSA_ALGO_BFV, level, 0, batch);
    const std::vector<const Key*> keys = glk.resolve(p.plan.galois, ck.who, [&](u64, const Key& k) { ck.key(k, "a Galois key"); });
    if (batch <= 0) return;
    const long long N = c.n;
    const int L = level + 1;
    const size_t w = 2 * (size_t)L * N;
    const layout::Span sp_in = ck.operand(in, sin, w, "in", false);
    const layout::Span sp_out0 = ck.output(out, sout, w);
    LSA_REQUIRE((s_index & 1) == 0, ck.who + ": s_index must be even");
    LSA_REQUIRE(s_index > 0 && (layout::u128)(unsigned long long)s_index >= (layout::u128)(unsigned)batch * (unsigned long long)sout,
                ck.who + ": s_index below batch * sout");
    LSA_REQUIRE((long long)count * batch <= 0x7fffffffLL, ck.who + ": count * batch does not fit a batch");
    {   // `in` is output 0 itself or shares no word with any output
        const layout::Span hull = layout::span_of(out, s_index, (size_t)(batch - 1) * (size_t)sout + w);
        const bool in_is_out0 = layout::same(sp_out0, sp_in);
        if (!in_is_out0 && !layout::apart(hull, layout::span_of(in, 0, (size_t)(batch - 1) * (size_t)sin + w), count)) {
            ck.same_or_apart(sp_out0, sp_in, "in");
            for (int i = 0; i < count; i++) ck.apart(layout::span_of(out + (long long)i * s_index, sout, w), sp_in, "in");
        }
        if (in_is_out0)
            for (int i = 1; i < count; i++) ck.apart(layout::span_of(out + (long long)i * s_index, sout, w), sp_in, "in");
    }
    if (p.plan.levels.empty()) {   // count == 1: a copy
        if (layout::same(sp_out0, sp_in)) return;
        std::vector<int> rows(2 * L);
        for (int i = 0; i < 2 * L; i++) rows[i] = i;
        launch_copy_rows(c, in, sin, out, sout, 2 * L, rows.data(), batch, s);
        return;
    }
    const bool gather = p.gather && c.fuse_tails && c.logn <= LSA_PERM_LDS_MAX_LOGN;
    std::map<u64, const Key*> key_of;
    for (size_t i = 0; i < keys.size(); i++) key_of[p.plan.galois[i]] = keys[i];
    const size_t ks_rows = KsTile::rows(c, level, KsSource::COEFF);
    const long long sp = 2LL * L * N, sL = (long long)L * N;
    const bool dense = (layout::u128)(unsigned long long)s_index == (layout::u128)(unsigned)batch * (unsigned long long)sout;
    // one key switch over `items` parents (stride spar) whose even children lie at `even` (stride sout)
    auto run_nodes = [&](const BfvExpandLevel& lv, const Key& key, const u32* perm, const u64* parent, long long spar, u64* even,
                         int items, int n_odd) {
        for_tiles(c, ks_rows + (gather ? 0 : 2 * (size_t)L), items, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t st) {
            const u64* ct = parent + (size_t)b0 * spar;
            u64* ev = even + (size_t)b0 * sout;
            const BfvExpandTail et{perm, (long long)lv.shift * s_index, lv.shift, b0, batch, n_odd};
            if (gather) {
                key_switch(c, level, KsSource::of_coeff(ct + sL, spar), key,
                           ks_onto_c0(ev, sout, ct, spar, L, {.form = KsOut::COEFF, .expand_tail = &et}), nb, ws, st);
                return;
            }
            u64* sg = ws + ks_rows * N * tb;   // (c0 + ks0, ks1), as bfv_rotate leaves it before its permutation
            key_switch(c, level, KsSource::of_coeff(ct + sL, spar), key, ks_onto_c0(sg, sp, ct, spar, L, {.form = KsOut::COEFF}), nb, ws, st);
            launch_bfv_expand_combine(c, level, et, sg, sp, ct, spar, ev, sout, nb, st);
        });
    };
    for (size_t j = 0; j < p.plan.levels.size(); j++) {
        const BfvExpandLevel& lv = p.plan.levels[j];
        const Key& key = *key_of.at(lv.g);
        const u32* perm = c.coeff_perm(lv.g);
        const u64* parent = j == 0 ? in : out;
        const long long spar = j == 0 ? sin : sout;
        if (dense || lv.nodes == 1) {
            run_nodes(lv, key, perm, parent, spar, out, lv.nodes * batch, lv.n_odd);
            continue;
        }
        for (int a = 0; a < lv.nodes; a++)
            run_nodes(lv, key, perm, parent + (long long)a * s_index, spar, out + (long long)a * s_index, batch, a < lv.n_odd ? 1 : 0);
    }
}

}  // namespace lsa
