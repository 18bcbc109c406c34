// bfv_pack.hip — the BFV coefficient packing (plan and point arithmetic: bfv_pack.h; semantics: include/lattisense_amd.h):
//   k_bfv_pack_diff     the head of a paired level: v = a - X^s b into the tile's workspace, the source of the level's key switch
//                       (polynomial 1 alone in the gather form, both in the two-step form); an unpaired node's rows pass through
//   k_bfv_pack_tail     the coefficient-domain ModDown tail of one level: (acc - conv) / P (+ a0 - xb0) staged in LDS, the rotation
//                       gathered from there and added to u = a + X^s b, which the thread kept from the staging loop
//   k_bfv_pack_combine  the two-step form: the key switch leaves (v0 + ks0, ks1) in the workspace and this kernel gathers the
//                       rotation from global memory (N > 2^14, unfused tails, the plan's gather switched off)
// and below them the runner on key_switch() (bfv_pack_run).  Every word equals the composition lsa_bfv_mul_monomial, lsa_poly_addsub
// (add, sub), lsa_bfv_rotate, lsa_poly_addsub (add): canonical residues, add_mod / sub_mod / neg_mod.
#include <atomic>

#include "bfv_pack.h"
#include "entry_check.h"
#include "key_switch.h"

namespace lsa {

namespace {

constexpr int TPB = 256;
#define LSA_PACK_TAIL_THREADS 1024
// pairs of points a thread of the tail owns at the largest ring: 2^14 / (2 * 1024)
constexpr int PACK_TAIL_PAIRS = (1 << LSA_PERM_LDS_MAX_LOGN) / (2 * LSA_PACK_TAIL_THREADS);

__device__ __forceinline__ ulonglong2 ld2(const u64* p) { return *reinterpret_cast<const ulonglong2*>(p); }
__device__ __forceinline__ void st2(u64* p, u64 x, u64 y) {
    ulonglong2 v;
    v.x = x;
    v.y = y;
    *reinterpret_cast<ulonglong2*>(p) = v;
}

// (X^s b)[x], (X^s b)[x + 1], x even, of one row of b.  s even: x - s is even and both points share the sign, one 16-byte load;
// s = 1: the shifted pair straddles the 16-byte grid (and the row's end at x = 0), so its words are loaded singly.
__device__ __forceinline__ ulonglong2 shifted_pair(const u64* b, unsigned x, unsigned s, int logn, u64 q) {
    const MonomialDest t0 = bfv_pack_source(x, s, logn), t1 = bfv_pack_source(x + 1, s, logn);
    ulonglong2 v;
    if ((s & 1) == 0) {
        v = ld2(b + t0.idx);
    } else {
        v.x = b[t0.idx];
        v.y = b[t1.idx];
    }
    if (t0.neg) v.x = neg_mod(v.x, q);
    if (t1.neg) v.y = neg_mod(v.y, q);
    return v;
}

struct PackArgs {
    const u32* perm;      // Context::coeff_perm(g)
    const u64* acc;       // tail: [2][acc_rpp][N] out of the NTT domain.  combine: the rotation's source (v0 + ks0, ks1), [2][L][N].  diff: unused
    const u64* conv;      // tail: [2][L][N]
    const u64* a;         // [2][L][N], coefficient domain (diff: from the first row it takes); the partner b lies b_off words on
    u64* out;             // tail, combine: [2][L][N], may be a.  diff: v, `limbs`-periodic rows
    const u64* kvec;      // [L] P^-1 mod q_j, Montgomery form
    const ModDev* mods;
    long long sacc, sconv, sa, sout, b_off;
    int acc_rpp, limbs, logn, shift;
    int item0, batch, n_pair;   // item item0 + blockIdx.y has a partner iff its index coordinate, item / batch, is below n_pair
};

// grid: x = rows * (N/2/TPB), y = items.  v[row][x] = a[row][x] - (X^s b)[row][x], or a[row][x] where the node has no partner
__global__ __launch_bounds__(TPB) void k_bfv_pack_diff(PackArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int row = blockIdx.x / chunks;
    const unsigned x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const long long b = blockIdx.y;
    const long long ro = (long long)row << g.logn;
    const u64 q = g.mods[row % g.limbs].q;
    const u64* a = g.a + b * g.sa + ro;
    const bool paired = (g.item0 + (int)blockIdx.y) / g.batch < g.n_pair;
    ulonglong2 v = ld2(a + x);
    if (paired) {
        const ulonglong2 xb = shifted_pair(a + g.b_off, x, (unsigned)g.shift, g.logn, q);
        v.x = sub_mod(v.x, xb.x, q);
        v.y = sub_mod(v.y, xb.y, q);
    }
    st2(g.out + b * g.sout + ro + x, v.x, v.y);
}

// grid: x = 2*limbs, y = items; dynamic LDS 8N bytes.  One workgroup per (row, item).  A thread reads a only at the points it writes
// (u stays in registers across the barrier), so out may lie over a; b belongs to a node no key switch of this level writes.
__global__ __launch_bounds__(LSA_PACK_TAIL_THREADS) void k_bfv_pack_tail(PackArgs g) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    const int n = 1 << g.logn;
    const int row = blockIdx.x;
    const int poly = row / g.limbs, limb = row % g.limbs;
    const ModDev m = g.mods[limb];
    const u64 k = g.kvec[limb];
    const long long b = blockIdx.y;
    const long long ro = ((long long)poly * g.limbs + limb) << g.logn;
    const u64* acc = g.acc + b * g.sacc + (((long long)poly * g.acc_rpp + limb) << g.logn);
    const u64* cv = g.conv + b * g.sconv + ro;
    const u64* a = g.a + b * g.sa + ro;
    u64* out = g.out + b * g.sout + ro;
    const bool paired = (g.item0 + (int)blockIdx.y) / g.batch < g.n_pair;   // uniform over the workgroup
    ulonglong2 ur[PACK_TAIL_PAIRS];
#pragma unroll
    for (int i = 0; i < PACK_TAIL_PAIRS; i++) {
        const int x = (i * LSA_PACK_TAIL_THREADS + (int)threadIdx.x) * 2;
        if (x < n) {
            const ulonglong2 va = ld2(acc + x), vv = ld2(cv + x);
            ulonglong2 u = ld2(a + x), d = u, r;
            if (paired) {
                const ulonglong2 xb = shifted_pair(a + g.b_off, (unsigned)x, (unsigned)g.shift, g.logn, m.q);
                d.x = sub_mod(u.x, xb.x, m.q);
                d.y = sub_mod(u.y, xb.y, m.q);
                u.x = add_mod(u.x, xb.x, m.q);
                u.y = add_mod(u.y, xb.y, m.q);
            }
            r.x = mont_mul(sub_mod(va.x, vv.x, m.q), k, m.q, m.qinv);
            r.y = mont_mul(sub_mod(va.y, vv.y, m.q), k, m.q, m.qinv);
            if (poly == 0) {
                r.x = add_mod(r.x, d.x, m.q);
                r.y = add_mod(r.y, d.y, m.q);
            }
            ur[i] = u;
            *reinterpret_cast<ulonglong2*>(lds + x) = r;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PACK_TAIL_PAIRS; i++) {
        const int y = (i * LSA_PACK_TAIL_THREADS + (int)threadIdx.x) * 2;
        if (y < n) {
            const uint2 p = *reinterpret_cast<const uint2*>(g.perm + y);
            u64 s0 = lds[p.x & 0x7fffffffu], s1 = lds[p.y & 0x7fffffffu];
            if (p.x >> 31) s0 = neg_mod(s0, m.q);
            if (p.y >> 31) s1 = neg_mod(s1, m.q);
            st2(out + y, add_mod(ur[i].x, s0, m.q), add_mod(ur[i].y, s1, m.q));
        }
    }
}

// grid: x = 2*limbs * (N/2/TPB), y = items.  acc: the rotation's source in the workspace.  A thread reads only the words of a it
// writes over.
__global__ __launch_bounds__(TPB) void k_bfv_pack_combine(PackArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int row = blockIdx.x / chunks;
    const unsigned y = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const long long b = blockIdx.y;
    const long long ro = (long long)row << g.logn;
    const u64 q = g.mods[row % g.limbs].q;
    const u64* src = g.acc + b * g.sacc + ro;
    const u64* a = g.a + b * g.sa + ro;
    const bool paired = (g.item0 + (int)blockIdx.y) / g.batch < g.n_pair;
    const uint2 p = *reinterpret_cast<const uint2*>(g.perm + y);
    u64 s0 = src[p.x & 0x7fffffffu], s1 = src[p.y & 0x7fffffffu];
    if (p.x >> 31) s0 = neg_mod(s0, q);
    if (p.y >> 31) s1 = neg_mod(s1, q);
    ulonglong2 u = ld2(a + y);
    if (paired) {
        const ulonglong2 xb = shifted_pair(a + g.b_off, y, (unsigned)g.shift, g.logn, q);
        u.x = add_mod(u.x, xb.x, q);
        u.y = add_mod(u.y, xb.y, q);
    }
    st2(g.out + b * g.sout + ro + y, add_mod(u.x, s0, q), add_mod(u.y, s1, q));
}

PackArgs pack_args(Context& c, int level, const BfvPackTail& t, const u64* a, long long sa, u64* out, long long sout) {
    LSA_REQUIRE(level >= 0 && level < c.nq, "BFV pack: level out of range");
    LSA_REQUIRE(a && out, "BFV pack: null operand");
    LSA_REQUIRE(t.batch >= 1 && t.item0 >= 0 && t.n_pair >= 0, "BFV pack: bad node geometry");
    LSA_REQUIRE(t.n_pair == 0 || (t.shift >= 1 && t.shift < c.n && t.b_off != 0), "BFV pack: a paired level needs its shift and partner");
    LSA_REQUIRE(((t.b_off | sa | sout) & 1) == 0, "BFV pack: odd stride");
    PackArgs g{};
    g.perm = t.perm;
    g.a = a;
    g.out = out;
    g.kvec = c.pinv_vec(level);
    g.mods = c.d_mods;
    g.sa = sa;
    g.sout = sout;
    g.b_off = t.b_off;
    g.limbs = level + 1;
    g.logn = c.logn;
    g.shift = t.shift;
    g.item0 = t.item0;
    g.batch = t.batch;
    g.n_pair = t.n_pair;
    return g;
}

// the items of a tile that have a partner
double pack_paired_items(const BfvPackTail& t, int nb) {
    double n = 0;
    for (int i = 0; i < nb; i++) n += (t.item0 + i) / t.batch < t.n_pair ? 1 : 0;
    return n;
}

// a: the first of the `rows` rows of an item the head takes (c1 alone: a + L * N, rows = L), v: rows rows per item
void launch_bfv_pack_diff(Context& c, int level, const BfvPackTail& t, const u64* a, long long sa, u64* v, long long sv, int rows, int nb,
                          hipStream_t s) {
    if (nb <= 0) return;
    LSA_REQUIRE(c.n >= 2 * TPB, "ring degree too small for the BFV pack head (need N >= 512)");
    LSA_REQUIRE(rows >= 1 && rows % (level + 1) == 0, "BFV pack head: whole polynomials");
    PackArgs g = pack_args(c, level, t, a, sa, v, sv);
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * rows * (2.0 * nb + pack_paired_items(t, nb)), s);
    hipLaunchKernelGGL(k_bfv_pack_diff, dim3((unsigned)(rows * (c.n / (2 * TPB))), (unsigned)nb), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

// sigma: (v0 + ks0, ks1), [2][L][N] per item, not yet rotated
void launch_bfv_pack_combine(Context& c, int level, const BfvPackTail& t, const u64* sigma, long long ssigma, const u64* a, long long sa,
                             u64* out, long long sout, int nb, hipStream_t s) {
    if (nb <= 0) return;
    const int L = level + 1;
    LSA_REQUIRE(sigma != nullptr && t.perm != nullptr, "BFV pack combine: null operand");
    LSA_REQUIRE(c.n >= 2 * TPB, "ring degree too small for the BFV pack combine (need N >= 512)");
    PackArgs g = pack_args(c, level, t, a, sa, out, sout);
    g.acc = sigma;
    g.sacc = ssigma;
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * 2 * L * (3.0 * nb + pack_paired_items(t, nb)) + 4.0 * c.n * 2 * L * nb, s);
    hipLaunchKernelGGL(k_bfv_pack_combine, dim3((unsigned)(2 * L * (c.n / (2 * TPB))), (unsigned)nb), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

}  // namespace

void launch_bfv_pack_tail(Context& c, int level, const BfvPackTail& t, const u64* acc, long long sacc, int acc_rpp, const u64* conv,
                          long long sconv, const u64* a, long long sa, u64* out, long long sout, int nb, hipStream_t s) {
    if (nb <= 0) return;
    const int L = level + 1;
    LSA_REQUIRE(acc && conv && t.perm && acc_rpp >= L, "BFV pack tail: null or short operand");
    LSA_REQUIRE(c.logn <= LSA_PERM_LDS_MAX_LOGN, "BFV pack tail: the ring's limbs do not fit in LDS");
    LSA_REQUIRE(c.n >= 2, "BFV pack tail: ring degree too small");
    PackArgs g = pack_args(c, level, t, a, sa, out, sout);
    g.acc = acc;
    g.conv = conv;
    g.sacc = sacc;
    g.sconv = sconv;
    g.acc_rpp = acc_rpp;
    // per row: acc, conv and a read, the partner where there is one, the result written, 4 bytes per point of the table
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * 2 * L * (4.0 * nb + pack_paired_items(t, nb)) + 4.0 * c.n * 2 * L * nb, s);
    const size_t lds_bytes = (size_t)c.n * sizeof(u64);
    if (lds_bytes > 65536) {   // opt in to more than 64 KiB of dynamic LDS, once per device (the attribute is per device)
        static std::atomic<unsigned long long> raised{0};
        int dev = 0;
        LSA_HIP(hipGetDevice(&dev));
        const unsigned long long bit = 1ull << (dev & 63);
        if (!(raised.load(std::memory_order_acquire) & bit)) {
            LSA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bfv_pack_tail), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        160 * 1024));
            raised.fetch_or(bit, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL(k_bfv_pack_tail, dim3((unsigned)(2 * L), (unsigned)nb), dim3(LSA_PACK_TAIL_THREADS), lds_bytes, s, g);
    LSA_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ the operator
BfvPackPlanHost bfv_pack_plan_checked(int n_ring, int count, int trace) {
    try {
        return bfv_pack_plan(n_ring, count, trace);
    } catch (const std::invalid_argument& e) {
        throw Error(LSA_ERR_ARG, e.what());
    }
}

BfvPack* bfv_pack_create(Context& c, int level, int count, int trace) {
    LSA_REQUIRE(c.algo == LSA_ALGO_BFV, "lsa_bfv_pack_create: context is not BFV");
    LSA_REQUIRE(level >= 0 && level < c.nq, "lsa_bfv_pack_create: level out of range (0.." + std::to_string(c.nq - 1) + ")");
    auto p = std::make_unique<BfvPack>(c, level);
    p->plan = bfv_pack_plan_checked(c.n, count, trace);
    LSA_REQUIRE(p->plan.n_keyswitch == 0 || c.np >= 1, "lsa_bfv_pack_create: count: key switching needs at least one special prime");
    LSA_REQUIRE(p->plan.levels.empty() || c.n >= 2 * TPB, "lsa_bfv_pack_create: ring degree too small (need N >= 512)");
    return p.release();
}

// All steps but the last work inside the input array: level j reads the nodes c[a], a < 2^j, and their partners c[a + 2^j], and
// writes c'[a] over c[a]; the last step (level 0, or the last trace level) writes `out`.  The tiles of a level write disjoint c[a]
// and read partners that no tile of that level writes, so tiles on two streams do not meet; a tile's head writes its own half of the
// workspace.  A level is one key switch with one key.  Dense layout (s_index == batch * sin): the nodes x batch items of a level are
// one strided batch -- one head, one tiled key switch and one tail launch per tile, head and tail telling from the item index
// whether the node has a partner.  Otherwise one tiled key switch per node.
void bfv_pack_run(BfvPack& p, u64* in, long long sin, long long s_index, u64* out, long long sout, int batch, const GaloisKeys& glk,
                  hipStream_t s) {
    Context& c = p.c;
    const int level = p.level, count = p.plan.count;
    const EntryCheck ck(c, "lsa_bfv_pack", LSA_ALGO_BFV, level, 0, batch);
    const std::vector<const Key*> keys = glk.resolve(p.plan.galois, ck.who, [&](u64, const Key& k) { ck.key(k, "a Galois key"); });
    if (batch <= 0) return;
    const long long N = c.n;
    const int L = level + 1;
    const size_t w = 2 * (size_t)L * N;
    const layout::Span sp_in0 = ck.operand(in, sin, w, "in", false);
    const layout::Span sp_out = ck.output(out, sout, w);
    LSA_REQUIRE((s_index & 1) == 0, ck.who + ": s_index must be even");
    LSA_REQUIRE(s_index > 0 && (layout::u128)(unsigned long long)s_index >= (layout::u128)(unsigned)batch * (unsigned long long)sin,
                ck.who + ": s_index below batch * sin");
    LSA_REQUIRE((long long)count * batch <= 0x7fffffffLL, ck.who + ": count * batch does not fit a batch");
    {   // `out` is input 0 itself or shares no word with any input
        const layout::Span hull = layout::span_of(in, s_index, (size_t)(batch - 1) * (size_t)sin + w);
        const bool out_is_in0 = layout::same(sp_out, sp_in0);
        if (!out_is_in0 && !layout::apart(hull, layout::span_of(out, 0, (size_t)(batch - 1) * (size_t)sout + w), count)) {
            ck.same_or_apart(sp_out, sp_in0, "input 0");
            for (int i = 0; i < count; i++) ck.apart(sp_out, layout::span_of(in + (long long)i * s_index, sin, w), "an input");
        }
        if (out_is_in0)
            for (int i = 1; i < count; i++) ck.apart(sp_out, layout::span_of(in + (long long)i * s_index, sin, w), "an input");
    }
    struct Step {
        int nodes, n_pair, shift;
        u64 g;
    };
    std::vector<Step> steps;
    for (const BfvPackLevel& lv : p.plan.levels) steps.push_back({lv.nodes, lv.n_pair, lv.shift, lv.g});
    for (u64 g : p.plan.trace_g) steps.push_back({1, 0, 0, g});
    if (steps.empty()) {   // count == 1 without the trace: a copy
        if (layout::same(sp_out, sp_in0)) return;
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
    const bool dense = (layout::u128)(unsigned long long)s_index == (layout::u128)(unsigned)batch * (unsigned long long)sin;
    // one key switch over `items` nodes a (stride sin) whose results go to dst (stride sdst); the partner lies b_off words after a
    auto run_nodes = [&](const Step& st, const Key& key, const u32* perm, const u64* a, long long b_off, u64* dst, long long sdst,
                         int items, int n_pair) {
        for_tiles(c, ks_rows + (gather ? 1 : 4) * (size_t)L, items, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t str) {
            const u64* ai = a + (size_t)b0 * sin;
            u64* o = dst + (size_t)b0 * sdst;
            const BfvPackTail pt{perm, n_pair ? b_off : 0, st.shift, b0, batch, n_pair};
            u64* v = ws + ks_rows * N * tb;   // the head's rows: L per item (v1), or 2L (v) and 2L behind them for (v0 + ks0, ks1)
            if (gather) {
                const u64* src = ai + sL;
                long long ssrc = sin;
                if (n_pair) {
                    launch_bfv_pack_diff(c, level, pt, ai + sL, sin, v, sL, L, nb, str);
                    src = v, ssrc = sL;
                }
                key_switch(c, level, KsSource::of_coeff(src, ssrc), key,
                           ks_onto_c0(o, sdst, ai, sin, L, {.form = KsOut::COEFF, .pack_tail = &pt}), nb, ws, str);
                return;
            }
            const u64* vv = ai;
            long long sv = sin;
            if (n_pair) {
                launch_bfv_pack_diff(c, level, pt, ai, sin, v, sp, 2 * L, nb, str);
                vv = v, sv = sp;
            }
            u64* sg = v + (size_t)sp * tb;   // (v0 + ks0, ks1), as bfv_rotate leaves it before its permutation
            key_switch(c, level, KsSource::of_coeff(vv + sL, sv), key, ks_onto_c0(sg, sp, vv, sv, L, {.form = KsOut::COEFF}), nb, ws, str);
            launch_bfv_pack_combine(c, level, pt, sg, sp, ai, sin, o, sdst, nb, str);
        });
    };
    for (size_t i = 0; i < steps.size(); i++) {
        const Step& st = steps[i];
        const Key& key = *key_of.at(st.g);
        const u32* perm = c.coeff_perm(st.g);
        const bool last = i + 1 == steps.size();   // nodes == 1 there
        u64* dst = last ? out : in;
        const long long sdst = last ? sout : sin;
        const long long b_off = (long long)st.nodes * s_index;
        if (dense || st.nodes == 1) {
            run_nodes(st, key, perm, in, b_off, dst, sdst, st.nodes * batch, st.n_pair);
            continue;
        }
        for (int a = 0; a < st.nodes; a++)
            run_nodes(st, key, perm, in + (long long)a * s_index, b_off, dst + (long long)a * s_index, sdst, batch, a < st.n_pair ? 1 : 0);
    }
}

}  // namespace lsa
