// bfv_select.hip — the BFV external product RLWE x RGSW, the CMux and the select-by-index operator (plan: bfv_select.h; the MAC's
// shared arithmetic: ks_mac_pair.h; semantics: include/lattisense_amd.h):
//   k_ks_mac_pair<KB>   the gadget MAC of an external product: two decompositions and two keys into ONE accumulator
// and below it the entry points on external_product() (key_switch.hip), which owns the decomposition, the choice of the MAC form and
// the ModDown.  Every word equals oracle/pyoracle.py's gadget_product twice, vec("add") on every row, moddown.
#include "bfv_select.h"
#include "entry_check.h"
#include "key_switch.h"
#include "ks_mac_groups.h"
#include "ks_mac_pair.h"

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

struct KsMacPairArgs {
    const u64 *cx0, *cx1;     // NTT(c0), NTT(c1): [L][N] per item
    const u64 *ext0, *ext1;   // their decompositions: [beta][L+k][N] per item
    const u64 *key0, *key1;   // R0, R1
    u64* acc;                 // [2][L+k][N] per item
    long long scx, sext, sacc;
    const ModDev* mods;
    int logn, L, np, nq, beta, klvl0, klvl1, batch, bpt;
};

struct PairSums {   // one point pair x, x+1 and both key halves
    u64 h00 = 0, l00 = 0, h01 = 0, l01 = 0, h10 = 0, l10 = 0, h11 = 0, l11 = 0;
    u64 r00 = 0, r01 = 0, r10 = 0, r11 = 0;
};
__device__ __forceinline__ void pair_term(PairSums& a, const ulonglong2& e, const ulonglong2& k0, const ulonglong2& k1) {
    mac128(a.h00, a.l00, e.x, k0.x);
    mac128(a.h01, a.l01, e.y, k0.y);
    mac128(a.h10, a.l10, e.x, k1.x);
    mac128(a.h11, a.l11, e.y, k1.y);
}
__device__ __forceinline__ void pair_fold(PairSums& a, const ModDev& m) {
    a.r00 = add_mod(a.r00, csub(mont_redc_lazy(a.h00, a.l00, m.q, m.qinv), m.q), m.q);
    a.r01 = add_mod(a.r01, csub(mont_redc_lazy(a.h01, a.l01, m.q, m.qinv), m.q), m.q);
    a.r10 = add_mod(a.r10, csub(mont_redc_lazy(a.h10, a.l10, m.q, m.qinv), m.q), m.q);
    a.r11 = add_mod(a.r11, csub(mont_redc_lazy(a.h11, a.l11, m.q, m.qinv), m.q), m.q);
    a.h00 = a.l00 = a.h01 = a.l01 = a.h10 = a.l10 = a.h11 = a.l11 = 0;
}

// grid: x = T * (N/2/TPB), y = groups of `bpt` batch items (k_ks_mac's walk, ks_mac_groups.h).  A thread owns target limb tl and the
// points x, x+1.  KB > 0: beta <= KB digits, the 4 * KB key words of both keys register-resident across the items the thread walks
// and the next item's 2 * KB digit values fetched before the current one is multiplied (k_ks_mac's prefetch); 2 * KB <= 8 products,
// one fold.  KB == 0: any beta, keys and digits streamed per item, a fold after every eighth product (ks_mac_pair.h).
template <int KB>
__global__ __launch_bounds__(TPB) void k_ks_mac_pair(KsMacPairArgs g) {
    static_assert(2 * KB <= KS_PAIR_FOLD, "a register-resident sum is folded once");
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int tl = blockIdx.x / chunks;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const int T = g.L + g.np;
    const ModDev m = g.mods[tl < g.L ? tl : g.nq + (tl - g.L)];
    const long long N = 1LL << g.logn;
    const int own_d = tl < g.L ? tl / g.np : -1;   // the digit that contains this limb reads NTT(c_h) directly
    const int kc0 = g.klvl0 + 1 + g.np, kc1 = g.klvl1 + 1 + g.np;
    const u64* pk0 = g.key0 + (long long)(tl < g.L ? tl : g.klvl0 + 1 + (tl - g.L)) * N + x;   // digit d: + 2 d kc N; half 1: + kc N
    const u64* pk1 = g.key1 + (long long)(tl < g.L ? tl : g.klvl1 + 1 + (tl - g.L)) * N + x;
    auto e_of = [&](const u64* cx, const u64* ext, long long b, int d) {
        return ld2(d == own_d ? cx + b * g.scx + tl * N + x : ext + b * g.sext + ((long long)d * T + tl) * N + x);
    };
    const int b_begin = blockIdx.y * g.bpt;
    const int b_end = min(g.batch, b_begin + g.bpt);
    if constexpr (KB > 0) {
        ulonglong2 ka0[KB], ka1[KB], kb0[KB], kb1[KB], en0[KB], en1[KB];
#pragma unroll
        for (int d = 0; d < KB; d++) {
            if (d < g.beta) {
                ka0[d] = ld2(pk0 + (long long)(2 * d) * kc0 * N);
                ka1[d] = ld2(pk0 + (long long)(2 * d + 1) * kc0 * N);
                kb0[d] = ld2(pk1 + (long long)(2 * d) * kc1 * N);
                kb1[d] = ld2(pk1 + (long long)(2 * d + 1) * kc1 * N);
            }
        }
        auto fetch = [&](long long b) {
#pragma unroll
            for (int d = 0; d < KB; d++) {
                if (d < g.beta) {
                    en0[d] = e_of(g.cx0, g.ext0, b, d);
                    en1[d] = e_of(g.cx1, g.ext1, b, d);
                }
            }
        };
        if (b_begin < b_end) fetch(b_begin);
        for (long long b = b_begin; b < b_end; b++) {
            ulonglong2 ec0[KB], ec1[KB];
#pragma unroll
            for (int d = 0; d < KB; d++) {
                ec0[d] = en0[d];
                ec1[d] = en1[d];
            }
            if (b + 1 < b_end) fetch(b + 1);
            PairSums a;
#pragma unroll
            for (int d = 0; d < KB; d++)
                if (d < g.beta) pair_term(a, ec0[d], ka0[d], ka1[d]);
#pragma unroll
            for (int d = 0; d < KB; d++)
                if (d < g.beta) pair_term(a, ec1[d], kb0[d], kb1[d]);
            pair_fold(a, m);
            u64* pa = g.acc + b * g.sacc + tl * N + x;
            st2(pa, a.r00, a.r01);
            st2(pa + (long long)T * N, a.r10, a.r11);
        }
    } else {
        for (long long b = b_begin; b < b_end; b++) {
            PairSums a;
            int p = 0;
            for (int d = 0; d < g.beta; d++, p++) {
                const ulonglong2 e = e_of(g.cx0, g.ext0, b, d);
                pair_term(a, e, ld2(pk0 + (long long)(2 * d) * kc0 * N), ld2(pk0 + (long long)(2 * d + 1) * kc0 * N));
                if (ks_pair_fold_after(p)) pair_fold(a, m);
            }
            for (int d = 0; d < g.beta; d++, p++) {
                const ulonglong2 e = e_of(g.cx1, g.ext1, b, d);
                pair_term(a, e, ld2(pk1 + (long long)(2 * d) * kc1 * N), ld2(pk1 + (long long)(2 * d + 1) * kc1 * N));
                if (ks_pair_fold_after(p)) pair_fold(a, m);
            }
            pair_fold(a, m);
            u64* pa = g.acc + b * g.sacc + tl * N + x;
            st2(pa, a.r00, a.r01);
            st2(pa + (long long)T * N, a.r10, a.r11);
        }
    }
}

// what the three entry points share: the scheme and level (EntryCheck), a special prime, the ring, the two keys of the selector
void rgsw_check(const EntryCheck& ck) {
    LSA_REQUIRE(ck.c.np >= 1, ck.who + ": the external product needs at least one special prime");
    LSA_REQUIRE(ck.c.n >= 2 * TPB, ck.who + ": ring degree too small (need N >= 512)");
}
void rgsw_keys(const EntryCheck& ck, const Key* r0, const Key* r1) {
    LSA_REQUIRE(r0 != nullptr, ck.who + ": r0 is null");
    LSA_REQUIRE(r1 != nullptr, ck.who + ": r1 is null");
    ck.key(*r0, "r0");
    ck.key(*r1, "r1");
}

}  // namespace

void launch_ks_mac_pair(Context& c, int level, const u64* cx0, const u64* cx1, long long scx, const u64* ext0, const u64* ext1,
                        long long sext, const Key& r0, const Key& r1, u64* acc, long long sacc, int batch, hipStream_t s) {
    if (batch <= 0) return;
    LSA_REQUIRE(cx0 && cx1 && ext0 && ext1 && acc && r0.data && r1.data, "pair key MAC: null operand");
    LSA_REQUIRE(level >= 0 && level < c.nq && c.np >= 1, "pair key MAC: level out of range or no special prime");
    LSA_REQUIRE(r0.level >= level && r1.level >= level, "pair key MAC: key exported at a lower level than the ciphertext");
    LSA_REQUIRE(c.n >= 2 * TPB, "ring degree too small for the pair key MAC (need N >= 512)");
    KsMacPairArgs g{};
    g.cx0 = cx0, g.cx1 = cx1, g.ext0 = ext0, g.ext1 = ext1;
    g.key0 = r0.data, g.key1 = r1.data;
    g.acc = acc;
    g.scx = scx, g.sext = sext, g.sacc = sacc;
    g.mods = c.d_mods;
    g.logn = c.logn;
    g.L = level + 1;
    g.np = c.np;
    g.nq = c.nq;
    g.beta = ceil_div(g.L, c.np);
    g.klvl0 = r0.level, g.klvl1 = r1.level;
    const int T = g.L + c.np;
    // per item: 2 beta T digit rows read, 2T written; per group the 4 beta T key rows (counted once, as launch_ks_mac does)
    ProfScope ps(c, PROF_KSMAC, 8.0 * c.n * (batch * (2.0 * g.beta * T + 2.0 * T) + 4.0 * g.beta * T), s);
    const unsigned gx = (unsigned)(T * (c.n / (2 * TPB)));
    const KsMacGroups gr = ks_mac_groups(gx, batch);
    g.batch = batch;
    g.bpt = gr.bpt;
    const dim3 grid(gx, (unsigned)gr.gy);
    switch (ks_pair_resident(g.beta)) {
    case 1: hipLaunchKernelGGL((k_ks_mac_pair<1>), grid, dim3(TPB), 0, s, g); break;
    case 2: hipLaunchKernelGGL((k_ks_mac_pair<2>), grid, dim3(TPB), 0, s, g); break;
    case 3: hipLaunchKernelGGL((k_ks_mac_pair<3>), grid, dim3(TPB), 0, s, g); break;
    case 4: hipLaunchKernelGGL((k_ks_mac_pair<4>), grid, dim3(TPB), 0, s, g); break;
    default: hipLaunchKernelGGL((k_ks_mac_pair<0>), grid, dim3(TPB), 0, s, g); break;
    }
    LSA_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ the operators
void bfv_external_product(Context& c, int level, const u64* ct, long long sct, const Key* r0, const Key* r1, const u64* base,
                          long long sbase, u64* out, long long sout, int batch, hipStream_t s) {
    const EntryCheck ck(c, "lsa_bfv_external_product", LSA_ALGO_BFV, level, 0, batch);
    rgsw_check(ck);
    rgsw_keys(ck, r0, r1);
    if (batch <= 0) return;
    const long long N = c.n;
    const int L = level + 1;
    const size_t w = 2 * (size_t)L * N;
    const layout::Span sp_out = ck.output(out, sout, w);
    // the decomposition has read ct before the tail writes, and the tail reads base only at the points it writes
    ck.same_or_apart(sp_out, ck.operand(ct, sct, w, "ct", false), "ct");
    if (base) ck.same_or_apart(sp_out, ck.operand(base, sbase, w, "base", false), "base");
    const size_t ks_rows = KsTile::rows(c, level, KsSource::COEFF);
    for_tiles(c, 2 * ks_rows, batch, s, [&](int nb, int b0, u64* ws, int, hipStream_t str) {
        const KsOut o = ks_onto(base ? 2 : 0, out + (size_t)b0 * sout, sout, base ? base + (size_t)b0 * sbase : nullptr, sbase, L,
                                {.form = KsOut::COEFF});
        external_product(c, level, ct + (size_t)b0 * sct, sct, *r0, *r1, o, nb, ws, str);
    });
}

// v = c1 - c0 lands dense in the tile's workspace behind the two decompositions; c0 joins as the tail's base
static void cmux_tiles(Context& c, int level, const u64* c0, long long s0, const u64* c1, long long s1, const Key& r0, const Key& r1,
                       u64* out, long long sout, int items, hipStream_t s) {
    const long long N = c.n;
    const int L = level + 1;
    const long long sp = 2LL * L * N;
    const size_t ks_rows = KsTile::rows(c, level, KsSource::COEFF);
    for_tiles(c, 2 * ks_rows + 2 * (size_t)L, items, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t str) {
        u64* v = ws + 2 * ks_rows * N * tb;
        const u64* a = c0 + (size_t)b0 * s0;
        launch_elementwise(c, EW_SUB, c1 + (size_t)b0 * s1, a, v, nb, s1, s0, sp, 2 * L, rm_seq(L), str);
        external_product(c, level, v, sp, r0, r1, ks_onto_ct(out + (size_t)b0 * sout, sout, a, s0, L, {.form = KsOut::COEFF}), nb, ws, str);
    });
}

void bfv_cmux(Context& c, int level, const u64* c0, long long s0, const u64* c1, long long s1, const Key* r0, const Key* r1, u64* out,
              long long sout, int batch, hipStream_t s) {
    const EntryCheck ck(c, "lsa_bfv_cmux", LSA_ALGO_BFV, level, 0, batch);
    rgsw_check(ck);
    rgsw_keys(ck, r0, r1);
    if (batch <= 0) return;
    const size_t w = 2 * (size_t)(level + 1) * c.n;
    const layout::Span sp_out = ck.output(out, sout, w);
    // the difference has read c1 (and c0) before the tail writes; c0 is the tail's base
    ck.same_or_apart(sp_out, ck.operand(c0, s0, w, "c0", false), "c0");
    ck.same_or_apart(sp_out, ck.operand(c1, s1, w, "c1", false), "c1");
    cmux_tiles(c, level, c0, s0, c1, s1, *r0, *r1, out, sout, batch, s);
}

BfvSelectPlanHost bfv_select_plan_checked(int count) {
    try {
        return bfv_select_plan(count);
    } catch (const std::invalid_argument& e) {
        throw Error(LSA_ERR_ARG, e.what());
    }
}

BfvSelect* bfv_select_create(Context& c, int level, int count) {
    LSA_REQUIRE(c.algo == LSA_ALGO_BFV, "lsa_bfv_select_create: context is not BFV");
    LSA_REQUIRE(level >= 0 && level < c.nq, "lsa_bfv_select_create: level out of range (0.." + std::to_string(c.nq - 1) + ")");
    auto p = std::make_unique<BfvSelect>(c, level);
    p->plan = bfv_select_plan_checked(count);
    LSA_REQUIRE(p->plan.levels.empty() || c.np >= 1, "lsa_bfv_select_create: count: the external product needs at least one special prime");
    LSA_REQUIRE(p->plan.levels.empty() || c.n >= 2 * TPB, "lsa_bfv_select_create: ring degree too small (need N >= 512)");
    return p.release();
}

// All levels but the last work inside the input array: level j reads the nodes c[a], a < n_pair, and their partners c[a + 2^j], and
// writes c'[a] over c[a]; the last level (j = 0) writes `out`.  The tiles of a level write disjoint c[a] and read partners that no tile
// of that level writes (a + 2^j >= 2^j > every node written), so tiles on two streams do not meet; a tile's difference lands in its
// own half of the workspace.  Dense layout (s_index == batch * sin): the n_pair x batch items of a level are one strided batch --
// one difference launch and one tiled external product.  Otherwise one tiled CMux per paired node.  Unpaired nodes get no launch.
void bfv_select_run(BfvSelect& p, u64* in, long long sin, long long s_index, u64* out, long long sout, int batch, int n_sel,
                    const Key* const* r0s, const Key* const* r1s, hipStream_t s) {
    Context& c = p.c;
    const int level = p.level, count = p.plan.count, k = (int)p.plan.levels.size();
    const EntryCheck ck(c, "lsa_bfv_select", LSA_ALGO_BFV, level, 0, batch);
    LSA_REQUIRE(n_sel >= k, ck.who + ": n_sel: " + std::to_string(k) + " selectors needed, " + std::to_string(n_sel) + " given");
    if (k > 0) {
        rgsw_check(ck);
        LSA_REQUIRE(r0s && r1s, ck.who + ": r0s / r1s is null");
        for (int j = 0; j < k; j++) rgsw_keys(ck, r0s[j], r1s[j]);
    }
    if (batch <= 0) return;
    const long long N = c.n;
    const int L = level + 1;
    const size_t w = 2 * (size_t)L * N;
    const layout::Span sp_in0 = ck.operand(in, sin, w, "in", false);
    // `out` is input 0 itself or shares no word with any input
    const auto [in_place, dense] = ck.indexed_array(ck.output(out, sout, w), sp_in0, s_index, count, "sin", "input 0", "an input");
    if (k == 0) {   // count == 1: a copy
        if (!in_place) copy_ciphertexts(c, level, in, sin, out, sout, batch, s);
        return;
    }
    for (const BfvSelectLevel& lv : p.plan.levels) {
        const Key &r0 = *r0s[lv.bit], &r1 = *r1s[lv.bit];
        const bool last = lv.bit == 0;   // one node there
        u64* dst = last ? out : in;
        const long long sdst = last ? sout : sin;
        const long long b_off = (long long)lv.nodes * s_index;
        if (dense || lv.n_pair == 1) {
            cmux_tiles(c, level, in, sin, in + b_off, sin, r0, r1, dst, sdst, lv.n_pair * batch, s);
            continue;
        }
        for (int a = 0; a < lv.n_pair; a++) {
            const u64* ca = in + (long long)a * s_index;
            cmux_tiles(c, level, ca, sin, ca + b_off, sin, r0, r1, dst + (long long)a * s_index, sdst, batch, s);
        }
    }
}

}  // namespace lsa
