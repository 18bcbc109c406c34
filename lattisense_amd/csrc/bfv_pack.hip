// bfv_pack.hip — the BFV coefficient packing (plan and point arithmetic: bfv_pack.h; semantics: include/lattisense_amd.h):
//   k_bfv_pack_diff     the head of a paired level: v = a - X^s b into the tile's workspace, the source of the level's key switch
//                       (polynomial 1 alone in the gather form, both in the two-step form); an unpaired node's rows pass through
//   k_bfv_pack_tail     the coefficient-domain ModDown tail of one level, the key switch's tail hook (BfvPackTail): the row skeleton
//                       of moddown_gather.h with PackOp -- (acc - conv) / P (+ a0 - xb0) staged in LDS, the rotation gathered from
//                       there and added to u = a + X^s b, which the thread kept from the staging loop
//   k_bfv_pack_combine  the two-step form: the key switch leaves (v0 + ks0, ks1) in the workspace and this kernel gathers the
//                       rotation from global memory (N > 2^14, unfused tails, the plan's gather switched off) into the same
//                       PackOp::finish
// and below them the runner on key_switch() (bfv_pack_run).  Every word equals the composition lsa_bfv_mul_monomial, lsa_poly_addsub
// (add, sub), lsa_bfv_rotate, lsa_poly_addsub (add): canonical residues, add_mod / sub_mod / neg_mod.
#include "bfv_pack.h"
#include "entry_check.h"
#include "moddown_gather.h"

namespace lsa {

namespace {

constexpr int TPB = 256;

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

// one level's tail over the items of a tile, a = KsOut::base and out = KsOut::p [2][L][N] per item (out may be a), b = a + b_off the
// partner:
//   xb[h][j][x] = +-b[h][j][(x - shift) mod N], negated when x < shift (0 where the node has no partner),
//   out = (a + xb) + rotate(a - xb, g), for the items whose index coordinate (item0 + i) / batch is below n_pair
struct BfvPackTail final : KsCoeffTail {
    const u32* perm;      // Context::coeff_perm(g)
    long long b_off;      // words from an item's a to its partner
    int shift;            // s = N / 2^l
    int item0, batch, n_pair;
    BfvPackTail(const u32* perm_, long long b_off_, int shift_, int item0_, int batch_, int n_pair_)
        : KsCoeffTail(1), perm(perm_), b_off(b_off_), shift(shift_), item0(item0_), batch(batch_), n_pair(n_pair_) {}
    void launch(Context& c, int level, const u64* acc, long long s_acc, int acc_rpp, const u64* conv, long long s_conv, const KsOut& o,
                int nb, hipStream_t s) const override;
};

struct PackArgs {
    RowTailArgs t;   // base: a (diff: from the first row it takes), out may be a (diff: v, `limbs`-periodic rows).  combine: acc is the
                     // rotation's source (v0 + ks0, ks1), [2][L][N]
    long long b_off;
    int shift;
    int item0, batch, n_pair;   // item item0 + blockIdx.y has a partner iff its index coordinate, item / batch, is below n_pair
};

// the packing's row `row` of item blockIdx.y.  A thread reads a only at the points it writes (u stays in registers across the
// barrier), so out may lie over a; b belongs to a node no key switch of this level writes.
struct PackOp {
    using Keep = ulonglong2;
    static constexpr bool KEEPS = true;
    const u64 *a, *b;   // b: the partner's row, or null
    u64* out;
    unsigned shift;
    int logn;
    u64 q;
    __device__ __forceinline__ PackOp(const PackArgs& g, int row) : shift((unsigned)g.shift), logn(g.t.logn), q(g.t.mods[row % g.t.limbs].q) {
        const long long i = blockIdx.y, ro = (long long)row << g.t.logn;
        a = g.t.base + i * g.t.sbase + ro;
        b = (g.item0 + (int)blockIdx.y) / g.batch < g.n_pair ? a + g.b_off : nullptr;   // uniform over the workgroup
        out = g.t.out + i * g.t.sout + ro;
    }
    // u = a + X^s b and d = a - X^s b at the points (x, x + 1); both a without a partner
    __device__ __forceinline__ void sum_diff(int x, ulonglong2& u, ulonglong2& d) const {
        u = d = ld2(a + x);
        if (!b) return;
        const ulonglong2 xb = shifted_pair(b, (unsigned)x, shift, logn, q);
        d.x = sub_mod(u.x, xb.x, q);
        d.y = sub_mod(u.y, xb.y, q);
        u.x = add_mod(u.x, xb.x, q);
        u.y = add_mod(u.y, xb.y, q);
    }
    __device__ __forceinline__ void stage(int x, int poly, ulonglong2& r, Keep& u) const {
        ulonglong2 d;
        sum_diff(x, u, d);
        if (poly == 0) {
            r.x = add_mod(r.x, d.x, q);
            r.y = add_mod(r.y, d.y, q);
        }
    }
    // out = u + sigma
    __device__ __forceinline__ void finish(int y, const Keep& u, ulonglong2 s) const { st2(out + y, add_mod(u.x, s.x, q), add_mod(u.y, s.y, q)); }
};

// grid: x = rows * (N/2/TPB), y = items.  v[row][x] = a[row][x] - (X^s b)[row][x], or a[row][x] where the node has no partner
__global__ __launch_bounds__(TPB) void k_bfv_pack_diff(PackArgs g) {
    const int chunks = (1 << g.t.logn) / (2 * TPB);
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const PackOp op(g, blockIdx.x / chunks);
    ulonglong2 u, d;
    op.sum_diff(x, u, d);
    st2(op.out + x, d.x, d.y);
}

__global__ __launch_bounds__(LSA_LDS_ROW_THREADS) void k_bfv_pack_tail(PackArgs g) { gathered_tail_row(g.t, PackOp(g, blockIdx.x)); }

// grid: x = 2*limbs * (N/2/TPB), y = items.  acc: the rotation's source in the workspace.  A thread reads only the words of a it
// writes over.
__global__ __launch_bounds__(TPB) void k_bfv_pack_combine(PackArgs g) {
    const int chunks = (1 << g.t.logn) / (2 * TPB);
    const int row = blockIdx.x / chunks;
    const int y = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const PackOp op(g, row);
    ulonglong2 u, d;
    op.sum_diff(y, u, d);
    op.finish(y, u, lds_gather_pair(g.t.acc + blockIdx.y * g.t.sacc + ((long long)row << g.t.logn), g.t.perm, y, op.q));
}

// the fields of a kernel outside the key switch (head, combine): a and out as the tail hook gets them from KsOut
PackArgs pack_args(Context& c, int level, const BfvPackTail& t, const u64* a, long long sa, u64* out, long long sout) {
    LSA_REQUIRE(level >= 0 && level < c.nq, "BFV pack: level out of range");
    LSA_REQUIRE(a && out, "BFV pack: null operand");
    LSA_REQUIRE(t.batch >= 1 && t.item0 >= 0 && t.n_pair >= 0, "BFV pack: bad node geometry");
    LSA_REQUIRE(t.n_pair == 0 || (t.shift >= 1 && t.shift < c.n && t.b_off != 0), "BFV pack: a paired level needs its shift and partner");
    LSA_REQUIRE(((t.b_off | sa | sout) & 1) == 0, "BFV pack: odd stride");
    PackArgs g{};
    g.t.perm = t.perm;
    g.t.base = a;
    g.t.sbase = sa;
    g.t.out = out;
    g.t.sout = sout;
    g.t.mods = c.d_mods;
    g.t.limbs = level + 1;
    g.t.logn = c.logn;
    g.b_off = t.b_off;
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
    g.t.acc = sigma;
    g.t.sacc = ssigma;
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * 2 * L * (3.0 * nb + pack_paired_items(t, nb)) + 4.0 * c.n * 2 * L * nb, s);
    hipLaunchKernelGGL(k_bfv_pack_combine, dim3((unsigned)(2 * L * (c.n / (2 * TPB))), (unsigned)nb), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

void BfvPackTail::launch(Context& c, int level, const u64* acc, long long s_acc, int acc_rpp, const u64* conv, long long s_conv,
                         const KsOut& o, int nb, hipStream_t s) const {
    if (nb <= 0) return;
    const int L = level + 1;
    LSA_REQUIRE(perm != nullptr, "BFV pack tail: null or short operand");
    const PackArgs g = pack_args(c, level, *this, o.base, o.sbase, o.p, o.sp);
    // per row: acc, conv and a read, the partner where there is one, the result written, 4 bytes per point of the table
    launch_lds_row_tail<&k_bfv_pack_tail>(c, level, "BFV pack tail", g, acc, s_acc, acc_rpp, conv, s_conv, o, nb,
                                          8.0 * c.n * 2 * L * (4.0 * nb + pack_paired_items(*this, nb)) + 4.0 * c.n * 2 * L * nb, s);
}

}  // namespace

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
    glk.resolve(p.plan.galois, ck.who, [&](u64, const Key& k) { ck.key(k, "a Galois key"); });
    if (batch <= 0) return;
    const long long N = c.n;
    const int L = level + 1;
    const size_t w = 2 * (size_t)L * N;
    const layout::Span sp_in0 = ck.operand(in, sin, w, "in", false);
    // `out` is input 0 itself or shares no word with any input
    const auto [in_place, dense] = ck.indexed_array(ck.output(out, sout, w), sp_in0, s_index, count, "sin", "input 0", "an input");
    struct Step {
        int nodes, n_pair, shift;
        u64 g;
    };
    std::vector<Step> steps;
    for (const BfvPackLevel& lv : p.plan.levels) steps.push_back({lv.nodes, lv.n_pair, lv.shift, lv.g});
    for (u64 g : p.plan.trace_g) steps.push_back({1, 0, 0, g});
    if (steps.empty()) {   // count == 1 without the trace: a copy
        if (!in_place) copy_ciphertexts(c, level, in, sin, out, sout, batch, s);
        return;
    }
    const bool gather = p.gather && c.fuse_tails && c.logn <= LSA_PERM_LDS_MAX_LOGN;
    const size_t ks_rows = KsTile::rows(c, level, KsSource::COEFF);
    const long long sp = 2LL * L * N, sL = (long long)L * N;
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
                           ks_onto_c0(o, sdst, ai, sin, L, {.form = KsOut::COEFF, .tail = &pt}), nb, ws, str);
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
        const Key& key = *glk.at(st.g);
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
