// bfv_expand.hip — the BFV oblivious expansion (plan and point arithmetic: bfv_expand.h; semantics: include/lattisense_amd.h):
//   k_bfv_expand_tail     the coefficient-domain ModDown tail of one level, the key switch's tail hook (BfvExpandTail): the row
//                         skeleton of moddown_gather.h with ExpandOp -- (acc - conv) / P (+ c0) staged in LDS, the rotation
//                         gathered from there, and BOTH children stored -- the even one over the parent, the odd one shifted
//   k_bfv_expand_combine  the two-step form: the key switch leaves (c0 + ks0, ks1) in the workspace and this kernel gathers the
//                         rotation from global memory (N > 2^14, unfused tails, the plan's gather switched off) into the same
//                         ExpandOp::finish
//   k_mul_monomial        X^e * in, the negacyclic shift (lsa_bfv_mul_monomial)
// and below them the runner on key_switch() (bfv_expand_run).  Every word equals the composition lsa_bfv_rotate, lsa_poly_addsub
// (add, sub), lsa_bfv_mul_monomial: canonical residues, add_mod / sub_mod / neg_mod.
#include "bfv_expand.h"
#include "entry_check.h"
#include "moddown_gather.h"

namespace lsa {

namespace {

constexpr int TPB = 256;

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

// one level's tail over the items of a tile, parent = KsOut::base and even = KsOut::p [2][L][N] per item (even may be parent),
// sigma = rotate(parent, g):
//   even[h][j][y] = parent[h][j][y] + sigma[h][j][y]
//   odd[h][j][(y - shift) mod N] = +-(parent[h][j][y] - sigma[h][j][y]), odd = even + odd_off, negated when y < shift,
//   for the items whose index coordinate (item0 + i) / batch is below n_odd
struct BfvExpandTail final : KsCoeffTail {
    const u32* perm;      // Context::coeff_perm(g)
    long long odd_off;    // words from an item's even child to its odd child
    int shift;            // s = 2^j
    int item0, batch, n_odd;
    BfvExpandTail(const u32* perm_, long long odd_off_, int shift_, int item0_, int batch_, int n_odd_)
        : KsCoeffTail(1), perm(perm_), odd_off(odd_off_), shift(shift_), item0(item0_), batch(batch_), n_odd(n_odd_) {}
    void launch(Context& c, int level, const u64* acc, long long s_acc, int acc_rpp, const u64* conv, long long s_conv, const KsOut& o,
                int nb, hipStream_t s) const override;
};

struct ExpandArgs {
    RowTailArgs t;        // base: the parent, out: the even child.  combine: acc is the rotated pair's source (c0 + ks0, ks1), [2][L][N]
    long long odd_off;
    int shift;
    int item0, batch, n_odd;   // item item0 + blockIdx.y has an odd child iff its index coordinate, item / batch, is below n_odd
};

// the expansion's row `row` of item blockIdx.y: the parent's words are kept from the staging loop on (read once), so the even child
// may be written over the parent
struct ExpandOp {
    using Keep = ulonglong2;
    static constexpr bool KEEPS = true;
    const u64* c;
    u64 *even, *odd;
    unsigned shift;
    int logn;
    u64 q;
    __device__ __forceinline__ ExpandOp(const ExpandArgs& g, int row) : shift((unsigned)g.shift), logn(g.t.logn), q(g.t.mods[row % g.t.limbs].q) {
        const long long b = blockIdx.y, ro = (long long)row << g.t.logn;
        c = g.t.base + b * g.t.sbase + ro;
        even = g.t.out + b * g.t.sout + ro;
        odd = (g.item0 + (int)blockIdx.y) / g.batch < g.n_odd ? even + g.odd_off : nullptr;   // uniform over the workgroup
    }
    __device__ __forceinline__ Keep keep(int y) const { return ld2(c + y); }
    __device__ __forceinline__ void stage(int x, int poly, ulonglong2& r, Keep& cv) const {
        cv = keep(x);
        if (poly == 0) {
            r.x = add_mod(r.x, cv.x, q);
            r.y = add_mod(r.y, cv.y, q);
        }
    }
    __device__ __forceinline__ void finish(int y, const Keep& cv, ulonglong2 s) const {
        expand_children(even, odd, (unsigned)y, shift, logn, cv, s.x, s.y, q);
    }
};

__global__ __launch_bounds__(LSA_LDS_ROW_THREADS) void k_bfv_expand_tail(ExpandArgs g) { gathered_tail_row(g.t, ExpandOp(g, blockIdx.x)); }

// grid: x = 2*limbs * (N/2/TPB), y = items.  acc: the rotation's source in the workspace.  A thread reads only the parent's words it
// writes over.
__global__ __launch_bounds__(TPB) void k_bfv_expand_combine(ExpandArgs g) {
    const int chunks = (1 << g.t.logn) / (2 * TPB);
    const int row = blockIdx.x / chunks;
    const int y = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const ExpandOp op(g, row);
    op.finish(y, op.keep(y), lds_gather_pair(g.t.acc + blockIdx.y * g.t.sacc + ((long long)row << g.t.logn), g.t.perm, y, op.q));
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
    g.t.perm = t.perm;
    g.t.base = parent;
    g.t.sbase = sparent;
    g.t.out = even;
    g.t.sout = seven;
    g.t.mods = c.d_mods;
    g.t.limbs = level + 1;
    g.t.logn = c.logn;
    g.odd_off = t.odd_off;
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

void BfvExpandTail::launch(Context& c, int level, const u64* acc, long long s_acc, int acc_rpp, const u64* conv, long long s_conv,
                           const KsOut& o, int nb, hipStream_t s) const {
    if (nb <= 0) return;
    const int L = level + 1;
    const ExpandArgs g = expand_args(c, level, *this, o.base, o.sbase, o.p, o.sp);
    // per row: acc, conv and the parent read, the children written, 4 bytes per point of the table
    launch_lds_row_tail<&k_bfv_expand_tail>(c, level, "BFV expand tail", g, acc, s_acc, acc_rpp, conv, s_conv, o, nb,
                                            8.0 * c.n * 2 * L * (3.0 * nb + expand_child_rows(*this, nb)) + 4.0 * c.n * 2 * L * nb, s);
}

// sigma: (c0 + ks0, ks1), [2][L][N] per item, not yet rotated
void launch_bfv_expand_combine(Context& c, int level, const BfvExpandTail& t, const u64* sigma, long long ssigma, const u64* parent,
                               long long sparent, u64* even, long long seven, int nb, hipStream_t s) {
    if (nb <= 0) return;
    const int L = level + 1;
    LSA_REQUIRE(sigma != nullptr, "BFV expand combine: null operand");
    LSA_REQUIRE(c.n >= 2 * TPB, "ring degree too small for the BFV expand combine (need N >= 512)");
    ExpandArgs g = expand_args(c, level, t, parent, sparent, even, seven);
    g.t.acc = sigma;
    g.t.sacc = ssigma;
    ProfScope ps(c, PROF_ELEMWISE, 8.0 * c.n * 2 * L * (2.0 * nb + expand_child_rows(t, nb)) + 4.0 * c.n * 2 * L * nb, s);
    hipLaunchKernelGGL(k_bfv_expand_combine, dim3((unsigned)(2 * L * (c.n / (2 * TPB))), (unsigned)nb), dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

}  // namespace

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
    glk.resolve(p.plan.galois, ck.who, [&](u64, const Key& k) { ck.key(k, "a Galois key"); });
    if (batch <= 0) return;
    const long long N = c.n;
    const int L = level + 1;
    const size_t w = 2 * (size_t)L * N;
    const layout::Span sp_in = ck.operand(in, sin, w, "in", false);
    // `in` is output 0 itself or shares no word with any output
    const auto [in_place, dense] = ck.indexed_array(sp_in, ck.output(out, sout, w), s_index, count, "sout", "in", "in");
    if (p.plan.levels.empty()) {   // count == 1: a copy
        if (!in_place) copy_ciphertexts(c, level, in, sin, out, sout, batch, s);
        return;
    }
    const bool gather = p.gather && c.fuse_tails && c.logn <= LSA_PERM_LDS_MAX_LOGN;
    const size_t ks_rows = KsTile::rows(c, level, KsSource::COEFF);
    const long long sp = 2LL * L * N, sL = (long long)L * N;
    // one key switch over `items` parents (stride spar) whose even children lie at `even` (stride sout)
    auto run_nodes = [&](const BfvExpandLevel& lv, const Key& key, const u32* perm, const u64* parent, long long spar, u64* even,
                         int items, int n_odd) {
        for_tiles(c, ks_rows + (gather ? 0 : 2 * (size_t)L), items, s, [&](int nb, int b0, u64* ws, int tb, hipStream_t st) {
            const u64* ct = parent + (size_t)b0 * spar;
            u64* ev = even + (size_t)b0 * sout;
            const BfvExpandTail et{perm, (long long)lv.shift * s_index, lv.shift, b0, batch, n_odd};
            if (gather) {
                key_switch(c, level, KsSource::of_coeff(ct + sL, spar), key,
                           ks_onto_c0(ev, sout, ct, spar, L, {.form = KsOut::COEFF, .tail = &et}), nb, ws, st);
                return;
            }
            u64* sg = ws + ks_rows * N * tb;   // (c0 + ks0, ks1), as bfv_rotate leaves it before its permutation
            key_switch(c, level, KsSource::of_coeff(ct + sL, spar), key, ks_onto_c0(sg, sp, ct, spar, L, {.form = KsOut::COEFF}), nb, ws, st);
            launch_bfv_expand_combine(c, level, et, sg, sp, ct, spar, ev, sout, nb, st);
        });
    };
    for (size_t j = 0; j < p.plan.levels.size(); j++) {
        const BfvExpandLevel& lv = p.plan.levels[j];
        const Key& key = *glk.at(lv.g);
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
