// bfv_poly.hip — BFV polynomial evaluation on a ciphertext (lsa_bfv_poly_* / lsa_bfv_poly_eval) and the constant operands of a
// BFV ciphertext (lsa_bfv_affine_const): the leaf kernel, the plan and the runner.  The planner and the kernel's constants are
// bfv_poly.h's (host only); DESIGN.md 4.15 explains the plan, tests/bfv_poly_model.py restates it over the CPU oracle.
//
//   k_bfv_poly_leaves  up to 8 linear combinations of the same (up to 15) coefficient-domain ciphertexts at ONE level by per-limb
//                      integer constants, each plus a constant in every slot: out_o = sum_i K_oi * src_i + scaleUp(c_o).  The
//                      per-element arithmetic is poly_lincomb.h's.  It differs from k_poly_lincomb (kernels.hip, CKKS, NTT domain)
//                      in three ways: the constant lands on ONE word per limb (coefficient 0 of polynomial 0: the scaled-up
//                      constant polynomial), all operands sit at one level, and every output has its own pointer and stride.
//   powers             bfv_mult_relin; the sum of leaf x giant-power products: bfv_dot, ONE scale-down and ONE relinearisation.
#include "bfv_poly.h"
#include "entry_check.h"
#include "linear_transform.h"
#include "tables.h"

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

struct BfvPolyLeavesArgs {
    const u64* src[LSA_PLC_MAX_SRC];   // [batch][2][L][N] each, coefficient domain
    long long ss[LSA_PLC_MAX_SRC];
    u64* out[LSA_PLC_MAX_OUT];         // [batch][2][L][N] each
    long long so[LSA_PLC_MAX_OUT];
    const u64* ktab;   // [n_out][nsrc][L], Montgomery form; 0: the output does not use the source
    const u64* stab;   // [n_out][L] plain residues: the word added to coefficient 0 of polynomial 0
    // IMM (one source, one output: lsa_bfv_affine_const): the two rows ride in the argument struct instead, as k_cconst's do -- a
    // caller's constants change from call to call and get no device allocation, no copy and no cache entry
    u64 kimm[LSA_BFV_AFFINE_MAX_LIMBS], simm[LSA_BFV_AFFINE_MAX_LIMBS];
    const ModDev* mods;
    int nsrc, n_out, L, logn;
};

// grid: x = 2 * L * (N/2/TPB) (polynomial, limb, 512-coefficient piece), y = batch: the element-wise grid; 16 B per lane.  The
// constants are uniform per workgroup (one limb): scalar loads.  Every source element is read once for all outputs.  An output
// may be a source of the same launch only as lsa_bfv_affine_const uses it (one source, same pointer and stride): a lane reads
// the two words it then writes.
template <int GMAX, bool IMM>
__global__ __launch_bounds__(TPB) void k_bfv_poly_leaves(BfvPolyLeavesArgs g) {
    const int chunks = (1 << g.logn) / (2 * TPB);
    const int prow = blockIdx.x / chunks;   // poly * L + limb
    const int limb = prow % g.L;
    const int x = ((blockIdx.x % chunks) * TPB + threadIdx.x) * 2;
    const long long b = blockIdx.y;
    const long long off = ((long long)prow << g.logn) + x;
    const ModDev m = g.mods[limb];
    PlcAcc a0[GMAX], a1[GMAX];
#pragma unroll
    for (int gi = 0; gi < GMAX; gi++) {
        plc_init(a0[gi]);
        plc_init(a1[gi]);
    }
    for (int i = 0; i < g.nsrc; i++) {
        const ulonglong2 v = ld2(g.src[i] + b * g.ss[i] + off);
#pragma unroll
        for (int gi = 0; gi < GMAX; gi++)
            if (gi < g.n_out) {
                const u64 k = IMM ? g.kimm[limb] : g.ktab[((long long)gi * g.nsrc + i) * g.L + limb];
                if (k) {   // uniform: a power this leaf does not use
                    plc_term(a0[gi], i, v.x, k, m.q, m.qinv);
                    plc_term(a1[gi], i, v.y, k, m.q, m.qinv);
                } else if (i == 8) {
                    plc_fold(a0[gi], m.q, m.qinv);
                    plc_fold(a1[gi], m.q, m.qinv);
                }
            }
    }
    const bool first = prow < g.L && x == 0;   // coefficient 0 of polynomial 0: v.x of one lane per limb
#pragma unroll
    for (int gi = 0; gi < GMAX; gi++)
        if (gi < g.n_out) {
            u64 r0 = plc_finish(a0[gi], m.q, m.qinv);
            const u64 r1 = plc_finish(a1[gi], m.q, m.qinv);
            if (first) r0 = add_mod(r0, IMM ? g.simm[limb] : g.stab[(long long)gi * g.L + limb], m.q);
            st2(g.out[gi] + b * g.so[gi] + off, r0, r1);
        }
}

// srcs / outs: [batch][2][level+1][N] with their batch strides; d_k [n_out][nsrc][level+1], d_s [n_out][level+1] on the device, or
// (imm, one source and one output) host rows h_k, h_s of level+1 words that travel in the argument struct
void launch_bfv_poly_leaves(Context& c, int level, int nsrc, const u64* const* src, const long long* ss, int n_out, u64* const* out,
                            const long long* so, const u64* d_k, const u64* d_s, int batch, hipStream_t s, const u64* h_k = nullptr,
                            const u64* h_s = nullptr) {
    if (batch <= 0) return;
    const int L = level + 1;
    LSA_REQUIRE(nsrc >= 0 && nsrc <= LSA_PLC_MAX_SRC && n_out >= 1 && n_out <= LSA_PLC_MAX_OUT, "bfv_poly: too many sources or outputs for one launch");
    LSA_REQUIRE(level >= 0 && level < c.nq, "bfv_poly: level out of range");
    LSA_REQUIRE(c.n >= 2 * TPB, "ring degree too small for the elementwise kernels (need N >= 512)");
    BfvPolyLeavesArgs g{};
    for (int i = 0; i < nsrc; i++) {
        g.src[i] = src[i];
        g.ss[i] = ss[i];
    }
    for (int i = 0; i < n_out; i++) {
        g.out[i] = out[i];
        g.so[i] = so[i];
    }
    g.ktab = d_k;
    g.stab = d_s;
    const bool imm = h_k != nullptr;
    if (imm) {
        LSA_REQUIRE(nsrc == 1 && n_out == 1 && h_s != nullptr && L <= LSA_BFV_AFFINE_MAX_LIMBS, "bfv_poly: internal: immediate constants");
        std::copy(h_k, h_k + L, g.kimm);
        std::copy(h_s, h_s + L, g.simm);
    }
    g.mods = c.d_mods;
    g.nsrc = nsrc;
    g.n_out = n_out;
    g.L = L;
    g.logn = c.logn;
    // algorithmic bytes: every source row read once, every output row written once
    ProfScope ps(c, PROF_ELEMWISE, 16.0 * c.n * L * batch * (nsrc + n_out), s);
    const dim3 grid((unsigned)(2 * L * (c.n / (2 * TPB))), (unsigned)batch);
    if (imm) hipLaunchKernelGGL((k_bfv_poly_leaves<1, true>), grid, dim3(TPB), 0, s, g);
    else if (n_out == 1) hipLaunchKernelGGL((k_bfv_poly_leaves<1, false>), grid, dim3(TPB), 0, s, g);
    else if (n_out == 2) hipLaunchKernelGGL((k_bfv_poly_leaves<2, false>), grid, dim3(TPB), 0, s, g);
    else if (n_out <= 4) hipLaunchKernelGGL((k_bfv_poly_leaves<4, false>), grid, dim3(TPB), 0, s, g);
    else hipLaunchKernelGGL((k_bfv_poly_leaves<8, false>), grid, dim3(TPB), 0, s, g);
    LSA_HIP(hipGetLastError());
}

// the two constant rows of one (coefficient, constant) pair: K in Montgomery form, the scaled-up constant as plain residues
void leaf_constants(const Context& c, int level, u64 k, u64 cst, u64* k_mont, u64* s_plain) {
    const int L = level + 1;
    u64 q_mod_t = 1 % c.t;
    for (int j = 0; j < L; j++) q_mod_t = mul_mod_host(q_mod_t, c.T.mod[j] % c.t, c.t);
    for (int j = 0; j < L; j++) {
        const u64 q = c.T.mod[j];
        if (k_mont) k_mont[j] = to_mont_host(bfv_poly_centred_mod(k, c.t, q), q);
        if (s_plain) s_plain[j] = cst ? bfv_poly_scale_up_word(cst, c.t, q_mod_t, q, inv_mod(c.t % q, q)) : 0;
    }
}

}  // namespace

BfvPolyPlan bfv_poly_plan_checked(u64 t, int n_coef, const u64* coef, int log_baby) {
    try {
        return bfv_poly_plan(t, n_coef, coef, log_baby);
    } catch (const std::invalid_argument& e) {
        LSA_REQUIRE(false, std::string(e.what()));
    }
    return BfvPolyPlan();
}

// ------------------------------------------------------------------------------------------------ plan
struct BfvPolyLaunch {   // one k_bfv_poly_leaves launch: up to 8 leaves, in leaf order
    std::vector<int> leaves;    // positions in BfvPolyPlan::leaves
    std::vector<int> sources;   // baby powers read, ascending
    u64* d_k = nullptr;         // [n_out][nsrc][level+1]
    u64* d_s = nullptr;         // [n_out][level+1]
};

struct BfvPolynomial {
    Context& c;
    int level = 0;
    BfvPolyPlan plan;
    std::vector<BfvPolyLaunch> launches;
    std::vector<u64*> owned;
    DevPool pool;
    explicit BfvPolynomial(Context& ctx) : c(ctx) {}
    ~BfvPolynomial() {
        (void)hipSetDevice(c.device);
        (void)hipDeviceSynchronize();
        for (u64* p : owned) (void)hipFree(p);
        pool.release();
    }
};

void bfv_poly_destroy(BfvPolynomial* p) { delete p; }
const BfvPolyPlan& bfv_poly_plan_of(const BfvPolynomial& p) { return p.plan; }
int bfv_poly_level(const BfvPolynomial& p) { return p.level; }

BfvPolynomial* bfv_poly_create(Context& c, int level, int n_coef, const u64* coef, int log_baby, hipStream_t s) {
    const EntryCheck ck(c, "bfv_poly", LSA_ALGO_BFV, level, 0, 1);
    LSA_REQUIRE(c.n >= 2 * TPB, "bfv_poly: ring degree too small for the elementwise kernels (need N >= 512)");
    auto p = std::make_unique<BfvPolynomial>(c);
    p->level = level;
    p->plan = bfv_poly_plan_checked(c.t, n_coef, coef, log_baby);
    const BfvPolyPlan& pl = p->plan;
    const int L = level + 1;
    {   // what bfv_mult and bfv_dot would refuse mid-run: the auxiliary basis of one product, and of the sum's largest group
        const BfvDotPlan dp = bfv_dot_plan(c.T.mod.data(), c.nq, level, c.logn, std::max(pl.n_pairs, 1));
        const int M = std::max(bfv_aux_count(c.T.mod.data(), L, c.logn), dp.aux_limbs);
        LSA_REQUIRE(M <= c.nmul && L + M <= LSA_MAX_PERIOD, ck.who + ": auxiliary basis too small for level " + std::to_string(level));
    }
    auto upload = [&](const std::vector<u64>& h) {
        u64* d = nullptr;
        LSA_HIP(hipMalloc(&d, h.size() * sizeof(u64)));
        p->owned.push_back(d);
        LSA_HIP(hipMemcpyAsync(d, h.data(), h.size() * sizeof(u64), hipMemcpyHostToDevice, s));
        LSA_HIP(hipStreamSynchronize(s));
        return d;
    };
    for (int l0 = 0; l0 < pl.n_leaves; l0 += LSA_PLC_MAX_OUT) {
        BfvPolyLaunch la;
        for (int li = l0; li < std::min(pl.n_leaves, l0 + LSA_PLC_MAX_OUT); li++) la.leaves.push_back(li);
        for (int j = 1; j < pl.m; j++)
            for (int li : la.leaves)
                if (pl.leaf_uses(pl.leaves[li], j)) {
                    la.sources.push_back(j);
                    break;
                }
        const int n_out = (int)la.leaves.size(), ns = (int)la.sources.size();
        LSA_REQUIRE(ns <= LSA_PLC_MAX_SRC, "bfv_poly: internal: a leaf launch with more than 15 powers");
        std::vector<u64> kt((size_t)n_out * std::max(ns, 1) * L, 0), st((size_t)n_out * L, 0);
        for (int o = 0; o < n_out; o++) {
            const int g = pl.leaves[la.leaves[o]];
            for (int i = 0; i < ns; i++) {
                const u64 k = pl.coef[(size_t)g * pl.m + la.sources[i]];
                if (k) leaf_constants(c, level, k, 0, &kt[((size_t)o * ns + i) * L], nullptr);
            }
            leaf_constants(c, level, 0, pl.coef[(size_t)g * pl.m], nullptr, &st[(size_t)o * L]);
        }
        la.d_k = upload(kt);
        la.d_s = upload(st);
        p->launches.push_back(la);
    }
    return p.release();
}

// ------------------------------------------------------------------------------------------------ run
void bfv_poly_run(BfvPolynomial& p, const u64* in, long long sin, u64* out, long long sout, int batch, const Key* rlk, hipStream_t s) {
    Context& c = p.c;
    const BfvPolyPlan& pl = p.plan;
    const int level = p.level, L = level + 1, m = pl.m;
    const EntryCheck ck(c, "bfv_poly", LSA_ALGO_BFV, level, 0, batch);
    LSA_REQUIRE(rlk != nullptr && rlk->data != nullptr, ck.who + ": the relinearisation key is missing");
    ck.key(*rlk, "the relinearisation key");
    if (batch <= 0) return;
    const long long N = c.n, w = 2LL * L * N;
    ck.apart(ck.output(out, sout, (size_t)w), ck.operand(in, sin, (size_t)w, "in", false), "in");
    // workspace: the computed powers and the leaves, one compact ciphertext batch each, in one pooled allocation
    int n_ct = 0;
    std::vector<int> slot_baby(m, -1), slot_giant(pl.G, -1), slot_leaf(pl.n_leaves, -1);
    for (int j = 2; j < m; j++)
        if (pl.baby[j]) slot_baby[j] = n_ct++;
    for (int g = 1; g < pl.G; g++)
        if (pl.giant[g]) slot_giant[g] = n_ct++;
    const bool lone_leaf = pl.n_pairs == 0;   // out = leaf_0: the kernel writes the caller's buffer
    if (!lone_leaf)
        for (int li = 0; li < pl.n_leaves; li++) slot_leaf[li] = n_ct++;
    // one workspace per plan: a run at another batch size gives the previous one back first instead of pooling both
    DCt wsb;
    if (n_ct) {
        const size_t words = (size_t)n_ct * batch * w;
        if (!p.pool.all.empty() && p.pool.free.find(words) == p.pool.free.end()) {
            LSA_HIP(hipStreamSynchronize(s));
            p.pool.release();
        }
        wsb = pool_alloc_words(p.pool, words);
    }
    auto at = [&](int slot) { return wsb.data() + (size_t)slot * batch * w; };
    // powers
    std::vector<const u64*> X(m, nullptr), Y(pl.G, nullptr);
    std::vector<long long> sX(m, w);
    if (m > 1) {
        X[1] = in;
        sX[1] = sin;
    }
    for (int j = 2; j < m; j++)
        if (pl.baby[j]) {
            const int a = (j + 1) / 2, b = j / 2;
            bfv_mult_relin(c, level, X[a], X[b], *rlk, at(slot_baby[j]), batch, sX[a], sX[b], w, s);
            X[j] = at(slot_baby[j]);
        }
    for (int g = 1; g < pl.G; g++)
        if (pl.giant[g]) {
            const u64 *a, *b;
            long long sa = w, sb = w;
            if (g == 1) {
                a = b = X[m / 2];
                sa = sb = sX[m / 2];
            } else {
                a = Y[(g + 1) / 2];
                b = Y[g / 2];
            }
            bfv_mult_relin(c, level, a, b, *rlk, at(slot_giant[g]), batch, sa, sb, w, s);
            Y[g] = at(slot_giant[g]);
        }
    // leaves
    std::vector<u64*> leaf(pl.n_leaves, nullptr);
    for (const BfvPolyLaunch& la : p.launches) {
        const u64* src[LSA_PLC_MAX_SRC];
        long long ss[LSA_PLC_MAX_SRC];
        u64* dst[LSA_PLC_MAX_OUT];
        long long so[LSA_PLC_MAX_OUT];
        const int ns = (int)la.sources.size(), n_out = (int)la.leaves.size();
        for (int i = 0; i < ns; i++) {
            src[i] = X[la.sources[i]];
            ss[i] = sX[la.sources[i]];
        }
        for (int o = 0; o < n_out; o++) {
            dst[o] = leaf[la.leaves[o]] = lone_leaf ? out : at(slot_leaf[la.leaves[o]]);
            so[o] = lone_leaf ? sout : w;
        }
        launch_bfv_poly_leaves(c, level, ns, src, ss, n_out, dst, so, la.d_k, la.d_s, batch, s);
    }
    if (lone_leaf) return;
    // the sum
    std::vector<const u64*> as, bs;
    const u64* addend = nullptr;
    for (int li = 0; li < pl.n_leaves; li++) {
        const int g = pl.leaves[li];
        if (g == 0) {
            addend = leaf[li];
        } else {
            as.push_back(leaf[li]);
            bs.push_back(Y[g]);
        }
    }
    const std::vector<long long> st(as.size(), w);
    const DotTerms t{(int)as.size(), as.data(), st.data(), nullptr, bs.data(), st.data(), nullptr, addend, w};
    bfv_dot(c, level, t, rlk, out, batch, sout, s);
}

// out = k * ct + c in every slot: the leaf kernel with one source and one output
void bfv_affine_const(Context& c, int level, const u64* ct, long long sct, u64 k, u64 cst, u64* out, long long sout, int batch,
                      hipStream_t s) {
    const EntryCheck ck(c, "lsa_bfv_affine_const", LSA_ALGO_BFV, level, 0, batch);
    LSA_REQUIRE(k < c.t && cst < c.t, ck.who + ": k and c must be below t");
    LSA_REQUIRE(c.n >= 2 * TPB, ck.who + ": ring degree too small for the elementwise kernels (need N >= 512)");
    LSA_REQUIRE(level + 1 <= LSA_BFV_AFFINE_MAX_LIMBS, ck.who + ": more than " + std::to_string(LSA_BFV_AFFINE_MAX_LIMBS) + " limbs");
    if (batch <= 0) return;
    const int L = level + 1;
    const size_t w = 2 * (size_t)L * c.n;
    ck.same_or_apart(ck.output(out, sout, w), ck.operand(ct, sct, w, "ct", false), "ct");
    // the 2 (level + 1) constant words travel in the kernel's arguments: nothing is allocated, copied or kept per (k, c)
    u64 k_mont[LSA_BFV_AFFINE_MAX_LIMBS], s_plain[LSA_BFV_AFFINE_MAX_LIMBS];
    leaf_constants(c, level, k, cst, k_mont, s_plain);
    launch_bfv_poly_leaves(c, level, 1, &ct, &sct, 1, &out, &sout, nullptr, nullptr, batch, s, k_mont, s_plain);
}

}  // namespace lsa
