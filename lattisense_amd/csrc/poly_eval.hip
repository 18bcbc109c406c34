// poly_eval.hip — CKKS polynomial evaluation on a ciphertext (lsa_poly_* / lsa_ckks_poly_eval): Paterson-Stockmeyer planner,
// plan, device evaluator.  DESIGN.md 4.8 explains the recursion; tests/poly_model.py restates it over the CPU oracle.
//
//   powers   P_1 = u; P_j = P_ceil(j/2) (x) P_floor(j/2): the baby powers j < 2^b and the giant powers 2^b .. 2^(k-1), only those
//            that a node or another needed power uses.  Monomial: the fused multiply+relinearise+rescale.  Chebyshev, even j:
//            2 P_a^2 - 1 (the same two launches as EvalMod's double-angle step); odd j: T_j = 2 T_a T_c - T_1 with the difference
//            formed BEFORE the rescale (tensor, relinearise, k_poly_lincomb {2, -K} over {product, u}, rescale).
//   tree     rec(c, level_out, scale_out) = rec(hi) * P_half + rec(lo) with top-down target scales, as EvalMod's binary splitting,
//            but a node of degree < 2^b whose powers sit above level_out is a LEAF: rescale(sum_j K_j P_j[rows <= level_out + 1])
//            + c_0.  All leaves of one level are one k_poly_lincomb launch and one rescale; c_0 rides in that launch as
//            round(c_0 * scale) * q_(level_out+1), which the rescale divides exactly: the words of an addition after it.
// Every constant is an integer fixed when the plan is made (lsa_poly_constants), so a CPU replay with the same integers gives
// the same words (tests/test_gpu_ckks_poly.py).
#include <algorithm>
#include <cmath>
#include <functional>

#include "layout_check.h"
#include "poly_eval.h"

namespace lsa {

namespace {

int ceil_log2(int x) {
    int r = 0;
    while ((1 << r) < x) r++;
    return r;
}

// 0: all zero, 1: only c_0, 2: a polynomial of degree >= 1
int shape_of(const std::vector<double>& v) {
    for (size_t i = 1; i < v.size(); i++)
        if (v[i] != 0.0) return 2;
    return v[0] != 0.0 ? 1 : 0;
}

struct Builder {
    PolyStructure& st;
    std::string who;

    PolyVal rec(const std::vector<double>& cf, int level_out) {
        const int len = (int)cf.size();
        int deg = len - 1;
        while (deg > 0 && cf[deg] == 0.0) deg--;
        bool leaf = deg < (1 << st.log_baby);
        for (int j = 1; leaf && j <= deg; j++)
            if (cf[j] != 0.0 && st.level_of(j) < level_out + 1) leaf = false;
        if (leaf) {
            PolyJob job;
            job.level = level_out;
            job.c0 = cf[0];
            for (int j = 1; j <= deg; j++)
                if (cf[j] != 0.0) {
                    job.terms.push_back({j, cf[j], 0});
                    st.needed[j] = 1;
                }
            st.jobs.push_back(job);
            return {PolyVal::JOB, (int)st.jobs.size() - 1};
        }
        LSA_REQUIRE(len > 2, who + ": internal: a degree-1 node above the level of its input");
        const int half = len / 2;
        std::vector<double> hi, lo(cf.begin(), cf.begin() + half);
        if (st.basis == POLY_CHEBYSHEV) {
            hi.assign(half, 0.0);
            hi[0] = cf[half];
            for (int j = 1; j < half; j++) {   // T_{half+j} = 2 T_half T_j - T_{half-j}
                hi[j] = 2 * cf[half + j];
                lo[half - j] -= cf[half + j];
            }
        } else {
            hi.assign(cf.begin() + half, cf.end());
        }
        const int sh = shape_of(hi), sl = shape_of(lo);
        if (sh == 0) return rec(lo, level_out);   // no multiplication for an all-zero upper half
        LSA_REQUIRE(st.level_of(half) >= level_out + 1, who + ": internal: a giant power below the level of its node");
        st.needed[half] = 1;
        const int idx = (int)st.nodes.size();
        st.nodes.emplace_back();
        st.nodes[idx].half = half;
        st.nodes[idx].level = level_out;
        PolyVal h;
        if (sh == 1) {   // hi_0 * P_half is one leaf term: no multiplication
            PolyJob job;
            job.level = level_out;
            job.terms.push_back({half, hi[0], 0});
            st.jobs.push_back(job);
            h = {PolyVal::JOB, (int)st.jobs.size() - 1};
            st.nodes[idx].hi_is_product = true;
        } else {
            h = rec(hi, level_out + 1);
            st.mults++;
        }
        st.nodes[idx].hi = h;
        if (sl == 1) {
            st.nodes[idx].lo_const = true;
            st.nodes[idx].c0 = lo[0];
        } else if (sl == 2) {
            const PolyVal l = rec(lo, level_out);
            st.nodes[idx].lo = l;
        }
        return {PolyVal::NODE, idx};
    }
};

std::vector<double> padded(int n_coef, const double* coef, int& k, const char* who) {
    LSA_REQUIRE(coef != nullptr && n_coef >= 1 && n_coef <= 256, std::string(who) + ": between 1 and 256 coefficients");
    k = std::max(1, ceil_log2(n_coef));
    std::vector<double> cf((size_t)1 << k, 0.0);
    for (int i = 0; i < n_coef; i++) {
        LSA_REQUIRE(std::isfinite(coef[i]), std::string(who) + ": coefficient not finite");
        cf[i] = coef[i];
    }
    LSA_REQUIRE(shape_of(cf) == 2, std::string(who) + ": a polynomial of degree 0 has no ciphertext to evaluate");
    return cf;
}

// the planner's b: fewest multiplications of this very recursion, ties to the smaller
int choose_log_baby(int basis, const std::vector<double>& cf, int k, int top_level, const char* who) {
    int best = 1, best_mults = -1;
    for (int b = 1; b <= std::min(4, k); b++) {
        const int mu = poly_structure(basis, cf, b, top_level, who).mults;
        if (best_mults < 0 || mu < best_mults) {
            best = b;
            best_mults = mu;
        }
    }
    return best;
}

u64 to_mont(long long k, u64 q) {
    long long r = k % (long long)q;
    if (r < 0) r += (long long)q;
    return (u64)((((unsigned __int128)(u64)r) << 64) % q);
}

u64* upload_words(Context& c, const std::vector<u64>& h, std::vector<u64*>& owned, hipStream_t s) {
    u64* d = nullptr;
    LSA_HIP(hipMalloc(&d, h.size() * sizeof(u64)));
    owned.push_back(d);
    LSA_HIP(hipMemcpyAsync(d, h.data(), h.size() * sizeof(u64), hipMemcpyHostToDevice, s));
    LSA_HIP(hipStreamSynchronize(s));
    return d;
}

}  // namespace

int PolyStructure::level_of(int j) const { return top_level - ceil_log2(j); }

PolyStructure poly_structure(int basis, const std::vector<double>& coef, int log_baby, int top_level, const char* who) {
    PolyStructure st;
    st.basis = basis;
    st.k = ceil_log2((int)coef.size());
    st.log_baby = log_baby;
    st.top_level = top_level;
    st.needed.assign(coef.size(), 0);
    Builder b{st, who};
    st.root = b.rec(coef, top_level - st.k);
    for (int j = (int)coef.size() - 1; j >= 2; j--)
        if (st.needed[j]) st.needed[(j + 1) / 2] = st.needed[j / 2] = 1;
    for (size_t j = 2; j < coef.size(); j++) st.mults += st.needed[j] ? 1 : 0;
    // leaf launches: the jobs of one level, in job order, cut where a launch would pass 8 outputs or 15 sources
    std::map<int, std::vector<int>> by_level;
    for (size_t i = 0; i < st.jobs.size(); i++) by_level[st.jobs[i].level].push_back((int)i);
    for (auto& kv : by_level) {
        PolyGroup g;
        g.level = kv.first;
        for (int ji : kv.second) {
            std::vector<int> src = g.sources;
            for (auto& t : st.jobs[ji].terms)
                if (!std::count(src.begin(), src.end(), t.j)) src.push_back(t.j);
            if (!g.jobs.empty() && ((int)g.jobs.size() == LSA_PLC_MAX_OUT || (int)src.size() > LSA_PLC_MAX_SRC)) {
                st.groups.push_back(g);
                g.jobs.clear();
                src.clear();
                for (auto& t : st.jobs[ji].terms) src.push_back(t.j);
            }
            g.sources = src;
            g.jobs.push_back(ji);
        }
        st.groups.push_back(g);
    }
    for (size_t gi = 0; gi < st.groups.size(); gi++) {
        PolyGroup& g = st.groups[gi];
        std::sort(g.sources.begin(), g.sources.end());
        LSA_REQUIRE((int)g.sources.size() <= LSA_PLC_MAX_SRC, std::string(who) + ": internal: a leaf with more than 15 powers");
        for (size_t i = 0; i < g.jobs.size(); i++) {
            st.jobs[g.jobs[i]].group = (int)gi;
            st.jobs[g.jobs[i]].slot = (int)i;
        }
    }
    return st;
}

void poly_plan(int basis, int n_coef, const double* coef, int log_baby, int level_in, bool interval, int* depth, int* chosen,
               int* mults, int* leaves, int* launches) {
    const char* who = "poly";
    LSA_REQUIRE(basis == POLY_CHEBYSHEV || basis == POLY_MONOMIAL, "poly: basis must be 0 (Chebyshev) or 1 (monomial)");
    int k = 0;
    const std::vector<double> cf = padded(n_coef, coef, k, who);
    LSA_REQUIRE(log_baby >= 0 && log_baby <= 4, "poly: log_baby outside 0..4");
    const int d = k + (interval ? 1 : 0);
    LSA_REQUIRE(level_in - d >= 0, "poly: the polynomial needs " + std::to_string(d) + " levels, the input has " + std::to_string(level_in));
    const int top = level_in - (interval ? 1 : 0);
    const int b = log_baby ? std::min(log_baby, k) : choose_log_baby(basis, cf, k, top, who);
    const PolyStructure st = poly_structure(basis, cf, b, top, who);
    if (depth) *depth = d;
    if (chosen) *chosen = b;
    if (mults) *mults = st.mults;
    if (leaves) *leaves = (int)st.jobs.size();
    if (launches) *launches = (int)st.groups.size();
}

// ------------------------------------------------------------------------------------------------ plan
Polynomial::~Polynomial() {
    (void)hipSetDevice(c.device);
    (void)hipDeviceSynchronize();
    for (u64* p : owned) (void)hipFree(p);
    pool.release();
}

Polynomial* poly_create(Context& c, int basis, int n_coef, const double* coef, double a, double b, int level_in, double scale_in,
                        double scale_out, int log_baby, hipStream_t s) {
    const char* who = "poly";
    LSA_REQUIRE(c.algo == LSA_ALGO_CKKS, "poly: CKKS context required");
    LSA_REQUIRE(level_in >= 0 && level_in < c.nq, "poly: level out of range");
    LSA_REQUIRE(std::isfinite(a) && std::isfinite(b) && a < b, "poly: the interval needs a < b");
    LSA_REQUIRE(scale_in > 0 && scale_out >= 0 && std::isfinite(scale_in) && std::isfinite(scale_out), "poly: scales must be positive");
    auto p = std::make_unique<Polynomial>(c);
    p->interval = !(a == -1.0 && b == 1.0);
    int chosen = 0;
    poly_plan(basis, n_coef, coef, log_baby, level_in, p->interval, &p->depth, &chosen, nullptr, nullptr, nullptr);
    int k = 0;
    const std::vector<double> cf = padded(n_coef, coef, k, who);
    const int top = level_in - (p->interval ? 1 : 0);
    p->st = poly_structure(basis, cf, chosen, top, who);
    PolyStructure& st = p->st;
    p->level_in = level_in;
    p->level_out = level_in - p->depth;
    p->scale_in = scale_in;
    p->scale_out = scale_out > 0 ? scale_out : (double)c.T.mod[p->level_out + 1];
    auto q = [&](int level) { return (double)c.T.mod[level]; };
    // u = (2x - a - b) / (b - a): one constant multiplication at the scale of the top prime, rescale, one constant addition
    p->u_scale = scale_in;
    if (p->interval) {
        const double cs = q(level_in);
        p->k_mul = round_even(2.0 / (b - a) * cs, who);
        p->u_scale = scale_in * cs / q(level_in);
        p->k_add = round_even(-(a + b) / (b - a) * p->u_scale, who);
        p->constants.push_back(p->k_mul);
        p->constants.push_back(p->k_add);
    }
    // powers: levels and scales
    std::vector<double> ps(cf.size(), 0.0);
    ps[1] = p->u_scale;
    for (int j = 2; j < (int)cf.size(); j++) {
        if (!st.needed[j]) continue;
        PolyPower pw;
        pw.j = j;
        pw.a = (j + 1) / 2;
        pw.c = j / 2;
        const int lvl = std::min(st.level_of(pw.a), st.level_of(pw.c));
        pw.level = lvl - 1;
        LSA_REQUIRE(pw.level == st.level_of(j) && pw.level >= 0, "poly: internal: power level");
        pw.scale = ps[pw.a] * ps[pw.c] / q(lvl);
        ps[j] = pw.scale;
        if (basis == POLY_CHEBYSHEV) {
            // even: 2 P_a^2 - 1; odd: 2 (P_a P_c) - K u with K u at the product's scale s_a s_c
            pw.k = (j & 1) ? round_even(ps[pw.a] * ps[pw.c] / ps[1], who) : round_even(-1.0 * pw.scale, who);
            p->constants.push_back(pw.k);
            if (j & 1) {
                const int R = lvl + 1;
                std::vector<u64> tab(2 * (size_t)R);
                for (int r = 0; r < R; r++) {
                    tab[r] = to_mont(2, c.T.mod[r]);
                    tab[R + r] = to_mont(-pw.k, c.T.mod[r]);
                }
                p->odd_tables.push_back(upload_words(c, tab, p->owned, s));
            }
        }
        p->powers.push_back(pw);
    }
    // target scales, top down
    std::function<void(const PolyVal&, double)> assign = [&](const PolyVal& v, double sc) {
        if (v.kind == PolyVal::JOB) {
            st.jobs[v.idx].scale = sc;
        } else if (v.kind == PolyVal::NODE) {
            PolyNode& n = st.nodes[v.idx];
            n.scale = sc;
            assign(n.hi, n.hi_is_product ? sc : sc * q(n.level + 1) / ps[n.half]);
            assign(n.lo, sc);
        }
    };
    assign(st.root, p->scale_out);
    for (PolyJob& job : st.jobs) {
        for (PolyTerm& t : job.terms) {
            t.k = round_even(t.coef * (job.scale * q(job.level + 1) / ps[t.j]), who);
            p->constants.push_back(t.k);
        }
        if (job.c0 != 0.0) {
            job.k0 = round_even(job.c0 * job.scale, who);
            p->constants.push_back(job.k0);
        }
    }
    for (PolyNode& n : st.nodes)
        if (n.lo_const) {
            n.k0 = round_even(n.c0 * n.scale, who);
            p->constants.push_back(n.k0);
        }
    // the launches' constant tables
    for (PolyGroup& g : st.groups) {
        const int R = g.level + 2, G = (int)g.jobs.size(), ns = (int)g.sources.size();
        std::vector<u64> kt((size_t)G * ns * R, 0), at((size_t)G * R, 0);
        bool any_a = false;
        for (int gi = 0; gi < G; gi++) {
            const PolyJob& job = st.jobs[g.jobs[gi]];
            for (const PolyTerm& t : job.terms) {
                const int si = (int)(std::find(g.sources.begin(), g.sources.end(), t.j) - g.sources.begin());
                for (int r = 0; r < R; r++) kt[((size_t)gi * ns + si) * R + r] = to_mont(t.k, c.T.mod[r]);
            }
            if (job.k0 != 0) {
                any_a = true;
                const u64 ql = c.T.mod[g.level + 1];
                for (int r = 0; r <= g.level; r++) {   // k0 * q_(level+1): zero at that prime itself
                    const u64 qr = c.T.mod[r];
                    long long kr = job.k0 % (long long)qr;
                    if (kr < 0) kr += (long long)qr;
                    at[(size_t)gi * R + r] = (u64)((unsigned __int128)(u64)kr * (ql % qr) % qr);
                }
            }
        }
        g.d_k = upload_words(c, kt, p->owned, s);
        g.d_a = any_a ? upload_words(c, at, p->owned, s) : nullptr;
    }
    return p.release();
}

// ------------------------------------------------------------------------------------------------ run
void poly_run(Polynomial& p, const u64* in, long long sin, u64* out, long long sout, int batch, const Key& rlk, hipStream_t s) {
    if (batch <= 0) return;
    Context& c = p.c;
    const long long N = c.n;
    const PolyStructure& st = p.st;
    LSA_REQUIRE(rlk.level >= p.level_in, "poly: the relinearisation key is below the input level");
    LSA_REQUIRE(in && out, "poly: null argument");
    LSA_REQUIRE(sin >= 2LL * (p.level_in + 1) * N && sout >= 2LL * (p.level_out + 1) * N, "poly: batch stride shorter than a ciphertext");
    // the row copies that gather `in` and store `out` move 16 bytes per lane at base + item * stride
    LSA_REQUIRE(layout::aligned16(layout::span_of(in, sin, 0)) && layout::aligned16(layout::span_of(out, sout, 0)),
                "poly: in and out must be 16-byte aligned with even batch strides");
    LSA_REQUIRE(layout::apart(out, sout, 2 * (size_t)(p.level_out + 1) * N, in, sin, 2 * (size_t)(p.level_in + 1) * N, batch),
                "poly: out overlaps in");
    static const GaloisKeys no_glk;
    CtEval ev(c, p.pool, s, batch, rlk, no_glk, "poly");
    const int m = batch;
    DCt u;
    if (sin == ev.stride(p.level_in)) {
        u = ev.wrap(const_cast<u64*>(in), p.level_in, p.scale_in);   // read only
    } else {
        u = ev.alloc(p.level_in, p.scale_in);
        std::vector<int> rows(2 * (p.level_in + 1));
        for (size_t i = 0; i < rows.size(); i++) rows[i] = (int)i;
        launch_copy_rows(c, in, sin, u.data(), ev.stride(p.level_in), (int)rows.size(), rows.data(), batch, s);
    }
    if (p.interval) u = ev.mul_int_add_int(ev.rescale(ev.mul_int_raw(u, p.k_mul, p.scale_in * ev.q(p.level_in))), 1, p.k_add);
    // powers
    std::vector<DCt> P((size_t)1 << st.k);
    P[1] = u;
    size_t odd = 0;
    for (const PolyPower& pw : p.powers) {
        const DCt &A = P[pw.a], &C = P[pw.c];
        if (st.basis == POLY_MONOMIAL) {
            P[pw.j] = ev.mul(A, C);
        } else if (!(pw.j & 1)) {
            P[pw.j] = ev.mul_int_add_int(ev.mul(A, A), 2, pw.k);
        } else {
            const int lam = std::min(A.level, C.level), R = lam + 1;
            const long long sd = 3LL * R * N;
            DCt d3 = ev.alloc_words((size_t)m * sd);
            launch_tensor(c, A.data(), C.data(), d3.data(), m, ev.stride(A.level), ev.stride(C.level), sd, R, ev.rm2(lam), s, A.level + 1,
                          C.level + 1);
            DCt prod = ev.alloc(lam, A.scale * C.scale);
            ckks_relin(c, lam, d3.data(), rlk, prod.data(), m, sd, ev.stride(lam), s);
            const u64* src[2] = {prod.data(), u.data()};
            const long long ss[2] = {ev.stride(lam), ev.stride(u.level)};
            const int rpp[2] = {R, u.level + 1};
            DCt t = ev.alloc(lam, prod.scale);
            launch_poly_lincomb(c, 2, src, ss, rpp, 1, p.odd_tables[odd++], nullptr, t.data(), R, m, s);
            P[pw.j] = ev.rescale(t);
        }
        P[pw.j].scale = pw.scale;
        LSA_REQUIRE(P[pw.j].level == pw.level, "poly: internal: power level at run time");
    }
    // leaves: one launch and one rescale per group
    std::vector<DCt> leaf(st.jobs.size());
    for (const PolyGroup& g : st.groups) {
        const int R = g.level + 2, G = (int)g.jobs.size(), ns = (int)g.sources.size();
        const u64* src[LSA_PLC_MAX_SRC];
        long long ss[LSA_PLC_MAX_SRC];
        int rpp[LSA_PLC_MAX_SRC];
        for (int i = 0; i < ns; i++) {
            const DCt& pj = P[g.sources[i]];
            src[i] = pj.data();
            ss[i] = ev.stride(pj.level);
            rpp[i] = pj.level + 1;
        }
        DCt sum = ev.alloc_words((size_t)G * m * ev.stride(g.level + 1));
        launch_poly_lincomb(c, ns, src, ss, rpp, G, g.d_k, g.d_a, sum.data(), R, m, s);
        DCt res = ev.alloc_words((size_t)G * m * ev.stride(g.level));
        ckks_rescale(c, g.level + 1, 2, sum.data(), res.data(), G * m, ev.stride(g.level + 1), ev.stride(g.level), s);
        for (int gi = 0; gi < G; gi++) {
            DCt o = res;
            o.level = g.level;
            o.scale = st.jobs[g.jobs[gi]].scale;
            o.off = (size_t)gi * m * ev.stride(g.level);
            leaf[g.jobs[gi]] = o;
        }
    }
    // the tree
    std::function<DCt(const PolyVal&)> eval = [&](const PolyVal& v) -> DCt {
        if (v.kind == PolyVal::JOB) return leaf[v.idx];
        const PolyNode& n = st.nodes[v.idx];
        DCt prod = eval(n.hi);
        if (!n.hi_is_product) prod = ev.mul(prod, P[n.half]);
        prod.scale = n.scale;
        if (n.lo_const) prod = ev.mul_int_add_int(prod, 1, n.k0);
        if (n.lo.kind != PolyVal::NONE) return ev.add(prod, eval(n.lo));
        return prod;
    };
    DCt y = eval(st.root);
    LSA_REQUIRE(y.level == p.level_out, "poly: internal: result level");
    std::vector<int> all(2 * (y.level + 1));
    for (size_t i = 0; i < all.size(); i++) all[i] = (int)i;
    launch_copy_rows(c, y.data(), ev.stride(y.level), out, sout, (int)all.size(), all.data(), batch, s);
}

}  // namespace lsa
