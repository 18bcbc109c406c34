// bootstrap.hip — CKKS bootstrapping as a program of the device operators (the `bootstrap` node of a task graph).
//
// Reference: mega_ag_runners/gpu/mega_ag_executors_gpu.cu:410-426 hands the ciphertext to HEonGPU's
// regular_bootstrapping_v2 (absent submodule); parameters mega_ag_runners/gpu/gpu_wrapper.cu:86-117 and
// frontend/custom_task.py:383-468; the rotations a caller generates Galois keys for: frontend/bootstrap_params.py:104-263.
// The algorithm is the one restated (and explained) in oracle/ckks_bootstrap.py, which is also its oracle:
//   scale-up by an integer -> (switch to the sparse secret) -> ModRaise -> (switch back) -> CoeffsToSlots (merged radix-2
//   layers of the inverse special FFT, baby-step / giant-step with the planner's split) -> conjugate split into real and
//   imaginary coefficients -> EvalMod (Chebyshev interpolant of cos on [-1,1] by binary splitting, double-angle steps) ->
//   recombine -> SlotsToCoeffs.
// Only floating-point CONSTANTS are computed here (the encoded diagonals, the Chebyshev coefficients); every operation on
// ciphertexts is one of the integer operators of ops.hip / kernels.hip, so a replay of the same program with the same
// constants on the CPU oracle gives identical residues (tests/test_gpu_bootstrap.py).
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <functional>
#include <map>
#include <memory>

#include "poly_eval.h"

namespace lsa {

namespace {

const double kPi = 3.14159265358979323846;

// one radix-2 layer of the special FFT (forward: slots <- coefficients) or of its inverse, as three diagonals
Diags layer_diagonals(int n, int length, bool inverse, const std::vector<int>& rg) {
    const long long m = 4LL * n;
    const int lenh = length / 2;
    const long long lenq = 4LL * length;
    std::vector<cplx> d0(n), dp(n), dm(n);
    auto root = [&](long long idx) { return std::polar(1.0, 2.0 * kPi * (double)idx / (double)m); };
    for (int t = 0; t < n; t++) {
        const int j = t % length;
        if (j < lenh) {
            d0[t] = 1.0;
            dp[t] = inverse ? cplx(1.0) : root((rg[j] % lenq) * (m / lenq));
        } else {
            const int jj = j - lenh;
            if (inverse) {
                const cplx w = root((lenq - (rg[jj] % lenq)) * (m / lenq));
                d0[t] = -w;
                dm[t] = w;
            } else {
                d0[t] = -root((rg[jj] % lenq) * (m / lenq));
                dm[t] = 1.0;
            }
        }
    }
    Diags out;
    out[0] = d0;
    const int kp = lenh % n, km = ((-lenh) % n + n) % n;
    if (kp == km) {   // the widest layer: +n/2 and -n/2 are the same rotation
        for (int t = 0; t < n; t++) dp[t] += dm[t];
        out[kp] = dp;
    } else {
        out[kp] = dp;
        out[km] = dm;
    }
    return out;
}

// diagonals of (second o first)
Diags compose(const Diags& first, const Diags& second, int n) {
    Diags out;
    for (auto& a : second)
        for (auto& b : first) {
            const int k = (a.first + b.first) % n;
            auto& dst = out[k];
            if (dst.empty()) dst.assign(n, cplx(0.0));
            for (int t = 0; t < n; t++) dst[t] += a.second[t] * b.second[(t + a.first) % n];
        }
    for (auto it = out.begin(); it != out.end();) {
        double mx = 0;
        for (auto& v : it->second) mx = std::max(mx, std::abs(v));
        it = mx > 1e-300 ? std::next(it) : out.erase(it);
    }
    return out;
}

// `depth` merged groups in application order, grouped like frontend/bootstrap_params.py:104-119
std::vector<Diags> merged_matrices(int n, int depth, bool inverse) {
    int log_n = 0;
    while ((1 << log_n) < n) log_n++;
    LSA_REQUIRE(depth >= 1 && depth <= log_n, "bootstrap: linear-transform depth out of range");
    const std::vector<int> rg = rot_group(n);
    std::vector<int> lengths;
    if (inverse)
        for (int l = log_n; l >= 1; l--) lengths.push_back(1 << l);
    else
        for (int l = 1; l <= log_n; l++) lengths.push_back(1 << l);
    std::vector<int> sizes;
    int left = log_n;
    for (int i = 0; i < depth; i++) {
        const int s = (left + (depth - i) - 1) / (depth - i);
        sizes.push_back(s);
        left -= s;
    }
    if (!inverse) std::reverse(sizes.begin(), sizes.end());
    std::vector<Diags> mats;
    size_t pos = 0;
    for (int s : sizes) {
        Diags m;
        for (int i = 0; i < s; i++) {
            Diags lay = layer_diagonals(n, lengths[pos + i], inverse, rg);
            m = i == 0 ? lay : compose(m, lay, n);
        }
        mats.push_back(std::move(m));
        pos += s;
    }
    return mats;
}

// group sizes of `depth` merged matrices over log_n layers (frontend/bootstrap_params.py:104-119)
std::vector<int> group_sizes(int log_n, int depth, bool inverse) {
    std::vector<int> sizes;
    int left = log_n;
    for (int i = 0; i < depth; i++) {
        const int s = (left + (depth - i) - 1) / (depth - i);
        sizes.push_back(s);
        left -= s;
    }
    if (!inverse) std::reverse(sizes.begin(), sizes.end());
    return sizes;
}

std::vector<cplx> tiled(const std::vector<cplx>& v, int n) {
    std::vector<cplx> out(n);
    for (int t = 0; t < n; t++) out[t] = v[t % v.size()];
    return out;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ plan
struct Bootstrap {
    Context& c;
    int cts_depth, stc_depth, K, r, top_level;
    double mr, in_scale, out_scale;
    int log_slots = 0;                   // 0 / logN-1: dense packing; less: sparse (subring of X^gap)
    bool sparse = false;
    std::vector<BtMatrix> cts, stc;
    BtMatrix p1, p2;                     // sparse: last CoeffsToSlots matrix split for x and conj(x), real | imaginary halves
    std::vector<double> cheb;            // 2^cheb_depth Chebyshev coefficients of cos(2 pi (K x - 1/4) / 2^r) on [-1,1]
    int sine_deg = 30, arcsine_deg = 0;  // reference: btp_eval_mod_sine_deg / _arcsine_deg (gpu_wrapper.cu:100-103)
    int cheb_depth = 5, asin_depth = 0;  // levels of the cosine interpolant (ceil log2(sine_deg + 1)) and of the arcsine polynomial
    std::vector<double> asin_coef;       // arcsine Taylor coefficients in the monomial basis, padded to 2^asin_depth (empty: none)
    // baby-step / giant-step matrices keep their sums over Q u P and divide by P once per giant step + once at the end
    // (Lattigo's MultiplyByDiagMatrixBSGS); LSA_BT_DOUBLE_HOIST=0 at plan creation: one division per rotation (A/B)
    bool double_hoist = true;
    int evalmod_depth() const { return cheb_depth + r + asin_depth; }
    u64* mono[2] = {nullptr, nullptr};   // NTT of +X^(N/2) and -X^(N/2), [top_level+1][N]
    std::vector<u64> galois;             // Galois elements a run needs (rotations + conjugation)
    long long mul_c = 1;                 // integer scale-up factor
    double d1 = 0, natural_scale = 0;
    std::vector<u64*> owned;
    // temporaries of a run, kept across runs (hipMalloc / hipFree of GiB-sized buffers cost more than the kernels); a plan
    // belongs to one context and is run on one in-order stream at a time, so reuse is ordered
    DevPool pool;

    explicit Bootstrap(Context& ctx) : c(ctx) {}
    ~Bootstrap() {
        (void)hipSetDevice(c.device);
        (void)hipDeviceSynchronize();
        for (u64* p : owned) (void)hipFree(p);
        pool.release();
    }

    u64* upload_plain(const std::vector<double>& coef, double scale, int level, hipStream_t s) {
        return lt_upload_plain(c, coef, scale, level, s, false, owned, "bootstrap");
    }

    double evalmod_out_scale(int level_in) const {
        int level = level_in - cheb_depth;
        double sc = (double)c.T.mod[level + 1];
        for (int i = 0; i < r; i++) {
            sc = sc * sc / (double)c.T.mod[level];
            level--;
        }
        if (asin_depth) sc = (double)c.T.mod[level - asin_depth + 1];   // a polynomial evaluation ends at the scale of the prime above its result
        return sc;
    }

    void build(hipStream_t s) {
        const int n = c.n / 2;
        top_level = c.nq - 1;
        double_hoist = sw::bt_double_hoist(double_hoist);
        LSA_REQUIRE(c.algo == LSA_ALGO_CKKS, "bootstrap: CKKS only");
        LSA_REQUIRE(sine_deg >= 1 && sine_deg <= 63, "bootstrap: sine degree outside 1..63");
        LSA_REQUIRE(arcsine_deg >= 0 && arcsine_deg <= 15 && (arcsine_deg == 0 || (arcsine_deg & 1)), "bootstrap: arcsine degree must be odd and at most 15");
        cheb_depth = 1;
        while ((1 << cheb_depth) < sine_deg + 1) cheb_depth++;
        asin_depth = 0;
        if (arcsine_deg > 0) {
            asin_depth = 1;
            while ((1 << asin_depth) < arcsine_deg + 1) asin_depth++;
        }
        LSA_REQUIRE(top_level - cts_depth - evalmod_depth() - stc_depth >= 0, "bootstrap: modulus chain too short");
        const std::vector<int> rg = rot_group(n);
        const double q0 = (double)c.T.mod[0];
        mul_c = std::max<long long>(1, round_even(q0 / (mr * in_scale), "bootstrap"));
        d1 = in_scale * (double)mul_c;
        const int evalmod_level = top_level - cts_depth;
        const int stc_level = evalmod_level - evalmod_depth();
        natural_scale = evalmod_out_scale(evalmod_level) * 2.0 * kPi * d1 / q0;
        int logn_ring = 0;
        while ((1 << logn_ring) < c.n) logn_ring++;
        sparse = log_slots > 0 && log_slots < logn_ring - 1;
        const int ns = sparse ? 1 << log_slots : n;
        std::vector<Diags> mc = merged_matrices(ns, cts_depth, true), ms;
        Diags dp1, dp2;
        if (!sparse) {
            ms = merged_matrices(n, stc_depth, false);
            const double g = 1.0 / (2.0 * (double)n * (double)K);   // 1/n (inverse FFT), 1/2 (t + conj t), 1/K (unit interval)
            for (auto& kv : mc[0])
                for (auto& v : kv.second) v *= g;
        } else {
            // see oracle/ckks_bootstrap.py SparseBootstrapper: last CtS matrix M as y = P1 x + P2 conj(x) on period 2*ns
            // (first half Re(Mx), second half Im(Mx)); StC's first matrix preceded by the repack R = {0, ns}
            const int gap = n / ns;
            Diags last = mc.back();
            mc.pop_back();
            for (auto& kv : last) {
                std::vector<cplx> a(2 * ns), b(2 * ns);
                for (int t = 0; t < ns; t++) {
                    const cplx d = kv.second[t];
                    a[t] = 0.5 * d;
                    a[t + ns] = cplx(0.0, -0.5) * d;
                    b[t] = 0.5 * std::conj(d);
                    b[t + ns] = cplx(0.0, 0.5) * std::conj(d);
                }
                dp1[kv.first] = a;
                dp2[kv.first] = b;
            }
            const double g = 1.0 / ((double)ns * (double)gap * (double)K);   // 1/slots, 1/gap (SubSum), 1/K
            if (!mc.empty()) {
                for (auto& kv : mc[0])
                    for (auto& v : kv.second) v *= g;
            } else {
                for (auto* dd : {&dp1, &dp2})
                    for (auto& kv : *dd)
                        for (auto& v : kv.second) v *= g;
            }
            const std::vector<int> rgs = rot_group(ns);
            const std::vector<int> sizes = group_sizes(log_slots, stc_depth, false);
            Diags m;
            {
                std::vector<cplx> e(2 * ns), f(2 * ns);
                for (int t = 0; t < ns; t++) {
                    e[t] = 1.0;
                    e[t + ns] = cplx(0.0, 1.0);
                    f[t] = cplx(0.0, 1.0);
                    f[t + ns] = 1.0;
                }
                m[0] = e;
                m[ns] = f;
            }
            int pos = 0;
            for (size_t gi = 0; gi < sizes.size(); gi++) {
                bool have = gi == 0;
                for (int i = 0; i < sizes[gi]; i++) {
                    Diags lay = layer_diagonals(ns, 1 << (pos + i + 1), false, rgs);
                    if (gi == 0) {
                        for (auto& kv : lay) kv.second = tiled(kv.second, 2 * ns);
                        m = compose(m, lay, 2 * ns);
                    } else {
                        m = have ? compose(m, lay, ns) : lay;
                        have = true;
                    }
                }
                ms.push_back(m);
                m.clear();
                pos += sizes[gi];
            }
        }
        if (out_scale > 0) {
            const double kappa = out_scale / natural_scale;
            for (auto& kv : ms[0])
                for (auto& v : kv.second) v *= kappa;
            natural_scale = out_scale;
        }
        std::map<u64, bool> gal;
        // one matrix -> plaintexts (diagonals of period `period`, tiled over the N/2 slots) + the rotations it needs
        auto make_one = [&](const Diags& mat, int level, int period) {
            return lt_make_matrix(c, mat, level, period, (double)c.T.mod[level], 2.0, double_hoist, s, owned, gal, "bootstrap");
        };
        for (size_t i = 0; i < mc.size(); i++) cts.push_back(make_one(mc[i], top_level - (int)i, ns));
        if (sparse) {
            p1 = make_one(dp1, top_level - (int)mc.size(), 2 * ns);
            p2 = make_one(dp2, top_level - (int)mc.size(), 2 * ns);
            for (int i = log_slots; i < logn_ring - 1; i++) gal[galois_of_rotation(1 << i, c.n)] = true;   // SubSum: 2^i < N/2
        }
        for (size_t i = 0; i < ms.size(); i++) stc.push_back(make_one(ms[i], stc_level - (int)i, sparse && i == 0 ? 2 * ns : ns));
        gal[2ULL * c.n - 1] = true;
        for (auto& kv : gal) galois.push_back(kv.first);
        // arcsine correction (btp_eval_mod_arcsine_deg > 0): after the double-angle steps y = sin(2 pi v); arcsin(y) = 2 pi eps exactly
        // where sin only approximates it -- Taylor series sum_k C(2k,k) / (4^k (2k+1)) y^(2k+1) up to the requested degree
        asin_coef.clear();
        if (asin_depth) {
            asin_coef.assign((size_t)1 << asin_depth, 0.0);
            double binom = 1.0, pow4 = 1.0;   // C(2k, k), 4^k
            for (int k = 0; 2 * k + 1 <= arcsine_deg; k++) {
                if (k > 0) {
                    binom = binom * (double)(2 * k) * (double)(2 * k - 1) / ((double)k * (double)k);
                    pow4 *= 4.0;
                }
                asin_coef[(size_t)(2 * k + 1)] = binom / (pow4 * (double)(2 * k + 1));
            }
        }
        // Chebyshev interpolant (first-kind nodes) of cos(2 pi (K x - 1/4) / 2^r), 2^cheb_depth coefficients
        const int M = 1 << cheb_depth;
        cheb.assign(M, 0.0);
        std::vector<double> f(M), th(M);
        for (int j = 0; j < M; j++) {
            th[j] = kPi * (j + 0.5) / M;
            f[j] = std::cos(2.0 * kPi * ((double)K * std::cos(th[j]) - 0.25) / (double)(1 << r));
        }
        for (int k = 0; k < M; k++) {
            double acc = 0;
            for (int j = 0; j < M; j++) acc += f[j] * std::cos(k * th[j]);
            cheb[k] = acc * (k == 0 ? 1.0 : 2.0) / M;
        }
        // monomials +-X^(N/2)  (times +-i on the slots)
        for (int sg = 0; sg < 2; sg++) {
            std::vector<double> xn2((size_t)c.n, 0.0);
            xn2[c.n / 2] = sg == 0 ? 1.0 : -1.0;
            mono[sg] = upload_plain(xn2, 1.0, top_level, s);
        }
    }
};

// ------------------------------------------------------------------------------------------------ device evaluator
namespace {

// the linear transforms and the ciphertext bookkeeping come from LtEval (linear_transform.h), the multiply and the constant
// helpers from CtEval (poly_eval.h, shared with the polynomial operator); what is added here is EvalMod
struct Eval : CtEval {
    Bootstrap& bt;

    Eval(Context& c_, Bootstrap& b, hipStream_t s_, int m_, const Key& rlk_, const GaloisKeys& g)
        : CtEval(c_, b.pool, s_, m_, rlk_, g, "bootstrap"), bt(b) {}
    DCt conj(const DCt& a) {
        const u64 e = 2ULL * c.n - 1;
        DCt o = alloc(a.level, a.scale);
        ckks_rotate(c, a.level, a.data(), e, gkey(e), o.data(), m, stride(a.level), stride(a.level), s);
        return o;
    }
    // every polynomial times a shared plaintext (stride 0 over the batch)
    DCt mul_plain(const DCt& a, const u64* pt, double pt_scale) {
        DCt o = alloc(a.level, a.scale * pt_scale);
        const int L = a.level + 1;
        for (int p = 0; p < 2; p++)
            launch_elementwise(c, EW_MUL, a.data() + (size_t)p * L * N, pt, o.data() + (size_t)p * L * N, m, stride(a.level), 0,
                               stride(a.level), L, rm2(a.level), s);
        return o;
    }
    DCt mul_by_i(const DCt& a, int sign) { return mul_plain_keep_scale(a, bt.mono[sign > 0 ? 0 : 1]); }
    DCt mul_plain_keep_scale(const DCt& a, const u64* pt) {
        DCt o = mul_plain(a, pt, 1.0);
        o.scale = a.scale;
        return o;
    }

    DCt eval_chebyshev(const DCt& u, const std::vector<double>& coeffs) {
        int k = 0;
        while ((1u << k) < coeffs.size()) k++;
        std::map<int, DCt> powers;
        powers[1] = u;
        for (int j = 1; j < k; j++) {   // T_{2^j} = 2 T_{2^(j-1)}^2 - 1
            const DCt& p = powers[1 << (j - 1)];
            powers[1 << j] = mul_int_add_const(mul(p, p), 2, -1.0);
        }
        std::function<DCt(const std::vector<double>&, int, double)> rec = [&](const std::vector<double>& cf, int level_out,
                                                                              double scale_out) -> DCt {
            if (cf.size() == 2) {
                const double cs = scale_out * q(level_out + 1) / u.scale;
                DCt rr = rescale(mul_const(u, cf[1], cs, level_out + 1));
                rr.scale = scale_out;
                return add_const(rr, cf[0]);
            }
            const size_t half = cf.size() / 2;
            std::vector<double> hi(half, 0.0), lo(cf.begin(), cf.begin() + half);
            hi[0] = cf[half];
            for (size_t j = 1; j < half; j++) {   // T_{half+j} = 2 T_half T_j - T_{half-j}
                hi[j] = 2 * cf[half + j];
                lo[half - j] -= cf[half + j];
            }
            const DCt& th = powers[(int)half];   // at or above level_out + 1: mul() reads its leading rows
            DCt h = rec(hi, level_out + 1, scale_out * q(level_out + 1) / th.scale);
            DCt prod = mul(h, th);
            prod.scale = scale_out;
            return add(prod, rec(lo, level_out, scale_out));
        };
        const int level_out = u.level - k;
        return rec(coeffs, level_out, q(level_out + 1));
    }

    // sum_k coeffs[k] u^k, len(coeffs) a power of two: the same binary splitting in the monomial basis (p = hi * u^half + lo)
    DCt eval_monomial(const DCt& u, const std::vector<double>& coeffs) {
        int k = 0;
        while ((1u << k) < coeffs.size()) k++;
        std::map<int, DCt> powers;
        powers[1] = u;
        for (int j = 1; j < k; j++) {
            const DCt& p = powers[1 << (j - 1)];
            powers[1 << j] = mul(p, p);
        }
        std::function<DCt(const std::vector<double>&, int, double)> rec = [&](const std::vector<double>& cf, int level_out,
                                                                              double scale_out) -> DCt {
            if (cf.size() == 2) {
                const double cs = scale_out * q(level_out + 1) / u.scale;
                DCt rr = rescale(mul_const(u, cf[1], cs, level_out + 1));
                rr.scale = scale_out;
                return add_const(rr, cf[0]);
            }
            const size_t half = cf.size() / 2;
            std::vector<double> hi(cf.begin() + half, cf.end()), lo(cf.begin(), cf.begin() + half);
            const DCt& th = powers[(int)half];   // at or above level_out + 1: mul() reads its leading rows
            DCt h = rec(hi, level_out + 1, scale_out * q(level_out + 1) / th.scale);
            DCt prod = mul(h, th);
            prod.scale = scale_out;
            return add(prod, rec(lo, level_out, scale_out));
        };
        const int level_out = u.level - k;
        return rec(coeffs, level_out, q(level_out + 1));
    }

    DCt eval_mod(const DCt& u) {
        DCt y = eval_chebyshev(u, bt.cheb);
        for (int i = 0; i < bt.r; i++) y = mul_int_add_const(mul(y, y), 2, -1.0);
        if (!bt.asin_coef.empty()) y = eval_monomial(y, bt.asin_coef);
        return y;
    }

    // level-0 ciphertext -> the same polynomials (centred mod q_0) over Q_top
    DCt mod_raise(const DCt& a, int top) {
        DCt o = alloc(top, q(0));
        DCt tmp = alloc(0, a.scale);   // [m][2][1][N] coefficient-domain copy
        RowMap r0;
        r0.period = 1;
        r0.mod_of[0] = 0;
        launch_ntt(c, a.data(), tmp.data(), m, stride(0), stride(0), 2, r0, true, s);
        // each polynomial is one "ring-t plaintext": centred lift from q_0 to every limb, then NTT
        launch_lift_ringt(c, 0, top, tmp.data(), N, o.data(), (long long)(top + 1) * N, 2 * m, s);
        launch_ntt(c, o.data(), o.data(), m, stride(top), 2 * (top + 1), rm2(top), false, s);
        return o;
    }
};

}  // namespace

Bootstrap* bootstrap_create(Context& c, int cts_depth, int stc_depth, int K, int double_angle, double message_ratio,
                            double in_scale, double out_scale, int log_slots, hipStream_t s, int sine_deg, int arcsine_deg) {
    auto b = std::make_unique<Bootstrap>(c);
    b->sine_deg = sine_deg;
    b->arcsine_deg = arcsine_deg;
    b->log_slots = log_slots;
    b->cts_depth = cts_depth;
    b->stc_depth = stc_depth;
    b->K = K;
    b->r = double_angle;
    b->mr = message_ratio;
    b->in_scale = in_scale;
    b->out_scale = out_scale;
    c.use_device();
    b->build(s);
    return b.release();
}
void bootstrap_destroy(Bootstrap* b) { delete b; }

// in: [batch][2][1][N] level-0 ciphertexts at the plan's input scale; out: [batch][2][out_level+1][N]
void bootstrap_run(Bootstrap& bt, const u64* in, long long sin, u64* out, long long sout, int batch, const Key& rlk,
                   const GaloisKeys& glk, const Key* swk_dts, const Key* swk_std, hipStream_t s) {
    Context& c = bt.c;
    c.use_device();
    Eval ev(c, bt, s, batch, rlk, glk);
    const long long N = c.n;
    // diagnostic: LSA_BT_STOP=<step> returns the first out_level+1 limbs of that step's intermediate instead
    const int stop = sw::bt_stop();
    const int out_level = bootstrap_out_level(bt);
    int step = 0;
    auto emit = [&](const DCt& v) {
        std::vector<int> rr;
        const int lv = std::min(v.level, out_level);
        for (int p = 0; p < 2; p++)
            for (int j = 0; j <= out_level; j++) rr.push_back(p * (v.level + 1) + std::min(j, lv));
        launch_copy_rows(c, v.data(), ev.stride(v.level), out, sout, (int)rr.size(), rr.data(), batch, s);
    };
#define LSA_BT_CHECK(v)            \
    if (++step == stop) {          \
        emit(v);                   \
        return;                    \
    }
    DCt x = ev.alloc(0, bt.in_scale);
    std::vector<int> rows = {0, 1};
    launch_copy_rows(c, in, sin, x.data(), 2 * N, 2, rows.data(), batch, s);
    x = ev.mul_int(x, bt.mul_c);
    LSA_BT_CHECK(x)   // 1
    if (swk_dts) {
        DCt y = ev.alloc(0, x.scale);
        ckks_switch_key(c, 0, x.data(), *swk_dts, y.data(), batch, 2 * N, 2 * N, s);
        x = y;
    }
    x = ev.mod_raise(x, bt.top_level);
    LSA_BT_CHECK(x)   // 2
    if (swk_std) {
        DCt y = ev.alloc(bt.top_level, x.scale);
        ckks_switch_key(c, bt.top_level, x.data(), *swk_std, y.data(), batch, ev.stride(bt.top_level), ev.stride(bt.top_level), s);
        x = y;
    }
    if (bt.sparse) {   // SubSum: trace onto the subring of the sparse packing
        int logn_ring = 0;
        while ((1 << logn_ring) < c.n) logn_ring++;
        for (int i = bt.log_slots; i < logn_ring - 1; i++) x = ev.add(x, ev.rotate(x, 1 << i));
    }
    for (auto& mt : bt.cts) {
        x = ev.linear_transform(x, mt);
        LSA_BT_CHECK(x)   // 3 .. 2+cts_depth
    }
    DCt y;
    if (bt.sparse) {
        DCt a = ev.linear_transform(x, bt.p1, false);
        DCt b = ev.linear_transform(ev.conj(x), bt.p2, false);
        DCt u = ev.rescale(ev.add(a, b));          // [Re(t)/K | Im(t)/K], period 2*slots
        LSA_BT_CHECK(u)
        y = ev.eval_mod(u);
        LSA_BT_CHECK(y)
    } else {
        DCt xc = ev.conj(x);
        DCt u_re = ev.add(x, xc);
        LSA_BT_CHECK(u_re)
        DCt u_im = ev.mul_by_i(ev.sub(x, xc), -1);
        LSA_BT_CHECK(u_im)
        // both halves go through EvalMod as ONE batch of 2m ciphertexts (ciphertexts of a batch are independent: same
        // residues as two separate evaluations, half the launches -- what a single-ciphertext bootstrap is bound by)
        Eval ev2(c, bt, s, 2 * batch, rlk, glk);
        DCt uu = ev2.alloc(u_re.level, u_re.scale);
        const size_t half_bytes = (size_t)batch * ev.stride(u_re.level) * sizeof(u64);
        LSA_HIP(hipMemcpyAsync(uu.data(), u_re.data(), half_bytes, hipMemcpyDeviceToDevice, s));
        LSA_HIP(hipMemcpyAsync(uu.data() + (size_t)batch * ev.stride(u_re.level), u_im.data(), half_bytes, hipMemcpyDeviceToDevice, s));
        DCt yy = ev2.eval_mod(uu);
        DCt y_re = ev.alloc(yy.level, yy.scale), y_im = ev.alloc(yy.level, yy.scale);
        const size_t out_bytes = (size_t)batch * ev.stride(yy.level) * sizeof(u64);
        LSA_HIP(hipMemcpyAsync(y_re.data(), yy.data(), out_bytes, hipMemcpyDeviceToDevice, s));
        LSA_HIP(hipMemcpyAsync(y_im.data(), yy.data() + (size_t)batch * ev.stride(yy.level), out_bytes, hipMemcpyDeviceToDevice, s));
        LSA_BT_CHECK(y_re)
        y = ev.add(y_re, ev.mul_by_i(y_im, 1));
        LSA_BT_CHECK(y)
    }
    for (auto& mt : bt.stc) y = ev.linear_transform(y, mt);
#undef LSA_BT_CHECK
    std::vector<int> all(2 * (y.level + 1));
    for (size_t i = 0; i < all.size(); i++) all[i] = (int)i;
    launch_copy_rows(c, y.data(), ev.stride(y.level), out, sout, (int)all.size(), all.data(), batch, s);
}

int bootstrap_out_level(const Bootstrap& bt) { return bt.top_level - bt.cts_depth - bt.evalmod_depth() - bt.stc_depth; }

// read-only views for the C API (constants are exported so that the oracle can replay the program with the same integers)
double bootstrap_out_scale(const Bootstrap& bt) { return bt.natural_scale; }
const std::vector<u64>& bootstrap_galois(const Bootstrap& bt) { return bt.galois; }
const std::vector<double>& bootstrap_chebyshev(const Bootstrap& bt) { return bt.cheb; }
const std::vector<double>& bootstrap_arcsine(const Bootstrap& bt) { return bt.asin_coef; }
// matrix order: the leading CoeffsToSlots matrices, (sparse packing: P1, P2,) the SlotsToCoeffs matrices
int bootstrap_matrices(const Bootstrap& bt) { return (int)(bt.cts.size() + bt.stc.size()) + (bt.sparse ? 2 : 0); }
int bootstrap_cts_matrices(const Bootstrap& bt) { return (int)bt.cts.size(); }
bool bootstrap_is_sparse(const Bootstrap& bt) { return bt.sparse; }
void bootstrap_matrix(const Bootstrap& bt, int i, int* level, int* n1, const std::vector<int>** ks, const std::vector<u64*>** plains,
                      int* rows) {
    LSA_REQUIRE(i >= 0 && i < bootstrap_matrices(bt), "bootstrap: matrix index out of range");
    const int nc = (int)bt.cts.size(), extra = bt.sparse ? 2 : 0;
    const BtMatrix& m = i < nc ? bt.cts[i] : (i < nc + extra ? (i == nc ? bt.p1 : bt.p2) : bt.stc[i - nc - extra]);
    *level = m.level;
    *n1 = m.naive ? 0 : m.n1;
    *ks = &m.ks;
    *plains = &m.plains;
    if (rows) *rows = m.rows;
}

}  // namespace lsa
