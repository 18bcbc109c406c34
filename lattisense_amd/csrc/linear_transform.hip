// linear_transform.hip — CKKS linear transforms in diagonal form (linear_transform.h): host-side encoding of the diagonals,
// the baby-step / giant-step plan of the reference's planner, and the single- / double-hoisted evaluation as a program of the
// integer operators of ops.hip / kernels.hip.  Only the encoded diagonals are floating-point work; a replay with the same
// plaintexts on the CPU oracle (oracle/ckks_bootstrap.py linear_transform) gives identical residues
// (tests/test_gpu_ckks_lt.py, tests/test_gpu_bootstrap.py).
#include <algorithm>
#include <cstdlib>

#include "bfv_encode.h"
#include "layout_check.h"
#include "linear_transform.h"

namespace lsa {

namespace {
const double kPi = 3.14159265358979323846;

// slots -> coefficients: t = U^-1 z (inverse special FFT), m_k = Re t_k, m_{k+n} = Im t_k
std::vector<double> slots_to_coeffs(std::vector<cplx> v, const std::vector<int>& rg) {
    const int n = (int)v.size();
    const long long m = 4LL * n;
    for (int len = n; len >= 2; len >>= 1) {
        const int lenh = len >> 1;
        const long long lenq = 4LL * len;
        for (int i = 0; i < n; i += len)
            for (int j = 0; j < lenh; j++) {
                const long long idx = (lenq - (rg[j] % lenq)) * (m / lenq);
                const cplx w = std::polar(1.0, 2.0 * kPi * (double)idx / (double)m);
                const cplx a = v[i + j], b = v[i + j + lenh];
                v[i + j] = a + b;
                v[i + j + lenh] = (a - b) * w;
            }
    }
    int lg = 0;
    while ((1 << lg) < n) lg++;
    std::vector<double> out(2 * (size_t)n);
    for (int i = 0; i < n; i++) {
        int r = 0;
        for (int b = 0; b < lg; b++) r |= ((i >> b) & 1) << (lg - 1 - b);
        out[i] = v[r].real() / n;
        out[i + n] = v[r].imag() / n;
    }
    return out;
}

}  // namespace

std::vector<int> rot_group(int n_slots) {
    std::vector<int> g(n_slots);
    long long v = 1;
    const long long m = 4LL * n_slots;
    for (int i = 0; i < n_slots; i++) {
        g[i] = (int)v;
        v = v * 5 % m;
    }
    return g;
}

void bsgs_sets(const std::vector<int>& ks, int n, int n1, std::vector<int>& giants, std::vector<int>& babies) {
    std::map<int, bool> g, b;
    for (int k : ks) {
        g[((k % n) / n1) * n1 % n] = true;
        b[(k % n) % n1] = true;
    }
    giants.clear();
    babies.clear();
    for (auto& kv : g) giants.push_back(kv.first);
    for (auto& kv : b) babies.push_back(kv.first);
}

int bsgs_split(const std::vector<int>& ks, int n, double ratio) {
    int n1 = 1;
    std::vector<int> g, b;
    while (n1 < n) {
        bsgs_sets(ks, n, n1, g, b);
        const int nb_g = (int)g.size() - 1, nb_b = (int)b.size() - 1;
        if (nb_g == 0 || (double)nb_b / nb_g == ratio) return n1;
        if ((double)nb_b / nb_g > ratio) return n1 / 2;
        n1 <<= 1;
    }
    return 1;
}

int lt_plan(const std::vector<int>& ks, int period, double ratio, std::vector<int>& rotations) {
    rotations.clear();
    if (ks.size() < 3) {
        for (int k : ks)
            if (k) rotations.push_back(k);
        return 0;
    }
    const int n1 = bsgs_split(ks, period, ratio);
    std::vector<int> g, b;
    bsgs_sets(ks, period, n1, g, b);
    std::map<int, bool> all;
    for (int r : g) all[r] = true;
    for (int r : b) all[r] = true;
    for (auto& kv : all)
        if (kv.first) rotations.push_back(kv.first);
    return n1;
}

// A constant beyond 2^62 means the modulus chain does not fit the level plan (e.g. EvalMod running on primes much smaller
// than its scale) or the scale does not fit the values: refuse instead of computing garbage.
long long round_even(double v, const char* who) {
    LSA_REQUIRE(std::fabs(v) < 4.6e18, std::string(who) + ": encoded constant out of range -- the modulus chain or the encoding "
                                                         "scale does not match the values (level plan: depths / scales)");
    return (long long)std::nearbyint(v);
}

u64* lt_upload_plain(Context& c, const std::vector<double>& coef, double scale, int level, hipStream_t s, bool ext,
                     std::vector<u64*>& owned, const char* who) {
    const int L = level + 1 + (ext ? c.np : 0);
    const size_t N = (size_t)c.n;
    std::vector<u64> host((size_t)L * N);
    RowMap rm;
    rm.period = L;
    for (int j = 0; j <= level; j++) rm.mod_of[j] = (unsigned char)j;
    for (int j = level + 1; j < L; j++) rm.mod_of[j] = (unsigned char)c.p_mod(j - level - 1);
    for (size_t x = 0; x < N; x++) {
        const long long v = round_even(coef[x] * scale, who);
        for (int j = 0; j < L; j++) {
            const long long q = (long long)c.T.mod[rm.mod_of[j]];
            long long r = v % q;
            if (r < 0) r += q;
            host[(size_t)j * N + x] = (u64)r;
        }
    }
    u64* d = nullptr;
    LSA_HIP(hipMalloc((void**)&d, host.size() * sizeof(u64)));
    owned.push_back(d);
    LSA_HIP(hipMemcpyAsync(d, host.data(), host.size() * sizeof(u64), hipMemcpyHostToDevice, s));
    launch_ntt(c, d, d, 1, (long long)L * N, L, rm, false, s);
    LSA_HIP(hipStreamSynchronize(s));   // `host` goes out of scope
    return d;
}

void ckks_encode(Context& c, int level, int log_slots, const double* values, double scale, u64* out, long long sout, int batch,
                 hipStream_t s) {
    const char* who = "lsa_ckks_encode";
    LSA_REQUIRE(c.algo == LSA_ALGO_CKKS, std::string(who) + ": context is not CKKS");
    LSA_REQUIRE(level >= 0 && level < c.nq, std::string(who) + ": level out of range");
    LSA_REQUIRE(log_slots >= 0 && (2 << log_slots) <= c.n, std::string(who) + ": log_slots beyond log2(N) - 1");
    LSA_REQUIRE(std::isfinite(scale) && scale > 0, std::string(who) + ": scale must be positive");
    if (batch <= 0) return;
    const int L = level + 1, n = c.n / 2, period = 1 << log_slots;
    const size_t N = (size_t)c.n;
    LSA_REQUIRE(values && out, std::string(who) + ": null argument");
    LSA_REQUIRE(sout >= (long long)(L * N), std::string(who) + ": output stride below one plaintext");
    // k_lift_i64 stores 16 bytes per lane at out + item * sout
    LSA_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0 && (sout & 1) == 0,
                std::string(who) + ": out must be 16-byte aligned with an even batch stride");
    const std::vector<int> rg = rot_group(n);
    std::vector<long long> coef((size_t)batch * N);
    std::vector<cplx> z(n);
    for (int b = 0; b < batch; b++) {
        const double* v = values + (size_t)b * period * 2;
        for (int t = 0; t < period; t++)
            LSA_REQUIRE(std::isfinite(v[2 * t]) && std::isfinite(v[2 * t + 1]), std::string(who) + ": value not finite");
        for (int t = 0; t < n; t++) z[t] = cplx(v[2 * (t % period)], v[2 * (t % period) + 1]);
        const std::vector<double> m = slots_to_coeffs(z, rg);
        for (size_t x = 0; x < N; x++) coef[(size_t)b * N + x] = round_even(m[x] * scale, who);
    }
    // nothing has been queued so far: a refused value leaves the output untouched
    long long* d = reinterpret_cast<long long*>(c.workspace(coef.size(), s));
    LSA_HIP(hipMemcpyAsync(d, coef.data(), coef.size() * sizeof(long long), hipMemcpyHostToDevice, s));
    launch_lift_i64(c, d, (long long)N, out, sout, L, batch, s);
    RowMap rm;
    rm.period = L;
    for (int j = 0; j < L; j++) rm.mod_of[j] = (unsigned char)j;
    launch_ntt(c, out, out, batch, sout, L, rm, false, s);
    LSA_HIP(hipStreamSynchronize(s));   // `coef` goes out of scope
}

BtMatrix lt_make_matrix(Context& c, const Diags& mat, int level, int period, double pt_scale, double ratio, bool double_hoist,
                        hipStream_t s, std::vector<u64*>& owned, std::map<u64, bool>& gal, const char* who) {
    const int n = c.n / 2;
    const std::vector<int> rg = rot_group(n);
    auto gel = [&](int rot) { return galois_of_rotation(rot % n, c.n); };   // rot in [0, period], period <= N/2
    BtMatrix bm;
    bm.level = level;
    bm.period = period;
    bm.pt_scale = pt_scale;
    for (auto& kv : mat) bm.ks.push_back(kv.first);
    bm.naive = bm.ks.size() < 3;
    bm.n1 = bm.naive ? 1 : bsgs_split(bm.ks, period, ratio);
    const bool ext = double_hoist && !bm.naive;
    bm.rows = bm.level + 1 + (ext ? c.np : 0);
    for (int k : bm.ks) {
        const int giant = bm.naive ? 0 : (k / bm.n1) * bm.n1;
        const std::vector<cplx>& d = mat.at(k);
        std::vector<cplx> rolled(n);
        for (int t = 0; t < n; t++) rolled[t] = d[(((t - giant) % period) + period) % period];   // rot_{-giant}(diag), tiled
        bm.plains.push_back(lt_upload_plain(c, slots_to_coeffs(rolled, rg), pt_scale, bm.level, s, ext, owned, who));
        const int baby = bm.naive ? k : k - giant;
        if (baby) gal[gel(baby)] = true;
        if (giant) gal[gel(giant)] = true;
    }
    return bm;
}

// ------------------------------------------------------------------------------------------------ device evaluator
void DevPool::release() {
    for (u64* p : all) (void)hipFree(p);
    all.clear();
    free.clear();
}

DCt LtEval::alloc_words(size_t words) { return pool_alloc_words(pool, words); }

DCt pool_alloc_words(DevPool& pool, size_t words) {
    auto b = std::make_shared<DBuf>();
    b->words = words;
    b->pool = &pool;
    auto it = pool.free.find(words);
    if (it != pool.free.end()) {
        b->p = it->second;
        pool.free.erase(it);
    } else {
        b->pool = nullptr;   // (a failed allocation must not enter the free list)
        LSA_HIP(hipMalloc((void**)&b->p, words * sizeof(u64)));
        b->pool = &pool;
        pool.all.push_back(b->p);
    }
    return DCt{b, 0, 0.0};
}

DCt LtEval::rotate(const DCt& a, int r) {
    const int n = c.n / 2;
    r = ((r % n) + n) % n;
    if (r == 0) return a;
    const u64 e = galois_of(r);
    DCt o = alloc(a.level, a.scale);
    ckks_rotate(c, a.level, a.data(), e, gkey(e), o.data(), m, stride(a.level), stride(a.level), s);
    return o;
}

std::map<int, DCt> LtEval::rotate_many(const DCt& a, const std::vector<int>& steps) {
    const int n = c.n / 2;
    std::map<int, DCt> out;
    std::vector<u64> els;
    std::vector<const Key*> keys;
    std::vector<u64*> ptrs;
    for (int r0 : steps) {
        const int r = ((r0 % n) + n) % n;
        if (out.count(r)) continue;
        if (r == 0) {
            out[0] = a;
            continue;
        }
        const u64 e = galois_of(r);
        const Key* k = &gkey(e);
        DCt o = alloc(a.level, a.scale);
        els.push_back(e);
        keys.push_back(k);
        ptrs.push_back(o.data());
        out[r] = o;
    }
    ckks_rotate_many(c, a.level, a.data(), (int)els.size(), els.data(), keys.data(), ptrs.data(), m, stride(a.level),
                     stride(a.level), s);
    return out;
}

std::map<int, DCt> LtEval::rotate_many_ext(const DCt& a, const std::vector<int>& steps) {
    const int n = c.n / 2;
    std::map<int, DCt> out;
    std::vector<u64> els;
    std::vector<const Key*> keys;
    std::vector<u64*> ptrs;
    for (int r0 : steps) {   // every key is looked up before anything is launched: a missing one leaves no work behind
        const int r = ((r0 % n) + n) % n;
        if (r) (void)gkey(galois_of(r));
    }
    for (int r0 : steps) {
        const int r = ((r0 % n) + n) % n;
        if (out.count(r)) continue;
        DCt o = alloc_ext(a.level, a.scale);
        out[r] = o;
        if (r == 0) {
            ckks_lift_ext(c, a.level, a.data(), o.data(), m, stride(a.level), stride_ext(a.level), s);
            continue;
        }
        const u64 e = galois_of(r);
        els.push_back(e);
        keys.push_back(&gkey(e));
        ptrs.push_back(o.data());
    }
    ckks_rotate_many_ext(c, a.level, a.data(), (int)els.size(), els.data(), keys.data(), ptrs.data(), m, stride(a.level),
                         stride_ext(a.level), s, c1_coef, s_coef);
    return out;
}

DCt LtEval::moddown(const DCt& a) {
    DCt o = alloc(a.level, a.scale);
    ckks_moddown_ext(c, a.level, a.data(), o.data(), m, stride_ext(a.level), stride(a.level), s);
    return o;
}

// The inner sums of a baby-step / giant-step matrix.  Up to 8 x 8 steps: one k_mac_plain_multi launch.  Beyond: blocks of
// 8 babies x 8 giants, each launch adding to the sums the previous baby block left (every baby-step ciphertext is read
// ceil(ng/8) times, every plaintext once), or -- LSA_LT_BLOCKED_MAC=0 -- one k_mac_plain launch per giant step and 16 terms
// (every baby-step ciphertext read once per giant step it occurs in).  All sums are fully reduced: the same words either way.
void LtEval::inner_sums(int nb, const u64* const* ct, long long sct, int ng, const u64* const* pt, u64* const* out, long long so,
                        int limbs, const RowMap& rm) {
    const bool one = nb <= LSA_MACM_MAX && ng <= LSA_MACM_MAX;
    if (one || sw::lt_blocked_mac()) {
        for (int g0 = 0; g0 < ng; g0 += LSA_MACM_MAX) {
            const int gn = std::min(LSA_MACM_MAX, ng - g0);
            for (int b0 = 0; b0 < nb; b0 += LSA_MACM_MAX) {
                const int bn = std::min(LSA_MACM_MAX, nb - b0);
                const u64* bp[LSA_MACM_MAX * LSA_MACM_MAX];
                long long bs[LSA_MACM_MAX];
                bool any = b0 == 0;   // the first block writes the sums even where it has no term
                for (int gi = 0; gi < gn; gi++)
                    for (int bi = 0; bi < bn; bi++) {
                        bp[gi * bn + bi] = pt[(size_t)(g0 + gi) * nb + b0 + bi];
                        any = any || bp[gi * bn + bi];
                    }
                if (!any) continue;
                for (int bi = 0; bi < bn; bi++) bs[bi] = sct;
                launch_mac_plain_multi(c, bn, ct + b0, bs, gn, bp, out + g0, so, m, 2, limbs, rm, s, /*accumulate=*/b0 > 0);
            }
        }
        return;
    }
    for (int g2 = 0; g2 < ng; g2++) {
        std::vector<int> bi;
        for (int b = 0; b < nb; b++)
            if (pt[(size_t)g2 * nb + b]) bi.push_back(b);
        for (size_t i0 = 0; i0 < bi.size(); i0 += LSA_MAC_MAX_TERMS) {
            const int cnt = (int)std::min<size_t>(LSA_MAC_MAX_TERMS, bi.size() - i0);
            const u64* tc[LSA_MAC_MAX_TERMS];
            const u64* tp[LSA_MAC_MAX_TERMS];
            long long ts[LSA_MAC_MAX_TERMS], tz[LSA_MAC_MAX_TERMS];
            for (int i = 0; i < cnt; i++) {
                tc[i] = ct[bi[i0 + i]];
                ts[i] = sct;
                tp[i] = pt[(size_t)g2 * nb + bi[i0 + i]];
                tz[i] = 0;
            }
            launch_mac_plain(c, cnt, tc, ts, tp, tz, i0 ? out[g2] : nullptr, so, out[g2], so, m, 2, limbs, rm, s);
        }
    }
}

// Baby-step / giant-step with the sums kept over Q u P ("double hoisting", Lattigo v4 ckks/linear_transform.go
// MultiplyByDiagMatrixBSGS; oracle twin: oracle/ckks_bootstrap.py linear_transform, double_hoist): the baby-step rotations
// are gadget products without their division by P, the plaintexts carry the special primes' residues, each giant step's
// inner sum is divided once, rotated without division into the running sum, and that sum is divided once:
// (giant steps + 1) ModDowns instead of (baby steps + giant steps).
DCt LtEval::linear_transform_dh(const DCt& ct, const BtMatrix& mt, bool do_rescale) {
    const double pt_scale = mt.pt_scale;
    const int T = ct.level + 1 + c.np;
    const int n = c.n / 2;
    std::vector<int> steps;
    for (int k : mt.ks) steps.push_back(k % mt.n1);
    std::map<int, std::vector<size_t>> by_giant;
    for (size_t i = 0; i < mt.ks.size(); i++) by_giant[(mt.ks[i] / mt.n1) * mt.n1].push_back(i);
    for (auto& kv : by_giant)   // the giant steps' keys too, before any work is queued
        if (kv.first % n) (void)gkey(galois_of(kv.first % n));
    std::map<int, DCt> babies = rotate_many_ext(ct, steps);
    std::vector<int> bsteps, gsteps;
    std::vector<const u64*> cp;
    for (auto& kv : babies) {
        bsteps.push_back(kv.first);
        cp.push_back(kv.second.data());
    }
    const int nb = (int)bsteps.size(), ng = (int)by_giant.size();
    std::vector<const u64*> pp((size_t)ng * nb, nullptr);
    std::vector<DCt> inner;
    std::vector<u64*> op;
    int gi = 0;
    for (auto& kv : by_giant) {
        for (size_t i : kv.second) {
            const int bi = (int)(std::find(bsteps.begin(), bsteps.end(), mt.ks[i] - kv.first) - bsteps.begin());
            LSA_REQUIRE(bi < nb, who + ": baby step without its rotation");
            pp[(size_t)gi * nb + bi] = mt.plains[i];
        }
        inner.push_back(alloc_ext(ct.level, ct.scale * pt_scale));
        op.push_back(inner.back().data());
        gsteps.push_back(kv.first);
        gi++;
    }
    inner_sums(nb, cp.data(), stride_ext(ct.level), ng, pp.data(), op.data(), stride_ext(ct.level), T, rm_ext(ct.level));
    babies.clear();
    DCt acc;
    bool have = false;
    for (int g2 = 0; g2 < ng; g2++) {
        const int r = ((gsteps[g2] % n) + n) % n;
        if (r == 0) {
            LSA_REQUIRE(!have, who + ": giant step 0 must come first");
            acc = inner[g2];
            have = true;
            continue;
        }
        DCt iq = moddown(inner[g2]);
        if (!have) acc = alloc_ext(ct.level, ct.scale * pt_scale);
        const u64 e = galois_of(r);
        ckks_rotate_ext(c, ct.level, iq.data(), e, gkey(e), acc.data(), have, m, stride(ct.level), stride_ext(ct.level), s, giant_scatter);
        have = true;
    }
    if (coeff_out) {   // BFV exit: the last division leaves in the coefficient domain, in the caller's buffer
        LSA_REQUIRE(!do_rescale, who + ": a coefficient-domain exit takes no rescale");
        ckks_moddown_ext(c, ct.level, acc.data(), coeff_out, m, stride_ext(ct.level), s_coeff_out, s, /*coeff_out=*/true);
        return wrap(coeff_out, ct.level, ct.scale * pt_scale);
    }
    DCt res = moddown(acc);
    return do_rescale ? rescale(res) : res;
}

DCt LtEval::linear_transform(const DCt& ct, const BtMatrix& mt, bool do_rescale) {
    LSA_REQUIRE(ct.level == mt.level, who + ": linear transform applied at an unexpected level");
    if (!mt.naive && mt.rows > ct.level + 1) return linear_transform_dh(ct, mt, do_rescale);
    const double pt_scale = mt.pt_scale;
    const int L = ct.level + 1;
    // every baby step is a rotation of the SAME ciphertext: one decomposition serves them all
    std::vector<int> steps;
    for (int k : mt.ks) steps.push_back(mt.naive ? k : k % mt.n1);
    std::map<int, std::vector<size_t>> by_giant;
    if (!mt.naive) {
        const int n = c.n / 2;
        for (size_t i = 0; i < mt.ks.size(); i++) by_giant[(mt.ks[i] / mt.n1) * mt.n1].push_back(i);
        for (auto& kv : by_giant)
            if (kv.first % n) (void)gkey(galois_of(kv.first % n));
    }
    std::map<int, DCt> babies = rotate_many(ct, steps);
    auto baby = [&](int b) -> const DCt& { return babies.at(b); };
    // sum of (shared plaintext) x (rotated ciphertext) terms, LSA_MAC_MAX_TERMS per launch
    auto mac = [&](const std::vector<std::pair<const u64*, const DCt*>>& terms) {
        DCt o = alloc(ct.level, ct.scale * pt_scale);
        for (size_t i0 = 0; i0 < terms.size(); i0 += LSA_MAC_MAX_TERMS) {
            const int cnt = (int)std::min<size_t>(LSA_MAC_MAX_TERMS, terms.size() - i0);
            const u64* cp[LSA_MAC_MAX_TERMS];
            const u64* pp[LSA_MAC_MAX_TERMS];
            long long cs[LSA_MAC_MAX_TERMS], ps[LSA_MAC_MAX_TERMS];
            for (int i = 0; i < cnt; i++) {
                cp[i] = terms[i0 + i].second->data();
                cs[i] = stride(ct.level);
                pp[i] = terms[i0 + i].first;
                ps[i] = 0;
            }
            launch_mac_plain(c, cnt, cp, cs, pp, ps, i0 ? o.data() : nullptr, stride(ct.level), o.data(), stride(ct.level), m, 2,
                             L, rm2(ct.level), s);
        }
        return o;
    };
    DCt acc;
    bool have = false;
    if (mt.naive) {
        std::vector<std::pair<const u64*, const DCt*>> terms;
        for (size_t i = 0; i < mt.ks.size(); i++) terms.push_back({mt.plains[i], &baby(mt.ks[i])});
        acc = mac(terms);
        return do_rescale ? rescale(acc) : acc;
    }
    const bool fits = babies.size() <= LSA_MACM_MAX && by_giant.size() <= LSA_MACM_MAX;
    if ((fits || sw::lt_blocked_mac()) && by_giant.size() > 1 && !sw::bt_no_multi_mac()) {
        // all inner sums together: every baby-step ciphertext is read once per block of giant steps, not once per giant step
        std::vector<int> bsteps;
        std::vector<const u64*> cp;
        for (auto& kv : babies) {
            bsteps.push_back(kv.first);
            cp.push_back(kv.second.data());
        }
        const int nb = (int)bsteps.size(), ng = (int)by_giant.size();
        std::vector<const u64*> pp((size_t)ng * nb, nullptr);
        std::vector<DCt> inner;
        std::vector<u64*> op;
        std::vector<int> gsteps;
        int gi = 0;
        for (auto& kv : by_giant) {
            for (size_t i : kv.second) {
                const int bs = mt.ks[i] - kv.first;
                const int bi = (int)(std::find(bsteps.begin(), bsteps.end(), bs) - bsteps.begin());
                LSA_REQUIRE(bi < nb, who + ": baby step without its rotation");
                pp[(size_t)gi * nb + bi] = mt.plains[i];
            }
            inner.push_back(alloc(ct.level, ct.scale * pt_scale));
            op.push_back(inner.back().data());
            gsteps.push_back(kv.first);
            gi++;
        }
        inner_sums(nb, cp.data(), stride(ct.level), ng, pp.data(), op.data(), stride(ct.level), L, rm2(ct.level));
        for (int g2 = 0; g2 < ng; g2++) {
            DCt r = rotate(inner[g2], gsteps[g2]);
            acc = have ? add(acc, r) : r;
            have = true;
        }
        return do_rescale ? rescale(acc) : acc;
    }
    for (auto& kv : by_giant) {
        std::vector<std::pair<const u64*, const DCt*>> terms;
        for (size_t i : kv.second) terms.push_back({mt.plains[i], &baby(mt.ks[i] - kv.first)});
        DCt inner = rotate(mac(terms), kv.first);
        acc = have ? add(acc, inner) : inner;
        have = true;
    }
    return do_rescale ? rescale(acc) : acc;
}

// ------------------------------------------------------------------------------------------------ public operator
LinearTransform::~LinearTransform() {
    (void)hipSetDevice(c.device);
    (void)hipDeviceSynchronize();
    for (u64* p : owned) (void)hipFree(p);
    pool.release();
}

// Giant-step rotations of the public operator: the accumulating scatter of the key MAC (out[perm[x]] += mac(x) + P base(x))
// or decompose + MAC (fused with the extension transform's second pass where the shape allows) + k_permute_ext.
// LSA_ROT_SCATTER=0 selects the permutation form everywhere; LSA_LT_GIANT_SCATTER=0 / 1 overrides the default for the giant
// steps alone (A/B, parity).  Default: DESIGN.md 4.7.
static bool lt_giant_scatter() { return sw::rot_scatter() && sw::lt_giant_scatter(); }

LinearTransform* lt_create(Context& c, int level, int log_slots, int n_diag, const int* diag_index, const double* values,
                           double pt_scale, double bsgs_ratio, bool double_hoist, hipStream_t s) {
    LSA_REQUIRE(c.algo == LSA_ALGO_CKKS, "linear transform: CKKS context required");
    LSA_REQUIRE(level >= 0 && level < c.nq, "linear transform: level out of range");
    LSA_REQUIRE(log_slots >= 0 && (2 << log_slots) <= c.n, "linear transform: log_slots beyond log2(N) - 1");
    LSA_REQUIRE(n_diag >= 1 && diag_index && values, "linear transform: at least one diagonal");
    LSA_REQUIRE(pt_scale >= 0 && bsgs_ratio >= 0, "linear transform: negative scale or ratio");
    LSA_REQUIRE(!double_hoist || c.np >= 1, "linear transform: double hoisting needs a special prime");
    const int period = 1 << log_slots;
    Diags mat;
    for (int i = 0; i < n_diag; i++) {
        const int k = ((diag_index[i] % period) + period) % period;
        LSA_REQUIRE(!mat.count(k), "linear transform: diagonal index " + std::to_string(diag_index[i]) + " repeats another modulo the period");
        std::vector<cplx>& d = mat[k];
        d.resize(period);
        const double* v = values + (size_t)i * period * 2;
        for (int t = 0; t < period; t++) {
            LSA_REQUIRE(std::isfinite(v[2 * t]) && std::isfinite(v[2 * t + 1]), "linear transform: diagonal value not finite");
            d[t] = cplx(v[2 * t], v[2 * t + 1]);
        }
    }
    auto lt = std::make_unique<LinearTransform>(c);
    lt->double_hoist = double_hoist;
    std::map<u64, bool> gal;
    lt->m = lt_make_matrix(c, mat, level, period, pt_scale > 0 ? pt_scale : (double)c.T.mod[level], bsgs_ratio > 0 ? bsgs_ratio : 2.0,
                           double_hoist, s, lt->owned, gal, "linear transform");
    for (auto& kv : gal) lt->galois.push_back(kv.first);
    return lt.release();
}

void lt_run(LinearTransform& lt, const u64* in, long long sin, u64* out, long long sout, int batch, bool rescale,
            const GaloisKeys& glk, hipStream_t s) {
    if (batch <= 0) return;
    Context& c = lt.c;
    const long long N = c.n;
    const int level = lt.m.level, out_level = rescale ? level - 1 : level;
    LSA_REQUIRE(!rescale || level >= 1, "linear transform: a rescale needs level >= 1");
    LSA_REQUIRE(in && out, "linear transform: null argument");
    LSA_REQUIRE(sin >= 2LL * (level + 1) * N && sout >= 2LL * (out_level + 1) * N, "linear transform: batch stride shorter than a ciphertext");
    // the row copies that gather `in` and store `out` move 16 bytes per lane at base + item * stride
    LSA_REQUIRE(layout::aligned16(layout::span_of(in, sin, 0)) && layout::aligned16(layout::span_of(out, sout, 0)),
                "linear transform: in and out must be 16-byte aligned with even batch strides");
    LSA_REQUIRE(layout::apart(out, sout, 2 * (size_t)(out_level + 1) * N, in, sin, 2 * (size_t)(level + 1) * N, batch),
                "linear transform: out overlaps in");
    LtEval ev(c, lt.pool, s, batch, glk, "linear transform");
    ev.giant_scatter = lt_giant_scatter();
    DCt x;
    if (sin == ev.stride(level)) {
        x = ev.wrap(const_cast<u64*>(in), level, 1.0);   // read only
    } else {
        x = ev.alloc(level, 1.0);
        std::vector<int> rows(2 * (level + 1));
        for (size_t i = 0; i < rows.size(); i++) rows[i] = (int)i;
        launch_copy_rows(c, in, sin, x.data(), ev.stride(level), (int)rows.size(), rows.data(), batch, s);
    }
    DCt y = ev.linear_transform(x, lt.m, rescale);
    std::vector<int> all(2 * (y.level + 1));
    for (size_t i = 0; i < all.size(); i++) all[i] = (int)i;
    launch_copy_rows(c, y.data(), ev.stride(y.level), out, sout, (int)all.size(), all.data(), batch, s);
}

// ------------------------------------------------------------------------------------------------ BFV operator
BfvLinearTransform::~BfvLinearTransform() {
    (void)hipSetDevice(c.device);
    (void)hipDeviceSynchronize();
    if (plains_dev) (void)hipFree(plains_dev);
    pool.release();
}

BfvLinearTransform* bfv_lt_create(Context& c, int level, int period, int n_diag, const int* diag_index, const u64* values,
                                  double bsgs_ratio, hipStream_t s) {
    const std::string who = "lsa_bfv_lt_create";
    LSA_REQUIRE(c.algo == LSA_ALGO_BFV, who + ": context is not BFV");
    LSA_REQUIRE(level >= 0 && level < c.nq, who + ": level out of range (0.." + std::to_string(c.nq - 1) + ")");
    LSA_REQUIRE(c.np >= 1, who + ": double hoisting needs a special prime");
    const int n = c.n / 2;
    LSA_REQUIRE(period >= 1 && (period & (period - 1)) == 0 && period <= n, who + ": period must be a power of two that divides N/2");
    LSA_REQUIRE(n_diag >= 1 && diag_index && values, who + ": at least one diagonal");
    LSA_REQUIRE(bsgs_ratio >= 0, who + ": negative bsgs_ratio");
    (void)bfv_encode_tables(c, who.c_str());   // refuses a t that has no slots
    std::map<int, const u64*> mat;   // reduced index -> the caller's [2][period]
    for (int i = 0; i < n_diag; i++) {
        const int k = ((diag_index[i] % period) + period) % period;
        LSA_REQUIRE(!mat.count(k), who + ": diagonal index " + std::to_string(diag_index[i]) + " repeats another modulo the period");
        const u64* v = values + (size_t)i * 2 * period;
        for (int x = 0; x < 2 * period; x++)
            LSA_REQUIRE(v[x] < c.t, who + ": value " + std::to_string(v[x]) + " of diagonal " + std::to_string(diag_index[i]) + " is not below t");
        mat[k] = v;
    }
    auto lt = std::make_unique<BfvLinearTransform>(c);
    BtMatrix& bm = lt->m;
    bm.level = level;
    bm.period = period;
    bm.pt_scale = 1.0;
    for (auto& kv : mat) bm.ks.push_back(kv.first);
    bm.naive = bm.ks.size() < 3;
    bm.n1 = bm.naive ? period : bsgs_split(bm.ks, period, bsgs_ratio > 0 ? bsgs_ratio : 2.0);
    bm.rows = bfv_pt_rows(c, level, BFV_PT_EXT);
    const size_t N = (size_t)c.n, D = bm.ks.size();
    std::map<int, bool> babies, giants;
    std::vector<u64> rolled(D * N);   // rot_{-giant}(d_k) of both slot rows, tiled over the N/2 columns
    for (size_t i = 0; i < D; i++) {
        const int k = bm.ks[i], giant = (k / bm.n1) * bm.n1;
        babies[k - giant] = true;
        giants[giant] = true;
        const u64* d = mat.at(k);
        for (int row = 0; row < 2; row++)
            for (int col = 0; col < n; col++)
                rolled[i * N + (size_t)row * n + col] = d[(size_t)row * period + (((col - giant) % period) + period) % period];
    }
    lt->n_baby = (int)babies.size();
    lt->n_giant = (int)giants.size();
    lt->n_moddown = lt->n_giant - (giants.count(0) ? 1 : 0) + 1;
    std::map<u64, bool> gal;
    for (auto& kv : babies)
        if (kv.first % n) gal[galois_of_rotation(kv.first % n, c.n)] = true;
    for (auto& kv : giants)
        if (kv.first % n) gal[galois_of_rotation(kv.first % n, c.n)] = true;
    for (auto& kv : gal) lt->galois.push_back(kv.first);
    // nothing has touched the device so far
    c.use_device();
    const long long spt = (long long)bm.rows * (long long)N;
    LSA_HIP(hipMalloc((void**)&lt->plains_dev, D * (size_t)spt * sizeof(u64)));
    bfv_encode_rows(c, level, BFV_PT_EXT, rolled.data(), lt->plains_dev, spt, (int)D, s);   // the public encoder's path
    for (size_t i = 0; i < D; i++) bm.plains.push_back(lt->plains_dev + i * (size_t)spt);
    return lt.release();
}

void bfv_lt_run(BfvLinearTransform& lt, const u64* in, long long sin, u64* out, long long sout, int batch,
                const GaloisKeys& glk, hipStream_t s) {
    const std::string who = "lsa_bfv_linear_transform";
    Context& c = lt.c;
    const int level = lt.m.level, L = level + 1;
    const long long N = c.n;
    (void)glk.resolve(lt.galois, who, [&](u64 e, const Key& k) {   // every key before anything is queued
        LSA_REQUIRE(k.level >= level, who + ": the Galois key for element " + std::to_string(e) + " was exported at a lower level than the plan");
    });
    if (batch <= 0) return;
    LSA_REQUIRE(in && out, who + ": null argument");
    const size_t w = 2 * (size_t)L * N;
    const layout::Span sp_in = layout::span_of(in, sin, w), sp_out = layout::span_of(out, sout, w);
    LSA_REQUIRE(layout::stride_ok(sp_in, false), who + ": batch stride of in below one ciphertext");
    LSA_REQUIRE(layout::stride_ok(sp_out, false), who + ": batch stride of out below one ciphertext");
    LSA_REQUIRE(layout::aligned16(sp_in) && layout::aligned16(sp_out), who + ": in and out must be 16-byte aligned with even batch strides");
    LSA_REQUIRE(layout::apart(sp_out, sp_in, batch), who + ": out overlaps in");
    LtEval ev(c, lt.pool, s, batch, glk, who.c_str());
    ev.giant_scatter = lt_giant_scatter();
    // entrance: c0 and c1 into the NTT domain once; the decomposition reads c1's coefficients where they lie
    DCt x = ev.alloc(level, 1.0);
    launch_ntt(c, in, x.data(), batch, sin, ev.stride(level), 2 * L, ev.rm2(level), false, s);
    ev.c1_coef = in + (size_t)L * N;
    ev.s_coef = sin;
    ev.coeff_out = out;
    ev.s_coeff_out = sout;
    (void)ev.linear_transform_dh(x, lt.m, false);
}

}  // namespace lsa
