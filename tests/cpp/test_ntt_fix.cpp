// Host-side check of the scalar conversions around the NTT butterflies (lattisense_amd/csrc/ntt_core.h): the load fix
// (rescale / ModDown head: integer lift with and without `near`, the FP64 lift, the merged add, raw hand-off), the store fix
// (final reduction lazy / not lazy, the fused tails merged and unmerged, with and without base, raw hand-off reduced and
// unreduced), fp_modmul, fp_reduce, the product prologue and the FP64 sums of the tensor-fold key MAC -- against unsigned
// __int128 arithmetic, for every (target prime, dropped prime) pair of the chain given on the command line, on edge operands
// {0, 1, h-1, h, h+1, q-2, q-1}, the ends of the lazy ranges the callers hand in, and 10^5 random values per case.  Inside the
// FP64 paths every intermediate must be an integer below 2^53, and the tighter bounds the comments claim are asserted on the
// inputs the comments assume.  Compiled and run by tests/test_ntt_fix_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../lattisense_amd/csrc/ntt_core.h"

typedef unsigned __int128 u128;
typedef __int128 i128;
static u64 rng_state = 0x13198A2E03707344ull;
static u64 rnd() {
    u64 z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static u64 g_q, g_ql;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s (line %d) q=%llu ql=%llu\n", #c, __LINE__, (unsigned long long)g_q, (unsigned long long)g_ql); std::exit(1); } } while (0)
static const int RANDOM = 100000;
static const double P53 = 9007199254740992.0, P51 = 2251799813685248.0;

static ModDev make_mod(u64 q) {
    ModDev m;
    m.q = q;
    u64 x = q;   // Newton: q^-1 mod 2^64
    for (int i = 0; i < 6; i++) x *= 2 - q * x;
    m.qinv = x;
    m.r1 = (u64)((((u128)1) << 64) % q);
    m.r2 = (u64)(((u128)m.r1 * m.r1) % q);
    return m;
}
static u64 to_mont(u64 a, u64 q) { return (u64)((((u128)a) << 64) % q); }
static bool is_int(double x) { return std::fabs(x) < P53 && x == std::nearbyint(x); }
static u64 mod_i(i128 x, u64 q) {
    i128 r = x % (i128)q;
    return (u64)(r < 0 ? r + (i128)q : r);
}
static bool fp_prime(u64 q) { return (q >> LSA_FP64_MAX_BITS) == 0; }

// fp_modmul step by step: h + l is the exact product, c within 2 of the quotient, d and d + l integers below 2^53,
// |result| < 1.1 q; returns the library function's value
static double checked_modmul(double v, double w, u64 q) {
    const double qd = (double)q, qinv = 1.0 / qd;
    CHECK(is_int(v) && is_int(w) && std::fabs(v) < P51 && w >= 0 && w < qd);
    const double h = v * w, l = __builtin_fma(v, w, -h), c = __builtin_rint(h * qinv), d = __builtin_fma(-c, qd, h);
    CHECK(is_int(l) && is_int(c) && is_int(d) && is_int(d + l));
    CHECK((i128)h + (i128)l == (i128)v * (i128)w);
    CHECK((i128)d == (i128)h - (i128)c * (i128)q);
    const double r = fp_modmul(v, w, qd, qinv);
    CHECK(r == d + l && std::fabs(r) < 1.1 * qd);
    CHECK(mod_i((i128)r, q) == mod_i((i128)v * (i128)w, q));
    return r;
}
static double checked_reduce(double x, u64 q) {
    const double qd = (double)q;
    CHECK(is_int(x));
    const double r = fp_reduce(x, qd, 1.0 / qd);
    CHECK(is_int(r) && std::fabs(r) <= qd / 2 + 1 && mod_i((i128)r, q) == mod_i((i128)x, q));
    return r;
}

static std::vector<u64> edges(u64 q) {
    const u64 h = (q - 1) >> 1;
    return {0, 1, h - 1, h, h + 1, q - 2, q - 1};
}
// value it of a sweep: the edge list first, then random below `bound`
static u64 pick(const std::vector<u64>& e, int it, u64 bound) { return it < (int)e.size() ? e[it] : rnd() % bound; }

static void test_fp_primitives(u64 q) {
    g_q = q;
    g_ql = 0;
    const double qd = (double)q;
    const std::vector<u64> e = edges(q);
    const double vs[] = {0, 1, -1, qd - 1, -(qd - 1), 4 * qd - 1, -(4 * qd - 1), 22.7 * qd > P51 - 1 ? P51 - 1 : std::floor(22.7 * qd), P51 - 1, -(P51 - 1)};
    for (double v : vs)
        for (u64 w : e) checked_modmul(v, (double)w, q);
    for (int it = 0; it < RANDOM; it++) {
        const double v = (double)(rnd() >> 13) * (it & 1 ? 1.0 : -1.0);   // |v| < 2^51
        checked_modmul(v, (double)(rnd() % q), q);
        checked_reduce((double)(rnd() >> 11) * (it & 2 ? 1.0 : -1.0), q);   // |x| < 2^53
    }
    const double xs[] = {0, qd / 2 - 0.5, qd / 2 + 0.5, -(qd / 2 - 0.5), -(qd / 2 + 0.5), qd, -qd, P53 - 1, -(P53 - 1), P51, 22.0 * qd};
    for (double x : xs) checked_reduce(x, q);
    // the product prologue: canonical operands -> |.| <= q/2 + 1 (the raw hand-off range)
    NttProdFix p;
    p.pa = p.pb = nullptr;
    p.mi = make_mod(q);
    p.qd = qd;
    p.qinvd = 1.0 / qd;
    for (int fp = 0; fp < 2; fp++) {
        p.fp = fp != 0;
        for (int it = 0; it < RANDOM + 49; it++) {
            const u64 x = it < 49 ? e[it / 7] : rnd() % q, y = it < 49 ? e[it % 7] : rnd() % q;
            const u64 want = (u64)(((u128)x * y) % q), got = ntt_prod_fix(p, x, y);
            if (fp) {
                const double r = d_from_bits(got);
                CHECK(is_int(r) && std::fabs(r) <= qd / 2 + 1 && mod_i((i128)r, q) == want);
            } else {
                CHECK(got == want);
            }
        }
    }
    // A MODEL of the fused key MAC's FP64 sums, not the kernel's code (r16_mac_digit is device-only): beta digits' terms plus
    // the tensor fold's two or three, every term an fp_modmul value.  With beta T <= 192 and T >= beta + 1 the fused kernel runs
    // beta <= 13, so at most 16 terms below 1.1 q each.  The first factor of a term is a canonical residue (the own digit, the
    // fold's operands) or an unreduced transform output of magnitude below 11 q (the other digits): both are run here.  The
    // kernel itself is compared with the oracle at beta = 13 in tests/test_gpu_boundary.py::test_digit_structure_edges.
    CHECK(16 * 1.1 * qd < P53);
    for (int pat = 0; pat < 3; pat++) {
        double acc = 0;
        for (int d = 0; d < 16; d++) {
            const u64 x = pat == 0 ? q - 1 : pat == 1 ? (q - 1) / 2 + (d & 1) : rnd() % q;
            const u64 k = pat == 0 ? (d & 1 ? q - 1 : 1) : pat == 1 ? q - 2 : rnd() % q;
            const double first = d & 2 ? std::floor(11 * qd) - (double)x : checked_modmul((double)x, (double)(q - 1), q);
            acc += checked_modmul(d & 4 ? -first : first, (double)k, q);
            CHECK(is_int(acc));
        }
        checked_reduce(acc, q);
    }
}

// the load-side constants as the kernel derives them (ntt_make_load_fix): the selectors under test are the library's own
static NttLoadFix make_load(u64 qi, u64 ql, bool head, bool add, bool allow_fp, bool raw) {
    static ModDev mods[2];
    static u64 dummy[2];
    mods[0] = make_mod(qi);
    mods[1] = make_mod(ql ? ql : qi);
    NttPassArgs a = NttPassArgs();
    a.src = a.fz_last = dummy;
    a.mods = mods;
    a.fz_ql_mod = 1;
    a.fz_limbs = 1;
    a.fz_pro = head ? (add ? 2 : 1) : 0;
    a.fz_first = 1;
    a.fp_raw_in = raw ? 1 : 0;
    NttBlockCtx bc = NttBlockCtx();
    bc.mod = 0;
    bc.fp = allow_fp && fp_prime(qi);
    const u64* g;
    const u64* gl;
    return ntt_make_load_fix<true>(a, bc, g, gl);
}
static int n_near[2], n_lift[2];
static void test_load(u64 qi, u64 ql) {
    g_q = qi;
    g_ql = ql;
    const u64 h = (ql - 1) >> 1;
    const std::vector<u64> et = edges(ql), ev = edges(qi);
    for (int allow_fp = 0; allow_fp < 2; allow_fp++)
        for (int add = 0; add < 2; add++) {
            const NttLoadFix f = make_load(qi, ql, true, add != 0, allow_fp != 0, false);
            n_near[f.near]++;
            if (f.fp) n_lift[f.fp_lift]++;
            for (int it = 0; it < RANDOM + 49; it++) {
                const u64 t = it < 49 ? et[it / 7] : rnd() % ql, v = it < 49 ? ev[it % 7] : rnd() % qi;
                const i128 centred = t <= h ? (i128)t : (i128)t - (i128)ql;
                const u64 want = mod_i(centred + (add ? (i128)v : 0), qi);
                const u64 got = ntt_load_fix(f, v, t);
                if (f.fp) {
                    const double r = d_from_bits(got);
                    CHECK(is_int(r) && mod_i((i128)r, qi) == want);
                    // the comment's bound: |in| < q + q_l / 2 < 2^48.6 for the lift, canonical otherwise
                    if (f.fp_lift) CHECK(std::fabs(r) < (double)qi + (double)ql / 2 && std::fabs(r) < 4.3e14);
                    else CHECK(r >= 0 && r < (double)qi);
                } else {
                    CHECK(got == want);
                }
            }
        }
    // no head: FP64-engine limbs take canonical or lazy (< 4q) words as exact doubles, raw hand-offs as they are
    const NttLoadFix p = make_load(qi, 0, false, false, true, false), r = make_load(qi, 0, false, false, true, true);
    const u64 ws[] = {0, 1, qi - 1, qi, 2 * qi, 4 * qi - 1, rnd() % (4 * qi)};
    for (u64 w : ws) {
        if (p.fp) CHECK(d_from_bits(ntt_load_fix(p, w, w)) == (double)w && (double)w < 4503599627370496.0);
        else CHECK(ntt_load_fix(p, w, w) == w);
        const u64 bits = d_to_bits(-(double)(w >> 3));
        CHECK(ntt_load_fix(r, bits, bits) == bits);
    }
}

static void test_store(u64 q) {
    g_q = q;
    g_ql = 0;
    const ModDev md = make_mod(q);
    const double qd = (double)q;
    const std::vector<u64> e = edges(q);
    const u64 k = e[(q >> 3) % 5 + 2], k2 = q - 1 - (q >> 7) % 1000;
    for (int variant = 0; variant < 5; variant++) {   // 0 plain, 1 tail, 2 tail + base, 3 merged, 4 merged + base
        NttStoreFix f;
        f.q = q;
        f.qinv = md.qinv;
        f.qd = qd;
        f.qinvd = 1.0 / qd;
        f.tail = variant >= 1;
        f.with_base = variant == 2 || variant == 4;
        f.merged = variant >= 3;
        f.k = to_mont(k, q);
        f.k2 = to_mont(k2, q);
        f.kd = (double)mont_mul(f.k, 1, q, md.qinv);   // as ntt_make_store_fix derives the plain factors
        f.k2d = (double)mont_mul(f.k2, 1, q, md.qinv);
        CHECK(f.kd == (double)k && f.k2d == (double)k2);
        f.one_s = (u64)((((u128)1) << 64) / q);
        f.final_reduce = true;
        f.raw = false;
        for (int fp = 0; fp < (fp_prime(q) ? 2 : 1); fp++)
            for (int inverse = 0; inverse < 2; inverse++) {
                f.fp = fp != 0;
                f.lazy = !f.fp && !inverse && ntt_int_lazy(q);
                f.skip_reduce = f.fp && inverse;
                // what the butterflies hand in: FP64 forward below 22.7 q (and below the engine's 2^51), inverse reduced
                // (|.| <= q/2 + 1); integer lazy forward anything below 2^64, otherwise below 8q (forward) / 4q (inverse)
                const double fp_bound = inverse ? std::floor(qd / 2) + 1 : std::fmin(std::floor(22.7 * qd), P51 - 1);
                for (int it = 0; it < RANDOM + 64; it++) {
                    const u64 va = pick(e, it % 8, q), vb = pick(e, (it / 8) % 8, q);
                    i128 x;
                    u64 in;
                    if (f.fp) {
                        double xd = it < 4 ? (it & 1 ? fp_bound : -fp_bound) : it < 8 ? (double)(it - 6) : std::floor(((double)(rnd() >> 11) / P53 * 2 - 1) * fp_bound);
                        if (it >= 8 && it < 16) xd = (it & 1 ? 1 : -1) * std::floor(qd / 2 + (it - 12));
                        if (std::fabs(xd) > fp_bound) xd = fp_bound;
                        x = (i128)xd;
                        in = d_to_bits(xd);
                    } else {
                        const u64 bound = f.lazy ? 0 : (inverse ? 4 : 8) * q;
                        in = f.lazy ? (it < 4 ? ~0ull - it : rnd()) : (it < 4 ? bound - 1 - it : it < 16 ? (u64)(it / 2) * q - (it & 1) * (it > 1) : rnd() % bound);
                        x = (i128)in;
                    }
                    const u64 xr = mod_i(x, q);
                    u64 want = xr;
                    if (f.tail && !f.merged) want = (u64)(((u128)((va + q - xr) % q) * k + (f.with_base ? vb : 0)) % q);
                    if (f.tail && f.merged) want = (u64)(((u128)((u64)(((u128)va * k) % q) + q - xr + (f.with_base ? vb : 0)) % q * k2) % q);
                    CHECK(ntt_store_fix(f, in, va, vb) == want);
                }
            }
    }
    if (!fp_prime(q)) return;
    // the raw hand-off of a forward first pass: below 2^46 the value is stored as it is (and must stay below the engine's
    // 2^51 over the whole transform: |in| < 4q, + 1.1q per stage over <= 17 stages), above it is reduced to |.| <= q/2 + 1
    NttStoreFix f;
    f.fp = f.raw = true;
    f.final_reduce = f.tail = f.with_base = f.merged = f.lazy = false;
    f.q = q;
    f.qd = qd;
    f.qinvd = 1.0 / qd;
    {   // the selector as the kernel derives it
        ModDev mods[1] = {md};
        u64 dummy[2] = {0, 0};
        NttPassArgs a = NttPassArgs();
        a.dst = dummy;
        a.mods = mods;
        a.tw = dummy;
        a.fp_raw_out = 1;
        NttBlockCtx bc = NttBlockCtx();
        bc.fp = 1;
        u64* g;
        const u64* pa;
        const u64* pb;
        const NttStoreFix s = ntt_make_store_fix<false>(a, bc, g, pa, pb);
        CHECK(s.fp && s.raw && !s.tail && !s.lazy);
        f.skip_reduce = s.skip_reduce;
    }
    if (f.skip_reduce) CHECK((4 + 17 * 1.1) * qd < P51);
    else CHECK((qd / 2 + 1 + 9 * 1.1 * qd) < P51);   // reduced hand-off, then a second pass of at most nine stages
    for (int it = 0; it < RANDOM; it++) {
        const double bound = std::floor((4 + 9 * 1.1) * qd);   // a first pass of at most nine stages
        const double xd = it < 2 ? (it ? bound : -bound) : std::floor(((double)(rnd() >> 11) / P53 * 2 - 1) * bound);
        const double r = d_from_bits(ntt_store_fix(f, d_to_bits(xd), 0, 0));
        if (f.skip_reduce) CHECK(r == xd);
        else CHECK(is_int(r) && std::fabs(r) <= qd / 2 + 1 && mod_i((i128)r, q) == mod_i((i128)xd, q));
    }
}

int main(int argc, char** argv) {
    std::vector<u64> primes;
    for (int i = 1; i < argc; i++) primes.push_back(std::strtoull(argv[i], nullptr, 10));
    if (primes.size() < 2) {
        std::printf("usage: test_ntt_fix prime prime ...\n");
        return 2;
    }
    for (u64 q : primes) {
        if (fp_prime(q)) test_fp_primitives(q);
        test_store(q);
        for (u64 ql : primes)
            if (ql != q) test_load(q, ql);
    }
    std::printf("pairs near=%d far=%d fp_lift=%d no_lift=%d\n", n_near[1], n_near[0], n_lift[1], n_lift[0]);
    if (!n_near[0] || !n_near[1] || !n_lift[0] || !n_lift[1]) {
        std::printf("FAIL the chain does not reach both values of near and fp_lift\n");
        return 1;
    }
    std::printf("OK ntt_fix\n");
    return 0;
}
