// Host-side check of the per-point arithmetic of k_ks_mac_multi and k_ext_sum (lattisense_amd/csrc/ks_mac_multi.h; the kernels
// call the same functions).  Stand-alone: generates its own cases and compares with unsigned __int128 arithmetic.
//   K = 1..4 keys, beta in {1, 2, 8, 9, 17} digits (9 and 17 cross the fold-every-8 rule), moduli at 2^61 - small, around 2^40 and
//   at 2^30, digit values / key words / c0 all at q - 1 (the largest 128-bit sums), all zero, and random;
//   r[k][h] = sum_d e_d * key_k[d][h] * 2^-64 (+ P c0 on h = 0) mod q against __int128;
//   K keys at once == K single-key evaluations, word for word;
//   ext_sum_point against __int128.
// Prints "ok <cases>" and returns 0, or the first mismatch and 1.  Driven by tests/test_ks_mac_multi_host.py (plain and with
// -fsanitize=address,undefined).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../lattisense_amd/csrc/ks_mac_multi.h"

typedef unsigned __int128 u128;

static u64 qinv_of(u64 q) {   // q^-1 mod 2^64 by Newton's iteration
    u64 x = q;
    for (int i = 0; i < 6; i++) x *= 2 - q * x;
    return x;
}
static u64 pow_mod(u64 b, u64 e, u64 q) {
    u64 r = 1;
    for (b %= q; e; e >>= 1, b = (u64)((u128)b * b % q))
        if (e & 1) r = (u64)((u128)r * b % q);
    return r;
}
static u64 rng_state = 0x243F6A8885A308D3ull;
static u64 rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

static long cases = 0;

template <int K>
static bool run(const ModDev& m, int beta, int fill) {
    const u64 q = m.q;
    auto val = [&]() { return fill == 0 ? q - 1 : fill == 1 ? 0 : rnd() % q; };
    std::vector<u64> e(beta), k0((size_t)beta * K), k1((size_t)beta * K);
    for (auto& v : e) v = val();
    for (auto& v : k0) v = val();
    for (auto& v : k1) v = val();
    const u64 c0 = val(), pm = val();
    const u64 rinv = pow_mod((u64)(((u128)1 << 64) % q), q - 2, q);   // 2^-64 mod q (q prime)
    KsmAcc<K> a;
    ksm_init(a);
    for (int d = 0; d < beta; d++) ksm_term(a, d, e[d], &k0[(size_t)d * K], &k1[(size_t)d * K], m);
    ksm_finish(a, beta, m);
    ksm_add_base(a, c0, pm, m);
    const u64 base = (u64)((u128)c0 * pm % q * rinv % q);
    for (int k = 0; k < K; k++) {
        u128 s0 = 0, s1 = 0;   // sums mod q of the plain products
        for (int d = 0; d < beta; d++) {
            s0 = (s0 + (u128)e[d] * k0[(size_t)d * K + k] % q) % q;
            s1 = (s1 + (u128)e[d] * k1[(size_t)d * K + k] % q) % q;
        }
        const u64 w0 = (u64)(((u128)(u64)s0 * rinv + base) % q), w1 = (u64)((u128)(u64)s1 * rinv % q);
        // the same key on its own
        KsmAcc<1> b;
        ksm_init(b);
        for (int d = 0; d < beta; d++) ksm_term(b, d, e[d], &k0[(size_t)d * K + k], &k1[(size_t)d * K + k], m);
        ksm_finish(b, beta, m);
        ksm_add_base(b, c0, pm, m);
        if (a.r[2 * k] != w0 || a.r[2 * k + 1] != w1 || b.r[0] != w0 || b.r[1] != w1) {
            std::printf("mismatch: q=%llu K=%d beta=%d fill=%d key=%d got %llu %llu single %llu %llu want %llu %llu\n", (unsigned long long)q, K,
                        beta, fill, k, (unsigned long long)a.r[2 * k], (unsigned long long)a.r[2 * k + 1], (unsigned long long)b.r[0],
                        (unsigned long long)b.r[1], (unsigned long long)w0, (unsigned long long)w1);
            return false;
        }
        cases++;
    }
    return true;
}

int main() {
    // primes: three at the 61-bit ceiling (2^61 - 1, 2^61 - 2^21 + 1, 2^61 - 7 * 2^19 + 1), 2^40 + ..., 2^45 + ..., 2^30 - 35
    const u64 primes[] = {0x1fffffffffffffffull, 0x1fffffffffe00001ull, 0x1fffffffffc80001ull, 1099511922689ull, 35184372121601ull, (1ull << 30) - 35};
    const int betas[] = {1, 2, 8, 9, 17};
    for (u64 q : primes) {
        ModDev m;
        m.q = q;
        m.qinv = qinv_of(q);
        m.r1 = (u64)((((u128)1) << 64) % q);
        m.r2 = (u64)(((u128)m.r1 * m.r1) % q);
        for (int beta : betas)
            for (int fill = 0; fill < 3; fill++)
                for (int rep = 0; rep < (fill == 2 ? 50 : 1); rep++)
                    if (!run<1>(m, beta, fill) || !run<2>(m, beta, fill) || !run<3>(m, beta, fill) || !run<4>(m, beta, fill)) return 1;
        for (int n = 0; n <= 3; n++)
            for (int fill = 0; fill < 3; fill++) {
                u64 in[3];
                for (auto& v : in) v = fill == 0 ? q - 1 : fill == 1 ? 0 : rnd() % q;
                const u64 v0 = fill == 0 ? q - 1 : rnd() % q;
                u128 want = v0;
                for (int k = 0; k < n; k++) want += in[k];
                if (ext_sum_point(v0, in, n, q) != (u64)(want % q)) {
                    std::printf("ext_sum mismatch: q=%llu n=%d fill=%d\n", (unsigned long long)q, n, fill);
                    return 1;
                }
                cases++;
            }
    }
    std::printf("ok %ld\n", cases);
    return 0;
}
