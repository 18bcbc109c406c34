// Host-side check of the merged ModDown + rescale tail of an FP64-engine limb (lattisense_amd/csrc/ntt_core.h, fp_merged_tail) --
// the one function both the epilogue pass and the tail variant of the fused key MAC store through -- against 128-bit integer
// arithmetic, for the moduli given on the command line (all below 2^47):
//   wide form (the key MAC's running sums): sums at the ends of the stated range (+-(2^53 - 1)), at +-(beta + 2) * 1.1 q for
//     every beta the fused kernel runs (1..13) and one either side of each, x at +-11 q, at the ends of its range and around
//     the multiples of q / 2 where fp_reduce changes its quotient, and random values of both over the whole range;
//   narrow form (the epilogue pass): x over [-q/2 - 1, q/2 + 1], canonical sums and base words;
//   the two forms on the same point: the same residue.
// Factors kd, k2d: 0, 1, q - 1, (q - 1) / 2 and random.  Built with -fsanitize=address,undefined and run by
// tests/test_ks_tail_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../lattisense_amd/csrc/ntt_core.h"

typedef __int128 i128;
static u64 rng_state = 0x243F6A8885A308D3ull;
static u64 rnd() {
    u64 z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static u64 g_q;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s (line %d) q=%llu\n", #c, __LINE__, (unsigned long long)g_q); std::exit(1); } } while (0)
static const long long P53 = 1LL << 53;

static u64 mod_i(i128 x, u64 q) {
    i128 r = x % (i128)q;
    return (u64)(r < 0 ? r + (i128)q : r);
}
// ((sum * kd - x + bd) * k2d) mod q, canonical
static u64 want(long long x, long long sum, u64 bd, u64 kd, u64 k2d, u64 q) {
    const u64 inner = mod_i((i128)sum * (i128)kd - (i128)x + (i128)bd, q);
    return mod_i((i128)inner * (i128)k2d, q);
}
static long long rnd_signed(long long bound) {   // uniform in (-bound, bound)
    const long long v = (long long)(rnd() % (u64)bound);
    return (rnd() & 1) ? -v : v;
}

static void test_modulus(u64 q) {
    g_q = q;
    CHECK((q >> LSA_FP64_MAX_BITS) == 0 && q > 16);
    const double qd = (double)q, qinv = 1.0 / qd;
    const long long ql = (long long)q;
    std::vector<u64> factors = {0, 1, q - 1, (q - 1) / 2};
    for (int i = 0; i < 4; i++) factors.push_back(rnd() % q);

    std::vector<long long> sums = {0, 1, -1, P53 - 1, -(P53 - 1), ql, -ql, ql / 2, -(ql / 2), ql / 2 + 1, -(ql / 2 + 1)};
    for (int beta = 1; beta <= 13; beta++) {
        const long long top = (long long)std::floor((beta + 2) * 1.1 * qd);
        for (long long d = -1; d <= 1; d++) {
            sums.push_back(top + d);
            sums.push_back(-(top + d));
        }
    }
    for (long long m = 0; m <= 32; m++)   // around the multiples of q / 2: where fp_reduce's quotient steps
        for (long long d = -1; d <= 1; d++) {
            sums.push_back(m * ql / 2 + d);
            sums.push_back(-(m * ql / 2 + d));
        }
    std::vector<long long> xs = {0, 1, -1, 11 * ql, -11 * ql, 11 * ql - 1, -(11 * ql - 1), P53 - 1, -(P53 - 1), ql / 2, -(ql / 2), ql / 2 + 1, -(ql / 2 + 1)};
    for (long long m = 0; m <= 22; m++)
        for (long long d = -1; d <= 1; d++) {
            xs.push_back(m * ql / 2 + d);
            xs.push_back(-(m * ql / 2 + d));
        }

    auto wide_point = [&](long long x, long long sum, u64 kd, u64 k2d) {
        CHECK(std::llabs(x) < P53 && std::llabs(sum) < P53);
        const u64 got = fp_merged_tail((double)x, (double)sum, 0.0, (double)kd, (double)k2d, qd, qinv, true);
        CHECK(got < q);
        CHECK(got == want(x, sum, 0, kd, k2d, q));
        // the epilogue pass on the same point: the reduced transform value and the canonical accumulator word
        const double xr = fp_reduce((double)x, qd, qinv);
        CHECK(std::fabs(xr) <= qd / 2 + 1);
        const u64 narrow = fp_merged_tail(xr, (double)mod_i(sum, q), 0.0, (double)kd, (double)k2d, qd, qinv, false);
        CHECK(narrow == got);
    };
    for (u64 kd : factors)
        for (u64 k2d : factors) {
            for (long long s : sums)
                for (long long x : xs) wide_point(x, s, kd, k2d);
            for (int it = 0; it < 2000; it++) wide_point(rnd_signed(P53), rnd_signed(P53), kd, k2d);
            for (int it = 0; it < 2000; it++) wide_point(rnd_signed(11 * ql), rnd_signed((long long)(15 * 1.1 * qd)), kd, k2d);
        }

    // narrow form with a base word (the unfolded merged tail)
    const std::vector<long long> xn = {0, 1, -1, ql / 2, -(ql / 2), ql / 2 + 1, -(ql / 2 + 1)};
    const std::vector<u64> words = {0, 1, (q - 1) / 2, q - 2, q - 1};
    for (u64 kd : factors)
        for (u64 k2d : factors) {
            for (long long x : xn)
                for (u64 a : words)
                    for (u64 b : words)
                        CHECK(fp_merged_tail((double)x, (double)a, (double)b, (double)kd, (double)k2d, qd, qinv, false) == want(x, (long long)a, b, kd, k2d, q));
            for (int it = 0; it < 2000; it++) {
                const long long x = rnd_signed(ql / 2 + 2);
                const u64 a = rnd() % q, b = rnd() % q;
                CHECK(fp_merged_tail((double)x, (double)a, (double)b, (double)kd, (double)k2d, qd, qinv, false) == want(x, (long long)a, b, kd, k2d, q));
            }
        }
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: test_ks_tail q...\n");
        return 2;
    }
    for (int i = 1; i < argc; i++) test_modulus(std::strtoull(argv[i], nullptr, 10));
    std::printf("OK ks_tail %d moduli\n", argc - 1);
    return 0;
}
