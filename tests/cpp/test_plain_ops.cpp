// Host-side check of the per-word arithmetic of k_lift_i64 and k_cconst (lattisense_amd/csrc/plain_ops.h; the kernels and the
// operator's constant formation call the same functions).  Lines on stdin, one answer line each on stdout:
//   "L q v"                       -> lift_i64(v) = v mod q in [0, q), v signed
//   "C q I kre kim bre bim w"     -> "kp km bp bm mul+ mul- add+ add- aff+ aff-": the constant pairs of (kre, kim) and (bre, bim)
//                                    and the word w through the mul, add and mul+add variants with the plus / minus constants
// Driven by tests/test_plain_ops_host.py, which compares with Python integers.
#include <cstdio>
#include "../../lattisense_amd/csrc/plain_ops.h"

typedef unsigned __int128 u128;

static u64 qinv_of(u64 q) {   // q^-1 mod 2^64 by Newton's iteration
    u64 x = q;
    for (int i = 0; i < 6; i++) x *= 2 - q * x;
    return x;
}

static ModDev mod_of(u64 q) {
    ModDev m;
    m.q = q;
    m.qinv = qinv_of(q);
    m.r1 = (u64)((((u128)1) << 64) % q);
    m.r2 = (u64)(((u128)m.r1 * m.r1) % q);
    return m;
}

int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        unsigned long long q;
        if (std::scanf("%llu", &q) != 1) return 2;
        const ModDev m = mod_of(q);
        if (kind == 'L') {
            long long v;
            if (std::scanf("%lld", &v) != 1) return 2;
            std::printf("%llu\n", (unsigned long long)lift_i64(v, m));
        } else if (kind == 'C') {
            unsigned long long I, w;
            long long kre, kim, bre, bim;
            if (std::scanf("%llu %lld %lld %lld %lld %llu", &I, &kre, &kim, &bre, &bim, &w) != 6) return 2;
            const CconstPair k = cconst_pair(kre, kim, I, m), b = cconst_pair(bre, bim, I, m);
            const u64 kp = cconst_to_mont(k.plus, m), km = cconst_to_mont(k.minus, m);
            std::printf("%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)k.plus, (unsigned long long)k.minus,
                        (unsigned long long)b.plus, (unsigned long long)b.minus,
                        (unsigned long long)cconst_word<true, false>(w, kp, 0, m), (unsigned long long)cconst_word<true, false>(w, km, 0, m),
                        (unsigned long long)cconst_word<false, true>(w, 0, b.plus, m), (unsigned long long)cconst_word<false, true>(w, 0, b.minus, m),
                        (unsigned long long)cconst_word<true, true>(w, kp, b.plus, m), (unsigned long long)cconst_word<true, true>(w, km, b.minus, m));
        } else {
            return 2;
        }
    }
    return 0;
}
