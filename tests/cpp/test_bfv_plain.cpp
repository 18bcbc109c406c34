// Host-side check of the per-word arithmetic of k_bfv_addsub_plain (lattisense_amd/csrc/bfv_plain.h; the kernel calls the same
// functions).  Lines on stdin, one answer line each on stdout:
//   "R t x"              -> bfv_plain_mod_t(x) = x mod t for any 64-bit x
//   "S t q qmt m c0"     -> "r u P ref w0 w1 w2": r = m mod t, u = (r qmt + floor(t/2)) mod t as the centred pair holds it,
//                           P = (u - floor(t/2)) (-t^-1) mod q, ref = bfv_poly_scale_up_word (bfv_poly.h) on the same word, and the
//                           ciphertext word c0 through op 0 (c0 + P), 1 (c0 - P) and 2 (P - c0)
// Driven by tests/test_bfv_plain_host.py, which compares with Python integers.
#include <cstdio>
#include "../../lattisense_amd/csrc/bfv_plain.h"
#include "../../lattisense_amd/csrc/bfv_poly.h"

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

static u64 pow_mod(u64 a, u64 e, u64 q) {
    u64 r = 1 % q;
    a %= q;
    for (; e; e >>= 1) {
        if (e & 1) r = (u64)((u128)r * a % q);
        a = (u64)((u128)a * a % q);
    }
    return r;
}

int main() {
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        unsigned long long t;
        if (std::scanf("%llu", &t) != 1) return 2;
        const u64 trec = (u64)((((u128)1) << 64) / t);
        if (kind == 'R') {
            unsigned long long x;
            if (std::scanf("%llu", &x) != 1) return 2;
            std::printf("%llu\n", (unsigned long long)bfv_plain_mod_t(x, t, trec));
        } else if (kind == 'S') {
            unsigned long long q, qmt, m, c0;
            if (std::scanf("%llu %llu %llu %llu", &q, &qmt, &m, &c0) != 4) return 2;
            const ModDev md = mod_of(q);
            const u64 t_inv = pow_mod(t % q, q - 2, q);                        // q is prime
            const u64 neg_tinv_mont = (u64)(((u128)(q - t_inv) << 64) % q);   // -(t^-1) in Montgomery form
            const BfvPlainWord w = bfv_plain_centre(m, t, trec, qmt);
            const u64 thalf = t >> 1;
            const u64 u = w.neg ? thalf - w.mag : thalf + w.mag;
            const u64 p = bfv_plain_scale_up(w, neg_tinv_mont, md);
            std::printf("%llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)bfv_plain_mod_t(m, t, trec), (unsigned long long)u,
                        (unsigned long long)p, (unsigned long long)lsa::bfv_poly_scale_up_word(m, t, qmt, q, t_inv),
                        (unsigned long long)bfv_plain_word<0>(c0, p, q), (unsigned long long)bfv_plain_word<1>(c0, p, q),
                        (unsigned long long)bfv_plain_word<2>(c0, p, q));
        } else {
            return 2;
        }
    }
    return 0;
}
