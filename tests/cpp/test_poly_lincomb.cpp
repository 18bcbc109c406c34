// Host-side check of k_poly_lincomb's per-element arithmetic (lattisense_amd/csrc/poly_lincomb.h; the kernel calls the same
// functions): lines "q nterms v_0 .. k_0 .." on stdin, one "r" per line on stdout with r = sum_i k_i v_i mod q, the constants
// converted to Montgomery form here as the plan does.  Driven by tests/test_poly_lincomb_host.py, which compares with Python
// integers on worst-case residues (every v and k equal to q - 1, 15 terms, primes of 30 to 61 bits).
#include <cstdio>
#include <vector>
#include "../../lattisense_amd/csrc/poly_lincomb.h"

typedef unsigned __int128 u128;

static u64 qinv_of(u64 q) {   // q^-1 mod 2^64 by Newton's iteration
    u64 x = q;
    for (int i = 0; i < 6; i++) x *= 2 - q * x;
    return x;
}

int main() {
    unsigned long long q;
    int n;
    while (std::scanf("%llu %d", &q, &n) == 2) {
        if (n < 1 || n > LSA_PLC_MAX_SRC) return 2;
        std::vector<u64> v(n), k(n);
        for (int i = 0; i < n; i++) {
            unsigned long long t;
            if (std::scanf("%llu", &t) != 1) return 2;
            v[i] = t;
        }
        for (int i = 0; i < n; i++) {
            unsigned long long t;
            if (std::scanf("%llu", &t) != 1) return 2;
            k[i] = (u64)((((u128)t) << 64) % q);
        }
        const u64 qinv = qinv_of(q);
        PlcAcc a;
        plc_init(a);
        for (int i = 0; i < n; i++) plc_term(a, i, v[i], k[i], q, qinv);
        std::printf("%llu\n", (unsigned long long)plc_finish(a, q, qinv));
    }
    return 0;
}
