// Host-side check of k_tensor_sum's per-coefficient arithmetic (lattisense_amd/csrc/tensor_sum.h; the kernel calls the same
// functions): lines "mode q n a0_0 .. a1_0 .. b0_0 .. b1_0 .. e0 e1" on stdin, one "d0 d1 d2" per line on stdout with
// d0 = e0 + sum a0 b0, d1 = e1 + sum (a0 b1 + a1 b0), d2 = sum a1 b1 mod q.  mode 0: one run of ts_term over all n terms (every
// fold boundary); mode 1: as the operator launches the kernel -- LSA_DOT_MAX_TERMS terms at a time, the addend (e0, e1) seeding
// the first launch and every later launch seeded with the finished residues of the one before.  "--max-terms" prints
// LSA_DOT_MAX_TERMS.  Driven by tests/test_tensor_sum_host.py, which compares with Python integers.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../lattisense_amd/csrc/tensor_sum.h"

typedef unsigned __int128 u128;

static u64 qinv_of(u64 q) {   // q^-1 mod 2^64 by Newton's iteration
    u64 x = q;
    for (int i = 0; i < 6; i++) x *= 2 - q * x;
    return x;
}

static bool read(std::vector<u64>& v) {
    for (auto& x : v) {
        unsigned long long t;
        if (std::scanf("%llu", &t) != 1) return false;
        x = t;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--max-terms")) {
        std::printf("%d\n", LSA_DOT_MAX_TERMS);
        return 0;
    }
    int mode, n;
    unsigned long long q;
    while (std::scanf("%d %llu %d", &mode, &q, &n) == 3) {
        if (n < 1 || mode < 0 || mode > 1) return 2;
        std::vector<u64> a0(n), a1(n), b0(n), b1(n), e(2);
        if (!read(a0) || !read(a1) || !read(b0) || !read(b1) || !read(e)) return 2;
        ModDev m;
        m.q = q;
        m.qinv = qinv_of(q);
        m.r1 = (u64)((((u128)1) << 64) % q);
        m.r2 = (u64)(((u128)m.r1 * m.r1) % q);
        const int step = mode == 0 ? n : LSA_DOT_MAX_TERMS;
        u64 d[3] = {e[0], e[1], 0};
        for (int i0 = 0; i0 < n; i0 += step) {
            TsAcc t;
            ts_init(t);
            ts_seed(t.l0, d[0]);
            ts_seed(t.l1, d[1]);
            ts_seed(t.l2, d[2]);
            for (int i = i0; i < n && i < i0 + step; i++) ts_term(t, i - i0, a0[i], a1[i], b0[i], b1[i], m);
            d[0] = ts_finish(t.h0, t.l0, m);
            d[1] = ts_finish(t.h1, t.l1, m);
            d[2] = ts_finish(t.h2, t.l2, m);
        }
        std::printf("%llu %llu %llu\n", (unsigned long long)d[0], (unsigned long long)d[1], (unsigned long long)d[2]);
    }
    return 0;
}
