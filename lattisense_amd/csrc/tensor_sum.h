// tensor_sum.h — per-coefficient arithmetic of k_tensor_sum (kernels.hip): the degree-2 tensor of a sum of ciphertext pairs,
//   d0 = sum_i a0_i b0_i,   d1 = sum_i (a0_i b1_i + a1_i b0_i),   d2 = sum_i a1_i b1_i   mod q,
// every operand a canonical residue.  The products are summed as 128-bit integers V and reduced once per output: one REDC gives
// V * 2^-64 mod q in [0, 2q), one Montgomery multiply by r2 = 2^128 mod q takes the 2^-64 away and leaves the canonical residue.
//
// Fold bound.  The lazy REDC takes V < q * 2^64.  A product of canonical residues is at most (q - 1)^2, and with q < 2^61
// eight of them stay below q * 2^64 (8 q^2 < q * 2^64 <=> q < 2^61).  So d0 and d2 (one product per term) fold before term
// 8, 16, ... and d1 (two products per term) before term 4, 8, ...  A fold works in place, V = hi * 2^64 + lo  ->
// (hi * 2^64 mod q in [0, 2q)) + lo < 2^64 + 2q, by one lazy Montgomery multiply of hi by r2 (any 64-bit hi: hi * r2 < q * 2^64),
// so nothing but the three accumulators lives across terms.  After a fold eight more products still fit:
//   2^64 + 2q + 8 (q - 1)^2 < q * 2^64   <=>   8 q (2^61 - q) + 14 q > 2^64 + 8,
// which holds for every q in [2^29, 2^61) (at q = 2^61 - 1 the left side is 22 q; for smaller q the first term alone is far
// larger).  The sums this file is seeded with (ts_seed: a previous partial sum and an addend, each < q) take 2q of the same
// room, which the first eight products leave: 2q + 8 (q - 1)^2 < 8 q^2 < q * 2^64.
// Host and device compile the same functions (tests/cpp/test_tensor_sum.cpp).
#pragma once
#include "modarith.h"

#define LSA_DOT_MAX_TERMS 16   // ciphertext pairs of one k_tensor_sum launch; a longer sum continues in accumulating launches

struct TsAcc {   // the three 128-bit sums of one coefficient
    u64 h0, l0, h1, l1, h2, l2;
};
LSA_HD void ts_init(TsAcc& t) { t.h0 = t.l0 = t.h1 = t.l1 = t.h2 = t.l2 = 0; }
// V += v for a canonical residue v (the partial sum of an earlier launch, the addend): at most two per accumulator, before term 0
LSA_HD void ts_seed(u64& l, u64 v) { l += v; }   // l < 2q < 2^62 afterwards: no carry
LSA_HD void ts_fold(u64& h, u64& l, u64 q, u64 qinv, u64 r2) {
    const u64 x = mont_mul_lazy(h, r2, q, qinv);   // h * 2^64 mod q, [0, 2q)
    l += x;
    h = l < x ? 1 : 0;
}
// term i (counted from 0) of the sum
LSA_HD void ts_term(TsAcc& t, int i, u64 a0, u64 a1, u64 b0, u64 b1, const ModDev& m) {
    if (i && (i & 3) == 0) {
        ts_fold(t.h1, t.l1, m.q, m.qinv, m.r2);
        if ((i & 7) == 0) {
            ts_fold(t.h0, t.l0, m.q, m.qinv, m.r2);
            ts_fold(t.h2, t.l2, m.q, m.qinv, m.r2);
        }
    }
    mac128(t.h0, t.l0, a0, b0);
    mac128(t.h1, t.l1, a0, b1);
    mac128(t.h1, t.l1, a1, b0);
    mac128(t.h2, t.l2, a1, b1);
}
LSA_HD u64 ts_finish(u64 h, u64 l, const ModDev& m) {
    return mont_mul(mont_redc_lazy(h, l, m.q, m.qinv), m.r2, m.q, m.qinv);
}
