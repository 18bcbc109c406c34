// poly_lincomb.h — per-element arithmetic of k_poly_lincomb (kernels.hip): sum_i K_i * v_i mod q for up to 15 terms, the
// constants K_i in Montgomery form (K_i * 2^64 mod q), the values v_i canonical residues.  The products are summed as 128-bit
// integers and reduced once (one REDC gives sum K_i v_i mod q directly: the constants carry the 2^64); a ninth term folds the
// first eight first, because eight products of < q^2 with q < 2^61 are the most that stay below q * 2^64, which is what the
// lazy REDC takes.  Host and device compile the same functions (tests/cpp/test_poly_lincomb.cpp).
#pragma once
#include "modarith.h"

#define LSA_PLC_MAX_SRC 15   // sources of one launch (the baby powers 1..15 of log_baby = 4)
#define LSA_PLC_MAX_OUT 8    // outputs of one launch

struct PlcAcc {
    u64 h, l, r;   // running 128-bit sum of at most 8 products; reduced sum of the folded ones
};
LSA_HD void plc_init(PlcAcc& a) { a.h = a.l = a.r = 0; }
LSA_HD void plc_fold(PlcAcc& a, u64 q, u64 qinv) {
    a.r = add_mod(a.r, csub(mont_redc_lazy(a.h, a.l, q, qinv), q), q);
    a.h = a.l = 0;
}
// term i (counted from 0) of the sum
LSA_HD void plc_term(PlcAcc& a, int i, u64 v, u64 k_mont, u64 q, u64 qinv) {
    if (i == 8) plc_fold(a, q, qinv);
    mac128(a.h, a.l, v, k_mont);
}
LSA_HD u64 plc_finish(PlcAcc a, u64 q, u64 qinv) {
    plc_fold(a, q, qinv);
    return a.r;
}
