// ks_mac_multi.h — per-point arithmetic of k_ks_mac_multi and k_ext_sum (slot_sum.hip): the gadget inner product of ONE
// decomposition with K keys at once,
//   r[k][h] = sum_{d<beta} e_d * key_k[d][h]  * 2^-64 mod q      (k < K, h = 0, 1; keys in Montgomery form, e_d canonical),
// each digit value e_d loaded once and used for all 2K sums.  The sums are 128-bit integers reduced by one lazy REDC; with q < 2^61
// eight products of canonical residues stay below q * 2^64 (8 q^2 < q * 2^64), so after every eighth digit the sum is folded into
// the canonical running residue r -- the rule of k_ks_mac.  Every fold leaves a canonical residue and REDC is additive mod q, so the
// words do not depend on where the folds fall: K = 1 is k_ks_mac's result, and K keys at once are K single-key results.
// Host and device compile the same functions (tests/cpp/test_ks_mac_multi.cpp).
#pragma once
#include "modarith.h"

#define LSA_KSM_MAX_KEYS 4   // keys of one k_ks_mac_multi launch (slot_sum.h: LSA_SLOTSUM_MAX_KEYS)
#define LSA_KSM_FOLD 8       // digits between folds

template <int K>
struct KsmAcc {   // one point: sums 2k (first key half) and 2k+1 (second) of key k
    u64 h[2 * K], l[2 * K], r[2 * K];
};
template <int K>
LSA_HD void ksm_init(KsmAcc<K>& a) {
#pragma unroll
    for (int i = 0; i < 2 * K; i++) a.h[i] = a.l[i] = a.r[i] = 0;
}
template <int K>
LSA_HD void ksm_fold(KsmAcc<K>& a, const ModDev& m) {
#pragma unroll
    for (int i = 0; i < 2 * K; i++) {
        a.r[i] = add_mod(a.r[i], csub(mont_redc_lazy(a.h[i], a.l[i], m.q, m.qinv), m.q), m.q);
        a.h[i] = a.l[i] = 0;
    }
}
// digit d (counted from 0) of the decomposition: e times the two words k0[k], k1[k] of every key
template <int K>
LSA_HD void ksm_term(KsmAcc<K>& a, int d, u64 e, const u64* k0, const u64* k1, const ModDev& m) {
#pragma unroll
    for (int k = 0; k < K; k++) {
        mac128(a.h[2 * k], a.l[2 * k], e, k0[k]);
        mac128(a.h[2 * k + 1], a.l[2 * k + 1], e, k1[k]);
    }
    if ((d & (LSA_KSM_FOLD - 1)) == LSA_KSM_FOLD - 1) ksm_fold(a, m);
}
// after `terms` digits: the canonical residues are in a.r (a sum that ended on a fold has nothing left to reduce)
template <int K>
LSA_HD void ksm_finish(KsmAcc<K>& a, int terms, const ModDev& m) {
    if (terms & (LSA_KSM_FOLD - 1)) ksm_fold(a, m);
}
// + P * c0 on the first sum of every key (Q rows of polynomial 0): pm = P mod q in Montgomery form, c0 canonical
template <int K>
LSA_HD void ksm_add_base(KsmAcc<K>& a, u64 c0, u64 pm, const ModDev& m) {
    const u64 v = mont_mul(c0, pm, m.q, m.qinv);
#pragma unroll
    for (int k = 0; k < K; k++) a.r[2 * k] = add_mod(a.r[2 * k], v, m.q);
}
// k_ext_sum: v (+)= sum of n canonical residues
LSA_HD u64 ext_sum_point(u64 v, const u64* in, int n, u64 q) {
    for (int k = 0; k < n; k++) v = add_mod(v, in[k], q);
    return v;
}
