// plain_ops.h — per-word arithmetic of the CKKS plaintext / constant operands (kernels.hip k_lift_i64, k_cconst; ops.hip forms
// the constants with the same functions on the host).
//
// lift_i64: the residue of a signed 64-bit integer.  An encoded coefficient is round(m * scale), |v| < 4.6e18 < 2^63
// (round_even refuses more), so |v| fits an unsigned word: reduce it (reduce_u64 takes any 64-bit value) and negate.
//
// Complex constants.  The slot-wise constant a + b i is the polynomial a + b X^(N/2), and in the NTT domain X^(N/2) takes only
// the two values +-I, I = psi^(N/2), I^2 = -1 mod q (psi^e with e odd: I^e = I for e = 1, -I for e = 3 mod 4).  So
//   ct x (kre + kim X^(N/2))  =  ct[x] * (kre +- kim I)  per point:
// two constants per limb, k+ = kre + kim I and k- = kre - kim I, selected by the point.  cconst_pair forms them as canonical
// residues from the rounded integers; a multiplier goes to the kernel in Montgomery form (cconst_to_mont), so a word costs one
// Montgomery multiply: v * (k 2^64) * 2^-64 = v k mod q, canonical -- the residue mul_mod(v, k) gives.  An addend stays a plain
// residue.  Host and device compile the same functions (tests/cpp/test_plain_ops.cpp).
#pragma once
#include "modarith.h"

#define LSA_CCONST_MAX_LIMBS 64   // limbs whose constants ride in k_cconst's argument struct

// v mod q in [0, q), signed v with |v| < 2^63
LSA_HD u64 lift_i64(long long v, const ModDev& m) {
    const bool neg = v < 0;
    const u64 a = neg ? (u64)0 - (u64)v : (u64)v;
    const u64 r = reduce_u64(a, m);
    return neg ? neg_mod(r, m.q) : r;
}

struct CconstPair {   // kre + kim I and kre - kim I, canonical residues
    u64 plus, minus;
};
LSA_HD CconstPair cconst_pair(long long kre, long long kim, u64 I, const ModDev& m) {
    const u64 a = lift_i64(kre, m);
    const u64 t = mul_mod(lift_i64(kim, m), I, m);
    CconstPair p;
    p.plus = add_mod(a, t, m.q);
    p.minus = sub_mod(a, t, m.q);
    return p;
}
LSA_HD u64 cconst_to_mont(u64 k, const ModDev& m) { return mont_mul(k, m.r2, m.q, m.qinv); }
struct CconstLimb {   // one limb's constants as k_cconst takes them: multipliers in Montgomery form, addends plain residues
    u64 k_plus, k_minus, b_plus, b_minus;
};

// one word: v * k (MUL; k_mont in Montgomery form) + beta (ADD; a canonical residue), v canonical
template <bool MUL, bool ADD>
LSA_HD u64 cconst_word(u64 v, u64 k_mont, u64 beta, const ModDev& m) {
    const u64 r = MUL ? mont_mul(v, k_mont, m.q, m.qinv) : v;
    return ADD ? add_mod(r, beta, m.q) : r;
}
