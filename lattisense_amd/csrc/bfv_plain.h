// bfv_plain.h — per-word arithmetic of the BFV ring-t plaintext operand (bfv_plain.hip k_bfv_addsub_plain): Lattigo's scaleUp of
// one plaintext coefficient and its sum with / difference from a ciphertext word.  With m the plaintext word (any 64-bit value),
// t < 2^32 the plaintext modulus and Q = q_0 ... q_level:
//     u   = ((m mod t) * (Q mod t) + floor(t/2)) mod t
//     P_j = (u - floor(t/2)) * (-t^-1) mod q_j
// the words of oracle/ls_oracle.c ora_bfv_scale_up and of k_lift_ringt mode 2.
//
// u does not depend on the limb: it is formed once per coefficient, as the sign and the magnitude of u - floor(t/2) (at most
// t/2 < 2^31), and a limb costs one Montgomery product by -t^-1 and a conditional negation.  Nothing divides: a value is reduced
// mod t through the reciprocal trec = floor(2^64 / t) -- x - mulhi(x, trec) t is in [0, 2t) for every 64-bit x, one conditional
// subtraction finishes it (tests/cpp/test_bfv_plain.cpp holds that against the division).  Host and device compile the same
// functions (-DLSA_EMULATE).
#pragma once
#include "modarith.h"

// x mod t for any 64-bit x; 2 <= t < 2^32, trec = floor(2^64 / t)
LSA_HD u64 bfv_plain_mod_t(u64 x, u64 t, u64 trec) {
    const u64 r = x - mul_lo64(mulhi64(x, trec), t);   // the quotient estimate is the true one or one below it
    return csub(r, t);
}

struct BfvPlainWord {   // u - floor(t/2) of one coefficient
    u64 mag;    // its magnitude, at most t/2
    bool neg;   // u < floor(t/2)
};
// q_mod_t = Q_level mod t.  (t - 1)^2 + t/2 < 2^64: the product and the rounding term fit one word
LSA_HD BfvPlainWord bfv_plain_centre(u64 m, u64 t, u64 trec, u64 q_mod_t) {
    const u64 thalf = t >> 1;
    const u64 u = bfv_plain_mod_t(bfv_plain_mod_t(m, t, trec) * q_mod_t + thalf, t, trec);
    BfvPlainWord w;
    w.neg = u < thalf;
    w.mag = w.neg ? thalf - u : u - thalf;
    return w;
}
// P_j, canonical.  neg_tinv_mont: -(t^-1) mod q_j in Montgomery form.  A modulus of 31 bits or more exceeds every magnitude
LSA_HD u64 bfv_plain_scale_up(const BfvPlainWord& w, u64 neg_tinv_mont, const ModDev& m) {
    const u64 r = (m.q >> 31) ? w.mag : reduce_u64(w.mag, m);
    const u64 p = mont_mul(r, neg_tinv_mont, m.q, m.qinv);
    return w.neg ? neg_mod(p, m.q) : p;
}
// the first polynomial's word: OP 0: c0 + P, 1: c0 - P, 2: P - c0; c0 and P canonical
template <int OP>
LSA_HD u64 bfv_plain_word(u64 c0, u64 p, u64 q) {
    return OP == 0 ? add_mod(c0, p, q) : OP == 1 ? sub_mod(c0, p, q) : sub_mod(p, c0, q);
}
