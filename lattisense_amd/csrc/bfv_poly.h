// bfv_poly.h — BFV polynomial evaluation  p(x) = sum_{k < n_coef} coef[k] x^k mod t,  slot-wise on a ciphertext: the flat
// baby-step / giant-step planner, the constants of the leaf kernel and the plan's structures (lsa_bfv_poly_*; the kernel, create
// and run are in bfv_poly.hip).  Everything in this header is host only, pure C++17: no device, no context
// (tests/cpp/test_bfv_poly_plan.cpp compiles it with g++).  DESIGN.md 4.15; restated in tests/bfv_poly_model.py.
//
//   m = 2^log_baby, G = ceil(n_coef / m), the coefficients zero-padded to G * m.
//   baby powers   x^j = x^ceil(j/2) * x^floor(j/2) for 2 <= j < m: those a non-zero coefficient needs, and their halves.
//   giant powers  y = x^m = x^(m/2) * x^(m/2);  y^g = y^ceil(g/2) * y^floor(g/2) for 2 <= g < G: those a non-zero leaf needs, and
//                 their halves.
//   leaves        leaf_g = coef[g m] + sum_{1 <= j < m} coef[g m + j] x^j; an all-zero leaf does not exist, a constant one is the
//                 trivial ciphertext (c1 = 0).
//   sum           out = leaf_0 + sum_{g >= 1} leaf_g * y^g: ONE scale-down by Q and ONE relinearisation (bfv_dot, leaf_0 its
//                 addend); with no term g >= 1, out = leaf_0.
// Counts: n_mult = key switches = baby powers + giant powers (y included) + 1 if the sum has a term; n_pairs = terms of the sum;
// depth from d(x^j) = ceil(log2 j), d(y^g) = log_baby + ceil(log2 g), d(leaf) = max over its used powers (0: a constant),
// depth = max(d(leaf_0), max_g(max(d(leaf_g), d(y^g)) + 1)).  log_baby = 0: the least depth, then the least n_mult, then the
// smaller value.
#pragma once
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "poly_lincomb.h"

namespace lsa {

#define LSA_BFV_POLY_MAX_COEF 256
#define LSA_BFV_AFFINE_MAX_LIMBS 64   // limbs whose two constants ride in the kernel's argument struct (lsa_bfv_affine_const)

struct BfvPolyPlan {
    u64 t = 0;
    int n_coef = 0, log_baby = 0, m = 0, G = 0;
    std::vector<u64> coef;      // [G * m], zero-padded
    std::vector<char> baby;     // [m]: x^j is computed (j >= 2)
    std::vector<char> giant;    // [G]: y^g is computed (g >= 1)
    std::vector<int> leaves;    // the g of every leaf that exists, ascending
    int depth = 0, n_mult = 0, n_pairs = 0, n_leaves = 0, n_leaf_launches = 0;
    bool leaf_uses(int g, int j) const { return coef[(size_t)g * m + j] != 0; }
};

inline int bfv_poly_ceil_log2(int x) {
    int r = 0;
    while ((1 << r) < x) r++;
    return r;
}

// the plan at one log_baby in 1..4; coef checked by the caller
inline BfvPolyPlan bfv_poly_plan_at(u64 t, int n_coef, const u64* coef, int log_baby) {
    BfvPolyPlan p;
    p.t = t;
    p.n_coef = n_coef;
    p.log_baby = log_baby;
    p.m = 1 << log_baby;
    p.G = (n_coef + p.m - 1) / p.m;
    p.coef.assign((size_t)p.G * p.m, 0);
    std::copy(coef, coef + n_coef, p.coef.begin());
    p.baby.assign(p.m, 0);
    p.giant.assign(p.G, 0);
    int d_rest = -1;   // max over g >= 1 of max(d(leaf_g), d(y^g))
    for (int g = 0; g < p.G; g++) {
        bool exists = p.coef[(size_t)g * p.m] != 0;
        int d_leaf = 0;
        for (int j = 1; j < p.m; j++)
            if (p.leaf_uses(g, j)) {
                exists = true;
                p.baby[j] = 1;
                d_leaf = std::max(d_leaf, bfv_poly_ceil_log2(j));
            }
        if (!exists) continue;
        p.leaves.push_back(g);
        if (g == 0) {
            p.depth = d_leaf;
        } else {
            p.giant[g] = 1;
            p.n_pairs++;
            d_rest = std::max(d_rest, std::max(d_leaf, log_baby + bfv_poly_ceil_log2(g)));
        }
    }
    if (d_rest >= 0) p.depth = std::max(p.depth, d_rest + 1);
    for (int g = p.G - 1; g >= 2; g--)
        if (p.giant[g]) p.giant[(g + 1) / 2] = p.giant[g / 2] = 1;
    if (p.n_pairs && p.m / 2 >= 2) p.baby[p.m / 2] = 1;   // y = x^(m/2) * x^(m/2)
    for (int j = p.m - 1; j >= 2; j--)
        if (p.baby[j]) p.baby[(j + 1) / 2] = p.baby[j / 2] = 1;
    p.baby[0] = 0;
    if (p.m > 1) p.baby[1] = 0;   // x itself is the input
    for (int j = 2; j < p.m; j++) p.n_mult += p.baby[j];
    for (int g = 1; g < p.G; g++) p.n_mult += p.giant[g];
    p.n_mult += p.n_pairs ? 1 : 0;
    p.n_leaves = (int)p.leaves.size();
    p.n_leaf_launches = (p.n_leaves + LSA_PLC_MAX_OUT - 1) / LSA_PLC_MAX_OUT;
    return p;
}

// The planner of the entry points.  Throws std::invalid_argument; the message begins "bfv_poly" and names the argument.
inline BfvPolyPlan bfv_poly_plan(u64 t, int n_coef, const u64* coef, int log_baby) {
    if (t < 2) throw std::invalid_argument("bfv_poly: the plaintext modulus t must be >= 2");
    if (coef == nullptr) throw std::invalid_argument("bfv_poly: null argument (coef)");
    if (n_coef < 1 || n_coef > LSA_BFV_POLY_MAX_COEF) throw std::invalid_argument("bfv_poly: n_coef: between 1 and 256 coefficients");
    if (log_baby < 0 || log_baby > 4) throw std::invalid_argument("bfv_poly: log_baby outside 0..4");
    int deg = 0;
    for (int k = 0; k < n_coef; k++) {
        if (coef[k] >= t) throw std::invalid_argument("bfv_poly: coefficient " + std::to_string(k) + " is not below t");
        if (coef[k]) deg = k;
    }
    if (deg == 0) throw std::invalid_argument("bfv_poly: a polynomial of degree 0 has no ciphertext to evaluate");
    if (log_baby) return bfv_poly_plan_at(t, n_coef, coef, log_baby);
    BfvPolyPlan best = bfv_poly_plan_at(t, n_coef, coef, 1);
    for (int b = 2; b <= 4; b++) {
        BfvPolyPlan p = bfv_poly_plan_at(t, n_coef, coef, b);
        if (p.depth < best.depth || (p.depth == best.depth && p.n_mult < best.n_mult)) best = std::move(p);
    }
    return best;
}

// ---- the leaf kernel's constants, as plain residues
// K mod q for the coefficient k < t centred into (-t/2, t/2]
inline u64 bfv_poly_centred_mod(u64 k, u64 t, u64 q) {
    return k > t / 2 ? (q - (t - k) % q) % q : k % q;
}
// Word 0 of limb q of Lattigo's scaleUp of the ring-t plaintext (c, 0, 0, ...): with u = (c * (Q mod t) + floor(t/2)) mod t,
// (u - floor(t/2)) * (-t^-1) mod q -- the arithmetic of k_lift_ringt mode 2 on one word.  q_mod_t = Q_level mod t,
// t_inv = t^-1 mod q.  Every other coefficient of that plaintext scales to 0.
inline u64 bfv_poly_scale_up_word(u64 c, u64 t, u64 q_mod_t, u64 q, u64 t_inv) {
    const u64 thalf = t >> 1;
    const u64 u = (u64)(((unsigned __int128)(c % t) * q_mod_t + thalf) % t);
    const u64 d = (u % q + q - thalf % q) % q;
    return (u64)((unsigned __int128)d * ((q - t_inv) % q) % q);
}

}  // namespace lsa
