// ks_mac_pair.h — what the host shares with k_ks_mac_pair (bfv_select.hip), the gadget MAC of an external product: the products of a
// point, the fold rule and the choice of the instantiation.  Plain C++ (tests/cpp/test_bfv_select.cpp compiles it for the host).
//
//   acc[h][tl][x] = sum_{d<beta} e0[d][tl][x] * R0[d][h][tl][x] + sum_{d<beta} e1[d][tl][x] * R1[d][h][tl][x]       (* 2^-64 mod q)
// One 128-bit sum takes the 2 * beta products in the order p = 0 .. 2 beta - 1 (p < beta: digit p of e0 with R0; else digit p - beta
// of e1 with R1).  With q < 2^61 eight products of canonical residues stay below q * 2^64 (8 q^2 < q * 2^64; tests/boundary.py
// is_ceiling names the bound), so the sum is folded into the canonical running residue after every eighth product -- k_ks_mac's rule
// over the longer sum.  A fold leaves a canonical residue and REDC is additive mod q: the words do not depend on where the folds fall
// and equal the sum (add_mod) of two k_ks_mac results.
#pragma once

namespace lsa {

constexpr int KS_PAIR_FOLD = 8;   // products between folds

constexpr int ks_pair_products(int beta) { return 2 * beta; }
constexpr bool ks_pair_fold_after(int p) { return (p & (KS_PAIR_FOLD - 1)) == KS_PAIR_FOLD - 1; }   // product p (from 0) ends a group
constexpr int ks_pair_folds(int beta) { return ks_pair_products(beta) / KS_PAIR_FOLD; }             // folds inside the sum

// The digits whose key words (both keys, both halves: 16 VGPRs per digit) a thread keeps in registers across the batch items it
// walks; 0: the keys are streamed per item.  A register-resident sum has at most KS_PAIR_FOLD products and needs no fold inside.
constexpr int ks_pair_resident(int beta) { return beta <= 4 ? (beta < 1 ? 1 : beta) : 0; }

}  // namespace lsa
