// bfv_pack.h — the plan of the BFV coefficient packing (PackLWEs of Chen, Dai, Kim, Song, "Efficient homomorphic conversion between
// (Ring) LWE ciphertexts", Alg. 3 plus the field trace; Lattigo's rlwe.Pack) and the point arithmetic of its tail.  Pure C++17: the
// plan is host only (no device, no context: lsa_bfv_pack_plan, tests/cpp/test_bfv_pack.cpp), the point function is shared with the
// kernels of bfv_pack.hip.  The expansion of bfv_expand.h run backwards.
//
// `count` ciphertexts c[i] become one, k = ceil(log2 count).  Levels run j = k-1 down to 0; with l = k - j a level has the shift
// s = N / 2^l and the Galois element g = 2^l + 1; for every node a < 2^j:
//   paired (a + 2^j < count):  xb = X^s * c[a + 2^j],  u = c[a] + xb,  v = c[a] - xb
//   unpaired:                  u = v = c[a]
//   c'[a] = u + rotate(v, g)                          (one key switch)
// Only the first level (j = k-1) can have unpaired nodes; its paired nodes are a < count - 2^(k-1).  With the trace the levels
// l = k+1 .. log2 N follow on c[0] alone: c[0] <- c[0] + rotate(c[0], 2^l + 1).  The result is c[0]: coefficient i * N/2^k holds
// F * (coefficient 0 of input i), F = 2^k without the trace and N with it; with the trace every other coefficient is 0.
#pragma once
#include "bfv_expand.h"

namespace lsa {

struct BfvPackLevel {
    int nodes;     // 2^j: one key switch each
    int n_pair;    // the nodes a < n_pair have the partner c[a + nodes]: min(2^j, count - 2^j)
    int shift;     // s = N / 2^l, l = k - j
    uint64_t g;    // 2^l + 1
};
struct BfvPackPlanHost {
    int n_ring = 0, count = 0, trace = 0;
    std::vector<BfvPackLevel> levels;    // j = k-1 down to 0
    std::vector<uint64_t> trace_g;       // 2^l + 1, l = k+1 .. log2 N (empty without the trace)
    int n_keyswitch = 0;                 // (2^k - 1) + (trace ? log2 N - k : 0)
    std::vector<uint64_t> galois;        // ascending, distinct
};

// Throws std::invalid_argument; the message begins "lsa_bfv_pack" and names the argument.
inline BfvPackPlanHost bfv_pack_plan(int n_ring, int count, int trace) {
    if (n_ring < 4 || (n_ring & (n_ring - 1))) throw std::invalid_argument("lsa_bfv_pack: n_ring must be a power of two >= 4");
    if (count < 1) throw std::invalid_argument("lsa_bfv_pack: count must be >= 1");
    if (count > n_ring) throw std::invalid_argument("lsa_bfv_pack: count exceeds the N coefficients");
    BfvPackPlanHost p;
    p.n_ring = n_ring;
    p.count = count;
    p.trace = trace ? 1 : 0;
    int k = 0, logn = 0;
    while ((1LL << k) < count) k++;
    while ((1 << logn) < n_ring) logn++;
    for (int j = k - 1; j >= 0; j--) {
        const int l = k - j, half = 1 << j;
        BfvPackLevel lv;
        lv.nodes = half;
        lv.n_pair = count - half < half ? count - half : half;
        lv.shift = n_ring >> l;
        lv.g = (uint64_t)(1LL << l) + 1;
        p.n_keyswitch += lv.nodes;
        p.levels.push_back(lv);
    }
    for (int l = 1; l <= (p.trace ? logn : k); l++) p.galois.push_back((uint64_t)(1LL << l) + 1);   // 2^l + 1 rises with l
    if (p.trace)
        for (int l = k + 1; l <= logn; l++) p.trace_g.push_back((uint64_t)(1LL << l) + 1);
    p.n_keyswitch += (int)p.trace_g.size();
    return p;
}

// The source point of X^s * b at x, 1 <= s <= N: coefficient (x - s) mod N of b, negated when x < s.  It is the inverse of
// monomial_dest(y, s) (y + s = x), which is monomial_dest with the exponent 2N - s: the odd child's rule of the expansion.
LSA_EXPAND_HD inline MonomialDest bfv_pack_source(unsigned x, unsigned s, int logn) { return monomial_dest(x, (2u << logn) - s, logn); }

}  // namespace lsa
