// bfv_expand.h — the plan of the BFV oblivious expansion (coefficient extraction: the Expand of SealPIR / OnionPIR / Spiral, Lattigo's
// rlwe.Expand) and the point arithmetic of its tail.  Pure C++17: the plan is host only (no device, no context: lsa_bfv_expand_plan,
// tests/cpp/test_bfv_expand.cpp), the point functions are shared with the kernels of bfv_expand.hip.
//
// One ciphertext of m(X) = sum_i m_i X^i becomes `count` ciphertexts, k = ceil(log2 count) levels.  State: a list c[a], c[0] = in.
// Level j = 0 .. k-1 has the Galois element g_j = N / 2^j + 1 and the shift s_j = 2^j; for every node a < min(2^j, count):
//   sigma   = rotate(c[a], g_j)                       (one key switch)
//   c'[a]   = c[a] + sigma                            the EVEN child, in the parent's place
//   c'[a+s] = X^(-s) * (c[a] - sigma)                 the ODD child, only if a + s < count
// X^(-s) sigma(c) = -sigma(X^(-s) c) for these g, which is why one key switch serves both children.  Output i decrypts to
// 2^k * sum_u m_(i + 2^k u) X^(2^k u).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define LSA_EXPAND_HD __host__ __device__
#else
#define LSA_EXPAND_HD
#endif

namespace lsa {

struct BfvExpandLevel {
    int nodes;     // min(2^j, count): the parents, one key switch each
    int n_odd;     // max(0, min(2^j, count - 2^j)): the parents a < n_odd have an odd child
    int shift;     // s_j = 2^j
    uint64_t g;    // N / 2^j + 1
};
struct BfvExpandPlanHost {
    int n_ring = 0, count = 0;
    std::vector<BfvExpandLevel> levels;
    int n_keyswitch = 0;            // sum_j min(2^j, count)
    std::vector<uint64_t> galois;   // ascending, distinct
};

// Throws std::invalid_argument; the message begins "lsa_bfv_expand" and names the argument.
inline BfvExpandPlanHost bfv_expand_plan(int n_ring, int count) {
    if (n_ring < 4 || (n_ring & (n_ring - 1))) throw std::invalid_argument("lsa_bfv_expand: n_ring must be a power of two >= 4");
    if (count < 1) throw std::invalid_argument("lsa_bfv_expand: count must be >= 1");
    if (count > n_ring) throw std::invalid_argument("lsa_bfv_expand: count exceeds the N coefficients");
    BfvExpandPlanHost p;
    p.n_ring = n_ring;
    p.count = count;
    for (int j = 0; (1LL << j) < count; j++) {
        const int s = 1 << j;
        BfvExpandLevel lv;
        lv.nodes = s < count ? s : count;
        lv.n_odd = count - s < s ? count - s : s;
        if (lv.n_odd < 0) lv.n_odd = 0;
        lv.shift = s;
        lv.g = (uint64_t)(n_ring >> j) + 1;
        p.n_keyswitch += lv.nodes;
        p.levels.push_back(lv);
    }
    for (auto it = p.levels.rbegin(); it != p.levels.rend(); ++it) p.galois.push_back(it->g);   // g_j falls with j
    return p;
}

// Where coefficient y of d lands in X^e * d over Z[X] / (X^N + 1), e in [0, 2N): index (y + e) mod N, negated when (y + e) mod 2N >= N.
struct MonomialDest {
    unsigned idx;
    unsigned neg;
};
LSA_EXPAND_HD inline MonomialDest monomial_dest(unsigned y, unsigned e, int logn) {
    const unsigned t = (y + e) & ((2u << logn) - 1);
    return MonomialDest{t & ((1u << logn) - 1), t >> logn};
}
// the odd child's rule, X^(-s) = X^(2N - s), 1 <= s <= N: coefficient y lands on (y - s) mod N, negated when y < s
LSA_EXPAND_HD inline MonomialDest bfv_expand_odd_dest(unsigned y, unsigned s, int logn) { return monomial_dest(y, (2u << logn) - s, logn); }
// any exponent reduced to [0, 2N)
inline unsigned monomial_exponent(long long exponent, int logn) {
    const long long m = 2LL << logn;
    return (unsigned)(((exponent % m) + m) % m);
}

}  // namespace lsa
