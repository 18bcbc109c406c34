// bfv_select.h — the plan of the BFV select-by-index operator (lsa_bfv_select_*; semantics: include/lattisense_amd.h): a CMux tree
// over `count` ciphertexts whose selectors are RGSW ciphertexts of the index bits.  Pure C++17, host only: no device, no context
// (lsa_bfv_select_plan, tests/cpp/test_bfv_select.cpp).
//
// k = ceil(log2 count).  Levels run j = k-1 down to 0; at level j the selector R_j encrypts bit j of the index and for every node
// a < 2^j that has a partner (a + 2^j < count)
//   c'[a] = cmux(c[a], c[a + 2^j], R_j) = c[a] + R_j [.] (c[a + 2^j] - c[a])              (one external product)
// Unpaired nodes are left alone.  The result is c[0]: with the index idx < count, the node that holds input idx after level j is
// idx mod 2^j (bit j of idx set: the partner a + 2^j = idx mod 2^(j+1) is taken; clear: c[a] stays, and an unpaired node has
// bit j clear because idx < count).  Every level below the first is full (2^j <= count - 2^j for j < k-1), so the products are
// sum_j n_pair(j) = (count - 2^(k-1)) + (2^(k-1) - 1) = count - 1.
#pragma once
#include <stdexcept>
#include <vector>

namespace lsa {

struct BfvSelectLevel {
    int bit;       // j: the selector R_j
    int nodes;     // 2^j: the partner of node a is a + nodes
    int n_pair;    // the nodes a < n_pair have a partner: min(2^j, count - 2^j)
};
struct BfvSelectPlanHost {
    int count = 0;
    std::vector<BfvSelectLevel> levels;   // j = k-1 down to 0
    int n_products = 0;                   // count - 1
};

constexpr int BFV_SELECT_MAX_COUNT = 1 << 20;

// Throws std::invalid_argument; the message begins "lsa_bfv_select" and names the argument.
inline BfvSelectPlanHost bfv_select_plan(int count) {
    if (count < 1) throw std::invalid_argument("lsa_bfv_select: count must be >= 1");
    if (count > BFV_SELECT_MAX_COUNT) throw std::invalid_argument("lsa_bfv_select: count exceeds 2^20");
    BfvSelectPlanHost p;
    p.count = count;
    int k = 0;
    while ((1LL << k) < count) k++;
    for (int j = k - 1; j >= 0; j--) {
        const int half = 1 << j;
        BfvSelectLevel lv;
        lv.bit = j;
        lv.nodes = half;
        lv.n_pair = count - half < half ? count - half : half;
        p.n_products += lv.n_pair;
        p.levels.push_back(lv);
    }
    return p;
}

}  // namespace lsa
