// Host-side check of the BFV inner product's headroom rule (lattisense_amd/csrc/tables.h: bfv_dot_plan, bfv_dot_aux_count; the
// operator and lsa_bfv_dot_plan call the same functions): lines "logn level terms nq q_0 .. q_{nq-1}" on stdin, one
// "G max_terms n_groups aux_limbs M(1) M(last group)" per line on stdout.  Driven by tests/test_bfv_dot_api.py, which states the
// rule independently on Python integers.
#include <cstdio>
#include <vector>
#include "../../lattisense_amd/csrc/tables.h"

int main() {
    int logn, level, terms, nq;
    while (std::scanf("%d %d %d %d", &logn, &level, &terms, &nq) == 4) {
        if (nq < 1 || level < 0 || level >= nq || terms < 1) return 2;
        std::vector<u64> q(nq);
        for (auto& x : q) {
            unsigned long long t;
            if (std::scanf("%llu", &t) != 1) return 2;
            x = t;
        }
        const lsa::BfvDotPlan p = lsa::bfv_dot_plan(q.data(), nq, level, logn, terms);
        const int last = terms - (p.n_groups - 1) * p.max_terms;
        std::printf("%d %d %d %d %d %d\n", p.headroom_bits, p.max_terms, p.n_groups, p.aux_limbs,
                    lsa::bfv_dot_aux_count(q.data(), level + 1, logn, 1), lsa::bfv_dot_aux_count(q.data(), level + 1, logn, last));
    }
    return 0;
}
