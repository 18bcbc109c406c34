// Host-side check of the BFV polynomial evaluator's planner (lattisense_amd/csrc/bfv_poly.h: bfv_poly_plan; lsa_bfv_poly_plan and
// lsa_bfv_poly_create call the same function): lines "t log_baby n_coef coef_0 .. coef_{n-1}" on stdin, one
// "log_baby depth n_mult n_leaves n_leaf_launches n_pairs" per line on stdout.  Driven by tests/test_bfv_poly_api.py, which states
// the plan independently in Python.  With the argument "consts": lines "t k c nq q_0 .. q_{nq-1}" (q_i prime), one line
// "K_0 S_0 .. K_{nq-1} S_{nq-1}" each: the leaf kernel's constants (bfv_poly_centred_mod, bfv_poly_scale_up_word) as plain residues.
#include <cstdio>
#include <vector>
#include "../../lattisense_amd/csrc/bfv_poly.h"

static u64 pow_mod(u64 a, u64 e, u64 q) {
    u64 r = 1 % q;
    for (a %= q; e; e >>= 1, a = (u64)((unsigned __int128)a * a % q))
        if (e & 1) r = (u64)((unsigned __int128)r * a % q);
    return r;
}

static int consts() {
    unsigned long long t, k, c;
    int nq;
    while (std::scanf("%llu %llu %llu %d", &t, &k, &c, &nq) == 4) {
        if (nq < 1 || nq > 64) return 2;
        std::vector<u64> q(nq);
        u64 q_mod_t = 1 % t;
        for (auto& x : q) {
            unsigned long long v;
            if (std::scanf("%llu", &v) != 1) return 2;
            x = v;
            q_mod_t = (u64)((unsigned __int128)q_mod_t * (x % t) % t);
        }
        for (u64 x : q)
            std::printf("%llu %llu ", (unsigned long long)lsa::bfv_poly_centred_mod(k, t, x),
                        (unsigned long long)lsa::bfv_poly_scale_up_word(c, t, q_mod_t, x, pow_mod(t % x, x - 2, x)));
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "consts") return consts();
    unsigned long long t;
    int log_baby, n;
    while (std::scanf("%llu %d %d", &t, &log_baby, &n) == 3) {
        if (n < 0 || n > 4096) return 2;
        std::vector<u64> cf(n);
        for (auto& x : cf) {
            unsigned long long v;
            if (std::scanf("%llu", &v) != 1) return 2;
            x = v;
        }
        try {
            const lsa::BfvPolyPlan p = lsa::bfv_poly_plan(t, n, cf.data(), log_baby);
            std::printf("%d %d %d %d %d %d\n", p.log_baby, p.depth, p.n_mult, p.n_leaves, p.n_leaf_launches, p.n_pairs);
        } catch (const std::invalid_argument& e) {
            std::printf("refused %s\n", e.what());
        }
    }
    return 0;
}
