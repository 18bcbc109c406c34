// Host program for lattisense_amd/csrc/bfv_select.h and ks_mac_pair.h (tests/test_bfv_select_host.py builds it with
// -fsanitize=address,undefined): the select plan against a brute-force walk of the CMux tree for every count <= 64 -- every index below
// count reaches node 0, count - 1 products, only the first level has unpaired nodes -- the refusals, and the pair MAC's fold rule.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../lattisense_amd/csrc/bfv_select.h"
#include "../../lattisense_amd/csrc/ks_mac_pair.h"

using namespace lsa;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond);     \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

// the tree walked node by node: node a holds input held[a]; a CMux under the selector of bit j takes the partner when bit j of the
// index is set
static void plan_against_brute_force() {
    for (int count = 1; count <= 64; count++) {
        const BfvSelectPlanHost p = bfv_select_plan(count);
        int k = 0;
        while ((1 << k) < count) k++;
        CHECK((int)p.levels.size() == k && p.count == count && p.n_products == count - 1);
        for (int idx = 0; idx < count; idx++) {
            std::vector<int> held(count);
            for (int i = 0; i < count; i++) held[i] = i;
            int products = 0;
            for (int lv = 0; lv < k; lv++) {
                const BfvSelectLevel& l = p.levels[lv];
                const int j = k - 1 - lv;
                CHECK(l.bit == j && l.nodes == 1 << j);
                int pairs = 0;
                for (int a = 0; a < l.nodes; a++) {
                    if (a + l.nodes < count) {
                        CHECK(a < l.n_pair);   // the runner's rule: the nodes below n_pair, and only they
                        pairs++;
                        if ((idx >> j) & 1) held[a] = held[a + l.nodes];
                    } else {
                        CHECK(a >= l.n_pair);
                        CHECK(lv == 0);        // only the first level has unpaired nodes
                    }
                }
                CHECK(pairs == l.n_pair);
                products += pairs;
                // the inputs from max(1, 2^(k-1)) on are never written: no node at or above l.nodes is
                CHECK(l.n_pair <= l.nodes && l.nodes <= (k ? 1 << (k - 1) : 1));
            }
            CHECK(products == count - 1);
            CHECK(held[0] == idx);
        }
    }
    std::printf("ok plan\n");
}

static void refusals() {
    for (int count : {0, -1, BFV_SELECT_MAX_COUNT + 1}) {
        bool threw = false;
        try {
            bfv_select_plan(count);
        } catch (const std::invalid_argument& e) {
            const std::string m = e.what();
            threw = m.rfind("lsa_bfv_select", 0) == 0 && m.find("count") != std::string::npos;
        }
        CHECK(threw);
    }
    CHECK(bfv_select_plan(BFV_SELECT_MAX_COUNT).levels.size() == 20);
    std::printf("ok refusals\n");
}

// no group of products between two folds is longer than 8, the register-resident instantiations hold a whole sum in one group
static void fold_rule() {
    for (int beta = 1; beta <= 32; beta++) {
        const int n = ks_pair_products(beta);
        CHECK(n == 2 * beta);
        int run = 0, folds = 0;
        for (int p = 0; p < n; p++) {
            run++;
            CHECK(run <= KS_PAIR_FOLD);
            if (ks_pair_fold_after(p)) run = 0, folds++;
        }
        CHECK(folds == ks_pair_folds(beta));
        const int kb = ks_pair_resident(beta);
        CHECK(kb == 0 || (kb >= beta && 2 * kb <= KS_PAIR_FOLD));
        CHECK((kb == 0) == (beta > 4));
    }
    CHECK(ks_pair_folds(4) == 1 && ks_pair_folds(5) == 1 && ks_pair_folds(9) == 2);   // 8, 10 and 18 products
    std::printf("ok fold\n");
}

int main() {
    plan_against_brute_force();
    refusals();
    fold_rule();
    return 0;
}
