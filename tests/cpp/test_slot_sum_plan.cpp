// Host-side print-out of the slot-sum planner (lattisense_amd/csrc/slot_sum.h) and of the element rule (galois_keys.h), compared
// by tests/test_slot_sum_plan_host.py with tests/golden/slot_sum_plans.txt and with Python's pow(5, r, 2N).
//   plans:    one line per plan of the grid at N = 2^10, "count step radix rows:" then the steps, separated by ';', each the
//             step's keys in order as element:tail separated by ','; a refused combination prints '!' and the message.
//             rows = 0 is the CKKS plan (slot_sum_plan), rows = 1 the BFV plan with the row fold (bfv_slot_sum_plan).
//   elements: "logn r element" for every r in [0, N/2) at N = 2^4 .. 2^12 and for 64 spread r at N = 2^16.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>
#include "../../lattisense_amd/csrc/slot_sum.h"

static void print_plans() {
    const int n_ring = 1 << 10;
    std::vector<int> counts;
    for (int c = 1; c <= 40; c++) counts.push_back(c);
    for (int c : {63, 64, 65, 127, 128, 129, 130, 512}) counts.push_back(c);
    for (int count : counts)
        for (long long step : {1LL, 3LL, -1LL, -64LL})
            for (int radix : {2, 4})
                for (int rows : {0, 1}) {
                    std::printf("%d %lld %d %d:", count, step, radix, rows);
                    try {
                        const lsa::SlotSumPlanHost p =
                            rows ? lsa::bfv_slot_sum_plan(n_ring, step, count, radix, rows) : lsa::slot_sum_plan(n_ring, step, count, radix);
                        for (size_t i = 0; i < p.steps.size(); i++) {
                            std::printf(i ? ";" : " ");
                            for (size_t k = 0; k < p.steps[i].keys.size(); k++)
                                std::printf("%s%llu:%d", k ? "," : "", (unsigned long long)p.steps[i].keys[k].g, p.steps[i].keys[k].tail ? 1 : 0);
                        }
                    } catch (const std::invalid_argument& e) {
                        std::printf(" ! %s", e.what());
                    }
                    std::printf("\n");
                }
}

static void print_elements() {
    for (int logn = 4; logn <= 12; logn++)
        for (int r = 0; r < (1 << logn) / 2; r++)
            std::printf("%d %d %llu\n", logn, r, (unsigned long long)lsa::galois_of_rotation(r, 1 << logn));
    for (int i = 0; i < 64; i++) {
        const int r = i == 63 ? 32767 : i * 521;   // 0 .. N/2 - 1
        std::printf("16 %d %llu\n", r, (unsigned long long)lsa::galois_of_rotation(r, 1 << 16));
    }
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "plans")) return print_plans(), 0;
    if (argc == 2 && !std::strcmp(argv[1], "elements")) return print_elements(), 0;
    std::fprintf(stderr, "usage: test_slot_sum_plan plans|elements\n");
    return 2;
}
