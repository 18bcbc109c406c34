// slot_sum.h — the plan of the CKKS slot sum  out = sum_{i<count} rot(ct, i*step)  (Lattigo InnerSum; Replicate is the same
// operation with a negative step).  Host only, pure C++17: no device, no context (lsa_slot_sum_plan, tests/test_ckks_slot_sum_api.py).
//
// State (x, s, n, tail), starting at (ct, step, count, none); invariant: result = S(x, s, n) + tail with
// S(x, s, n) = sum_{i<n} rot(x, i*s).  While n > 1 one STEP -- one decomposition of x's c1 -- runs:
//   1. n odd:  the rotation (n-1)*s joins the step's keys with destination TAIL, n -= 1
//      (S(x, s, n) = S(x, s, n-1) + rot(x, (n-1)*s));
//   2. n even: radix 4 and n % 4 == 0: the rotations s, 2s, 3s with destination NEXT, s *= 4, n /= 4
//              otherwise:              the rotation s with destination NEXT,          s *= 2, n /= 2
//      (S(x, s, n) = S(x + rot(x, s), 2s, n/2), and the same with four terms);
//   3. x <- x + ModDown(sum of the step's NEXT extended rotations); the TAIL rotation is added to the extended tail
//      accumulator, which is not divided.
// At n == 1: out = x + ModDown(tail) if a tail exists, else x.  Every rotation is reduced mod N/2.  A step carries at most four
// keys.  Radix 2 asks for the keys of Lattigo's InnerSumLog: 2^i * step for i < floor(log2 count), and for every set bit k of
// count but the highest the offset (count with its low k+1 bits cleared) * step.
//
// The BFV slot sum  out = sum_{i<count} rot_cols(y, i*step),  y = ct + rot_rows(ct) if rows != 0, else ct, is the same plan: BFV
// slots form a 2 x N/2 matrix, the column rotation r is the Galois element 5^(r mod N/2) mod 2N, the row swap is 2N-1.  The plan
// starts at x = y; with rows != 0 one more step runs first, one decomposition of ct's c1 with one NEXT key, the key of 2N-1.
// Every key is named by its Galois element (galois_keys.h); rows = 0 is the CKKS plan.
#pragma once
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "galois_keys.h"

namespace lsa {

#define LSA_SLOTSUM_MAX_KEYS 4   // keys of one step (one decomposition): 3 NEXT + 1 TAIL at radix 4

struct SlotSumKey {
    uint64_t g;   // the key's Galois element
    int rot;      // the rotation, reduced mod N/2, never 0; 0: the row swap
    bool tail;    // destination: the extended tail accumulator (else the step's NEXT sum)
};
struct SlotSumStep {
    std::vector<SlotSumKey> keys;   // the TAIL key, if any, first; then the NEXT keys by ascending multiple of s
};
struct SlotSumPlanHost {
    int n_ring = 0, count = 0, radix = 2, rows = 0;
    long long step = 0;
    std::vector<SlotSumStep> steps;
    bool has_tail = false;
    int n_keyswitch = 0;            // key MACs (one per key of every step)
    int n_moddown = 0;              // divisions by P: one per step + one for the tail
    std::vector<int> rotations;     // ascending, distinct, reduced mod N/2 (the row swap is not among them)
    std::vector<uint64_t> galois;   // ascending, distinct: the element of every key
};

// dflt_radix: what radix 0 stands for (the measured default).  Throws std::invalid_argument with a message that names
// the argument.
inline SlotSumPlanHost slot_sum_plan(int n_ring, long long step, int count, int radix, int dflt_radix = 2, int rows = 0) {
    if (n_ring < 4 || (n_ring & (n_ring - 1))) throw std::invalid_argument("slot sum: n_ring must be a power of two >= 4");
    const long long h = n_ring / 2;
    if (count < 1) throw std::invalid_argument("slot sum: count must be >= 1");
    if (count > h) throw std::invalid_argument("slot sum: count exceeds the N/2 slots");
    if (radix != 0 && radix != 2 && radix != 4) throw std::invalid_argument("slot sum: radix must be 0 (default), 2 or 4");
    SlotSumPlanHost p;
    p.n_ring = n_ring;
    p.count = count;
    p.step = step;
    p.radix = radix ? radix : dflt_radix;
    p.rows = rows ? 1 : 0;
    long long s = ((step % h) + h) % h;
    int n = count;
    auto add = [&](SlotSumStep& st, long long mult, bool tail) {
        const int r = (int)((mult % h) * s % h);
        if (r == 0)
            throw std::invalid_argument("slot sum: step " + std::to_string(step) + " makes a planned rotation a multiple of N/2 (count " +
                                        std::to_string(count) + ")");
        st.keys.push_back({galois_of_rotation(r, n_ring), r, tail});
    };
    if (p.rows) p.steps.push_back({{{2 * (uint64_t)n_ring - 1, 0, false}}});
    while (n > 1) {
        SlotSumStep st;
        if (n & 1) {
            add(st, n - 1, true);
            p.has_tail = true;
            n -= 1;
        }
        if (p.radix == 4 && n % 4 == 0) {
            for (int i = 1; i <= 3; i++) add(st, i, false);
            s = s * 4 % h;
            n /= 4;
        } else {
            add(st, 1, false);
            s = s * 2 % h;
            n /= 2;
        }
        p.steps.push_back(st);
    }
    p.n_moddown = (int)p.steps.size() + (p.has_tail ? 1 : 0);
    for (const auto& st : p.steps)
        for (const auto& k : st.keys) {
            p.n_keyswitch++;
            if (k.rot) p.rotations.push_back(k.rot);
            p.galois.push_back(k.g);
        }
    std::sort(p.rotations.begin(), p.rotations.end());
    p.rotations.erase(std::unique(p.rotations.begin(), p.rotations.end()), p.rotations.end());
    std::sort(p.galois.begin(), p.galois.end());
    p.galois.erase(std::unique(p.galois.begin(), p.galois.end()), p.galois.end());
    return p;
}

// The BFV entry points' planner.  Throws std::invalid_argument; the message begins "lsa_bfv_slot_sum" and names the argument.
inline SlotSumPlanHost bfv_slot_sum_plan(int n_ring, long long step, int count, int radix, int rows, int dflt_radix = 4) {
    try {
        return slot_sum_plan(n_ring, step, count, radix, dflt_radix, rows);
    } catch (const std::invalid_argument& e) {
        const std::string m = e.what(), pre = "slot sum: ";
        throw std::invalid_argument("lsa_bfv_slot_sum: " + (m.compare(0, pre.size(), pre) == 0 ? m.substr(pre.size()) : m));
    }
}

}  // namespace lsa
