// Host-side check of the span arithmetic behind every operator's argument checks (lattisense_amd/csrc/layout_check.h).
// Lines on stdin, one answer line each on stdout:
//   "base_a stride_a words_a base_b stride_b words_b batch"   (bases in BYTES, strides and sizes in words)
//     -> "apart same same_or_apart ok_a ok_shared_a aligned_a end_hi end_lo"
//        ok_a / ok_shared_a: stride_ok(a) without / with shared operands accepted; end: span_end(a) as two 64-bit halves
// With the argument "many" the lines are calls of the hoisted rotations' rule (one_of_outputs_may_be_input) instead:
//   "batch words base_in stride_in stride_out n base_out_0 .. base_out_{n-1}"   (n <= 8)
//     -> "code in_place"   code: 0 accepted, 1 two outputs overlap, 2 an output partly overlaps the input, 3 two outputs are the input
// With the argument "array" the lines are calls of the indexed-array operators' rule (one_against_array, dense_array):
//   "batch words base_one stride_one base_arr stride_arr s_index count"
//     -> "code dense"   code: 0 apart from every entry, 1 `one` is entry 0, 2 it shares words with entry 0 without being it, 3 it shares
//                       words with a later entry
// Driven by tests/test_layout_check_host.py, which marks every word of the operands in an array and compares.
#include <cstdio>
#include <cstring>
#include "../../lattisense_amd/csrc/layout_check.h"

using namespace lsa::layout;

static int many() {
    int batch, n;
    unsigned long long words, bi;
    long long si, so;
    while (std::scanf("%d %llu %llu %lld %lld %d", &batch, &words, &bi, &si, &so, &n) == 6) {
        if (n < 0 || n > 8) return 4;
        Span outs[8];
        for (int i = 0; i < n; i++) {
            unsigned long long b;
            if (std::scanf("%llu", &b) != 1) return 5;
            outs[i] = Span{(uintptr_t)b, so, (size_t)words};
        }
        int in_place = -7;
        const OneOf r = one_of_outputs_may_be_input(Span{(uintptr_t)bi, si, (size_t)words}, outs, n, batch, &in_place);
        std::printf("%d %d\n", (int)r, in_place);
    }
    return 0;
}

static int array() {
    int batch, count;
    unsigned long long words, bo, ba;
    long long so, sa, s_index;
    while (std::scanf("%d %llu %llu %lld %llu %lld %lld %d", &batch, &words, &bo, &so, &ba, &sa, &s_index, &count) == 8) {
        const Span one{(uintptr_t)bo, so, (size_t)words}, arr{(uintptr_t)ba, sa, (size_t)words};
        std::printf("%d %d\n", (int)one_against_array(one, arr, s_index, count, batch), dense_array(arr, s_index, batch) ? 1 : 0);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "many") == 0) return many();
    if (argc > 1 && std::strcmp(argv[1], "array") == 0) return array();
    unsigned long long ba, wa, bb, wb;
    long long sa, sb;
    int batch;
    while (std::scanf("%llu %lld %llu %llu %lld %llu %d", &ba, &sa, &wa, &bb, &sb, &wb, &batch) == 7) {
        const Span a{(uintptr_t)ba, sa, (size_t)wa}, b{(uintptr_t)bb, sb, (size_t)wb};
        const u128 end = span_end(a, batch);
        // the pointer overload must agree with the span one
        if (apart(reinterpret_cast<const void*>(a.base), sa, wa, reinterpret_cast<const void*>(b.base), sb, wb, batch) != apart(a, b, batch)) return 3;
        std::printf("%d %d %d %d %d %d %llu %llu\n", apart(a, b, batch) ? 1 : 0, same(a, b) ? 1 : 0, same_or_apart(a, b, batch) ? 1 : 0,
                    stride_ok(a, false) ? 1 : 0, stride_ok(a, true) ? 1 : 0, aligned16(a) ? 1 : 0, (unsigned long long)(end >> 64),
                    (unsigned long long)end);
    }
    return 0;
}
