// entry_check.h — argument checks of the first-generation entry points and the plan runners.
// The layout, overlap and argument contract of the first-generation entry points (include/lattisense_amd.h, "Layout and
// aliasing"), checked in the operators themselves so that the task dispatcher and the plan runners get it too.  Everything is
// decided on the host before a kernel or a copy is queued; every refusal is LSA_ERR_ARG with a message that begins with the entry
// point's name.  The span arithmetic is layout_check.h's.
#pragma once
#include "layout_check.h"
#include "lsa_internal.h"

namespace lsa {

struct EntryCheck {
    using Span = layout::Span;
    const Context& c;
    std::string who;
    int level, batch;
    size_t N;
    // algo: LSA_ALGO_BFV / LSA_ALGO_CKKS, or -1 for an operator both schemes use; min_level: 1 for the operators that drop a limb
    EntryCheck(const Context& c_, const char* who_, int algo, int level_, int min_level, int batch_)
        : c(c_), who(who_), level(level_), batch(batch_), N((size_t)c_.n) {
        LSA_REQUIRE(algo < 0 || c.algo == algo, who + (algo == LSA_ALGO_BFV ? ": context is not BFV" : ": context is not CKKS"));
        LSA_REQUIRE(level >= min_level && level < c.nq,
                    who + ": level out of range (" + std::to_string(min_level) + ".." + std::to_string(c.nq - 1) + ")");
    }
    void polys(int polys) const {   // a plaintext or one polynomial, a ciphertext, a degree-2 ciphertext
        LSA_REQUIRE(polys >= 1 && polys <= 3, who + ": polys must be 1, 2 or 3");
    }
    void key(const Key& k, const char* what) const {
        LSA_REQUIRE(k.data != nullptr, who + ": " + what + " is null");
        LSA_REQUIRE(k.level >= level, who + ": " + what + " was exported at a lower level than the ciphertext");
    }
    // an operand of `words` words per batch item; shared_ok: a batch stride of 0 (one operand for the whole batch) is accepted
    Span operand(const u64* p, long long stride, size_t words, const char* what, bool shared_ok) const {
        LSA_REQUIRE(p != nullptr, who + ": " + what + " is null");
        const Span sp = layout::span_of(p, stride, words);
        LSA_REQUIRE(layout::stride_ok(sp, shared_ok), who + ": batch stride of " + what +
                                                          (shared_ok ? " below one operand (0: shared by the batch)" : " below one operand"));
        // the element-wise kernels move 16 bytes per lane at base + item * stride
        LSA_REQUIRE(layout::aligned16(sp), who + ": " + what + " must be 16-byte aligned with an even batch stride");
        return sp;
    }
    Span output(const u64* p, long long stride, size_t words, const char* what = "out") const { return operand(p, stride, words, what, false); }
    void apart(const Span& out, const Span& in, const char* what) const {
        LSA_REQUIRE(layout::apart(out, in, batch), who + ": the output overlaps " + what);
    }
    void same_or_apart(const Span& out, const Span& in, const char* what) const {
        LSA_REQUIRE(layout::same_or_apart(out, in, batch),
                    who + ": the output must be " + what + " itself (same pointer, same stride) or not overlap it");
    }
    // the n outputs of a hoisted rotation (one stride, `words` each) against its input: layout::one_of_outputs_may_be_input.
    // Returns the output that IS the input, or -1
    int rotate_many_outputs(const Span& in, u64* const* outs, int n, long long sout, size_t words) const {
        LSA_REQUIRE(outs != nullptr, who + ": null argument");
        std::vector<Span> sp(n);
        for (int i = 0; i < n; i++) sp[i] = output(outs[i], sout, words, "an output");
        int in_place = -1;
        const layout::OneOf r = layout::one_of_outputs_may_be_input(in, sp.data(), n, batch, &in_place);
        LSA_REQUIRE(r != layout::ONE_OF_OUTPUTS_OVERLAP, who + ": two outputs overlap");
        LSA_REQUIRE(r != layout::ONE_OF_TWO_ARE_INPUT, who + ": at most one output may be the input");
        LSA_REQUIRE(r == layout::ONE_OF_OK, who + ": an output must be in itself (same pointer, same stride) or not overlap it");
        return in_place;
    }
    // an array of `count` batched ciphertexts at stride s_index (arr: entry 0; stride_name: what its batch stride is called) against
    // the one batched operand on the other side of the call: layout::one_against_array.  The OUTPUT side is named in the refusals
    // whichever it is -- `one` for the packing and the selection, the array for the expansion -- and the input side as in0 where entry
    // 0 is met in part, as in_any where a later entry is.
    struct IndexedArray {
        bool in_place;   // `one` is entry 0 itself
        bool dense;      // s_index == batch * stride: the array is one strided batch of count * batch items
    };
    IndexedArray indexed_array(const Span& one, const Span& arr, long long s_index, int count, const char* stride_name, const char* in0,
                               const char* in_any) const {
        LSA_REQUIRE((s_index & 1) == 0, who + ": s_index must be even");
        LSA_REQUIRE(s_index > 0 && (layout::u128)(unsigned long long)s_index >= (layout::u128)(unsigned)batch * (unsigned long long)arr.stride,
                    who + ": s_index below batch * " + stride_name);
        LSA_REQUIRE((long long)count * batch <= 0x7fffffffLL, who + ": count * batch does not fit a batch");
        const layout::OneVsArray r = layout::one_against_array(one, arr, s_index, count, batch);
        LSA_REQUIRE(r != layout::ONE_PARTLY_ENTRY0,
                    who + ": the output must be " + in0 + " itself (same pointer, same stride) or not overlap it");
        LSA_REQUIRE(r != layout::ONE_OVERLAPS_ENTRY, who + ": the output overlaps " + in_any);
        return {r == layout::ONE_IS_ENTRY0, layout::dense_array(arr, s_index, batch)};
    }
};

// out = in for `batch` ciphertexts at `level` (what an indexed-array operator of count 1 comes to)
inline void copy_ciphertexts(Context& c, int level, const u64* in, long long sin, u64* out, long long sout, int batch, hipStream_t s) {
    std::vector<int> rows(2 * (level + 1));
    for (size_t i = 0; i < rows.size(); i++) rows[i] = (int)i;
    launch_copy_rows(c, in, sin, out, sout, (int)rows.size(), rows.data(), batch, s);
}

}  // namespace lsa
