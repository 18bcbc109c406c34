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
};

}  // namespace lsa
