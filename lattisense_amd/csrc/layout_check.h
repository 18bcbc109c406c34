// layout_check.h — where a batched operand lives in memory, and whether two of them may be used together.  Plain C++, host only:
// the argument checks of every operator (entry_check.h for ops.hip and slot_sum.hip, linear_transform.hip, poly_eval.hip) go through these functions, and
// tests/cpp/test_layout_check.cpp compares them with a word-by-word model.
//
// An operand is `batch` items of `words` 64-bit words, item b at base + b * stride (stride in words).  stride == 0 means ONE item
// shared by the whole batch.  The kernels index exactly that way, and the element-wise ones move 16 bytes per lane, so every
// item has to start on a 16-byte boundary: base 16-byte aligned, stride even.
//
// Overlap is exact: two operands are `apart` when no item of one shares a word with an item of the other.  Padding belongs to
// nobody, so operands may interleave -- the task runtime hands over inputs that lie wherever their producers put them, with a
// fresh output slab possibly between two of them.  Disjoint HULLS (first word of item 0 to last word of the last item) settle
// the usual case in O(1); only interleaved hulls are walked, item by item over the operand with fewer items, two candidates
// of the other operand per item.  The hull of a shared operand (stride 0) and of a batch of one is the single item.  All
// arithmetic is 128-bit on byte addresses: a stride near 2^40 words times a batch near 2^31 does not fit 64 bits.
#pragma once
#include <cstddef>
#include <cstdint>

namespace lsa {
namespace layout {

typedef unsigned __int128 u128;

struct Span {
    uintptr_t base;     // byte address of item 0
    long long stride;   // words from one item to the next; 0: one item for the whole batch
    size_t words;       // words of one item
};
inline Span span_of(const void* p, long long stride, size_t words) { return Span{reinterpret_cast<uintptr_t>(p), stride, words}; }

// a stride the kernels can index: at least one item, or 0 where a shared operand is accepted
inline bool stride_ok(const Span& s, bool shared_ok) {
    if (s.stride == 0) return shared_ok;
    return s.stride > 0 && (unsigned long long)s.stride >= (unsigned long long)s.words;
}
// every item starts on a 16-byte boundary
inline bool aligned16(const Span& s) { return (s.base & 15) == 0 && (s.stride & 1) == 0; }

// words of the hull, batch >= 1 (a negative stride is no layout: stride_ok refuses it, here it counts as 0)
inline u128 hull_words(const Span& s, int batch) {
    const u128 step = s.stride > 0 ? (u128)(unsigned long long)s.stride : 0;
    return (u128)(batch > 1 ? batch - 1 : 0) * step + s.words;
}
// byte address one past the hull
inline u128 span_end(const Span& s, int batch) { return (u128)s.base + 8 * hull_words(s, batch); }

inline int item_count(const Span& s, int batch) { return s.stride == 0 || batch < 1 ? 1 : batch; }
// item [x, x + bytes) against the items of `s`, which lie in ascending order and do not overlap each other (stride_ok)
inline bool item_hits(u128 x, u128 bytes, const Span& s, int n) {
    const u128 base = s.base, step = 8 * (u128)(unsigned long long)s.stride, len = 8 * (u128)s.words;
    // j: the last item of s that starts at or before x (none: the first); only it and its successor can reach [x, x + bytes)
    u128 j = 0;
    if (n > 1 && x > base) {
        j = (x - base) / step;
        if (j > (u128)(n - 1)) j = (u128)(n - 1);
    }
    for (int k = 0; k < 2 && j + k < (u128)n; k++) {
        const u128 y = base + (j + k) * step;
        if (y < x + bytes && x < y + len) return true;
    }
    return false;
}
inline bool apart(const Span& a, const Span& b, int batch) {
    if (span_end(a, batch) <= (u128)b.base || span_end(b, batch) <= (u128)a.base) return true;   // disjoint hulls
    // a layout whose own items overlap (or run backwards) has no item order to rely on: its hull decides
    if ((a.stride != 0 && !stride_ok(a, false)) || (b.stride != 0 && !stride_ok(b, false))) return false;
    const int na = item_count(a, batch), nb = item_count(b, batch);
    const Span& few = na <= nb ? a : b;
    const Span& many = na <= nb ? b : a;
    const int nf = na <= nb ? na : nb, nm = na <= nb ? nb : na;
    for (int i = 0; i < nf; i++)
        if (item_hits((u128)few.base + 8 * (u128)i * (u128)(unsigned long long)few.stride, 8 * (u128)few.words, many, nm)) return false;
    return true;
}
// the same items: what an in-place call passes
inline bool same(const Span& a, const Span& b) { return a.base == b.base && a.stride == b.stride && a.words == b.words; }
// the rule of the element-wise operators: an output is one of its inputs, item for item, or shares no word with it
inline bool same_or_apart(const Span& a, const Span& b, int batch) { return same(a, b) || apart(a, b, batch); }

inline bool apart(const void* a, long long sa, size_t wa, const void* b, long long sb, size_t wb, int batch) {
    return apart(span_of(a, sa, wa), span_of(b, sb, wb), batch);
}

// the rule of the hoisted rotations (lsa_ckks_rotate_many, lsa_bfv_rotate_many): one input, n outputs.  The outputs are pairwise
// apart; each one IS the input (same) or is apart from it; at most one is the input -- that rotation is computed last, in two
// steps, from the intact input.  Returns ONE_OF_OK with *in_place = the output that is the input (-1: none), or the first violation
// (*in_place is then -1): a partial overlap with the input lets one tile store over what another still reads.
enum OneOf { ONE_OF_OK = 0, ONE_OF_OUTPUTS_OVERLAP = 1, ONE_OF_PARTLY_INPUT = 2, ONE_OF_TWO_ARE_INPUT = 3 };
inline OneOf one_of_outputs_may_be_input(const Span& in, const Span* outs, int n, int batch, int* in_place) {
    int found = -1;
    *in_place = -1;
    for (int i = 0; i < n; i++) {
        if (same(outs[i], in)) {
            if (found >= 0) return ONE_OF_TWO_ARE_INPUT;
            found = i;
        } else if (!apart(outs[i], in, batch)) {
            return ONE_OF_PARTLY_INPUT;
        }
        for (int j = 0; j < i; j++)
            if (!apart(outs[i], outs[j], batch)) return ONE_OF_OUTPUTS_OVERLAP;
    }
    *in_place = found;
    return ONE_OF_OK;
}

// the rule of the indexed-array operators (lsa_bfv_expand, lsa_bfv_pack, lsa_bfv_select): one batched operand against an array of
// `count` batched entries, entry i the span `arr` moved on by i * s_index words.  The levels of these operators work inside the
// array, entry 0 being read and written by the same tile, so `one` IS entry 0 (same) or shares no word with any entry, and being
// entry 0 it shares none with the others.  Disjoint hulls of the operand and of the whole array settle the usual case in O(1);
// else the entries are walked.  s_index >= batch * arr.stride is the caller's to check (dense below: equality).
enum OneVsArray { ONE_APART_FROM_ALL = 0, ONE_IS_ENTRY0 = 1, ONE_PARTLY_ENTRY0 = 2, ONE_OVERLAPS_ENTRY = 3 };
inline OneVsArray one_against_array(const Span& one, const Span& arr, long long s_index, int count, int batch) {
    const bool is0 = same(one, arr);
    const u128 step = s_index > 0 ? 8 * (u128)(unsigned long long)s_index : 0;
    if (!is0) {
        const u128 arr_end = span_end(arr, batch) + (u128)(count > 1 ? count - 1 : 0) * step;
        if (span_end(one, batch) <= (u128)arr.base || arr_end <= (u128)one.base) return ONE_APART_FROM_ALL;
        if (!apart(one, arr, batch)) return ONE_PARTLY_ENTRY0;
    }
    for (int i = 1; i < count; i++) {
        const u128 at = (u128)arr.base + (u128)i * step;
        if (at >> 64) break;   // past the address space: no operand has words there
        if (!apart(one, Span{(uintptr_t)at, arr.stride, arr.words}, batch)) return ONE_OVERLAPS_ENTRY;
    }
    return is0 ? ONE_IS_ENTRY0 : ONE_APART_FROM_ALL;
}
// the entries follow each other without a gap: the array is ONE batch of count * batch items of stride arr.stride
inline bool dense_array(const Span& arr, long long s_index, int batch) {
    return s_index > 0 && (u128)(unsigned long long)s_index == (u128)(unsigned)batch * (u128)(unsigned long long)arr.stride;
}

}  // namespace layout
}  // namespace lsa
