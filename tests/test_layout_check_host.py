"""CPU-only: the span arithmetic behind every operator's argument checks (lattisense_amd/csrc/layout_check.h, compiled for the
host by tests/cpp/test_layout_check.cpp with g++ -fsanitize=address,undefined) against a word-by-word model.

An operand is `batch` items of `words` words, item b at base + b * stride; stride 0 is one item shared by the batch.  Overlap is
exact: padding belongs to nobody, operands may interleave.  The model marks, in a small array, every word the items of each
operand really occupy (and every word of each hull, to see that interleaved cases are reached), and requires
  apart  <=>  the items share no word            (layouts whose own items overlap: the hulls decide)
over every combination of base offset, stride (0, dense, padded, padded odd) and batch 1..4 of two operands of equal and of
different item sizes.  Two hand-made cases put strides near 2^40 words, where a 32-bit or a 64-bit intermediate would wrap.

The rule of the hoisted rotations (one_of_outputs_may_be_input: lsa_ckks_rotate_many and lsa_bfv_rotate_many) gets the same
treatment: one input and two or three outputs of one stride, every base offset, accepted exactly when no two outputs share a word,
every output either has the input's base and stride or shares no word with it, and at most one output is the input.

The rule of the indexed-array operators (one_against_array, dense_array: lsa_bfv_expand, lsa_bfv_pack, lsa_bfv_select) likewise:
one batched operand against `count` batched entries at stride s_index, accepted exactly when the operand is entry 0 itself (and
then shares no word with a later entry) or shares no word with any entry; the refusal names entry 0 or a later entry as the
marked words do."""
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACE = 112       # words of the model's address space
ORIGIN = 1 << 20  # byte address of word 0 (16-byte aligned)


def _exe(tmp_path):
    exe = str(tmp_path / "test_layout_check")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_layout_check.cpp"), "-o", exe])
    return exe


def _run(exe, cases, mode=None):
    lines = [" ".join("%d" % x for x in c) + "\n" for c in cases]
    out = subprocess.run([exe] + ([mode] if mode else []), input="".join(lines), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    got = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    assert len(got) == len(cases)
    return got


def _hull(base_w, stride, words, batch):
    return set(range(base_w, base_w + (batch - 1) * stride + words))


def _items(base_w, stride, words, batch):
    s = set()
    for b in range(batch):
        s.update(range(base_w + b * stride, base_w + b * stride + words))
    return s


def test_spans_against_marked_words(tmp_path):
    exe = _exe(tmp_path)
    WA = 4
    cases, model = [], []
    for wb in (4, 2):
        for sa, sb in itertools.product((0, WA, WA + 2, WA + 3, WA + 8), (0, wb, wb + 2, wb + 5, wb + 9)):
            for batch in (1, 2, 3, 4):
                base_a = 24
                for base_b in range(0, 64):
                    cases.append((ORIGIN + 8 * base_a, sa, WA, ORIGIN + 8 * base_b, sb, wb, batch))
                    model.append((base_a, sa, WA, base_b, sb, wb, batch))
    got = _run(exe, cases)
    seen = {"apart": 0, "hull_only": 0, "real": 0, "same": 0, "interleaved": 0}
    for (ba, sa, wa, bb, sb, wb, batch), g in zip(model, got):
        apart, same, same_or_apart, ok, ok_shared, aligned, end_hi, end_lo = g
        ha, hb = _hull(ba, sa, wa, batch), _hull(bb, sb, wb, batch)
        assert max(ha) < SPACE and max(hb) < SPACE
        ia, ib = _items(ba, sa, wa, batch), _items(bb, sb, wb, batch)
        assert ia <= ha and ib <= hb
        key = (ba, sa, wa, bb, sb, wb, batch)
        valid = (sa == 0 or sa >= wa) and (sb == 0 or sb >= wb)
        want_apart = not (ia & ib) if valid else not (ha & hb)
        assert bool(apart) == want_apart, key
        want_same = ba == bb and sa == sb and wa == wb
        assert bool(same) == want_same, key
        assert bool(same_or_apart) == (want_same or want_apart), key
        assert bool(ok) == (sa >= wa), key
        assert bool(ok_shared) == (sa >= wa or sa == 0), key
        assert bool(aligned) == (ba % 2 == 0 and sa % 2 == 0), key
        assert (end_hi << 64) + end_lo == ORIGIN + 8 * (max(ha) + 1), key
        seen["apart"] += bool(apart)
        seen["hull_only"] += bool((ha & hb) and not (ia & ib))
        seen["interleaved"] += bool(apart and (ha & hb))
        seen["real"] += bool(ia & ib)
        seen["same"] += want_same
    assert all(seen.values()), seen     # the sweep reached every kind of case


def test_misaligned_base_and_negative_stride(tmp_path):
    exe = _exe(tmp_path)
    got = _run(exe, [(ORIGIN + 8, 8, 4, ORIGIN + 512, 8, 4, 2),       # base on an 8-byte, not a 16-byte boundary
                     (ORIGIN + 4, 8, 4, ORIGIN + 512, 8, 4, 2),       # not even word aligned
                     (ORIGIN, -8, 4, ORIGIN + 512, 8, 4, 2),          # a negative stride is no layout
                     (ORIGIN, 3, 4, ORIGIN + 512, 8, 4, 2)])          # items overlap each other
    assert [g[5] for g in got] == [0, 0, 1, 0]
    assert [g[3] for g in got] == [1, 1, 0, 0]
    assert [g[4] for g in got] == [1, 1, 0, 0]


def test_strides_near_2_to_40_words(tmp_path):
    exe = _exe(tmp_path)
    S, W = (1 << 40) + 6, 1 << 12
    base_a = 1 << 30
    # batch 3: the hull is 2 S + W words.  (2 S * 8 = 2^44 + 96 bytes: a 32-bit product keeps only the 96.)
    end3 = base_a + 8 * (2 * S + W)
    # batch 2^31 - 1: the hull passes 2^64 bytes.  With 64-bit arithmetic the end wraps to a small address and everything
    # above `a` would look apart.
    big = (1 << 31) - 1
    end_big = base_a + 8 * ((big - 1) * S + W)
    assert end_big >= 1 << 64
    k = 1 << 20                                            # item k of a starts past 2^63 bytes
    item_k = base_a + 8 * k * S
    assert (1 << 63) < item_k < (1 << 64)
    cases = [(base_a, S, W, end3, S, W, 3),                 # b starts exactly where a's hull ends
             (base_a, S, W, end3 - 8, S, W, 3),             # one word earlier: b's item 0 shares a's last word
             (base_a, S, W, base_a + 8 * W, 0, W, 3),       # b shared, in a's first padding: interleaved, no common word
             (base_a, S, W, base_a + 8 * (W - 1), 0, W, 3), # ... one word earlier
             (base_a, S, W, base_a + 8 * W, S, W, 3),       # b's items all in a's paddings
             (end3, 0, W, base_a, S, W, 3),                 # a shared and behind b's hull
             (base_a, S, W, item_k + 8 * (W - 1), 0, W, big),   # a's hull passes 2^64; b shared, on the last word of item k
             (base_a, S, W, item_k + 8 * W, 0, W, big),     # ... just behind item k
             (base_a, S, W, base_a - 8 * W, 0, W, big)]     # ... and before a altogether
    got = _run(exe, cases)
    assert [g[0] for g in got] == [1, 0, 1, 0, 1, 1, 0, 1, 1]
    assert (got[0][6] << 64) + got[0][7] == end3
    assert (got[6][6] << 64) + got[6][7] == end_big


def _many_model(batch, words, base_in, s_in, s_out, outs):
    """(accepted, in_place, violated rules) from the marked words; bases in words"""
    inp = _items(base_in, s_in, words, batch)
    its = [_items(b, s_out, words, batch) for b in outs]
    is_in = [b == base_in and s_out == s_in for b in outs]
    broken = set()
    if any(its[i] & its[j] for i in range(len(outs)) for j in range(i)):
        broken.add(1)
    if any((it & inp) and not same for it, same in zip(its, is_in)):
        broken.add(2)
    if sum(is_in) > 1:
        broken.add(3)
    return not broken, (is_in.index(True) if not broken and any(is_in) else -1), broken


def test_rotate_many_rule_against_marked_words(tmp_path):
    exe = _exe(tmp_path)
    W, base_in = 4, 24
    model = []
    for s_in, s_out in itertools.product((W, W + 2, W + 6), repeat=2):
        for batch in (1, 2, 3):
            for b0, b1 in itertools.product(range(0, 64, 2), repeat=2):
                model.append((batch, W, base_in, s_in, s_out, (b0, b1)))
    for batch in (2, 3):                                    # three outputs: the input, one interleaved with it, one moving
        for b2 in range(0, 80, 2):
            model.append((batch, W, base_in, 3 * W + 4, 3 * W + 4, (base_in, base_in + W + 2, b2)))
            model.append((batch, W, base_in, 3 * W + 4, 3 * W + 4, (b2, base_in + W + 2, base_in)))
    cases = [(batch, w, ORIGIN + 8 * bi, si, so, len(outs)) + tuple(ORIGIN + 8 * b for b in outs) for batch, w, bi, si, so, outs in model]
    got = _run(exe, cases, "many")
    seen = {"ok": 0, "in_place": 0, "interleaved_in_place": 0, 1: 0, 2: 0, 3: 0}
    for m, (code, in_place) in zip(model, got):
        ok, want_in_place, broken = _many_model(*m)
        assert (code == 0) == ok, (m, code, broken)
        assert in_place == want_in_place, (m, in_place)
        if not ok:
            assert code in broken, (m, code, broken)       # the rule it names is one that the layout breaks
            seen[code] += 1
        seen["ok"] += ok
        seen["in_place"] += ok and in_place >= 0
        seen["interleaved_in_place"] += ok and in_place >= 0 and len(m[5]) == 3
    assert all(seen.values()), seen
    # no output at all, and one output: the rule holds trivially / is same-or-apart
    assert _run(exe, [(2, W, ORIGIN, W, W, 0), (2, W, ORIGIN, W, W, 1, ORIGIN), (2, W, ORIGIN, W, W, 1, ORIGIN + 8 * W),
                      (2, W, ORIGIN, 2 * W, 2 * W, 1, ORIGIN + 8 * W)], "many") == [(0, -1), (0, 0), (2, -1), (0, -1)]


def _array_model(batch, words, base_one, s_one, base_arr, s_arr, s_index, count):
    """the code one_against_array owes, from the marked words of every entry; bases in words"""
    one = _items(base_one, s_one, words, batch)
    entries = [_items(base_arr + i * s_index, s_arr, words, batch) for i in range(count)]
    is0 = base_one == base_arr and s_one == s_arr
    if not is0 and one & entries[0]:
        return 2
    if any(one & e for e in entries[1:]):
        return 3
    return 1 if is0 else 0


def test_indexed_array_rule_against_marked_words(tmp_path):
    """lsa_bfv_expand / lsa_bfv_pack / lsa_bfv_select: one batched operand against `count` batched entries at stride s_index.  Every
    word of every entry is marked; the operand is moved word by word from before the array to behind it, at the array's own stride,
    at a wider one (its items then interleave with the items of an entry) and at a narrower one."""
    exe = _exe(tmp_path)
    base_arr = 16
    model = []
    for words in (2, 4, 6):
        for batch in (1, 2, 3):
            for s_arr in (words, words + 2, 2 * words + 2):
                for gap in (0, 2, batch * s_arr + words):               # dense; a small gap; room for a whole operand
                    s_index = batch * s_arr + gap
                    for count in (1, 2, 3, 4):
                        end = base_arr + (count - 1) * s_index + (batch - 1) * s_arr + words
                        for s_one in {s_arr, words, 2 * words + 2}:
                            for base_one in range(0, end + 3):
                                model.append((batch, words, base_one, s_one, base_arr, s_arr, s_index, count))
    cases = [(b, w, ORIGIN + 8 * bo, so, ORIGIN + 8 * ba, sa, si, n) for b, w, bo, so, ba, sa, si, n in model]
    got = _run(exe, cases, "array")
    seen = {0: 0, 1: 0, 2: 0, 3: 0, "in_padding": 0, "between_items": 0, "one_word_of_later_entry": 0, "dense": 0, "not_dense": 0}
    for m, (code, dense) in zip(model, got):
        batch, words, base_one, s_one, base_arr, s_arr, s_index, count = m
        assert code == _array_model(*m), (m, code)
        assert bool(dense) == (s_index == batch * s_arr), m
        seen[code] += 1
        seen["dense" if dense else "not_dense"] += 1
        one = _items(base_one, s_one, words, batch)
        hulls = [_hull(base_arr + i * s_index, s_arr, words, batch) for i in range(count)]
        whole = set(range(base_arr, max(hulls[-1]) + 1))
        if code == 0 and one <= whole:
            seen["in_padding"] += not any(one & h for h in hulls)            # wholly in the padding between two entries
            seen["between_items"] += any(one & h for h in hulls)            # between the items of an entry
        if code == 3:
            entries = [_items(base_arr + i * s_index, s_arr, words, batch) for i in range(1, count)]
            seen["one_word_of_later_entry"] += sum(len(one & e) for e in entries) == 1
    assert all(seen.values()), seen     # the sweep reached every kind of case


def test_indexed_array_dense_and_one_word_below(tmp_path):
    """s_index == batch * stride exactly, and one word below (which the entry points refuse: the entries then run into each other):
    `dense` holds at equality alone, and the answer still follows the marked words"""
    exe = _exe(tmp_path)
    batch, words, s_arr, count, base_arr = 3, 4, 6, 3, 16
    for s_index, want_dense in ((batch * s_arr, 1), (batch * s_arr - 1, 0), (batch * s_arr + 1, 0)):
        model = [(batch, words, base_one, s_arr, base_arr, s_arr, s_index, count) for base_one in range(0, base_arr + count * s_index + 8)]
        got = _run(exe, [(b, w, ORIGIN + 8 * bo, so, ORIGIN + 8 * ba, sa, si, n) for b, w, bo, so, ba, sa, si, n in model], "array")
        for m, (code, dense) in zip(model, got):
            assert dense == want_dense, m
            assert code == _array_model(*m), (m, code)


def test_indexed_array_strides_near_2_to_40_words(tmp_path):
    exe = _exe(tmp_path)
    W, S = 1 << 12, (1 << 40) + 6
    base_arr = 1 << 30
    # a batch near 2^31: the entries' batch stride A keeps s_index = batch * A (+ padding) below 2^63 words and the array below 2^64
    # bytes; the operand's own stride is S, so ITS hull passes 2^64 bytes -- a 64-bit end would wrap to a small address
    big, A = (1 << 31) - 1, (1 << 28) + 2
    s_index, count = big * A + 2 * W, 3
    entry_words = (big - 1) * A + W
    arr_end = base_arr + 8 * ((count - 1) * s_index + entry_words)
    assert arr_end < (1 << 64) and base_arr + 8 * ((big - 1) * S + W) >= (1 << 64)
    e1 = base_arr + 8 * s_index
    cases = [(big, W, arr_end, S, base_arr, A, s_index, count),                     # starts where the array ends: disjoint hulls
             (big, W, arr_end, 0, base_arr, A, s_index, count),                     # one shared item there
             (big, W, arr_end - 8, 0, base_arr, A, s_index, count),                 # ... one word earlier: the last word of the last entry
             (big, W, base_arr - 8 * W, 0, base_arr, A, s_index, count),            # just before the array
             (big, W, base_arr - 8 * (W - 1), 0, base_arr, A, s_index, count),      # ... on the first word of entry 0
             (big, W, base_arr + 8 * entry_words, 0, base_arr, A, s_index, count),  # in the padding behind entry 0
             (big, W, e1 - 8 * (W - 1), 0, base_arr, A, s_index, count),            # ... reaching the first word of entry 1
             (big, W, base_arr, A, base_arr, A, s_index, count),                    # entry 0 itself
             (big, W, base_arr, A, base_arr, A, big * A, count)]                    # ... of a dense array
    got = _run(exe, cases, "array")
    assert got == [(0, 0), (0, 0), (3, 0), (0, 0), (2, 0), (0, 0), (3, 0), (1, 0), (1, 1)]
    # batch 3 at stride S: the operand's items lie in the paddings between the items of entry 0 / one word into an item of entry 2
    s_index, count = 4 * S, 4
    e2 = base_arr + 8 * 2 * s_index
    cases = [(3, W, base_arr + 8 * W, S, base_arr, S, s_index, count),
             (3, W, base_arr + 8 * (W - 1), S, base_arr, S, s_index, count),
             (3, W, e2 + 8 * (S + W - 1), S, base_arr, S, s_index, count),
             (3, W, e2 + 8 * (S + W), S, base_arr, S, s_index, count)]
    assert [g[0] for g in _run(exe, cases, "array")] == [0, 2, 3, 0]
