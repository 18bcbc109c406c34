// Host-side check of lattisense_amd/csrc/ntt_chunk.h: how launch_ntt cuts a batch into chunks under lsa_set_ntt_chunk_mib
// (ntt_chunk_items) and what a chunk's launches get as their fused operands (ntt_chunk_rebase).
//
//   ntt_chunk_items   against a search in exact integer arithmetic (the largest count whose limbs fit, at least one, at most
//                     the batch), n = 2^13 .. 2^17, active rows 1 .. 64, batch 1 .. 9, mib in {0, 1, 2, 256}; the chunks tile
//                     the batch exactly, ragged last chunk included
//   ntt_chunk_rebase  every fusion shape the operators build (ops.hip), on fake base addresses and pairwise distinct strides:
//                     each non-null operand moved by b0 items of ITS stride, a shared operand (stride 0) and a null one where
//                     they were, every other byte of the arguments as it was
// Compiled and run by tests/test_ntt_chunk_host.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../lattisense_amd/csrc/ntt_chunk.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s (line %d) %s\n", #c, __LINE__, g_what); std::exit(1); } } while (0)
static const char* g_what = "";

static void test_items() {
    g_what = "ntt_chunk_items";
    const int mibs[] = {0, 1, 2, 256};
    long long split = 0, ragged = 0;
    for (int logn = 13; logn <= 17; logn++)
        for (int rows = 1; rows <= 64; rows++)
            for (int batch = 1; batch <= 9; batch++)
                for (int mib : mibs) {
                    const int n = 1 << logn;
                    const int got = ntt_chunk_items(n, rows, batch, mib);
                    int want = batch;
                    if (mib > 0) {   // the largest count in [1, batch] whose active limbs fit, one if not even one does
                        want = 1;
                        for (int c = 2; c <= batch; c++)
                            if ((unsigned __int128)c * 8u * (unsigned)n * (unsigned)rows <= ((unsigned __int128)mib << 20)) want = c;
                    }
                    CHECK(got == want);
                    CHECK(got >= 1 && got <= batch);
                    int covered = 0, chunks = 0, last = 0;
                    for (int b0 = 0; b0 < batch; b0 += got) {   // the launcher's walk
                        const int nb = batch - b0 < got ? batch - b0 : got;
                        CHECK(nb >= 1 && nb <= got && b0 == covered);
                        CHECK(nb == got || b0 + nb == batch);   // only the last chunk may be short
                        covered += nb;
                        chunks++;
                        last = nb;
                    }
                    CHECK(covered == batch && chunks == (batch + got - 1) / got);
                    split += chunks > 1;
                    ragged += chunks > 1 && last != got;
                }
    CHECK(split > 0 && ragged > 0);   // (the ranges above do cut batches, unevenly too)
    CHECK(ntt_chunk_items(8192, 0, 5, 1) == 5);      // no active row counts as one: 16 items fit
    CHECK(ntt_chunk_items(1 << 17, 0, 5, 1) == 1);
    CHECK(ntt_chunk_items(8192, 6, 5, -3) == 5);     // (the setter refuses negative values; here they mean "off")
    CHECK(ntt_chunk_items(8192, 6, 5, 1) == 2 && ntt_chunk_items(8192, 8, 5, 1) == 2 && ntt_chunk_items(8192, 9, 5, 1) == 1);
}

// ---- rebasing
struct Operand { bool present; long long stride; };
struct Shape {
    const char* name;
    int epi, pro;
    Operand a, b, base, out, last, pt;
    bool k, k2, scatter;
};

static u64* fake(int slot) { return reinterpret_cast<u64*>((uintptr_t)0x100000000000ull + (uintptr_t)slot * 0x001000000000ull); }

static NttPassArgs make_args(const Shape& s) {
    NttPassArgs a;
    unsigned char* raw = reinterpret_cast<unsigned char*>(&a);
    for (size_t i = 0; i < sizeof a; i++) raw[i] = (unsigned char)(37 * i + 11);   // every field (later ones too) tells
    a.fz_epi = s.epi;
    a.fz_pro = s.pro;
    a.fz_a = s.a.present ? fake(1) : nullptr;
    a.fz_b = s.b.present ? fake(2) : nullptr;
    a.fz_base = s.base.present ? fake(3) : nullptr;
    a.fz_out = s.out.present ? fake(4) : nullptr;
    a.fz_last = s.last.present ? fake(5) : nullptr;
    a.fz_pt = s.pt.present ? fake(6) : nullptr;
    a.fz_k = s.k ? fake(7) : nullptr;
    a.fz_k2 = s.k2 ? fake(8) : nullptr;
    a.fz_scatter = s.scatter ? reinterpret_cast<const unsigned*>(fake(9)) : nullptr;
    a.src = fake(10);
    a.dst = fake(11);
    a.fz_a_stride = s.a.stride;
    a.fz_b_stride = s.b.stride;
    a.fz_base_stride = s.base.stride;
    a.fz_out_stride = s.out.stride;
    a.fz_last_stride = s.last.stride;
    a.fz_pt_stride = s.pt.stride;
    return a;
}

static void moved(const u64* got, const u64* was, long long b0, long long stride) {
    if (!was) {
        CHECK(got == nullptr);
        return;
    }
    CHECK((uintptr_t)got == (uintptr_t)was + (uintptr_t)(b0 * stride) * sizeof(u64));
}

static void test_rebase() {
    // strides: pairwise distinct, none the data stride; {true, 0}: an operand the whole batch shares; {false, s}: absent, and a
    // stride it would have had (must not matter)
    const Shape shapes[] = {
        // ModDown tail (relin: plain store; rotate: through the index map), base on the leading polynomials
        {"epi 1, ModDown tail", 1, 0, {true, 147472}, {false, 3}, {true, 98326}, {true, 65610}, {false, 5}, {false, 7}, true, false, false},
        {"epi 1, ModDown tail of a rotation", 1, 0, {true, 147472}, {false, 3}, {true, 98326}, {true, 98326 + 26}, {false, 5}, {false, 7}, true, false, true},
        // ckks_rescale: head (last limb) + tail, no base
        {"pro 1 + epi 1, rescale", 1, 1, {true, 98310}, {false, 3}, {false, 11}, {true, 73754}, {true, 98310 + 2}, {false, 7}, true, false, false},
        // HMult + relin + rescale: merged ModDown + rescale
        {"pro 2 + epi 2, merged rescale tail", 2, 2, {true, 163870}, {false, 3}, {true, 65574}, {true, 49178}, {true, 163870 + 8192}, {false, 7}, true, true, false},
        // BFV ct x pt_mul: plaintexts per item or shared, with and without a running sum
        {"epi 3, pt_mul", 3, 0, {true, 32774}, {false, 3}, {false, 11}, {true, 65562}, {false, 5}, {false, 7}, false, false, false},
        {"epi 3, pt_mul with a running sum, shared plaintext", 3, 0, {true, 0}, {false, 3}, {true, 65546}, {true, 65562}, {false, 5}, {false, 7}, false, false, false},
        // BFV rotate-and-MAC
        {"epi 4, rotate-and-MAC", 4, 0, {true, 114698}, {false, 3}, {true, 65546}, {true, 65562}, {false, 5}, {true, 32774}, true, false, true},
        {"epi 4, rotate-and-MAC, shared plaintext, no base", 4, 0, {true, 114698}, {false, 3}, {false, 11}, {true, 65562}, {false, 5}, {true, 0}, true, false, true},
        // the prologues without an epilogue
        {"pro 3, product prologue", 0, 3, {true, 65546}, {true, 65554}, {false, 11}, {false, 13}, {false, 5}, {false, 7}, false, false, false},
        {"pro 3, product prologue, shared second factor", 0, 3, {true, 65546}, {true, 0}, {false, 11}, {false, 13}, {false, 5}, {false, 7}, false, false, false},
        {"pro 4, lift prologue", 0, 4, {false, 1}, {false, 3}, {false, 11}, {false, 13}, {true, 49162}, {false, 7}, false, false, false},
    };
    const long long b0s[] = {0, 1, 2, 4, 7, 100000};   // (100000 items x 163870 words: the product needs 64 bits)
    for (const Shape& s : shapes) {
        g_what = s.name;
        const NttPassArgs in = make_args(s);
        for (long long b0 : b0s) {
            const NttPassArgs got = ntt_chunk_rebase(in, (int)b0);
            moved(got.fz_a, in.fz_a, b0, in.fz_a_stride);
            moved(got.fz_b, in.fz_b, b0, in.fz_b_stride);
            moved(got.fz_base, in.fz_base, b0, in.fz_base_stride);
            moved(got.fz_out, in.fz_out, b0, in.fz_out_stride);
            moved(got.fz_last, in.fz_last, b0, in.fz_last_stride);
            moved(got.fz_pt, in.fz_pt, b0, in.fz_pt_stride);
            // everything else, bit for bit: the per-limb constants, the index map, src / dst / batch, the tables, the shape
            CHECK(got.fz_k == in.fz_k && got.fz_k2 == in.fz_k2 && got.fz_scatter == in.fz_scatter);
            CHECK(got.src == in.src && got.dst == in.dst && got.batch == in.batch && got.tw == in.tw && got.mods == in.mods);
            NttPassArgs back = got;
            back.fz_a = in.fz_a;
            back.fz_b = in.fz_b;
            back.fz_base = in.fz_base;
            back.fz_out = in.fz_out;
            back.fz_last = in.fz_last;
            back.fz_pt = in.fz_pt;
            CHECK(std::memcmp(&back, &in, sizeof in) == 0);
            if (b0 == 0) CHECK(std::memcmp(&got, &in, sizeof in) == 0);   // the first chunk and an unchunked launch: unchanged
        }
    }
}

int main() {
    test_items();
    test_rebase();
    std::printf("OK ntt_chunk\n");
    return 0;
}
