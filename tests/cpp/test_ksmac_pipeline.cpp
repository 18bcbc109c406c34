// Host-side checks of the fused key MAC's cached twiddles (lattisense_amd/csrc/ntt_r16.h, "twiddles once per workgroup"), for the
// splits that take them (MU = 8 and MU = 7):
//   cache: with tables filled with their own indices, r16_twc_fill followed by r16_twc_get returns, for every tile of N = 2^14 ..
//     2^17, every lane, both radix groups, every stage and butterfly, exactly the entry ntt_load_tw_fp reads; no two lanes' private
//     slots overlap; a word is read only by the wave that wrote it; the footprint is the one the launch requests;
//   group parity: r16_group_twc agrees bit for bit with r16_group on random FP64-engine inputs, both images of either split.
// Built with -fsanitize=address,undefined and run by tests/test_ksmac_pipeline_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../lattisense_amd/csrc/ntt_r16.h"

static u64 rng_state = 0x13198A2E03707344ull;
static u64 rnd() {
    u64 z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static const char* g_what = "";
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s (line %d) %s\n", #c, __LINE__, g_what); std::exit(1); } } while (0)

template <int MU>
static R16Limb make_limb(const double* table, int logn, u64 q) {
    R16Limb L;
    std::memset(&L, 0, sizeof(L));
    L.md.q = q;
    L.twd = table;
    L.q = (double)q;
    L.qinv = 1.0 / L.q;
    L.s_lo = logn - MU;
    return L;
}
template <int MU>
static void lane_groups(int tile, int tid, unsigned& G1, unsigned& G2) {   // as k_ntt_r16_ksmac forms them
    NttBlockCtx bc;
    std::memset(&bc, 0, sizeof(bc));
    bc.tile = tile;
    int k, i;
    r16_lane<1, MU>(tid, k, i);
    G1 = r16_G1<1, MU>(bc, k);
    G2 = (G1 << 4) + ((unsigned)i << (8 - MU));
}

// ------------------------------------------------------------------------------------------------ cache
template <int MU>
static void test_cache_layout() {
    typedef R16Twc<MU> C;
    g_what = MU == 8 ? "layout MU=8" : "layout MU=7";
    CHECK(ks_fused_twc(MU, true) ? ks_fused_lds_bytes(MU, true) == (size_t)(LSA_R16_LDS_WORDS + C::WORDS) * 8
                                 : ks_fused_lds_bytes(MU, true) == (size_t)LSA_R16_LDS_WORDS * 8);
    CHECK(ks_fused_lds_bytes(MU, false) == (size_t)LSA_R16_LDS_WORDS * 8);   // integer engine: the image alone
    CHECK(2 * ((size_t)(LSA_R16_LDS_WORDS + C::WORDS) * 8) <= 160 * 1024);    // two workgroups per CU
    std::vector<int> owner(C::WORDS, -1);   // the wave that writes the word
    int used = 0;
    for (int tid = 0; tid < LSA_R16_THREADS; tid++) {
        int k, i;
        r16_lane<1, MU>(tid, k, i);
        for (int g = 0; g < C::NG; g++)
            for (int e = 0; e < C::E2; e++) {
                const int p = C::priv(tid, g, e);
                CHECK(p >= C::SHARED && p < C::WORDS);
                CHECK(owner[p] == -1);   // no two lanes (and no two entries of a lane) share a slot
                owner[p] = tid >> 6;
                used++;
                if (e & 1) CHECK(p % 2 == 0 && C::priv(tid, g, e + 1) == p + 1);   // the pair of one 16-byte read
            }
        for (int e = 0; e < 15; e++) {
            const int p = C::shared(k, e);
            CHECK(p >= 0 && p < C::SHARED);
            if (i == 0) {   // the transform's filling lane
                CHECK(owner[p] == -1);
                owner[p] = tid >> 6;
                used++;
            }
            if (e & 1) CHECK(p % 2 == 0 && C::shared(k, e + 1) == p + 1);
        }
    }
    for (int tid = 0; tid < LSA_R16_THREADS; tid++) {   // a wave reads only what it wrote
        int k, i;
        r16_lane<1, MU>(tid, k, i);
        for (int e = 0; e < 15; e++) CHECK(owner[C::shared(k, e)] == tid >> 6);
        for (int g = 0; g < C::NG; g++)
            for (int e = 0; e < C::E2; e++) CHECK(owner[C::priv(tid, g, e)] == tid >> 6);
    }
    CHECK(used == (15 << (12 - MU)) + LSA_R16_THREADS * C::NG * C::E2);
    // conflict-free private reads: the lanes of a wave read consecutive 8-byte (stage 0) or 16-byte (pairs) words
    for (int g = 0; g < C::NG; g++)
        for (int e = 0; e < C::E2; e++)
            for (int lane = 1; lane < 64; lane++) CHECK(C::priv(lane, g, e) - C::priv(lane - 1, g, e) == (e == 0 ? 1 : 2));
}
template <int MU>
static void test_cache_values(int logn) {
    typedef R16Twc<MU> C;
    static char what[64];
    std::snprintf(what, sizeof(what), "values MU=%d logn=%d", MU, logn);
    g_what = what;
    const long long N = 1LL << logn;
    std::vector<double> table(N);
    for (long long x = 0; x < N; x++) table[x] = (double)x;   // every entry names itself
    const R16Limb L = make_limb<MU>(table.data(), logn, (1ull << 46) + 1);
    std::vector<double> twc(C::WORDS);
    for (int tile = 0; tile < (1 << (logn - 12)); tile++) {
        for (auto& x : twc) x = -1.0;
        for (int tid = 0; tid < LSA_R16_THREADS; tid++) {
            unsigned G1, G2;
            lane_groups<MU>(tile, tid, G1, G2);
            r16_twc_fill<MU>(twc.data(), tid, L, G1, G2);
        }
        for (int tid = 0; tid < LSA_R16_THREADS; tid++) {
            unsigned G1, G2;
            lane_groups<MU>(tile, tid, G1, G2);
            double w0[15], w1[15], want[8];
            r16_twc_get<MU, 0>(twc.data(), tid, w0);
            r16_twc_get<MU, 1>(twc.data(), tid, w1);
            for (int j = 0; j < 4; j++) {
                const int s = L.s_lo + j;
                ntt_load_tw_fp(L.twd + (1LL << s), s, j, G1, want);
                for (int k = 0; k < (1 << j); k++) {
                    CHECK(want[k] >= (double)(1LL << s) && want[k] < (double)(2LL << s));   // an entry of stage s
                    CHECK(w0[(1 << j) - 1 + k] == want[k]);
                }
            }
            for (int g = 0; g < C::NG; g++)
                for (int j = 0; j < C::R2; j++) {
                    const int s = L.s_lo + 4 + j;
                    ntt_load_tw_fp(L.twd + (1LL << s), s, j, G2 + (unsigned)g, want);
                    for (int k = 0; k < (1 << j); k++) {
                        CHECK(want[k] >= (double)(1LL << s) && want[k] < (double)(2LL << s));
                        CHECK(w1[g * C::E2 + (1 << j) - 1 + k] == want[k]);
                    }
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------ group parity
template <int MU>
static void test_group_parity(int logn) {
    typedef R16Twc<MU> C;
    g_what = MU == 8 ? "group parity MU=8" : "group parity MU=7";
    const u64 q = 70368743489537ull;   // (any modulus below 2^47: the comparison is bit for bit)
    const long long N = 1LL << logn;
    std::vector<double> table(N);
    for (auto& x : table) x = (double)(rnd() % q);
    const R16Limb L = make_limb<MU>(table.data(), logn, q);
    NttPassArgs a;
    std::memset(&a, 0, sizeof(a));
    a.logn = logn;
    a.s_lo = logn - MU;
    a.mu = MU;
    a.tau = 12;
    NttBlockCtx bc;
    std::memset(&bc, 0, sizeof(bc));
    bc.fp = 1;
    std::vector<double> twc(C::WORDS);
    for (int tile : {0, 1, (1 << (logn - 12)) - 1}) {
        bc.tile = tile;
        for (int tid = 0; tid < LSA_R16_THREADS; tid++) {
            unsigned G1, G2;
            lane_groups<MU>(tile, tid, G1, G2);
            r16_twc_fill<MU>(twc.data(), tid, L, G1, G2);
        }
        for (int tid = 0; tid < LSA_R16_THREADS; tid++) {
            unsigned G1, G2;
            lane_groups<MU>(tile, tid, G1, G2);
            u64 v0[16], v1[16], u0[16], u1[16];
            for (int e = 0; e < 16; e++) {
                const double x = (double)(long long)(rnd() % q) - (double)(q / 2);   // |x| <= q / 2: a raw hand-off between passes
                v0[e] = u0[e] = d_to_bits(x);
                const double y = (double)(long long)(rnd() % (8 * q)) - (double)(4 * q);   // after four forward stages: < 5.4 q
                v1[e] = u1[e] = d_to_bits(y);
            }
            double w[15];
            r16_group<1, 0, MU>(v0, a, bc, L, G1);
            r16_twc_get<MU, 0>(twc.data(), tid, w);
            r16_group_twc<0, MU>(u0, false, L, w);
            CHECK(std::memcmp(v0, u0, sizeof(v0)) == 0);
            r16_group<1, 1, MU>(v1, a, bc, L, G2);
            r16_twc_get<MU, 1>(twc.data(), tid, w);
            r16_group_twc<1, MU>(u1, false, L, w);
            CHECK(std::memcmp(v1, u1, sizeof(v1)) == 0);
        }
    }
}

int main() {
    test_cache_layout<8>();
    test_cache_layout<7>();
    for (int logn = 14; logn <= 17; logn++) {
        test_cache_values<8>(logn);
        test_cache_values<7>(logn);
    }
    test_group_parity<8>(15);
    test_group_parity<8>(16);
    test_group_parity<7>(14);
    std::printf("OK ksmac_pipeline\n");
    return 0;
}
