// Host-side check of the merged ModDown + rescale head per coefficient (lattisense_amd/csrc/ntt_core.h, rescale_head_t /
// rescale_head_centre / rescale_head_lift / rescale_head_in) -- the functions the load-side prologue of the forward transform
// (ntt_load_fix, integer branch) and the rescale-head form of the base conversion (k_baseconv<.., HEAD>: t and c) call -- against
// 128-bit integer arithmetic, for the modulus pairs (q_l, q_j) given on the command line:
//   t     = (A_l - conv_l) * P^-1 (+ B_l) mod q_l
//   c     = (t + h) mod q_l, h = (q_l - 1) / 2
//   lift_j = centred(t) mod q_j, centred(t) = t if t <= h else t - q_l     (what (c mod q_j) - (h mod q_j) has to equal)
//   in_j  = conv_j + lift_j mod q_j
// Residues 0, 1, h - 1, h, h + 1, q_l - 2, q_l - 1 and random ones for every operand of q_l; 0, 1, (q_j - 1) / 2, q_j - 1 and random
// ones for conv_j; factors 1, 2, q_l - 1, (q_l + 1) / 2 and random ones for P^-1.  The reduction is taken both ways wherever both
// apply: `near` (q_l <= 2 q_j, one conditional subtraction) and the general one (reduce_u64, any 64-bit value), and the prologue's
// ntt_load_fix is held to the same value, and so is the identity the conversion kernel's sum rests on: lift_j is the integer
// c - h reduced modulo q_j.  Built with -fsanitize=address,undefined and run by tests/test_rescale_head_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../lattisense_amd/csrc/ntt_core.h"

typedef __int128 i128;
typedef unsigned __int128 u128;
static u64 rng_state = 0x13198A2E03707344ull;
static u64 rnd() {
    u64 z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static u64 g_ql, g_qj;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s (line %d) q_l=%llu q_j=%llu\n", #c, __LINE__, (unsigned long long)g_ql, (unsigned long long)g_qj); std::exit(1); } } while (0)

static ModDev make_mod(u64 q) {
    ModDev m;
    m.q = q;
    u64 inv = q;   // Newton: q * inv == 1 mod 2^64 (q odd)
    for (int i = 0; i < 6; i++) inv *= 2 - q * inv;
    m.qinv = inv;
    m.r1 = (u64)((((u128)1) << 64) % q);
    m.r2 = (u64)(((u128)m.r1 * m.r1) % q);
    return m;
}
static u64 mod_i(i128 x, u64 q) {
    i128 r = x % (i128)q;
    return (u64)(r < 0 ? r + (i128)q : r);
}

static long long checks = 0;
static void test_pair(u64 ql, u64 qj) {
    g_ql = ql;
    g_qj = qj;
    CHECK((ql & 1) && (qj & 1) && (ql >> 61) == 0 && (qj >> 61) == 0 && ql > 16 && qj > 16);
    const ModDev ml = make_mod(ql), mj = make_mod(qj);
    CHECK(ml.q * ml.qinv == 1 && mj.q * mj.qinv == 1);
    const u64 h = (ql - 1) >> 1;
    const u64 hq = reduce_u64(h, mj);
    CHECK(hq == h % qj);
    const bool near = ql <= 2 * qj;

    std::vector<u64> rl = {0, 1, h - 1, h, h + 1, ql - 2, ql - 1};
    for (int i = 0; i < 6; i++) rl.push_back(rnd() % ql);
    std::vector<u64> rj = {0, 1, (qj - 1) / 2, qj - 1};
    for (int i = 0; i < 4; i++) rj.push_back(rnd() % qj);
    std::vector<u64> pinvs = {1, 2, ql - 1, (ql + 1) / 2};
    for (int i = 0; i < 3; i++) pinvs.push_back(1 + rnd() % (ql - 1));

    // t: every operand over the edge residues
    for (u64 pinv : pinvs) {
        const u64 pinv_m = (u64)(((u128)pinv << 64) % ql);   // Montgomery form, as Context::pinv_vec holds it
        for (u64 a : rl)
            for (u64 cv : rl) {
                const u64 t = rescale_head_t(a, cv, pinv_m, ml);
                CHECK(t < ql);
                CHECK(t == mod_i(((i128)a - (i128)cv) * (i128)pinv, ql));
                for (u64 bb : rl) {   // with a base word: the addition k_sub_mul makes
                    CHECK(add_mod(t, bb, ql) == mod_i(((i128)a - (i128)cv) * (i128)pinv + (i128)bb, ql));
                    checks++;
                }
            }
    }
    // a factor and operands that land t on each edge residue exactly: t = (a - 0) * 1
    NttLoadFix f;
    f.head = f.add = true;
    f.fp = f.raw = f.fp_lift = f.lift = false;
    f.near = near;
    f.ql = ql;
    f.h = h;
    f.hq = hq;
    f.hd = f.qld = 0.0;
    f.mi = mj;
    for (u64 want_t : rl) {
        const u64 t = rescale_head_t(want_t, 0, ml.r1, ml);
        CHECK(t == want_t);
        const u64 c = rescale_head_centre(t, h, ql);
        CHECK(c < ql && c == mod_i((i128)t + (i128)h, ql));
        const i128 centred = t <= h ? (i128)t : (i128)t - (i128)ql;
        const u64 want_lift = mod_i(centred, qj);
        const u64 general = rescale_head_lift(c, false, mj, hq);
        CHECK(general == want_lift);
        if (near) CHECK(rescale_head_lift(c, true, mj, hq) == want_lift);
        CHECK(mod_i((i128)c - (i128)h, qj) == want_lift);   // the conversion kernel's form: the integer c - h, reduced by its sum
        for (u64 cj : rj) {
            const u64 want_in = mod_i((i128)cj + centred, qj);
            const u64 got = rescale_head_in(cj, c, near, mj, hq);
            CHECK(got < qj && got == want_in);
            CHECK(rescale_head_in(cj, c, false, mj, hq) == want_in);
            CHECK(ntt_load_fix(f, cj, t) == want_in);   // the prologue's integer branch: the same word
            checks++;
        }
    }
    // random points end to end
    for (int it = 0; it < 20000; it++) {
        const u64 a = rnd() % ql, cv = rnd() % ql, bb = rnd() % ql, cj = rnd() % qj, pinv = 1 + rnd() % (ql - 1);
        const bool base = it & 1;
        u64 t = rescale_head_t(a, cv, (u64)(((u128)pinv << 64) % ql), ml);
        if (base) t = add_mod(t, bb, ql);
        const u64 tw = mod_i(((i128)a - (i128)cv) * (i128)pinv + (base ? (i128)bb : 0), ql);
        CHECK(t == tw);
        const i128 centred = tw <= h ? (i128)tw : (i128)tw - (i128)ql;
        CHECK(rescale_head_in(cj, rescale_head_centre(t, h, ql), near, mj, hq) == mod_i((i128)cj + centred, qj));
        CHECK(mod_i((i128)cj + (i128)rescale_head_centre(t, h, ql) - (i128)h, qj) == mod_i((i128)cj + centred, qj));
        checks++;
    }
}

int main(int argc, char** argv) {
    if (argc < 3 || !(argc & 1)) {
        std::printf("usage: test_rescale_head q_l q_j [q_l q_j ...]\n");
        return 2;
    }
    int near = 0, general = 0;
    for (int i = 1; i + 1 < argc; i += 2) {
        const u64 ql = std::strtoull(argv[i], nullptr, 10), qj = std::strtoull(argv[i + 1], nullptr, 10);
        (ql <= 2 * qj ? near : general)++;
        test_pair(ql, qj);
    }
    std::printf("OK rescale_head %d pairs (%d near, %d general) %lld points\n", (argc - 1) / 2, near, general, checks);
    return 0;
}
