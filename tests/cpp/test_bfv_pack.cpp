// Host program for lattisense_amd/csrc/bfv_pack.h (tests/test_bfv_pack_host.py builds it with -fsanitize=address,undefined): the
// plan against a brute-force walk for every count <= 64 with and without the trace, every input consumed exactly once and input i
// landing on coefficient i * N / 2^k, and the shifted-source rule of the tail against a schoolbook multiplication by X^s.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../../lattisense_amd/csrc/bfv_pack.h"

using namespace lsa;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond);     \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

// the packing walked node by node on index sets: which inputs a node holds, and at which coefficient each of them sits
static void plan_against_brute_force(int n) {
    int logn = 0;
    while ((1 << logn) < n) logn++;
    for (int trace = 0; trace <= 1; trace++) {
        for (int count = 1; count <= 64 && count <= n; count++) {
            const BfvPackPlanHost p = bfv_pack_plan(n, count, trace);
            int k = 0;
            while ((1 << k) < count) k++;
            CHECK((int)p.levels.size() == k && p.count == count && p.n_ring == n && p.trace == trace);
            std::vector<std::vector<std::pair<int, int>>> held(count);   // node -> (input, coefficient)
            for (int i = 0; i < count; i++) held[i] = {{i, 0}};
            std::vector<int> consumed(count, 0);
            int ks = 0;
            std::set<uint64_t> elements;
            for (int j = k - 1, lv = 0; j >= 0; j--, lv++) {
                const BfvPackLevel& l = p.levels[lv];
                const int half = 1 << j;
                CHECK(l.nodes == half && l.shift == n >> (k - j) && l.g == (uint64_t)(1 << (k - j)) + 1);
                int pairs = 0;
                for (int a = 0; a < half; a++) {
                    ks++;
                    if (a + half < count) {
                        CHECK(a < l.n_pair);   // the kernels' rule: the nodes below n_pair, and only they
                        pairs++;
                        CHECK(!held[a + half].empty());
                        for (auto e : held[a + half]) held[a].push_back({e.first, e.second + l.shift});
                        held[a + half].clear();
                        consumed[a + half]++;
                    } else {
                        CHECK(a >= l.n_pair);
                        CHECK(lv == 0);        // only the first level has unpaired nodes
                    }
                }
                CHECK(pairs == l.n_pair);
                elements.insert(l.g);
            }
            CHECK(p.trace_g.size() == (size_t)(trace ? logn - k : 0));
            for (size_t i = 0; i < p.trace_g.size(); i++) {
                CHECK(p.trace_g[i] == (uint64_t)(1 << (k + 1 + (int)i)) + 1);
                elements.insert(p.trace_g[i]);
                ks++;
            }
            CHECK(ks == p.n_keyswitch && ks == (1 << k) - 1 + (trace ? logn - k : 0));
            CHECK(std::vector<uint64_t>(elements.begin(), elements.end()) == p.galois);
            CHECK(consumed[0] == 0);
            for (int i = 1; i < count; i++) CHECK(consumed[i] == 1 && held[i].empty());
            CHECK((int)held[0].size() == count);
            std::set<int> seen;
            for (auto e : held[0]) {
                CHECK(e.second == e.first * (n >> k));
                seen.insert(e.first);
            }
            CHECK((int)seen.size() == count);
        }
    }
}

static void refusals() {
    const int bad[][2] = {{1024, 0}, {1024, -1}, {1024, 1025}, {1000, 4}, {2, 1}};
    for (const auto& b : bad) {
        for (int trace = 0; trace <= 1; trace++) {
            bool threw = false;
            try {
                bfv_pack_plan(b[0], b[1], trace);
            } catch (const std::invalid_argument& e) {
                threw = std::string(e.what()).rfind("lsa_bfv_pack", 0) == 0;
            }
            CHECK(threw);
        }
    }
    CHECK(bfv_pack_plan(1024, 1024, 1).levels.size() == 10 && bfv_pack_plan(1024, 1024, 1).n_keyswitch == 1023);
    CHECK(bfv_pack_plan(1024, 1024, 0).levels.front().shift == 512 && bfv_pack_plan(1024, 1024, 0).levels.back().shift == 1);
    CHECK(bfv_pack_plan(1024, 1, 0).levels.empty() && bfv_pack_plan(1024, 1, 0).galois.empty() && bfv_pack_plan(1024, 1, 0).n_keyswitch == 0);
    CHECK(bfv_pack_plan(1024, 1, 1).levels.empty() && bfv_pack_plan(1024, 1, 1).n_keyswitch == 10 && bfv_pack_plan(1024, 1, 1).galois.back() == 1025);
}

// X^s * b over Z[X] / (X^N + 1) by the schoolbook product, b with the coefficients 1 .. N: out[x] as a signed integer
static std::vector<long long> schoolbook(int n, int s) {
    std::vector<long long> mono(n, 0), b(n), out(n, 0);
    mono[s % n] = s >= n ? -1 : 1;
    for (int i = 0; i < n; i++) b[i] = i + 1;
    for (int i = 0; i < n; i++) {
        if (!mono[i]) continue;
        for (int y = 0; y < n; y++) {
            const int d = i + y;
            out[d % n] += (d >= n ? -1 : 1) * mono[i] * b[y];
        }
    }
    return out;
}

static void point_function(int logn) {
    const int n = 1 << logn;
    for (int s : {1, 2, n / 2}) {
        const std::vector<long long> want = schoolbook(n, s);
        for (int x : {0, s - 1, s, n - 1}) {
            const MonomialDest d = bfv_pack_source((unsigned)x, (unsigned)s, logn);
            CHECK(d.idx == (unsigned)(((x - s) % n + n) % n) && d.neg == (unsigned)(x < s));
            CHECK(want[x] == (d.neg ? -1 : 1) * (long long)(d.idx + 1));
            // the inverse of monomial_dest: what lands on x came from there
            const MonomialDest f = monomial_dest(d.idx, (unsigned)s, logn);
            CHECK(f.idx == (unsigned)x && f.neg == d.neg);
        }
        std::vector<char> hit(n, 0);   // a permutation of the row
        for (int x = 0; x < n; x++) hit[bfv_pack_source((unsigned)x, (unsigned)s, logn).idx]++;
        for (int x = 0; x < n; x++) CHECK(hit[x] == 1);
    }
}

int main() {
    plan_against_brute_force(1 << 10);
    plan_against_brute_force(64);
    plan_against_brute_force(8);
    std::printf("ok plan\n");
    refusals();
    std::printf("ok refusals\n");
    for (int logn : {3, 10, 14}) point_function(logn);
    std::printf("ok point\n");
    return 0;
}
