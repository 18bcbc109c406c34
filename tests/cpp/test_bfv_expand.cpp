// Host program for lattisense_amd/csrc/bfv_expand.h (tests/test_bfv_expand_host.py builds it with -fsanitize=address,undefined):
// the plan against brute force for every count <= 64, the children's indices being exactly 0 .. count-1 once each, and the point
// function of the tail against a schoolbook multiplication by X^(-s).
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../../lattisense_amd/csrc/bfv_expand.h"

using namespace lsa;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond);     \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

// the expansion walked node by node on index sets: which outputs exist after every level
static void plan_against_brute_force(int n) {
    for (int count = 1; count <= 64; count++) {
        const BfvExpandPlanHost p = bfv_expand_plan(n, count);
        std::vector<int> live{0};
        int ks = 0;
        size_t lv = 0;
        std::set<uint64_t> elements;
        for (int s = 1; s < count; s *= 2, lv++) {
            CHECK(lv < p.levels.size());
            const BfvExpandLevel& l = p.levels[lv];
            CHECK(l.shift == s && l.g == (uint64_t)(n / s + 1) && l.nodes == (int)live.size());
            std::vector<int> next = live;
            int odd = 0;
            for (int a : live) {
                CHECK(a < l.nodes);
                ks++;
                if (a + s < count) {
                    next.push_back(a + s);
                    odd++;
                    CHECK(a < l.n_odd);   // the kernel's rule: the parents below n_odd, and only they
                } else {
                    CHECK(a >= l.n_odd);
                }
            }
            CHECK(odd == l.n_odd);
            live = next;
            elements.insert(l.g);
        }
        CHECK(lv == p.levels.size() && ks == p.n_keyswitch);
        CHECK(std::vector<uint64_t>(elements.begin(), elements.end()) == p.galois);
        std::set<int> once(live.begin(), live.end());
        CHECK((int)live.size() == count && (int)once.size() == count && *once.begin() == 0 && *once.rbegin() == count - 1);
    }
}

static void refusals() {
    const int bad[][2] = {{1024, 0}, {1024, -1}, {1024, 1025}, {1000, 4}, {2, 1}};
    for (const auto& b : bad) {
        bool threw = false;
        try {
            bfv_expand_plan(b[0], b[1]);
        } catch (const std::invalid_argument& e) {
            threw = std::string(e.what()).rfind("lsa_bfv_expand", 0) == 0;
        }
        CHECK(threw);
    }
    CHECK(bfv_expand_plan(1024, 1024).levels.size() == 10 && bfv_expand_plan(1024, 1024).n_keyswitch == 1023);
    CHECK(bfv_expand_plan(1024, 1).levels.empty() && bfv_expand_plan(1024, 1).galois.empty());
}

// X^(-s) * X^y over Z[X] / (X^N + 1) by the schoolbook product with X^(2N - s) = X^(-s): exponents are reduced with X^N = -1
static void schoolbook(int logn, long long e, int y, unsigned* idx, unsigned* neg) {
    const long long n = 1LL << logn;
    long long deg = y + e;   // e in [0, 2N)
    int sign = 0;
    while (deg >= n) {
        deg -= n;
        sign ^= 1;
    }
    *idx = (unsigned)deg;
    *neg = (unsigned)sign;
}

static void point_function(int logn) {
    const int n = 1 << logn;
    for (int s : {1, 2, n / 2}) {
        for (int y : {0, s - 1, s, n - 1}) {
            unsigned idx, neg;
            schoolbook(logn, 2LL * n - s, y, &idx, &neg);
            const MonomialDest d = bfv_expand_odd_dest((unsigned)y, (unsigned)s, logn);
            CHECK(d.idx == idx && d.neg == neg);
            CHECK(d.idx == (unsigned)(((y - s) % n + n) % n) && d.neg == (unsigned)(y < s));
        }
        // a permutation of the row
        std::vector<char> hit(n, 0);
        for (int y = 0; y < n; y++) hit[bfv_expand_odd_dest((unsigned)y, (unsigned)s, logn).idx]++;
        for (int y = 0; y < n; y++) CHECK(hit[y] == 1);
    }
    for (long long e : {0LL, 1LL, -1LL, 2LL, (long long)n - 1, (long long)n, (long long)n + 1, 2LL * n - 1, -(2LL * n + 3)}) {
        const unsigned r = monomial_exponent(e, logn);
        CHECK(r < 2u * n && ((long long)r - e) % (2LL * n) == 0);
        for (int y : {0, 1, n / 2, n - 1}) {
            unsigned idx, neg;
            schoolbook(logn, r, y, &idx, &neg);
            const MonomialDest d = monomial_dest((unsigned)y, r, logn);
            CHECK(d.idx == idx && d.neg == neg);
        }
    }
}

int main() {
    plan_against_brute_force(1 << 10);
    plan_against_brute_force(64);
    std::printf("ok plan\n");
    refusals();
    std::printf("ok refusals\n");
    for (int logn : {3, 10, 14, 16}) point_function(logn);
    std::printf("ok point\n");
    return 0;
}
