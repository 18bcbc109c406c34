// Host-side check of the Galois key set (lattisense_amd/csrc/galois_keys.h: GaloisKeySet), on a key type of its own that has the
// one field the set reads.  Prints "ok <case>" per case and exits 0; a failed expectation prints what it saw and exits 1.
// Driven by tests/test_galois_keys_host.py.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../lattisense_amd/csrc/galois_keys.h"

struct TestKey {
    const void* data;
    int id;
};
using Keys = lsa::GaloisKeySet<TestKey>;

static void expect(bool ok, const char* what, const std::string& saw = "") {
    if (ok) return;
    std::printf("FAILED %s %s\n", what, saw.c_str());
    std::exit(1);
}
// the refusal of f(): code LSA_ERR_ARG and the message, or "" if f() returns
template <typename F>
static std::string refusal(F&& f) {
    try {
        f();
    } catch (const lsa::Error& e) {
        expect(e.code == LSA_ERR_ARG, "error code");
        return e.what();
    }
    return "";
}

int main() {
    static const int word = 0;
    TestKey k5{&word, 5}, k25{&word, 25}, k125{&word, 125}, later{&word, 99}, no_data{nullptr, 7};
    const auto self = [](const TestKey* k) { return k; };
    {   // a missing element: the message, and the first one in the order of the plan's list
        const uint64_t el[] = {125, 5};
        const TestKey* ks[] = {&k125, &k5};
        const Keys g(2, el, ks, self);
        expect(refusal([&] { g.require(25, "lsa_op"); }) == "lsa_op: Galois key for element 25 missing", "missing: message");
        const std::string m = refusal([&] { g.resolve({5, 25, 125, 625}, "lsa_op"); });
        expect(m == "lsa_op: Galois key for element 25 missing", "missing: first in the list's order", m);
        int seen = 0;   // the caller's check runs on the keys before the missing one, in order
        (void)refusal([&] { g.resolve({5, 25, 125}, "lsa_op", [&](uint64_t e, const TestKey& k) { expect(e == 5 && k.id == 5 && !seen++, "each"); }); });
        expect(seen == 1, "missing: keys ahead of it were checked");
        std::printf("ok missing\n");
    }
    {   // a null key and a key without data are missing keys
        const uint64_t el[] = {5, 25};
        const TestKey* ks[] = {nullptr, &no_data};
        const Keys g(2, el, ks, self);
        expect(refusal([&] { g.require(5, "who"); }) == "who: Galois key for element 5 missing", "null key");
        expect(refusal([&] { g.require(25, "who"); }) == "who: Galois key for element 25 missing", "null key data");
        expect(refusal([&] { g.resolve({25}, "who"); }) == "who: Galois key for element 25 missing", "null key data, resolve");
        std::printf("ok null\n");
    }
    {   // a repeated element: the later key wins, with the arrays and with insert
        const uint64_t el[] = {5, 25, 5};
        const TestKey* ks[] = {&k5, &k25, &later};
        Keys g(3, el, ks, self);
        expect(g.require(5, "who").id == 99 && g.require(25, "who").id == 25, "duplicate: arrays");
        g.insert(25, &later);
        g.insert(25, &k25);
        g.insert(125, &k125);
        expect(g.require(25, "who").id == 25 && g.require(125, "who").id == 125, "duplicate: insert");
        std::printf("ok duplicate\n");
    }
    {   // nothing to look up: an empty list against an empty set (and against any set)
        const Keys none;
        expect(none.resolve({}, "who").empty(), "empty list, empty set");
        expect(Keys(0, nullptr, (const TestKey* const*)nullptr, self).resolve({}, "who").empty(), "empty arrays");
        expect(refusal([&] { none.require(1, "who"); }) == "who: Galois key for element 1 missing", "empty set");
        std::printf("ok empty\n");
    }
    {   // resolve returns the keys in the list's order, whatever the order they came in, and hands each to the caller's check
        const uint64_t el[] = {125, 5, 25, 3125};
        const TestKey other{&word, 3125};
        const TestKey* ks[] = {&k125, &k5, &k25, &other};
        const Keys g(4, el, ks, self);
        std::vector<uint64_t> checked;
        const std::vector<const TestKey*> r = g.resolve({25, 125, 5}, "who", [&](uint64_t e, const TestKey& k) {
            expect((uint64_t)k.id == e, "each: key of its element");
            checked.push_back(e);
        });
        expect(r.size() == 3 && r[0] == &k25 && r[1] == &k125 && r[2] == &k5, "order");
        expect(checked == std::vector<uint64_t>({25, 125, 5}), "each: order");
        std::printf("ok order\n");
    }
    return 0;
}
