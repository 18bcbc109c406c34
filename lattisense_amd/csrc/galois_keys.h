// galois_keys.h — what every operator that works through a plan shares about its Galois keys: the element of a rotation and the
// set of keys a caller hands in (element -> key), with the one look-up that refuses a missing key.  Host only, pure C++17: no
// device, no context (tests/cpp/test_galois_keys.cpp).  Templated on the key type, of which it reads `data` only.
#pragma once
#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/lattisense_amd.h"

namespace lsa {

// the library's exception: guard() (c_api.hip) turns it into its code and lsa_last_error()
struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// 5^r mod 2N, the Galois element of the rotation by r slots; r in [0, N/2)
inline uint64_t galois_of_rotation(int r, int n_ring) {
    const uint64_t mask = 2 * (uint64_t)n_ring - 1;
    uint64_t e = 1, b = 5;
    for (; r > 0; r >>= 1, b = b * b & mask)
        if (r & 1) e = e * b & mask;
    return e;
}

template <typename K>
struct GaloisKeySet {
    std::map<uint64_t, const K*> by_element;

    GaloisKeySet() = default;
    // the C arrays of an entry point; key_of turns a handle into its key (and refuses a null one).  A repeated element: the
    // later key wins.
    template <typename H, typename F>
    GaloisKeySet(int n, const uint64_t* elements, const H* handles, F&& key_of) {
        for (int i = 0; i < n; i++) insert(elements[i], key_of(handles[i]));
    }
    void insert(uint64_t element, const K* key) { by_element[element] = key; }
    const K* at(uint64_t element) const { return by_element.at(element); }   // a key that is known to be there (resolved before)

    const K& require(uint64_t element, const std::string& who) const {
        const auto it = by_element.find(element);
        if (it == by_element.end() || !it->second || !it->second->data)
            throw Error(LSA_ERR_ARG, who + ": Galois key for element " + std::to_string(element) + " missing");
        return *it->second;
    }
    // every key of a plan's element list, in the list's order, looked up before anything is queued: the first element without
    // a key is refused.  each(element, key) is the caller's own check of a key (its level), run as soon as the key is found.
    template <typename F>
    std::vector<const K*> resolve(const std::vector<uint64_t>& elements, const std::string& who, F&& each) const {
        std::vector<const K*> keys;
        for (uint64_t e : elements) {
            keys.push_back(&require(e, who));
            each(e, *keys.back());
        }
        return keys;
    }
    std::vector<const K*> resolve(const std::vector<uint64_t>& elements, const std::string& who) const {
        return resolve(elements, who, [](uint64_t, const K&) {});
    }
};

}  // namespace lsa
