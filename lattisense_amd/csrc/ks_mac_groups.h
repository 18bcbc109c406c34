// ks_mac_groups.h — how the stand-alone key MACs (k_ks_mac, k_ks_mac_multi) cut a batch into grid.y groups.
// Plain C++ (tests/cpp/test_ks_mac_groups.cpp compiles it for the host; tests/ks_groups.py restates it).
//
// A thread keeps its key words in registers and walks `bpt` consecutive batch items with them, so fewer groups mean fewer key
// reads; but a launch needs about 2048 workgroups to fill the chip.  With gx workgroups per batch item:
//   groups = clamp(ceil(2048 / gx), 1, batch)      as many groups as filling the chip takes, no more than items
//   bpt    = ceil(batch / groups)                  items per group
//   gy     = ceil(batch / bpt)                     grid.y: groups that hold an item (<= groups)
// Group y walks [y * bpt, min(batch, (y + 1) * bpt)); the last may be shorter, none is empty.
#pragma once

namespace lsa {

constexpr int KS_MAC_FILL_WORKGROUPS = 2048;

struct KsMacGroups {
    int groups, bpt, gy;
};

inline KsMacGroups ks_mac_groups(unsigned gx, int batch) {
    KsMacGroups r;
    const int want = (int)((KS_MAC_FILL_WORKGROUPS + gx - 1) / gx);
    r.groups = want < batch ? want : batch;
    if (r.groups < 1) r.groups = 1;
    r.bpt = (batch + r.groups - 1) / r.groups;
    r.gy = (batch + r.bpt - 1) / r.bpt;
    return r;
}

}  // namespace lsa
