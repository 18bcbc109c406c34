// Host test of lattisense_amd/csrc/ks_mac_groups.h (tests/test_ks_mac_groups_host.py builds and runs it).
//   check: for every gx in [1, 4096] and batch in [1, 1100] the groups [y * bpt, min(batch, (y + 1) * bpt)), y < gy, tile
//          [0, batch) exactly, none is empty, gy <= groups <= batch, and gy fits grid.y; prints "ok <pairs>"
//   print: the triple "gx batch groups bpt gy" of every (gx, batch) given as further arguments, two numbers each
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../lattisense_amd/csrc/ks_mac_groups.h"

static int fail(unsigned gx, int batch, const lsa::KsMacGroups& r, const char* what) {
    std::printf("gx %u batch %d -> groups %d bpt %d gy %d: %s\n", gx, batch, r.groups, r.bpt, r.gy, what);
    return 1;
}

static int check() {
    long long pairs = 0;
    for (unsigned gx = 1; gx <= 4096; gx++) {
        for (int batch = 1; batch <= 1100; batch++) {
            const lsa::KsMacGroups r = lsa::ks_mac_groups(gx, batch);
            if (r.groups < 1 || r.groups > batch) return fail(gx, batch, r, "groups outside [1, batch]");
            if (r.bpt < 1 || r.bpt > batch) return fail(gx, batch, r, "bpt outside [1, batch]");
            if (r.gy < 1 || r.gy > r.groups || r.gy > 65535) return fail(gx, batch, r, "gy outside [1, groups]");
            const int want = (int)((2048 + gx - 1) / gx);
            if (r.groups != (want < batch ? want : batch)) return fail(gx, batch, r, "groups is not min(ceil(2048 / gx), batch)");
            int next = 0;   // the first item no group has walked yet
            for (int y = 0; y < r.gy; y++) {
                const int b_begin = y * r.bpt;                                     // the kernels' walk
                const int b_end = batch < b_begin + r.bpt ? batch : b_begin + r.bpt;
                if (b_begin != next) return fail(gx, batch, r, "a gap or an overlap between two groups");
                if (b_end <= b_begin) return fail(gx, batch, r, "an empty group");
                next = b_end;
            }
            if (next != batch) return fail(gx, batch, r, "the groups do not end at the batch");
            pairs++;
        }
    }
    std::printf("ok %lld\n", pairs);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "check")) return check();
    if (argc >= 2 && !std::strcmp(argv[1], "print") && argc % 2 == 0) {
        for (int i = 2; i + 1 < argc; i += 2) {
            const unsigned gx = (unsigned)std::strtoul(argv[i], nullptr, 10);
            const int batch = std::atoi(argv[i + 1]);
            const lsa::KsMacGroups r = lsa::ks_mac_groups(gx, batch);
            std::printf("%u %d %d %d %d\n", gx, batch, r.groups, r.bpt, r.gy);
        }
        return 0;
    }
    std::fprintf(stderr, "usage: %s check | print gx batch [gx batch ...]\n", argv[0]);
    return 2;
}
