#!/usr/bin/env python3
"""Records tests/golden/ks_callers.json: for every case of tests/ks_callers_cases.py the SHA-256 of the output words and the
launches and algorithmic bytes per profiler kind, as the library in use produces them.  Point LSA_NATIVE_LIB at the build of the
commit whose behaviour is to be kept (the parent of a refactor) and run on the GPU:

    LSA_NATIVE_LIB=/path/to/parent/liblattisense_amd.so python tools/record_ks_callers.py [--out FILE]

tests/test_gpu_ks_callers.py then asks the current build for the same figures."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import ks_callers_cases as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ks_callers.json"))
    args = ap.parse_args()
    from lattisense_amd._native import LIB_PATH
    out, rigs = {}, {}
    for rig, case, setting in K.CASE_IDS:
        if rig not in rigs:
            rigs[rig] = K.make_rig(rig)
        out[K.golden_key(rig, case, setting)] = K.measure(rigs[rig], case, setting)
    for r in rigs.values():
        r.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases recorded with %s -> %s" % (len(out), LIB_PATH, args.out))


if __name__ == "__main__":
    main()
