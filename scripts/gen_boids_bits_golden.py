"""Writes tests/golden/boids_bits.json: what the boids sweep and the flock analysis compute at ONE commit, as SHA-256
hashes of the arrays as they are, with the integer counts.

    python scripts/gen_boids_bits_golden.py --commit <full id of the commit the library was built from>

Run it once, on a GPU, with the library of the commit whose bits are to be kept (build that commit in a checkout of its
own and point NBMI_LIB at its libnbmi.so).  tests/test_gpu_boids_bits.py owns the cases and the hashing (this script
imports them, so the two cannot drift apart) and compares the library under test against the file.

Before it writes anything the script makes sure that every case runs twice to the same values.
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conftest  # noqa: E402,F401  (puts the package on the path)
import test_gpu_boids_bits as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="full id of the commit the loaded library was built from")
    ap.add_argument("-o", "--output", default=T.GOLDEN_PATH)
    a = ap.parse_args()
    assert len(a.commit) == 40, "give the full commit id"
    import nbmi_native
    nbmi_native.load()
    assert nbmi_native.device_count() > 0, "needs a HIP device"
    print("library:", nbmi_native.LIB_PATH)
    cases = {}
    for name in T.CASES:
        cases[name] = T.run_case(nbmi_native, name)
        assert cases[name] == T.run_case(nbmi_native, name), f"{name}: two runs differ"
        print(name, {k: v for k, v in cases[name].items() if isinstance(v, int)})
    with open(a.output, "w") as f:
        json.dump({"commit": a.commit, "steps": T.STEPS, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{a.output}: {len(cases)} cases")


if __name__ == "__main__":
    main()
