"""Writes tests/golden/probe_bits.json: what the float64 probe family computes - potentials, nbmi_field_at, the tidal
tensor at points and bodies, tracers, on a tree and by the direct sums - at ONE commit, as SHA-256 hashes of the float64
arrays and the int32 term counts as they are.

    python scripts/gen_probe_bits_golden.py --commit <full id of the commit the library was built from>

Run it once, on a GPU, with the library of the commit whose bits are to be kept (build that commit in a checkout of its
own and point NBMI_LIB at its libnbmi.so).  tests/test_gpu_probe_bits.py owns the cases, the inputs and the hashing
(this script imports them, so the two cannot drift apart) and compares the library under test against the file.

Before it writes anything the script makes sure that the walk order changes no bit (NBMI_FIELD_SORT=0 against the
sorted twin), that every case runs twice to the same values, and that every tracer moved.
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conftest  # noqa: E402,F401  (puts the package on the path)
import test_gpu_probe_bits as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="full id of the commit the loaded library was built from")
    ap.add_argument("-o", "--output", default=T.GOLDEN_PATH)
    a = ap.parse_args()
    assert len(a.commit) == 40, "give the full commit id"
    inputs = {dist: T.make_input(dist) for dist in T.DISTS}
    cases = {}
    for name, case in T.CASES.items():
        cases[name] = T.run_case(case, inputs[case["dist"]])
        assert cases[name] == T.run_case(case, inputs[case["dist"]]), f"{name}: two runs differ"
        if case["kind"] == "tracers":
            assert cases[name]["moved"] == case["m"], name
        print(name, {k: v for k, v in cases[name].items() if not isinstance(v, dict)})
    for name, twin in T.SORT_TWINS.items():
        assert cases[name] == cases[twin], f"{name} differs from {twin}"
    head = {"commit": a.commit, "n": T.N, "steps": T.STEPS}
    with open(a.output, "w") as f:  # one line per case: the term counts are long lists
        f.write("{\n")
        for k, v in head.items():
            f.write(f" {json.dumps(k)}: {json.dumps(v)},\n")
        f.write(' "cases": {\n')
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(cases[k], sort_keys=True)}" for k in sorted(cases)))
        f.write("\n }\n}\n")
    print(f"{a.output}: {len(cases)} cases")


if __name__ == "__main__":
    main()
