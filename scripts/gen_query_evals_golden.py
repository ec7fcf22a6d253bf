"""Writes tests/golden/query_evals.json: the work counters of the three tree queries - `evals` of knn(k, evals=True) and
find_groups(b, evals=True), `evals` and `cell_pairs` of pair_counts(e, evals=True) - at ONE commit.

    python scripts/gen_query_evals_golden.py --commit <full id of the commit the library was built from>

Run it once, on a GPU, with the library of the commit whose counters are to be kept (build that commit in a checkout of
its own and point NBMI_LIB at its libnbmi.so).  tests/test_gpu_query_shared.py owns the systems, the parameters and the
collection (this script imports them, so the two cannot drift apart) and compares the library under test against the
file.  Only the public Python methods are used.
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conftest  # noqa: E402,F401  (puts the package on the path)
import test_gpu_query_shared as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="full id of the commit the loaded library was built from")
    ap.add_argument("-o", "--output", default=T.GOLDEN_PATH)
    a = ap.parse_args()
    assert len(a.commit) == 40, "give the full commit id"
    systems = {}
    for name in T.EVAL_SYSTEMS:
        systems[name] = T.collect(name)
        print(name, systems[name])
    with open(a.output, "w") as f:
        json.dump({"commit": a.commit, "ks": list(T.EVAL_KS), "edges": {k: [float(x) for x in e] for k, e in T.EDGES.items()},
                   "systems": systems}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{a.output}: {len(systems)} systems")


if __name__ == "__main__":
    main()
