"""Cost of the binned pair counts (nbmi_pair_counts).  JSON lines in <out>/pairs_bench.jsonl, one per case:

  {"kind": "pairs", "case": ..., "whole_cells": 1 | 0, "d1": ..., "single_ms": ..., "single_evals_per_body": ...,
   "single_cell_pairs_per_body": ..., "auto_ms": ..., "auto_evals_per_body": ..., "auto_cell_pairs_per_body": ...,
   "auto_pairs_per_body": ..., "d2": ..., "fof_ms": ..., "knn8_ms": ..., "step_ms": ..., "single_over_fof": ...,
   "auto_over_single": ..., "auto_over_step": ...}

d1 = the median nearest-neighbour distance of the state (one knn(1)).  "single" = pair_counts([0, 2 d1]), one bin ending at
the recorder's "auto" linking length; "auto" = pair_counts of the recorder's 13 "auto" edges, 0.5 d1 .. 32 d1.  ms = host
wall time of one blocking call (mean over --reps after one warm-up call; the auto call over at most two, and with
NBMI_PAIRS_CELLS=0 a single call): the two pair
counts, find_groups(2 d1), knn(8), and one default step (mean over --reps after --warmup, synchronised) of the same handle
in the same process.  *_evals_per_body = the distances the call evaluated / N, *_cell_pairs_per_body = the pairs it counted
through whole cells / N, auto_pairs_per_body = the pairs within 32 d1 / N.  whole_cells = 0 is the other side of the A/B:
no cell is ever counted whole (NBMI_PAIRS_CELLS=0).

    python scripts/pairs_bench.py [--out profiles]    every step below as a child process under its own `timeout`, each
                                                      started only if the one before succeeded:
        --what calls --case galaxy_1m                 the line of one case, then the same with NBMI_PAIRS_CELLS=0
        --what calls --case collision_10m
        rocprofv3 --kernel-trace --stats ... -- --what one --case galaxy_1m
                                                      one 1 M call on its own, no counters -> <out>/pairs_1m_kernel_stats.csv
"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (distribution, N, R, G, eps, theta, dt) - bench.py's galaxy_1m_bh and collision_10m_bh
CASES = {
    "galaxy_1m": ("galaxy", 1_000_000, 800.0, 0.07, 1.5, 0.5, 0.05),
    "collision_10m": ("collision", 10_000_000, 2000.0, 0.08, 6.0, 0.5, 0.25),
}
STEP_TIMEOUT = {"galaxy_1m": 240, "collision_10m": 420, "profile": 240}


def _sim(case):
    sys.path.insert(0, ROOT)
    import importlib
    importlib.import_module("3d-spatial-sim-for-boid-and-nbody_amd")
    from nbody.gpu_backend import HIPBarnesHutSimulation
    dist, n, R, G, eps, theta, dt = CASES[case]
    sim = HIPBarnesHutSimulation.generated(dist, n, R, G, eps, 1.0, theta, seed=42)
    return sim, n, theta, dt


def _timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def _edges(sim):
    """(d1, the single bin ending at 2 d1, the recorder's auto edges)"""
    from nbody.pairs import auto_pair_edges
    auto = auto_pair_edges(sim.knn(1)[0])
    d1 = auto[2]
    return d1, [0.0, 2.0 * d1], auto


def calls(case, reps, warmup, out):
    sim, n, theta, dt = _sim(case)
    from nbody.pairs import correlation_dimension
    for _ in range(warmup):
        sim.step(dt)
    sim.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        sim.step(dt)
    sim.sync()
    step_ms = (time.perf_counter() - t0) * 1e3 / reps
    d1, single, auto = _edges(sim)
    knn_ms = _timed(lambda: sim.knn(8), reps)
    fof_ms = _timed(lambda: sim.find_groups(2.0 * d1), reps)
    single_ms = _timed(lambda: sim.pair_counts(single), reps)
    s_counts, s_below, s_ev, s_cp = sim.pair_counts(single, evals=True)
    whole = os.environ.get("NBMI_PAIRS_CELLS") != "0"
    if whole:
        auto_ms = _timed(lambda: sim.pair_counts(auto), min(reps, 2))
    t0 = time.perf_counter()
    a_counts, a_below, a_ev, a_cp = sim.pair_counts(auto, evals=True)
    if not whole:  # every pair within 32 d1 is a distance then: one call, timed as it is
        auto_ms = (time.perf_counter() - t0) * 1e3
    rec = {"kind": "pairs", "case": case, "n": n, "whole_cells": 1 if whole else 0,
           "d1": d1, "single_ms": round(single_ms, 3), "single_evals_per_body": round(s_ev / n, 1),
           "single_cell_pairs_per_body": round(s_cp / n, 1), "single_pairs_per_body": round((s_below + int(s_counts.sum())) / n, 2),
           "auto_ms": round(auto_ms, 3), "auto_evals_per_body": round(a_ev / n, 1),
           "auto_cell_pairs_per_body": round(a_cp / n, 1), "auto_pairs_per_body": round((a_below + int(a_counts.sum())) / n, 1),
           "d2": round(correlation_dimension(auto, a_below, a_counts)[0], 3), "fof_ms": round(fof_ms, 3),
           "knn8_ms": round(knn_ms, 3), "step_ms": round(step_ms, 3), "single_over_fof": round(single_ms / fof_ms, 2),
           "auto_over_single": round(auto_ms / single_ms, 2), "auto_over_step": round(auto_ms / step_ms, 2)}
    sim.close()
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(out, "pairs_bench.jsonl"), "a") as f:
        f.write(line + "\n")


def one(case):
    sim, n, _theta, dt = _sim(case)
    sim.step(dt)
    d1, single, auto = _edges(sim)
    _c, _b, ev, cp = sim.pair_counts(single, evals=True)
    _c, _b, ev_a, cp_a = sim.pair_counts(auto, evals=True)
    print(json.dumps({"kind": "one", "case": case, "d1": d1, "single_evals_per_body": round(ev / n, 1),
                      "auto_evals_per_body": round(ev_a / n, 1), "auto_cell_pairs_per_body": round(cp_a / n, 1)}))
    sim.close()


def drive(out, reps, warmup, cases):
    os.makedirs(out, exist_ok=True)
    me = os.path.abspath(__file__)
    path = os.path.join(out, "pairs_bench.jsonl")
    if os.path.exists(path):
        os.remove(path)
    raw = os.path.join(out, "pairs_1m_raw")

    def call(case, cells):
        return (["timeout", "-k", "10", str(STEP_TIMEOUT[case]), sys.executable, me, "--what", "calls", "--case", case, "--out",
                 out, "--reps", str(reps), "--warmup", str(warmup)], dict(os.environ, NBMI_PAIRS_CELLS="1" if cells else "0"))
    steps = [call(c, True) for c in cases]
    if "galaxy_1m" in cases:
        steps.append((["timeout", "-k", "10", str(STEP_TIMEOUT["profile"]), "rocprofv3", "--kernel-trace", "--stats",
                       "--output-format", "csv", "-d", raw, "--", sys.executable, me, "--what", "one", "--case", "galaxy_1m"],
                      dict(os.environ)))
        steps.append(call("galaxy_1m", False))  # the A/B's other side last: it is the longest
    for cmd, env in steps:  # chained: a step that fails, faults or runs out of time ends the run
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:
            print(f"[pairs_bench] step failed with status {rc}; stopping: {' '.join(cmd)}", file=sys.stderr)
            return rc
    if "galaxy_1m" in cases:
        stats = sorted(glob.glob(os.path.join(raw, "**", "*kernel_stats.csv"), recursive=True))
        if not stats:
            print("[pairs_bench] rocprofv3 wrote no kernel_stats.csv", file=sys.stderr)
            return 1
        shutil.copyfile(stats[0], os.path.join(out, "pairs_1m_kernel_stats.csv"))
        shutil.rmtree(raw, ignore_errors=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", default="all", choices=("all", "calls", "one"))
    ap.add_argument("--case", default=None, choices=sorted(CASES), help="one case only (default: both)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.what == "calls":
        calls(a.case or "galaxy_1m", a.reps, a.warmup, a.out)
    elif a.what == "one":
        one(a.case or "galaxy_1m")
    else:
        return drive(a.out, a.reps, a.warmup, [a.case] if a.case else list(CASES))
    return 0


if __name__ == "__main__":
    sys.exit(main())
