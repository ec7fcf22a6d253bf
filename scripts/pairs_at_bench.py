"""Cost of the counts about arbitrary points (nbmi_pair_counts_at).  JSON lines in <out>/pairs_at_bench.jsonl,
one per side of the A/B:

  {"kind": "pairs_at", "case": ..., "n": ..., "m": ..., "whole_cells": 1 | 0, "d1": ..., "radius": ..., "at_ms": ...,
   "at_per_point_ms": ..., "at_evals_per_point": ..., "at_cell_pairs_per_point": ..., "at_pairs_per_point": ...,
   "pairs_ms": ..., "pairs_evals_per_body": ..., "pairs_cell_pairs_per_body": ..., "bodies_ms": ...,
   "bodies_evals_per_point": ..., "step_ms": ..., "at_over_pairs": ..., "bodies_over_pairs": ..., "at_over_step": ...}

The state is bench.py's galaxy of a million bodies after the warm-up steps; the points are m = N random points, uniform in
the bounding sphere of the bodies about the origin ("radius"); the edges are the recorder's 13 "auto" edges, 0.5 d1 ..
32 d1 with d1 the median nearest-neighbour distance (one knn(1)).  ms = host wall time of one blocking call (mean over
--reps after one warm-up call): "at" = pair_counts_at(points, auto), "at_per_point" the same with the (m, 13) per-point
rows, "pairs" = pair_counts(auto) of the same handle, "bodies" = pair_counts_at at the bodies' own positions - the
like-for-like against pair_counts: the same pairs, each from both ends - and one default step (mean over --reps after
--warmup, synchronised), all in the same process.  *_evals_per_point = the distances the call
evaluated / m, *_cell_pairs_per_point = the pairs it counted through whole cells / m, at_pairs_per_point = the bodies within
32 d1 of a point on average.  whole_cells = 0 is the other side of the A/B: no cell is ever counted whole
(NBMI_PAIRS_CELLS=0); that line has "at" and "pairs" only, each one call timed as it is.

    python scripts/pairs_at_bench.py [--out profiles]    both sides as child processes under their own `timeout`, the
                                                         second started only if the first succeeded:
        --what calls                                     the line of the default, then the same with NBMI_PAIRS_CELLS=0
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (distribution, N, R, G, eps, theta, dt) - bench.py's galaxy_1m_bh
CASES = {"galaxy_1m": ("galaxy", 1_000_000, 800.0, 0.07, 1.5, 0.5, 0.05)}
STEP_TIMEOUT = 420


def _sim(case):
    sys.path.insert(0, ROOT)
    import importlib
    importlib.import_module("3d-spatial-sim-for-boid-and-nbody_amd")
    from nbody.gpu_backend import HIPBarnesHutSimulation
    dist, n, R, G, eps, theta, dt = CASES[case]
    sim = HIPBarnesHutSimulation.generated(dist, n, R, G, eps, 1.0, theta, seed=42)
    return sim, n, dt


def _timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def _ball(m, radius, seed):
    rng = np.random.RandomState(seed)
    u = rng.normal(size=(m, 3))
    u *= (radius * rng.uniform(size=m) ** (1.0 / 3.0) / np.linalg.norm(u, axis=1))[:, None]
    return np.ascontiguousarray(u)


def calls(case, reps, warmup, out):
    whole = os.environ.get("NBMI_PAIRS_CELLS") != "0"
    sim, n, dt = _sim(case)
    from nbody.pairs import auto_pair_edges
    for _ in range(warmup):
        sim.step(dt)
    sim.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        sim.step(dt)
    sim.sync()
    step_ms = (time.perf_counter() - t0) * 1e3 / reps
    auto = auto_pair_edges(sim.knn(1)[0])
    x = sim.get_positions_f64()
    radius = float(np.sqrt((x * x).sum(1).max()))
    m = n
    pts = _ball(m, radius, 7)
    rec = {"kind": "pairs_at", "case": case, "n": n, "m": m, "whole_cells": 1 if whole else 0, "d1": auto[2],
           "radius": round(radius, 1), "step_ms": round(step_ms, 3)}
    if whole:
        rec["at_ms"] = round(_timed(lambda: sim.pair_counts_at(pts, auto), reps), 3)
        rec["at_per_point_ms"] = round(_timed(lambda: sim.pair_counts_at(pts, auto, per_point=True), reps), 3)
        rec["pairs_ms"] = round(_timed(lambda: sim.pair_counts(auto), reps), 3)
        rec["bodies_ms"] = round(_timed(lambda: sim.pair_counts_at(x, auto), reps), 3)
        b_counts, b_below, b_ev, b_cp = sim.pair_counts_at(x, auto, evals=True)
        rec.update(bodies_evals_per_point=round(b_ev / n, 1), bodies_cell_pairs_per_point=round(b_cp / n, 1),
                   bodies_over_pairs=round(rec["bodies_ms"] / rec["pairs_ms"], 2))
    t0 = time.perf_counter()
    a_counts, a_below, a_ev, a_cp = sim.pair_counts_at(pts, auto, evals=True)
    t1 = time.perf_counter()
    p_counts, p_below, p_ev, p_cp = sim.pair_counts(auto, evals=True)
    if not whole:  # without whole cells every pair within 32 d1 is a distance: one call each, timed as it is
        rec["at_ms"], rec["pairs_ms"] = round((t1 - t0) * 1e3, 3), round((time.perf_counter() - t1) * 1e3, 3)
    else:
        assert np.array_equal(b_counts, 2 * p_counts) and b_below == 2 * p_below + n
    rec.update(at_evals_per_point=round(a_ev / m, 1), at_cell_pairs_per_point=round(a_cp / m, 1),
               at_pairs_per_point=round((a_below + int(a_counts.sum())) / m, 1), pairs_evals_per_body=round(p_ev / n, 1),
               pairs_cell_pairs_per_body=round(p_cp / n, 1), at_over_pairs=round(rec["at_ms"] / rec["pairs_ms"], 2),
               at_over_step=round(rec["at_ms"] / step_ms, 2))
    sim.close()
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(out, "pairs_at_bench.jsonl"), "a") as f:
        f.write(line + "\n")


def drive(out, reps, warmup, case):
    os.makedirs(out, exist_ok=True)
    me = os.path.abspath(__file__)
    path = os.path.join(out, "pairs_at_bench.jsonl")
    if os.path.exists(path):
        os.remove(path)
    for cells in ("1", "0"):  # chained: a side that fails, faults or runs out of time ends the run
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, me, "--what", "calls", "--case", case, "--out", out,
               "--reps", str(reps), "--warmup", str(warmup)]
        rc = subprocess.run(cmd, env=dict(os.environ, NBMI_PAIRS_CELLS=cells)).returncode
        if rc != 0:
            print(f"[pairs_at_bench] step failed with status {rc}; stopping: {' '.join(cmd)}", file=sys.stderr)
            return rc
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", default="all", choices=("all", "calls"))
    ap.add_argument("--case", default="galaxy_1m", choices=sorted(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.what == "calls":
        calls(a.case, a.reps, a.warmup, a.out)
        return 0
    return drive(a.out, a.reps, a.warmup, a.case)


if __name__ == "__main__":
    sys.exit(main())
