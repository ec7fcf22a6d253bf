"""Cost of the friends-of-friends query (nbmi_fof).  JSON lines in <out>/fof_bench.jsonl, one per case:

  {"kind": "fof", "case": ..., "link": ..., "fof_ms": ..., "evals_per_body": ..., "n_groups": ..., "largest": ...,
   "catalogue_ms": ..., "colors_ms": ..., "knn8_ms": ..., "step_ms": ..., "fof_over_knn8": ..., "fof_over_step": ...}

link = twice the median nearest-neighbour distance of the state (one knn(1)), the recorder's "auto".  ms = host wall time of
one blocking call (mean over --reps after one warm-up call): find_groups(link), group_catalogue(link, 20) (which runs the
query again), color_by_groups + sync, knn(8), and one default step (mean over --reps after --warmup, synchronised) of
the same handle.  evals_per_body = the distances one find_groups evaluated / N.

    python scripts/fof_bench.py [--out profiles]      every step below as a child process under its own `timeout`, each
                                                      started only if the one before succeeded:
        --what calls --case galaxy_1m                 the line of one case
        --what calls --case collision_10m
        rocprofv3 --kernel-trace --stats ... -- --what one --case galaxy_1m
                                                      one 1 M call on its own, no counters -> <out>/fof_1m_kernel_stats.csv
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
STEP_TIMEOUT = {"galaxy_1m": 240, "collision_10m": 420, "profile": 300}


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


def _link(sim):
    return 2.0 * float(np.median(np.sqrt(sim.knn(1)[0])))


def calls(case, reps, warmup, out):
    sim, n, theta, dt = _sim(case)
    for _ in range(warmup):
        sim.step(dt)
    sim.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        sim.step(dt)
    sim.sync()
    step_ms = (time.perf_counter() - t0) * 1e3 / reps
    link = _link(sim)
    knn_ms = _timed(lambda: sim.knn(8), reps)
    fof_ms = _timed(lambda: sim.find_groups(link), reps)
    labels, ev = sim.find_groups(link, evals=True)
    cat_ms = _timed(lambda: sim.group_catalogue(link, 20, capacity=64), reps)
    cat = sim.group_catalogue(link, 20, capacity=64)

    def colours():
        sim.color_by_groups(link, 20)
        sim.sync()
    col_ms = _timed(colours, reps)
    rec = {"kind": "fof", "case": case, "n": n, "link": link, "fof_ms": round(fof_ms, 3),
           "evals_per_body": round(ev / n, 1), "n_groups": sim.n_groups,
           "groups_of_20": cat["count"], "largest": int(cat["members"][0]) if len(cat["members"]) else 0,
           "catalogue_ms": round(cat_ms, 3), "colors_ms": round(col_ms, 3), "knn8_ms": round(knn_ms, 3),
           "step_ms": round(step_ms, 3), "fof_over_knn8": round(fof_ms / knn_ms, 2), "fof_over_step": round(fof_ms / step_ms, 2)}
    sim.close()
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(out, "fof_bench.jsonl"), "a") as f:
        f.write(line + "\n")


def one(case):
    sim, n, _theta, dt = _sim(case)
    sim.step(dt)
    link = _link(sim)
    _labels, ev = sim.find_groups(link, evals=True)
    cat = sim.group_catalogue(link, 20, capacity=64)
    print(json.dumps({"kind": "one", "case": case, "link": link, "evals_per_body": round(ev / n, 1), "n_groups": sim.n_groups,
                      "groups_of_20": cat["count"]}))
    sim.close()


def drive(out, reps, warmup, cases):
    os.makedirs(out, exist_ok=True)
    me = os.path.abspath(__file__)
    path = os.path.join(out, "fof_bench.jsonl")
    if os.path.exists(path):
        os.remove(path)
    raw = os.path.join(out, "fof_1m_raw")

    steps = [(["timeout", "-k", "10", str(STEP_TIMEOUT[c]), sys.executable, me, "--what", "calls", "--case", c, "--out", out,
               "--reps", str(reps), "--warmup", str(warmup)], dict(os.environ)) for c in cases]
    if "galaxy_1m" in cases:
        steps.append((["timeout", "-k", "10", str(STEP_TIMEOUT["profile"]), "rocprofv3", "--kernel-trace", "--stats",
                       "--output-format", "csv", "-d", raw, "--", sys.executable, me, "--what", "one", "--case", "galaxy_1m"],
                      dict(os.environ)))
    for cmd, env in steps:  # chained: a step that fails, faults or runs out of time ends the run
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:
            print(f"[fof_bench] step failed with status {rc}; stopping: {' '.join(cmd)}", file=sys.stderr)
            return rc
    if "galaxy_1m" in cases:
        stats = sorted(glob.glob(os.path.join(raw, "**", "*kernel_stats.csv"), recursive=True))
        if not stats:
            print("[fof_bench] rocprofv3 wrote no kernel_stats.csv", file=sys.stderr)
            return 1
        shutil.copyfile(stats[0], os.path.join(out, "fof_1m_kernel_stats.csv"))
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
