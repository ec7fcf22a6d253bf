"""Cost of the minimum spanning tree (nbmi_mst).  JSON lines in <out>/mst_bench.jsonl, one per case and library:

  {"kind": "mst", "case": ..., "lib": ..., "n": ..., "mst_ms": [...], "mst_ms_mean": ..., "last_call_round_ms": [...],
   "rounds": ..., "evals_per_body": ...,
   "per_round": [{"evals": ..., "edges": ..., "ms": ...}, ...], "link": ..., "fof_ms": ..., "fof_evals_per_body": ...,
   "knn1_ms": ..., "mst_over_fof": ..., "mst_over_knn1": ..., "longest_edge": ..., "median_edge": ...}

The state is the case's after --warmup default steps.  ms = host wall time of one blocking call: mst_ms lists the --reps
calls after one warm-up call, mean beside them; fof_ms and knn1_ms are means over --reps after one warm-up call of
find_groups(link) and knn(1) on the same state, link = twice the median nearest-neighbour distance (the recorder's "auto").
per_round comes from one more call with evals=True (nbmi_mst_rounds): the distances a round evaluated, the edges it
appended, the host's wall time for it.

    python scripts/mst_bench.py [--out profiles] [--lib other.so ...]
        every step below as a child process under its own `timeout`, each started only if the one before succeeded; with
        --lib the cases run twice per library, the shipped one first, alternating (an A/B: scripts/experiments/mst_no_carry.patch):
        --what calls --case galaxy_1m
        --what calls --case collision_10m
"lib" is "shipped" or the file name of the other library.  The first process of a session has twice been 20 ms slower
outside the rounds than every later one: with --lib read the second alternation.
"""
import argparse
import json
import os
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
STEP_TIMEOUT = {"galaxy_1m": 240, "collision_10m": 420}


def _sim(case):
    sys.path.insert(0, ROOT)
    import importlib
    importlib.import_module("3d-spatial-sim-for-boid-and-nbody_amd")
    from nbody.gpu_backend import HIPBarnesHutSimulation
    dist, n, R, G, eps, theta, dt = CASES[case]
    sim = HIPBarnesHutSimulation.generated(dist, n, R, G, eps, 1.0, theta, seed=42)
    return sim, n, dt


def _times(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def calls(case, reps, warmup, out):
    sim, n, dt = _sim(case)
    for _ in range(warmup):
        sim.step(dt)
    sim.sync()
    knn_ms = _times(lambda: sim.knn(1), reps)
    link = 2.0 * float(np.median(np.sqrt(sim.knn(1)[0])))
    fof_ms = _times(lambda: sim.find_groups(link), reps)
    _labels, fof_ev = sim.find_groups(link, evals=True)
    mst_ms = _times(lambda: sim.minimum_spanning_tree(), reps)
    last_round_ms = [round(r["ms"], 3) for r in sim.mst_rounds()]  # of the last timed call: what is left is build, sort, copies
    edges, d2, rounds, ev = sim.minimum_spanning_tree(evals=True)
    per_round = sim.mst_rounds()
    kept = int((d2 <= link * link).sum())
    assert kept == n - sim.n_groups, (kept, n, sim.n_groups)  # the header's consequence, at the size measured
    mean = float(np.mean(mst_ms))
    rec = {"kind": "mst", "case": case, "lib": os.path.basename(os.environ.get("NBMI_LIB", "shipped")), "n": n,
           "mst_ms": [round(x, 3) for x in mst_ms], "mst_ms_mean": round(mean, 3), "last_call_round_ms": last_round_ms,
           "rounds": rounds,
           "evals_per_body": round(ev / n, 1),
           "per_round": [{"evals": r["evals"], "edges": r["edges"], "ms": round(r["ms"], 3)} for r in per_round],
           "link": link, "fof_ms": round(float(np.mean(fof_ms)), 3), "fof_evals_per_body": round(fof_ev / n, 1),
           "knn1_ms": round(float(np.mean(knn_ms)), 3), "mst_over_fof": round(mean / float(np.mean(fof_ms)), 2),
           "mst_over_knn1": round(mean / float(np.mean(knn_ms)), 2), "longest_edge": float(np.sqrt(d2[-1])),
           "median_edge": float(np.sqrt(np.median(d2)))}
    sim.close()
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(out, "mst_bench.jsonl"), "a") as f:
        f.write(line + "\n")


def drive(out, reps, warmup, cases, libs):
    os.makedirs(out, exist_ok=True)
    me = os.path.abspath(__file__)
    path = os.path.join(out, "mst_bench.jsonl")
    if os.path.exists(path):
        os.remove(path)
    steps = []
    for c in cases:
        for lib in ([None] + list(libs)) * (2 if libs else 1):  # an A/B alternates twice: the spread beside the difference
            env = dict(os.environ)
            if lib:
                env["NBMI_LIB"] = os.path.abspath(lib)
            steps.append((["timeout", "-k", "10", str(STEP_TIMEOUT[c]), sys.executable, me, "--what", "calls", "--case", c,
                           "--out", out, "--reps", str(reps), "--warmup", str(warmup)], env))
    for cmd, env in steps:  # chained: a step that fails, faults or runs out of time ends the run
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:
            print(f"[mst_bench] step failed with status {rc}; stopping: {' '.join(cmd)}", file=sys.stderr)
            return rc
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", default="all", choices=("all", "calls"))
    ap.add_argument("--case", default=None, choices=sorted(CASES), help="one case only (default: both)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", action="append", default=[], help="another build of the library to run beside the shipped one")
    a = ap.parse_args()
    if a.what == "calls":
        calls(a.case or "galaxy_1m", a.reps, a.warmup, a.out)
        return 0
    return drive(a.out, a.reps, a.warmup, [a.case] if a.case else list(CASES), a.lib)


if __name__ == "__main__":
    sys.exit(main())
