"""Cost of the tidal tensor (nbmi_tidal_at / nbmi_get_tidal_f64) beside the calls whose walk it shares, at
galaxy 1 M bodies, theta 0.5.  JSON lines in <out>/tidal_bench.jsonl, one per child process and multipole mode:

  {"kind": "tidal", "tree": "branch" | "parent", "round": r, "multipole": ..., "n": ..., "field_at_ms": ...,
   "potentials_ms": ..., "tracer_step_ms": ..., "step_ms": ..., "tidal_at_ms": ..., "tidal_bodies_ms": ...,
   "tidal_norm_ms": ..., "tidal_at_over_field_at": ..., "tidal_bodies_over_potentials": ..., "bit_equal": ...}

ms = host wall time of one blocking call, which ends in a device synchronise and includes the upload of the points and the
download of the results (mean over --reps, default 20, after --warmup calls of the same shape):
  field_at_ms       nbmi_field_at at the bodies' own positions (m = N = 1 M), acc, phi and terms: 24 bytes per point up, 36 down
  tidal_at_ms       nbmi_tidal_at at the same points, tidal6 and terms: 24 up, 52 down
  potentials_ms     nbmi_get_potentials_f64: 8 bytes per body down
  tidal_bodies_ms   nbmi_get_tidal_f64, tidal6 and norm: 56 down;  tidal_norm_ms: norm only, 8 down
  step_ms           one step of a fresh handle of the same bodies, synchronised
  tracer_step_ms    the same with 262 144 tracers on the bodies' first positions
A tree without the new calls (the parent commit) gets the first three and the steps: the existing instantiations of the
probe walk share a source function with the new one, so they are timed on both sides with this one script.

    python scripts/tidal_bench.py [--out profiles] [--parent PATH] [--rounds R]
        every child a process of its own under its own `timeout`, each started only if the one before succeeded; with
        --parent (a checkout of the parent commit, built) the two trees alternate, R rounds each, so that the run-to-run
        spread and the difference between the trees come from one session; then
        rocprofv3 --kernel-trace --stats ... -- --what one
        two calls of each probe kind in both modes on their own, no counters -> <out>/tidal_kernel_stats.csv
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

# bench.py's galaxy_1m_bh: distribution, N, R, G, eps, theta, dt
CASE = ("galaxy", 1_000_000, 800.0, 0.07, 1.5, 0.5, 0.05)
TRACERS = 262144
CHILD_TIMEOUT = 420


def _timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def _step_ms(sim, dt, reps, warmup):
    for _ in range(warmup):
        sim.step(dt)
    sim.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        sim.step(dt)
    sim.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def calls(tree, label, rnd, reps, warmup, out):
    sys.path.insert(0, tree)
    import importlib
    importlib.import_module("3d-spatial-sim-for-boid-and-nbody_amd")
    from nbody.gpu_backend import HIPBarnesHutSimulation
    dist, n, R, G, eps, theta, dt = CASE
    for multipole in ("monopole", "quadrupole"):
        sim = HIPBarnesHutSimulation.generated(dist, n, R, G, eps, 1.0, theta, seed=42, multipole=multipole)
        x = sim.get_positions_f64()
        rec = {"kind": "tidal", "tree": label, "round": rnd, "multipole": multipole, "n": n,
               "field_at_ms": round(_timed(lambda: sim.field_at(x, terms=True), reps, warmup), 3),
               "potentials_ms": round(_timed(sim.potentials, reps, warmup), 3)}
        if hasattr(sim, "tidal_at"):
            rec["tidal_at_ms"] = round(_timed(lambda: sim.tidal_at(x, terms=True), reps, warmup), 3)
            rec["tidal_bodies_ms"] = round(_timed(lambda: sim.tidal(norm=True), reps, warmup), 3)
            rec["tidal_norm_ms"] = round(_timed(sim.tidal_norm, reps, warmup), 3)
            rec["tidal_at_over_field_at"] = round(rec["tidal_at_ms"] / rec["field_at_ms"], 3)
            rec["tidal_bodies_over_potentials"] = round(rec["tidal_bodies_ms"] / rec["potentials_ms"], 3)
            t6, terms = sim.tidal_at(x, terms=True)
            rec["bit_equal"] = bool(np.array_equal(t6.view(np.uint64), sim.tidal().view(np.uint64))
                                    and np.array_equal(terms, sim.field_at(x, terms=True)[2]))
            rec["terms_per_body"] = round(float(terms.mean()), 1)
        sim.close()
        # the steps on a handle of their own: the same history on both trees
        sim = HIPBarnesHutSimulation.generated(dist, n, R, G, eps, 1.0, theta, seed=42, multipole=multipole)
        rec["step_ms"] = round(_step_ms(sim, dt, reps, warmup), 3)
        sim.set_tracers(x[:TRACERS])
        rec["tracer_step_ms"] = round(_step_ms(sim, dt, reps, warmup), 3)
        sim.close()
        line = json.dumps(rec)
        print(line, flush=True)
        with open(os.path.join(out, "tidal_bench.jsonl"), "a") as f:
            f.write(line + "\n")


def one(tree):
    """one call of each probe kind in both modes, for the kernel trace"""
    sys.path.insert(0, tree)
    import importlib
    importlib.import_module("3d-spatial-sim-for-boid-and-nbody_amd")
    from nbody.gpu_backend import HIPBarnesHutSimulation
    dist, n, R, G, eps, theta, dt = CASE
    for multipole in ("monopole", "quadrupole"):
        sim = HIPBarnesHutSimulation.generated(dist, n, R, G, eps, 1.0, theta, seed=42, multipole=multipole)
        x = sim.get_positions_f64()
        for _ in range(2):
            sim.field_at(x, terms=True)
            sim.tidal_at(x, terms=True)
            sim.potentials()
            norm = sim.tidal(norm=True)[1]
        print(json.dumps({"kind": "one", "multipole": multipole, "norm_median": float(np.median(norm))}))
        sim.close()


def drive(out, parent, rounds, reps, warmup):
    os.makedirs(out, exist_ok=True)
    me = os.path.abspath(__file__)
    path = os.path.join(out, "tidal_bench.jsonl")
    if os.path.exists(path):
        os.remove(path)
    trees = [("branch", ROOT)] + ([("parent", os.path.abspath(parent))] if parent else [])
    for rnd in range(rounds):
        for label, tree in trees:  # chained: a child that fails, faults or runs out of time ends the run
            cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, me, "--what", "calls", "--tree", tree, "--label", label,
                   "--round", str(rnd), "--out", out, "--reps", str(reps), "--warmup", str(warmup)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print(f"[tidal_bench] child failed with status {rc}; stopping: {' '.join(cmd)}", file=sys.stderr)
                return rc
    raw = os.path.join(out, "tidal_raw")
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", raw,
           "--", sys.executable, me, "--what", "one"]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"[tidal_bench] the kernel trace failed with status {rc}: {' '.join(cmd)}", file=sys.stderr)
        return rc
    stats = sorted(glob.glob(os.path.join(raw, "**", "*kernel_stats.csv"), recursive=True))
    if not stats:
        print("[tidal_bench] rocprofv3 wrote no kernel_stats.csv", file=sys.stderr)
        return 1
    shutil.copyfile(stats[0], os.path.join(out, "tidal_kernel_stats.csv"))
    shutil.rmtree(raw, ignore_errors=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", default="all", choices=("all", "calls", "one"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit to alternate with")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="branch")
    ap.add_argument("--round", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.what == "calls":
        calls(a.tree, a.label, a.round, a.reps, a.warmup, a.out)
        return 0
    if a.what == "one":
        one(a.tree)
        return 0
    return drive(a.out, a.parent, a.rounds, a.reps, a.warmup)


if __name__ == "__main__":
    sys.exit(main())
