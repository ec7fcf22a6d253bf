"""Device time of nbmi_radial_profile and nbmi_mass_radii on bench.py's two inputs, beside the yardstick:
nbmi_deposit with MASS under NGP on the same state.  JSON lines in <out>/profile_bench.jsonl, one per (shape, run, case):

  {"kind": "profile" | "mass_radii" | "deposit", "shape": "galaxy_1m" | "collision_10m", "n": ..., "run": 0 | 1 ...,
   "case": ..., "planes": ..., "shells": ..., "device_ms": ..., "device_ms_min": ..., "call_ms": ..., "stats": [...],
   "stream_floor_ms": ...}

cases      auto48_all / auto48_mass: 48 log-spaced shells (nbody/profile.py auto_edges), all 8 planes / NUMBER and MASS;
           one_shell_all / one_shell_mass: every body in the one shell (0, 100 R] - the worst case for the LDS table;
           fractions5: nbmi_mass_radii with 0.1, 0.25, 0.5, 0.75, 0.9;
           cube64_ngp_mass: nbmi_deposit, MASS, NGP, 64^3 cells over [-R, R]^3 (the yardstick: also one pass over the
           maxima and one scatter pass over N rows)
device_ms  hipEvent time of the call's kernels (no copies): what nbmi_enable_timers adds to "other" per call, mean over
           --reps calls after --warmup, and the smallest of them
call_ms    host wall time of the whole blocking call
stream_floor_ms  56 bytes per body (the seven float64 columns a pass reads) at 3.6 TB/s: a floor, not a target
The handle takes 2 steps first, so its state rows lie in key order as in a running simulation.  The centre is the centre
of mass, taken once before the timed calls.

    python scripts/profile_bench.py [--out profiles]   every (shape, run) as a child process under its own `timeout`,
                                                       each started only if the one before succeeded
        --runs 2                                       child processes per shape
        --what one --shape S                           the lines of one shape (PROFILE_BENCH_RUN of the environment names the run)
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# bench.py's galaxy_1m_bh and collision_10m_bh: distribution, N, R, G, eps, theta, dt
SHAPES = {"galaxy_1m": ("galaxy", 1_000_000, 800.0, 0.07, 1.5, 0.5, 0.05),
          "collision_10m": ("collision", 10_000_000, 2000.0, 0.08, 6.0, 0.5, 0.25)}
ALL = ("number", "mass", "radial_momentum", "radial_kinetic", "kinetic", "angular_momentum")
FRACTIONS = (0.1, 0.25, 0.5, 0.75, 0.9)
STEP_TIMEOUT = 240
STREAM_TBS = 3.6


def one(shape, reps, warmup, out):
    sys.path.insert(0, ROOT)
    import importlib
    importlib.import_module("3d-spatial-sim-for-boid-and-nbody_amd")
    from nbody.gpu_backend import HIPBarnesHutSimulation
    from nbody.profile import auto_edges
    dist, n, R, G, eps, theta, dt = SHAPES[shape]
    run = int(os.environ.get("PROFILE_BENCH_RUN", "0"))
    sim = HIPBarnesHutSimulation.generated(dist, n, R, G, eps, 1.0, theta, seed=42)
    try:
        sim.step_many(dt, 2)
        sim.sync()
        d = sim.diagnostics(potential=False)
        c, b = np.array(d.center_of_mass), np.array(d.momentum) / d.mass
        sim.enable_timers(True)
        auto, shell = auto_edges(R), [0.0, 100.0 * R]
        cases = {
            "auto48_all": ("profile", 8, 48, lambda: sim.radial_profile(auto, c, b, ALL, stats=True)["stats"]),
            "auto48_mass": ("profile", 2, 48, lambda: sim.radial_profile(auto, c, b, ("number", "mass"), stats=True)["stats"]),
            "one_shell_all": ("profile", 8, 1, lambda: sim.radial_profile(shell, c, b, ALL, stats=True)["stats"]),
            "one_shell_mass": ("profile", 2, 1, lambda: sim.radial_profile(shell, c, b, ("number", "mass"), stats=True)["stats"]),
            "fractions5": ("mass_radii", 0, 0, lambda: sim.mass_radii(FRACTIONS, center=c)["stats"]),
            "cube64_ngp_mass": ("deposit", 1, 0, lambda: sim.deposit((-R,) * 3, (R,) * 3, (64, 64, 64), scheme="ngp",
                                                                     quantities=("mass",), stats=True)["stats"]),
        }
        for name, (kind, planes, shells, call) in cases.items():
            for _ in range(warmup):
                stats = call()
            dev, wall = [], []
            for _ in range(reps):
                sim.timers(reset=True)
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(sim.timers()["other_ms"])
            line = {"kind": kind, "shape": shape, "n": n, "run": run, "case": name, "planes": planes, "shells": shells,
                    "device_ms": round(float(np.mean(dev)), 4), "device_ms_min": round(float(np.min(dev)), 4),
                    "call_ms": round(float(np.mean(wall)), 3), "stats": [int(x) for x in stats],
                    "stream_floor_ms": round(56.0 * n / (STREAM_TBS * 1e12) * 1e3, 4)}
            print(json.dumps(line), flush=True)
            with open(os.path.join(out, "profile_bench.jsonl"), "a") as f:
                f.write(json.dumps(line) + "\n")
    finally:
        sim.close()


def drive(out, reps, warmup, runs):
    for shape in SHAPES:
        for run in range(runs):
            env = dict(os.environ, PROFILE_BENCH_RUN=str(run))
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--what", "one",
                   "--shape", shape, "--out", out, "--reps", str(reps), "--warmup", str(warmup)]
            rc = subprocess.run(cmd, env=env).returncode
            if rc != 0:
                print(f"[profile_bench] {shape} run {run} ended with status {rc}: stopping here", flush=True)
                return rc
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", default="all", choices=("all", "one"))
    ap.add_argument("--shape", default="galaxy_1m", choices=sorted(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=2, help="child processes per shape")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.what == "one":
        one(args.shape, args.reps, args.warmup, args.out)
        return 0
    return drive(args.out, args.reps, args.warmup, args.runs)


if __name__ == "__main__":
    sys.exit(main())
