"""The measurements of DESIGN 4.25 (bdmi_velocity_correlation, include/bdmi.h): what one blocking call costs on the host.

    python scripts/vcorr_bench.py                       every size, walled and periodic, one process each, then the
                                                        rocprofv3 run; results in profiles/vcorr_bench.jsonl and
                                                        profiles/vcorr_500k_kernel_stats.csv
    python scripts/vcorr_bench.py --what calls --boids 500000 [--periodic]
                                                        boids.Flock(seed 42) after 1000 steps of 1/60: the wall time of
                                                        Flock.velocity_correlation at reach 1, 2 and 4 cells with 16
                                                        linear bins from 0 (tools.flock_video's auto convention at reach
                                                        4), of heading_moments, and in the same process of neighbour_stats
                                                        at the perception radius and of one step.  Per call: two
                                                        unrecorded runs, then seven timed; the median, the fastest and the
                                                        slowest.  evals per boid is recorded with every reach.
    python scripts/vcorr_bench.py --what one            500 000 walled boids, one call per reach: for
        rocprofv3 --kernel-trace --stats ... -- python scripts/vcorr_bench.py --what one

Every step runs under a time limit of its own and a step that fails ends the run.  There is no CPU path to time.
"""
import argparse
import glob
import importlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3d-spatial-sim-for-boid-and-nbody_amd")
import numpy as np  # noqa: E402

DT = 1.0 / 60.0
SIZES = (100_000, 500_000, 2_000_000)
REACHES = (1, 2, 4)
STEP_TIMEOUT = 240


def timed(call, runs=7, unrecorded=2):
    for _ in range(unrecorded):
        out = call()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = call()
        ms.append(1e3 * (time.perf_counter() - t0))
    return out, dict(median_ms=round(statistics.median(ms), 3), min_max_ms=[round(min(ms), 3), round(max(ms), 3)])


def _flock(boids, periodic, presteps):
    from boids import Flock
    fl = Flock(boids, seed=42, periodic=periodic)
    fl.update(DT, presteps)
    fl.sync()
    return fl


def calls(boids, periodic, presteps, out):
    fl = _flock(boids, periodic, presteps)
    try:
        cell = fl.box["cell_size"]
        rec = dict(kind="calls", boids=boids, periodic=periodic, presteps=presteps, bins=16)
        nb, rec["neighbour_stats"] = timed(fl.periodic_neighbour_stats if periodic else fl.neighbour_stats)
        rec["neighbour_stats"]["evals_per_boid"] = round(nb["evals"] / boids, 2)
        _, rec["heading_moments"] = timed(fl.heading_moments)
        for m in REACHES:
            res, t = timed(lambda: fl.velocity_correlation(np.linspace(0.0, m * cell, 17)))
            assert res["reach"] == m
            t.update(evals_per_boid=round(res["evals"] / boids, 2), pairs_in_range=int(res["pairs"].sum()))
            rec[f"reach_{m}"] = t
        rec["occupied"] = fl.grid_info()["occupied"]

        def step():
            fl.update(DT)
            fl.sync()
        _, rec["step"] = timed(step)
    finally:
        fl.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "vcorr_bench.jsonl"), "a") as f:
            f.write(line + "\n")


def one(boids, presteps):
    fl = _flock(boids, False, presteps)
    try:
        cell = fl.box["cell_size"]
        ev = {m: fl.velocity_correlation(np.linspace(0.0, m * cell, 17))["evals"] for m in REACHES}
        fl.neighbour_stats()
    finally:
        fl.close()
    print(json.dumps(dict(kind="one", boids=boids, evals_per_boid={m: round(e / boids, 2) for m, e in ev.items()})))


def drive(out, presteps):
    os.makedirs(out, exist_ok=True)
    me = os.path.abspath(__file__)
    path = os.path.join(out, "vcorr_bench.jsonl")
    if os.path.exists(path):
        os.remove(path)
    raw = os.path.join(out, "vcorr_500k_raw")
    limit = ["timeout", "-k", "10", str(STEP_TIMEOUT)]
    steps = [limit + [sys.executable, me, "--what", "calls", "--boids", str(n), "--presteps", str(presteps), "--out", out] + p
             for n in SIZES for p in ([], ["--periodic"])]
    steps.append(limit + ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", raw, "--", sys.executable, me,
                          "--what", "one", "--presteps", str(presteps)])
    for cmd in steps:  # chained: a step that fails, faults or runs out of time ends the run
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"[vcorr_bench] step failed with status {rc}; stopping: {' '.join(cmd)}", file=sys.stderr)
            return rc
    stats = sorted(glob.glob(os.path.join(raw, "**", "*kernel_stats.csv"), recursive=True))
    if not stats:
        print("[vcorr_bench] rocprofv3 wrote no kernel_stats.csv", file=sys.stderr)
        return 1
    shutil.copyfile(stats[0], os.path.join(out, "vcorr_500k_kernel_stats.csv"))
    shutil.rmtree(raw, ignore_errors=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", default="all", choices=("all", "calls", "one"))
    ap.add_argument("--boids", type=int, default=500_000)
    ap.add_argument("--periodic", action="store_true")
    ap.add_argument("--presteps", type=int, default=1000)
    ap.add_argument("--out", default=None, help="directory of vcorr_bench.jsonl (default for --what all: profiles/)")
    a = ap.parse_args()
    if a.what != "all":  # (the driver itself never opens the device: its steps do)
        import nbmi_native
        if nbmi_native.device_count() <= 0:
            raise SystemExit("vcorr_bench: no HIP device (there is no CPU path to time)")
    if a.what == "calls":
        calls(a.boids, a.periodic, a.presteps, a.out)
    elif a.what == "one":
        one(a.boids, a.presteps)
    else:
        sys.exit(drive(a.out or os.path.join(ROOT, "profiles"), a.presteps))


if __name__ == "__main__":
    main()
