"""Cost of the field evaluation at arbitrary points (nbmi_field_at) at galaxy 1 M bodies.  JSON lines in
<out>/field_at_bench.jsonl, one per run:

  {"kind": "field_at", "sorted": 1 | 0, "n": ..., "potentials_ms": ..., "bodies_phi_ms": ..., "bodies_all_ms": ...,
   "bodies_all_over_potentials": ..., "bodies_phi_over_potentials": ..., "slice_1024_ms": ..., "slice_over_bodies_all_per_point": ...,
   "ring_256_ms": ..., "terms_per_body": ..., "terms_per_slice_point": ..., "step_ms": ...}

ms = host wall time of one blocking call, which ends in a device synchronise and includes the upload of the points and the
download of the results (mean over --reps after --warmup calls of the same shape):
  potentials_ms    nbmi_get_potentials_f64, the yardstick: the same build and the same walk with one accumulator, 8 bytes per
                   body downloaded
  bodies_phi_ms    field_at at the bodies' own positions (m = N), phi only: 24 bytes per point up, 8 down
  bodies_all_ms    the same with acc, phi and terms: 24 up, 36 down
  slice_1024_ms    potential_slice's 1024 x 1024 points in the plane z = 0, half extent R, acc and phi (one full chunk)
  ring_256_ms      rotation_curve's points: 16 radii x 16 azimuths (a call of one small chunk: the build and the waits)
  step_ms          one default step of the same handle, synchronised
sorted = 0 is the other side of the A/B: NBMI_FIELD_SORT=0, the points walk in the caller's order (the bodies' positions
come in the caller's order, which for generated bodies is not the key order; the slice comes row by row).

    python scripts/field_bench.py [--out profiles]    every step below as a child process under its own `timeout`, each
                                                      started only if the one before succeeded:
        --what calls                                  the line with the sort
        NBMI_FIELD_SORT=0 ... --what calls            the line without
        rocprofv3 --kernel-trace --stats ... -- --what one
                                                      one slice call on its own, no counters -> <out>/field_at_kernel_stats.csv
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
STEP_TIMEOUT = 300


def _sim():
    sys.path.insert(0, ROOT)
    import importlib
    importlib.import_module("3d-spatial-sim-for-boid-and-nbody_amd")
    from nbody.gpu_backend import HIPBarnesHutSimulation
    dist, n, R, G, eps, theta, dt = CASE
    return HIPBarnesHutSimulation.generated(dist, n, R, G, eps, 1.0, theta, seed=42), n, R, dt


def _timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def _slice_points(R, res=1024):
    u = (np.arange(res) + 0.5) * (2.0 * R / res) - R
    pts = np.zeros((res, res, 3))
    pts[:, :, 0] = u[None, :]
    pts[:, :, 1] = u[:, None]
    return pts.reshape(-1, 3)


def calls(reps, warmup, out):
    sim, n, R, dt = _sim()
    import nbmi_native as nat
    from nbody.field import ring_points
    for _ in range(warmup):
        sim.step(dt)
    sim.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        sim.step(dt)
    sim.sync()
    step_ms = (time.perf_counter() - t0) * 1e3 / reps
    x = sim.get_positions_f64()
    phi = np.empty(n)

    def phi_only():
        nat.check(sim._lib.nbmi_field_at(sim._h, n, nat.ptr(x), None, nat.ptr(phi), None), "nbmi_field_at")
    pot_ms = _timed(sim.potentials, reps, warmup)
    phi_ms = _timed(phi_only, reps, warmup)
    all_ms = _timed(lambda: sim.field_at(x, terms=True), reps, warmup)
    same = bool(np.array_equal(phi.view(np.uint64), sim.potentials().view(np.uint64)))
    terms_b = sim.field_at(x, terms=True)[2]
    grid = _slice_points(R)
    slice_ms = _timed(lambda: sim.field_at(grid), reps, warmup)
    terms_s = sim.field_at(grid, terms=True)[2]
    ring = ring_points(sim.diagnostics(potential=False).center_of_mass, R * np.arange(1, 17) / 16.0)
    ring_ms = _timed(lambda: sim.field_at(ring), 4 * reps, warmup)
    rec = {"kind": "field_at", "sorted": 0 if os.environ.get("NBMI_FIELD_SORT") == "0" else 1, "n": n,
           "potentials_ms": round(pot_ms, 3), "bodies_phi_ms": round(phi_ms, 3), "bodies_all_ms": round(all_ms, 3),
           "bodies_phi_over_potentials": round(phi_ms / pot_ms, 2), "bodies_all_over_potentials": round(all_ms / pot_ms, 2),
           "phi_equals_potentials": same, "slice_1024_ms": round(slice_ms, 3),
           "slice_over_bodies_all_per_point": round((slice_ms / len(grid)) / (all_ms / n), 2), "ring_256_ms": round(ring_ms, 3),
           "terms_per_body": round(float(terms_b.mean()), 1), "terms_per_slice_point": round(float(terms_s.mean()), 1),
           "step_ms": round(step_ms, 3)}
    sim.close()
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(out, "field_at_bench.jsonl"), "a") as f:
        f.write(line + "\n")


def one():
    sim, n, R, dt = _sim()
    sim.step(dt)
    grid = _slice_points(R)
    sim.field_at(grid)
    acc, phi = sim.field_at(grid)
    print(json.dumps({"kind": "one", "points": len(grid), "phi_min": float(phi.min()), "phi_max": float(phi.max())}))
    sim.close()


def drive(out, reps, warmup):
    os.makedirs(out, exist_ok=True)
    me = os.path.abspath(__file__)
    path = os.path.join(out, "field_at_bench.jsonl")
    if os.path.exists(path):
        os.remove(path)
    raw = os.path.join(out, "field_at_raw")

    def call(sort):
        return (["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, me, "--what", "calls", "--out", out, "--reps",
                 str(reps), "--warmup", str(warmup)], dict(os.environ, NBMI_FIELD_SORT="1" if sort else "0"))
    steps = [call(True), call(False),
             (["timeout", "-k", "10", str(STEP_TIMEOUT), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d",
               raw, "--", sys.executable, me, "--what", "one"], dict(os.environ))]
    for cmd, env in steps:  # chained: a step that fails, faults or runs out of time ends the run
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:
            print(f"[field_bench] step failed with status {rc}; stopping: {' '.join(cmd)}", file=sys.stderr)
            return rc
    stats = sorted(glob.glob(os.path.join(raw, "**", "*kernel_stats.csv"), recursive=True))
    if not stats:
        print("[field_bench] rocprofv3 wrote no kernel_stats.csv", file=sys.stderr)
        return 1
    shutil.copyfile(stats[0], os.path.join(out, "field_at_kernel_stats.csv"))
    shutil.rmtree(raw, ignore_errors=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", default="all", choices=("all", "calls", "one"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.what == "calls":
        calls(a.reps, a.warmup, a.out)
    elif a.what == "one":
        one()
    else:
        return drive(a.out, a.reps, a.warmup)
    return 0


if __name__ == "__main__":
    sys.exit(main())
