"""The measurements of DESIGN 4.23 (periodic box and noise; include/bdmi.h), as JSON lines on stdout
(profiles/boids_periodic_noise.txt is one run of both parts).

    python scripts/gpu_periodic_noise_bench.py sweeps   periodic against walled sweep at 2 M boids (bench.py's boids_2m
                                                        flock), metric and topological k = 7, on the initial state and
                                                        after 1000 steps, then the four of them with eta = 0.5.  After
                                                        presteps + 3 steps, five consecutive batches of 20 steps from
                                                        the handle's device timers (Flock.timers()); reported: the batch
                                                        with the median sweep time, and the fastest and slowest one
                                                        (the state drifts, later batches are slower).
    python scripts/gpu_periodic_noise_bench.py demo     boids.analysis.noise_sweep on a periodic flock of 40 000 boids in
                                                        a box of bounds 40 (about 40 metric neighbours each): polarisation
                                                        and Binder cumulant per eta.

Each part is one process; run them under `timeout` one after the other.  There is no CPU path to time.
"""
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3d-spatial-sim-for-boid-and-nbody_amd")
import config.boids as bcfg  # noqa: E402
import nbmi_native  # noqa: E402
from boids import Flock  # noqa: E402
from boids.analysis import noise_sweep  # noqa: E402

DT = 1.0 / 60.0


def sweep_line(periodic, mode, eta, presteps, boids=2_000_000):
    fl = Flock(boids, seed=42, periodic=periodic)
    try:
        if mode == "topological":
            fl.set_neighbour_mode("topological", 7)
        if eta:
            fl.set_noise(eta, seed=1)
        fl.update(DT, presteps + 3)
        fl.sync()
        fl.enable_timers(True)
        batches = []
        for _ in range(5):
            fl.timers(reset=True)
            fl.update(DT, 20)
            fl.sync()
            tm = fl.timers(reset=True)
            batches.append([tm[k] / tm["steps"] for k in ("sort_ms", "table_ms", "sweep_ms")])
        batches.sort(key=lambda r: r[2])
        med = batches[len(batches) // 2]
        print(json.dumps(dict(periodic=periodic, mode=mode, eta=eta, presteps=presteps, sort_ms=round(med[0], 4),
                              table_ms=round(med[1], 4), sweep_ms=round(med[2], 4),
                              sweep_min_max=[round(batches[0][2], 4), round(batches[-1][2], 4)],
                              polarisation=round(float(fl.diagnostics()[7]), 4), occupied=fl.grid_info()["occupied"])),
              flush=True)
    finally:
        fl.close()


def sweeps():
    for presteps in (0, 1000):
        for mode in ("metric", "topological"):
            for periodic in (False, True):
                sweep_line(periodic, mode, 0.0, presteps)
    for periodic in (False, True):
        for mode in ("metric", "topological"):
            sweep_line(periodic, mode, 0.5, 0)


def demo(boids=40_000, bounds=40.0, steps=3000, discard=2000, every=20):
    bcfg.BOIDS["bounds"] = bounds

    def make():
        fl = Flock(boids, seed=42, periodic=True)
        fl.set_noise(0.0, seed=7)
        return fl

    t0 = time.perf_counter()
    rows = noise_sweep(make, [0.0, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0], steps, discard, every, DT)
    print(json.dumps(dict(n=boids, bounds=bounds, dt=DT, steps=steps, discard=discard, every=every, seed=42, noise_seed=7,
                          mode="metric", seconds=round(time.perf_counter() - t0, 1), inv_sqrt_n=boids ** -0.5)))
    for r in rows:
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    if nbmi_native.device_count() <= 0:
        raise SystemExit("gpu_periodic_noise_bench: no HIP device (there is no CPU path to time)")
    {"sweeps": sweeps, "demo": demo}[sys.argv[1] if len(sys.argv) > 1 else "sweeps"]()
