"""The measurements of DESIGN 4.24 (flock analysis on periodic handles; include/bdmi.h), as JSON lines on stdout
(profiles/boids_periodic_flocks.txt is one run of both parts).

    python scripts/gpu_periodic_flocks_bench.py calls   the three periodic calls on bench.py's 2 M flock in a periodic
                                                        handle beside the walled calls of DESIGN 4.21 on the walled handle,
                                                        in one process: on the initial state and after 1000 steps, at
                                                        link = the perception radius, catalogue with min_members 20 and
                                                        capacity 64.  Per call: two unrecorded runs, then seven timed on
                                                        the host (every call waits for its own work); reported: the
                                                        median and the fastest and slowest.  The state is the same for
                                                        all runs of a line: the calls change nothing a step reads.
    python scripts/gpu_periodic_flocks_bench.py demo    order against noise with the flock picture: the periodic flock of
                                                        40 000 boids of DESIGN 4.23 (bounds 40), per eta the polarisation
                                                        beside the number of flocks, the largest flock's share and
                                                        whether it spans (boids.analysis.percolation_summary), at a
                                                        quarter and at half the perception radius, after `steps` updates.

Each part is one process; run them under `timeout` one after the other.  There is no CPU path to time.
"""
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3d-spatial-sim-for-boid-and-nbody_amd")
import config.boids as bcfg  # noqa: E402
import nbmi_native  # noqa: E402
from boids import Flock  # noqa: E402
from boids.analysis import percolation_summary  # noqa: E402

DT = 1.0 / 60.0


def timed(call, runs=7, unrecorded=2):
    for _ in range(unrecorded):
        out = call()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = call()
        ms.append(1e3 * (time.perf_counter() - t0))
    return out, dict(median_ms=round(statistics.median(ms), 3), min_max_ms=[round(min(ms), 3), round(max(ms), 3)])


def calls(boids=2_000_000):
    for presteps in (0, 1000):
        for periodic in (False, True):
            fl = Flock(boids, seed=42, periodic=periodic)
            try:
                if presteps:
                    fl.update(DT, presteps)
                    fl.sync()
                names = ("periodic_flocks", "periodic_flock_catalogue", "periodic_neighbour_stats") if periodic else \
                    ("flocks", "flock_catalogue", "neighbour_stats")
                f, t_f = timed(lambda: getattr(fl, names[0])())
                c, t_c = timed(lambda: getattr(fl, names[1])(min_members=20, capacity=64))
                nb, t_n = timed(lambda: getattr(fl, names[2])())
                print(json.dumps(dict(periodic=periodic, presteps=presteps, boids=boids, flocks=t_f, catalogue=t_c,
                                      neighbour_stats=t_n, n_flocks=f["n_flocks"], links=f["links"], evals=f["evals"],
                                      qualifying=c["count"], largest=int(c["members"][0]) if len(c["members"]) else 0,
                                      mean_neighbours=round(float(nb["count"].mean()), 3),
                                      occupied=fl.grid_info()["occupied"])), flush=True)
            finally:
                fl.close()


def demo(boids=40_000, bounds=40.0, steps=3000):
    bcfg.BOIDS["bounds"] = bounds
    links = [0.25 * float(bcfg.BOIDS["perception_radius"]), 0.5 * float(bcfg.BOIDS["perception_radius"])]
    print(json.dumps(dict(n=boids, bounds=bounds, dt=DT, steps=steps, seed=42, noise_seed=7, mode="metric", links=links)))
    for eta in (0.0, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0):
        fl = Flock(boids, seed=42, periodic=True)
        try:
            fl.set_noise(eta, seed=7)
            fl.update(DT, steps)
            for link in links:  # the same state at both linking lengths
                f = fl.periodic_flocks(link)
                cat = fl.periodic_flock_catalogue(link, min_members=1, capacity=64)
                s = percolation_summary(cat, boids)
                print(json.dumps(dict(eta=eta, link=link, polarisation=round(float(fl.diagnostics()[7]), 4),
                                      n_flocks=f["n_flocks"], links=f["links"],
                                      mean_neighbours=round(float(fl.periodic_neighbour_stats(link)["count"].mean()), 3),
                                      largest_fraction=round(s["largest_fraction"], 4), largest_spans=s["largest_spans"],
                                      spanning_of_64_largest=s["spanning_flocks"],
                                      largest_extent=[round(float(h - l), 2) for l, h in zip(cat["rows"][0, 10:13],
                                                                                             cat["rows"][0, 13:16])])),
                      flush=True)
        finally:
            fl.close()


if __name__ == "__main__":
    if nbmi_native.device_count() <= 0:
        raise SystemExit("gpu_periodic_flocks_bench: no HIP device (there is no CPU path to time)")
    {"calls": calls, "demo": demo}[sys.argv[1] if len(sys.argv) > 1 else "calls"]()
