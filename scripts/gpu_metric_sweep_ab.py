"""Phase times of the metric boids step from the handle's device timers (Flock.timers()), for ONE checkout of this
repository: the tool behind "the metric mode does not pay for the topological one" (DESIGN 4.22).  One JSON line:

  {"tag": ..., "initial": {"sort_ms", "table_ms", "sweep_ms"}, "after_1000_steps": {...}}

bench.py's boids_2m flock (2 M boids, seed 42, dt = 1/60): 5 warm-up steps and 200 timed ones on the initial state, then
on to step 1000 and 200 timed steps there; each figure is the mean per step.  To compare two builds, run it for each
checkout in turn, several times, in one session (each run under its own `timeout`), and compare the sweep_ms:

    python scripts/gpu_metric_sweep_ab.py <checkout root> <tag>
"""
import importlib
import json
import sys

DT = 1.0 / 60.0


def main():
    root, tag = sys.argv[1], sys.argv[2]
    sys.path.insert(0, root)
    importlib.import_module("3d-spatial-sim-for-boid-and-nbody_amd")
    import nbmi_native
    from boids import Flock
    if nbmi_native.device_count() <= 0:
        raise SystemExit("gpu_metric_sweep_ab: no HIP device (there is no CPU path to time)")
    fl = Flock(2_000_000, seed=42)
    out = {"tag": tag}
    fl.enable_timers(True)
    for state, pre in (("initial", 5), ("after_1000_steps", 795)):
        fl.update(DT, pre)
        fl.sync()
        fl.timers(reset=True)
        fl.update(DT, 200)
        fl.sync()
        t = fl.timers(reset=True)
        out[state] = {k: round(t[k] / t["steps"], 5) for k in ("sort_ms", "table_ms", "sweep_ms")}
    fl.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
