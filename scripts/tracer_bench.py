"""Cost of massless tracers carried by the integrator (nbmi_set_tracers) at galaxy 1 M bodies, theta 0.5,
kick-drift.  JSON lines in <out>/tracers_bench.jsonl, one per case:

  {"kind": "tracers", "case": "none" | "rings_65536" | "rings_1048576" | "bodies", "n": ..., "m": ...,
   "step_ms": [three runs], "step_ms_mean": ..., "added_ms": ..., "added_us_per_1000_tracers": ...}

step_ms = host wall time per step of `--steps` steps enqueued one by one and synchronised once at the end, after
`--warmup` steps of the same handle; every case is run `--repeats` times on one handle (the spread).  added_ms = the
case's mean minus the mean of "none" (the same handle before it got its tracers).
  none             no tracers: what bench.py's default case measures
  rings_M          M tracers from nbody.field.circular_tracers: M / 16 rings out to the spawn radius about the centre of mass
  bodies           m = N tracers at the bodies' own positions with the bodies' velocities

    python scripts/tracer_bench.py [--out profiles]   every step below as a child process under its own `timeout`, each
                                                      started only if the one before succeeded:
        --what cases                                  the lines above
        rocprofv3 --kernel-trace --stats ... -- --what one --case bodies | rings_65536
                                                      five steps of that case on their own, no counters
                                                      -> <out>/tracers_kernel_stats.csv, tracers_kernel_stats_rings_65536.csv
        --what ab --parent DIR                        only with --parent, a built checkout of the parent commit: bench.py's
                                                      default case there and here, alternated, `--repeats` runs each
                                                      -> <out>/tracers_parent_ab.txt (the hooks' cost without tracers)
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


def _steps_ms(sim, dt, steps, warmup):
    for _ in range(warmup):
        sim.step(dt)
    sim.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        sim.step(dt)
    sim.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def _rings(sim, m, R):
    from nbody.field import circular_tracers
    rings = m // 16
    center = sim.diagnostics(potential=False).center_of_mass
    return circular_tracers(sim, R * np.arange(1, rings + 1) / rings, center, per_ring=16)


def cases(steps, warmup, repeats, out):
    sim, n, R, dt = _sim()
    base = None
    for name, m in (("none", 0), ("rings_65536", 65536), ("rings_1048576", 1048576), ("bodies", n)):
        if name == "bodies":
            sim.set_tracers(sim.get_positions_f64(), sim.get_velocities())
        elif m:
            sim.set_tracers(*_rings(sim, m, R))
        assert sim.tracer_count == m
        runs = [_steps_ms(sim, dt, steps, warmup) for _ in range(repeats)]
        mean = float(np.mean(runs))
        base = mean if base is None else base
        rec = {"kind": "tracers", "case": name, "n": n, "m": m, "step_ms": [round(r, 3) for r in runs],
               "step_ms_mean": round(mean, 3), "added_ms": round(mean - base, 3),
               "added_us_per_1000_tracers": round((mean - base) * 1e6 / m, 3) if m else 0.0}
        if m:
            assert np.isfinite(sim.get_tracers()[0]).all()
        line = json.dumps(rec)
        print(line, flush=True)
        with open(os.path.join(out, "tracers_bench.jsonl"), "a") as f:
            f.write(line + "\n")
    sim.close()


def one(case):
    sim, n, R, dt = _sim()
    if case == "bodies":
        sim.set_tracers(sim.get_positions_f64(), sim.get_velocities())
    else:
        sim.set_tracers(*_rings(sim, int(case.split("_")[1]), R))
    for _ in range(5):
        sim.step(dt)
    p, _ = sim.get_tracers()
    print(json.dumps({"kind": "one", "case": case, "tracers": len(p), "largest": float(np.abs(p).max())}))
    sim.close()


def ab(parent, out, steps, warmup, repeats):
    """bench.py's own result line from the parent's checkout and from this one, in turn"""
    lines = []
    for i in range(1, repeats + 1):
        for name, where in (("parent", os.path.abspath(parent)), ("new", ROOT)):
            r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, "bench.py", "--gpus", "1", "--steps",
                                str(steps), "--warmup", str(warmup), "--no-cpu-baseline"], cwd=where, capture_output=True, text=True)
            if r.returncode != 0:
                print(r.stdout + r.stderr, file=sys.stderr)
                return r.returncode
            d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            lines += [f"== {name} {i}", json.dumps({k: d[k] for k in ("value", "ms_per_step", "steps", "warmup")})]
            print(lines[-2], lines[-1], flush=True)
    with open(os.path.join(out, "tracers_parent_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


def drive(out, steps, warmup, repeats, parent):
    os.makedirs(out, exist_ok=True)
    me = os.path.abspath(__file__)
    path = os.path.join(out, "tracers_bench.jsonl")
    if os.path.exists(path):
        os.remove(path)
    limit = ["timeout", "-k", "10", str(STEP_TIMEOUT)]
    traces = {"bodies": "tracers_kernel_stats.csv", "rings_65536": "tracers_kernel_stats_rings_65536.csv"}
    run = [limit + [sys.executable, me, "--what", "cases", "--out", out, "--steps", str(steps), "--warmup", str(warmup),
                    "--repeats", str(repeats)]]
    run += [limit + ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(out, "raw_" + case),
                     "--", sys.executable, me, "--what", "one", "--case", case] for case in traces]
    if parent:
        run.append([sys.executable, me, "--what", "ab", "--parent", parent, "--out", out, "--steps", str(steps), "--warmup",
                    str(warmup), "--repeats", str(repeats)])
    for cmd in run:  # chained: a step that fails, faults or runs out of time ends the run
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"[tracer_bench] step failed with status {rc}; stopping: {' '.join(cmd)}", file=sys.stderr)
            return rc
    for case, name in traces.items():
        raw = os.path.join(out, "raw_" + case)
        stats = sorted(glob.glob(os.path.join(raw, "**", "*kernel_stats.csv"), recursive=True))
        if not stats:
            print(f"[tracer_bench] rocprofv3 wrote no kernel_stats.csv for {case}", file=sys.stderr)
            return 1
        shutil.copyfile(stats[0], os.path.join(out, name))
        shutil.rmtree(raw, ignore_errors=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", default="all", choices=("all", "cases", "one", "ab"))
    ap.add_argument("--case", default="bodies", choices=("bodies", "rings_65536"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (for --what ab)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.what == "cases":
        cases(a.steps, a.warmup, a.repeats, a.out)
    elif a.what == "one":
        one(a.case)
    elif a.what == "ab":
        if not a.parent:
            ap.error("--what ab needs --parent DIR")
        return ab(a.parent, a.out, a.steps, a.warmup, a.repeats)
    else:
        return drive(a.out, a.steps, a.warmup, a.repeats, a.parent)
    return 0


if __name__ == "__main__":
    sys.exit(main())
