"""Quadrupole mode (nbmi_set_multipole): step time, force error and energy drift against monopole terms.
JSON lines:

  {"kind": "step", ...}   per case and force precision: device ms per step (the library's phase timers: total, walk, tree)
                          of quadrupole handles at several theta, of a monopole handle at theta 0.5 and - with --parent-lib -
                          of the PARENT build's monopole handle at theta 0.5 (a second libnbmi.so loaded into the same
                          process; the same device-generated bodies).  The variants are alternated block by block after a
                          warm-up; median and spread over --reps blocks.
  {"kind": "error", ...}  the same variants: rms / p99 relative acceleration error of 2 048 sampled bodies against the
                          float64 direct sum of the oracle over all bodies
  {"kind": "drift", ...}  galaxy 1 M, leapfrog, 1 000 steps of dt 0.05: max |E - E0| / |E0| at theta 0.5 and 0.8, both modes

    python scripts/multipole_bench.py [--what step,error,drift] [--cases galaxy_1m,collision_10m,galaxy_10k]
                                      [--parent-lib PATH/libnbmi.so] [--reps 7] [--out profiles/multipole_bench.jsonl]
    python scripts/multipole_bench.py --what one --case galaxy_1m        (a few quadrupole steps: for rocprofv3)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import importlib  # noqa: E402

importlib.import_module("3d-spatial-sim-for-boid-and-nbody_amd")

import numpy as np  # noqa: E402

import nbmi_native  # noqa: E402
from nbody.gpu_backend import GENERATED_DISTRIBUTIONS, HIPBarnesHutSimulation  # noqa: E402

# name: (distribution, N, R, G, eps, dt, steps per timed block)
CASES = {
    "galaxy_10k": ("galaxy", 10_000, 500.0, 0.15, 3.0, 0.05, 100),
    "galaxy_1m": ("galaxy", 1_000_000, 800.0, 0.07, 1.5, 0.05, 10),        # bench.py galaxy_1m_bh
    "collision_10m": ("collision", 10_000_000, 2000.0, 0.08, 6.0, 0.25, 3),  # collision_10m_bh
}
THETAS = (0.5, 0.7, 0.8, 1.0)
OUT = []


def emit(rec):
    line = json.dumps(rec)
    OUT.append(line)
    print(line, flush=True)


def load_parent(path):
    """The parent build's library beside this build's: the symbols both have, bound like nbmi_native.load()"""
    lib = C.CDLL(path)
    for name, (res, args) in nbmi_native.PROTOTYPES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def make(case, theta, multipole="monopole", prec="auto", lib=None, integrator="kick_drift"):
    dist, n, R, G, eps, _, _ = CASES[case]
    if lib is None:
        sim = HIPBarnesHutSimulation.generated(dist, n, R, G, eps, 1.0, theta, seed=42, integrator=integrator,
                                               multipole=multipole)
    else:  # HIPBarnesHutSimulation.generated on another library (no multipole calls: the parent has none)
        sim = HIPBarnesHutSimulation.__new__(HIPBarnesHutSimulation)
        sim.n, sim.G, sim.softening, sim.damping, sim.theta, sim.device, sim._lib = n, G, eps, 1.0, theta, 0, lib
        sim._h = lib.nbmi_create_generated(GENERATED_DISTRIBUTIONS[dist], n, R, 42, G, eps, 1.0, theta, 0, 0)
        assert sim._h, "nbmi_create_generated failed on the parent library"
    sim.set_force_precision(prec)
    return sim


def variants(case, prec, parent):
    v = {}
    if parent is not None:
        v["parent_mono_0.5"] = make(case, 0.5, prec=prec, lib=parent)
    v["mono_0.5"] = make(case, 0.5, prec=prec)
    for th in THETAS:
        v[f"quad_{th}"] = make(case, th, "quadrupole", prec=prec)
    return v


def _block(sim, dt, k):
    sim.timers(reset=True)
    sim.step_many(dt, k)
    sim.sync()
    t = sim.timers(reset=True)
    tot = (t["keys_ms"] + t["sort_ms"] + t["tree_ms"] + t["walk_ms"]) / k
    return tot, t["walk_ms"] / k, t["tree_ms"] / k


def step(cases, precs, reps, warmup, parent):
    for case in cases:
        dt, k = CASES[case][5], CASES[case][6]
        for prec in precs:
            v = variants(case, prec, parent)
            for s in v.values():
                s.enable_timers(True)
                s.step_many(dt, warmup)
                s.sync()
            t = {name: [] for name in v}
            for _ in range(reps):
                for name, s in v.items():
                    t[name].append(_block(s, dt, k))
            for name, s in v.items():
                a = np.array(t[name])
                emit({"kind": "step", "case": case, "n": CASES[case][1], "precision": prec, "variant": name, "dt": dt,
                      "block_steps": k, "reps": reps, "ms_per_step": round(float(np.median(a[:, 0])), 4),
                      "spread_ms": [round(float(a[:, 0].min()), 4), round(float(a[:, 0].max()), 4)],
                      "walk_ms": round(float(np.median(a[:, 1])), 4), "tree_ms": round(float(np.median(a[:, 2])), 4),
                      "tree_spread_ms": [round(float(a[:, 2].min()), 4), round(float(a[:, 2].max()), 4)]})
                s.close()


def error(cases, precs):
    from oracle import pyref
    for case in cases:
        G, eps = CASES[case][3], CASES[case][4]
        ref = None
        for prec in precs:
            for name, (th, mp) in {"mono_0.5": (0.5, "monopole"), **{f"quad_{t}": (t, "quadrupole") for t in THETAS}}.items():
                s = make(case, th, mp, prec=prec)
                if ref is None:
                    p, m = s.get_positions_f64(), s.get_masses()
                    rows = np.linspace(0, len(p) - 1, 2048).astype(np.int64)
                    ref = pyref.direct_forces_subset(np.ascontiguousarray(p), np.ascontiguousarray(m), rows, G, eps)
                a = s.accelerations()[rows]
                s.close()
                e = np.linalg.norm(a - ref, axis=1) / np.linalg.norm(ref, axis=1)
                emit({"kind": "error", "case": case, "precision": prec, "variant": name, "sampled": len(rows),
                      "rms": float(f"{np.sqrt((e * e).mean()):.4e}"), "p99": float(f"{np.quantile(e, 0.99):.4e}"),
                      "max": float(f"{e.max():.4e}")})


def drift():
    for th in (0.5, 0.8):
        for mp in ("monopole", "quadrupole"):
            sim = make("galaxy_1m", th, mp, integrator="leapfrog")
            d0 = sim.diagnostics()
            rows = []
            t0 = time.perf_counter()
            for k in range(20):
                sim.step_many(0.05, 50)
                d = sim.diagnostics()
                rows.append([(k + 1) * 50, abs(d.total - d0.total) / abs(d0.total)])
            emit({"kind": "drift", "case": "galaxy_1m", "integrator": "leapfrog", "multipole": mp, "theta": th, "dt": 0.05,
                  "steps": 1000, "max_dE": max(r[1] for r in rows), "final_dE": rows[-1][1],
                  "every_50": [[r[0], float(f"{r[1]:.3e}")] for r in rows], "wall_s": round(time.perf_counter() - t0, 1)})
            sim.close()


def one(case):
    sim = make(case, 0.5, "quadrupole")
    sim.step_many(CASES[case][5], 5)
    sim.sync()
    sim.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="step,error,drift")
    ap.add_argument("--cases", default="galaxy_1m,collision_10m,galaxy_10k")
    ap.add_argument("--case", default="galaxy_1m")
    ap.add_argument("--precisions", default="f32,auto")
    ap.add_argument("--parent-lib", default=None, help="libnbmi.so of the parent commit, built beside this one")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    what = args.what.split(",")
    if "one" in what:
        one(args.case)
        return
    cases, precs = args.cases.split(","), args.precisions.split(",")
    parent = load_parent(args.parent_lib) if args.parent_lib else None
    if "step" in what:
        step(cases, precs, args.reps, args.warmup, parent)
    if "error" in what:
        error([c for c in cases if c != "galaxy_10k"], precs)
    if "drift" in what:
        drift()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("".join(line + "\n" for line in OUT))


if __name__ == "__main__":
    main()
