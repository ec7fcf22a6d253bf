"""Frame fetch and recorder timing: sequential against pipelined, and this tree against another checkout.

Figures, seconds per frame of `--substeps` steps (every timed block ends in a synchronise or in the frame_wait of its
last frame; blocks of `--frames` frames, `--blocks` of each, the figures alternating inside one process):

  A        compute only: step_many + sync per frame   (A, S and P blocks all start from the same state: the one
           after the case's warm-up steps, restored with set_state, plus two untimed frames)
  S_raw    sequential fetch, no file: step_many, compute_colors, get_positions, get_colors   (bench.py frame_rates)
  S_delta  the same with frame_delta (after one keyframe)
  P_raw    pipelined fetch, no file: step_many, frame_begin("f32"), frame_wait + frame_release of the previous frame
  P_delta  the same with "delta" frames (after one "key" frame)
  R_*      record() end to end into a temporary directory (removed afterwards): R_raw, R_zstd sequential,
           R_raw_pipe, R_zstd_pipe with "pipeline": True; seconds per frame of the whole call, set-up included
  H_raw    host only: the payloads of one frame written from memory with save_frame, no GPU call
  H_zstd   host only: pack_container + write_bytes_atomic of one delta payload

A tree without frame_begin (a checkout of an earlier commit) is timed by the same script: the P and *_pipe figures are
left out.  With --other DIR the same worker runs in DIR's tree as a second process and the blocks of the two alternate:

    python scripts/record_bench.py --case galaxy_1m --figures A,S_raw,S_delta,P_raw,P_delta,R_raw,R_raw_pipe,H_raw \\
        --other ../parent --out profiles/record_pipeline_bench.jsonl
    python scripts/record_bench.py --case galaxy_1m --trace-run P_raw      (one block, for rocprofv3 --kernel-trace)

One JSON line per (tree, figure) with the median over the blocks, every block's value and the spread (max - min) is
appended to --out; figures derived from them (P / A and so on) go into a last "summary" line.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "3d-spatial-sim-for-boid-and-nbody_amd"

# name: (distribution, N, R, G, eps, theta, dt per step, steps before the timed blocks)
CASES = {
    "galaxy_1m": ("galaxy", 1_000_000, 800.0, 0.07, 1.5, 0.5, 0.05, 200),          # bench.py galaxy_1m_bh; the
    # force-precision switch has settled after 200 steps
    "collision_10m": ("collision", 10_000_000, 2000.0, 0.08, 6.0, 0.5, 0.25, 20),  # bench.py collision_10m_bh
    "galaxy_20k": ("galaxy", 20_000, 500.0, 0.15, 3.0, 0.5, 0.05, 10),             # rehearsal size
}


# ---- the worker: one tree, one process; a figure name per line on stdin, a JSON line per block on stdout -------------
def worker(root, case, substeps, frames, rec_frames, zstd_frames, commands=None):
    import contextlib
    import importlib
    sys.path.insert(0, root)
    with contextlib.redirect_stdout(sys.stderr):
        importlib.import_module(PKG)
        from nbody.gpu_backend import HIPBarnesHutSimulation
        from tools import record as rec
        dist, n, R, G, eps, theta, dt, presteps = CASES[case]
        sim = HIPBarnesHutSimulation.generated(dist, n, R, G, eps, 1.0, theta, seed=42)
        sim.step_many(dt, presteps)
        sim.sync()
        # every A / S / P block starts from this state: a block advances the system by hundreds of steps, and the step
        # time follows the system's evolution (the blocks of one figure would otherwise not time the same work)
        x0, v0 = sim.get_positions_f64(), sim.get_velocities()
    has_async = hasattr(sim, "frame_begin")
    tmp_root = tempfile.mkdtemp(prefix="record_bench_")
    host = {}

    def seq(delta):
        if delta:
            sim.compute_colors(15.0)
            sim.frame_keyframe()

        def run(k):
            for _ in range(k):
                sim.step_many(dt, substeps)
                sim.compute_colors(15.0)
                if delta:
                    sim.frame_delta()
                else:
                    sim.get_positions()
                    sim.get_colors()
        return run

    def pipe(delta):
        if delta:
            s = sim.frame_begin("key", 15.0)
            sim.frame_wait(s)
            sim.frame_release(s)

        def run(k):
            prev = None
            for _ in range(k):
                sim.step_many(dt, substeps)
                s = sim.frame_begin("delta" if delta else "f32", 15.0)
                if prev is not None:
                    sim.frame_wait(prev)
                    sim.frame_release(prev)
                prev = s
            sim.frame_wait(prev)
            sim.frame_release(prev)
        return run

    def compute(k):
        for _ in range(k):
            sim.step_many(dt, substeps)
            sim.sync()

    def recording(zstd, pipeline):
        def run(k):
            cfg = {"name": "bench", "session_name": "s", "distribution": dist, "num_bodies": n, "spawn_radius": R, "G": G,
                   "softening": eps, "damping": 1.0, "theta": theta, "dt_per_frame": dt * substeps, "substeps": substeps,
                   "total_frames": k, "device_ic": True}
            if zstd:
                cfg["zstd"] = True
            if pipeline:
                cfg["pipeline"] = True
            try:
                with contextlib.redirect_stdout(sys.stderr):
                    rec.record(cfg, root=tmp_root, quiet=True, seed=42)
            finally:
                shutil.rmtree(os.path.join(tmp_root, "recordings"), ignore_errors=True)
        return run

    def host_only(zstd):
        def run(k):
            if not host:  # one frame's payloads, taken once (outside the timed region of every later block)
                sim.compute_colors(15.0)
                host["p"], host["c"] = sim.get_positions(), sim.get_colors()
                sim.frame_keyframe()
                sim.step_many(dt, substeps)
                sim.compute_colors(15.0)
                host["dp"], host["dc"] = sim.frame_delta()
            d = os.path.join(tmp_root, "host")
            os.makedirs(d, exist_ok=True)
            try:
                for i in range(k):
                    if zstd:
                        rec.write_bytes_atomic(rec._frame_paths(d, i)[0],
                                               rec.pack_container(2, host["dp"].tobytes(), host["dc"].tobytes()))
                    else:
                        rec.save_frame(d, i, host["p"], host["c"])
            finally:
                shutil.rmtree(d, ignore_errors=True)
        return run

    makers = {"A": lambda: compute, "S_raw": lambda: seq(False), "S_delta": lambda: seq(True),
              "R_raw": lambda: recording(False, False), "R_zstd": lambda: recording(True, False),
              "H_raw": lambda: host_only(False), "H_zstd": lambda: host_only(True)}
    if has_async:
        makers.update({"P_raw": lambda: pipe(False), "P_delta": lambda: pipe(True),
                       "R_raw_pipe": lambda: recording(False, True), "R_zstd_pipe": lambda: recording(True, True)})
    warmed = set()
    print(json.dumps({"ready": True, "figures": sorted(makers), "n": n}), flush=True)
    try:
        for line in (commands if commands is not None else sys.stdin):
            fig = line.strip()
            if not fig or fig == "quit":
                break
            if fig not in makers:
                print(json.dumps({"figure": fig, "skipped": "not in this tree"}), flush=True)
                continue
            k = rec_frames if fig[0] in "RH" else frames
            slow = "zstd" in fig  # level-19 zstd of a 1 M-body frame takes seconds: its own, smaller frame count
            if slow:
                k = zstd_frames
            run = makers[fig]()
            if fig not in warmed and fig[0] != "R" and not slow:  # first use of a path: untimed
                run(2)
                warmed.add(fig)
            if fig[0] not in "RH":
                sim.set_state(x0, v0)
                sim.step_many(dt, 2 * substeps)  # untimed: the first steps after a new state rebuild the order from scratch
            sim.sync()
            t0 = time.perf_counter()
            run(k)
            if fig[0] not in "RH":
                sim.sync()
            t = time.perf_counter() - t0
            print(json.dumps({"figure": fig, "frames": k, "block_s": t, "s_per_frame": t / k}), flush=True)
    finally:
        sim.close()
        shutil.rmtree(tmp_root, ignore_errors=True)


# ---- the driver -------------------------------------------------------------------------------------------------------
class Tree:
    def __init__(self, name, root, a):
        self.name, self.root = name, root
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", root, "--case", a.case, "--substeps", str(a.substeps),
               "--frames", str(a.frames), "--rec-frames", str(a.rec_frames), "--zstd-frames", str(a.zstd_frames)]
        self.p = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=root)
        self.info = self._read()
        self.blocks = {}

    def _read(self):
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError(f"worker of {self.name} ended (exit code {self.p.wait()})")
        return json.loads(line)

    def block(self, fig):
        self.p.stdin.write(fig + "\n")
        self.p.stdin.flush()
        r = self._read()
        if "s_per_frame" in r:
            self.blocks.setdefault(fig, []).append(r)
        return r

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait(timeout=120)


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", default="galaxy_1m", choices=sorted(CASES))
    ap.add_argument("--figures", default="A,S_raw,S_delta,P_raw,P_delta")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--frames", type=int, default=150, help="frames per block of A / S / P (a block should last >= 1 s)")
    ap.add_argument("--rec-frames", type=int, default=60, help="frames per block of R / H")
    ap.add_argument("--zstd-frames", type=int, default=3, help="frames per block of R_zstd* / H_zstd")
    ap.add_argument("--substeps", type=int, default=5)
    ap.add_argument("--other", default=None, help="a second checkout (built), timed in alternation with this tree")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "record_pipeline_bench.jsonl"))
    ap.add_argument("--trace-run", default=None, metavar="FIGURE", help="one block of FIGURE in this process (for a profiler)")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.case, a.substeps, a.frames, a.rec_frames, a.zstd_frames)
        return
    if a.trace_run:  # in this process, so that a profiler started on this command sees the kernels
        worker(HERE, a.case, a.substeps, a.frames, a.rec_frames, a.zstd_frames, commands=[a.trace_run])
        return
    figures = a.figures.split(",")
    trees = [Tree("this", HERE, a)]
    if a.other:
        trees.append(Tree("other", os.path.abspath(a.other), a))
    try:
        for _ in range(a.blocks):
            for fig in figures:
                for t in trees:  # the same figure in the two trees back to back: the blocks alternate
                    r = t.block(fig)
                    print(f"[{t.name}] {json.dumps(r)}", file=sys.stderr, flush=True)
    finally:
        for t in trees:
            t.close()
    dist, n, *_ = CASES[a.case]
    lines, med = [], {}
    for t in trees:
        for fig, bl in t.blocks.items():
            v = [b["s_per_frame"] for b in bl]
            m = median(v)
            med[(t.name, fig)] = (m, max(v) - min(v))
            lines.append({"case": a.case, "n": n, "substeps": a.substeps, "tree": t.name, "figure": fig, "frames": bl[0]["frames"],
                          "blocks": len(v), "ms_per_frame": round(1e3 * m, 3), "spread_ms": round(1e3 * (max(v) - min(v)), 3),
                          "block_ms_per_frame": [round(1e3 * x, 3) for x in v],
                          "body_steps_per_s": n * a.substeps / m})
    summary = {"case": a.case, "summary": True}
    for t in trees:
        g = lambda f: med.get((t.name, f), (None, None))[0]  # noqa: E731
        if g("A"):
            for f in ("S_raw", "S_delta", "P_raw", "P_delta"):
                if g(f):
                    summary[f"{t.name}:{f}_rate_over_A"] = round(g("A") / g(f), 4)
            for f, h in (("R_raw_pipe", "H_raw"), ("R_zstd_pipe", "H_zstd"), ("R_raw", "H_raw"), ("R_zstd", "H_zstd")):
                if g(f) and g(h):
                    summary[f"{t.name}:{f}_over_max_A_H"] = round(g(f) / max(g("A"), g(h)), 4)
    lines.append(summary)
    for rec in lines:
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
