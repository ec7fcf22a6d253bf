"""Device flock renderer throughput (bdmi_render_flock, tools/flock_video.py).  Prints JSON lines:

  {"kind": "frame", ...}  per (boids, bounds, resolution, state): device ms per frame by phase (project + rasterise,
                          resolve, copy to the host; hipEvents, mean over --reps frames after --warmup), host wall ms
                          per blocking render_flock call, the frame's stats, and the yardstick: host wall ms of
                          Flock.visible_vertices() with the same camera (device cull + cones + 144 bytes per visible
                          boid to the host), timed in the same process, alternating with render_flock
  {"kind": "video", ...}  frames/s of tools.flock_video (raw output) and the share of the frame that is the step

    python scripts/flock_render_bench.py [--rows 500k,2m,dense,video] [--reps 10] [--warmup 3] [--video-frames 300]
    rocprofv3 --kernel-trace --stats -d <dir> -o flock2m --output-format csv -- python scripts/flock_render_bench.py --rows trace

State "flocked" = after --flock-steps (1 000) updates of 1/60 (DESIGN 4.4's steady state); "t0" = the initial state.
The dense row shrinks the box (--dense-bounds) and moves the camera in (--dense-radius) until a pixel holds tens of
fragments; `fragment_gbs` = fragments x 8 bytes over the rasterise time, an upper bound of the 64-bit atomic rate
(a fragment whose plain load already sees a smaller word issues no atomic).
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import importlib  # noqa: E402

importlib.import_module("3d-spatial-sim-for-boid-and-nbody_amd")

import numpy as np  # noqa: E402

from boids import Flock  # noqa: E402
from boids.render import HIPFlockRenderer, OrbitCamera  # noqa: E402
from config import boids as config  # noqa: E402
from tools.export import RESOLUTION_PRESETS  # noqa: E402


def make_flock(n, bounds, seed=1):
    saved = config.BOIDS
    config.BOIDS = dict(saved, bounds=float(bounds))
    try:
        return Flock(n, seed=seed)
    finally:
        config.BOIDS = saved


def frame_rows(n, bounds, radius, resolutions, states, flock_steps, reps, warmup):
    fl = make_flock(n, bounds)
    cam = OrbitCamera(radius=radius)
    f, right, up = cam.get_camera_axes()
    for state in states:
        if state == "flocked":
            fl.update(1.0 / 60.0, flock_steps)
            fl.sync()
        for res in resolutions:
            W, H = RESOLUTION_PRESETS[res]
            r = HIPFlockRenderer(W, H)
            out = np.empty((H, W, 3), dtype=np.uint8)
            vis = lambda: fl.visible_vertices(cam.get_position(), f, right, up, 90.0, W / H)  # noqa: E731
            for _ in range(warmup):
                r.render_flock(fl, cam, out=out)
                vis()
            acc = np.zeros(4)
            t_render = t_vis = 0.0
            for _ in range(reps):
                t0 = time.perf_counter()
                r.render_flock(fl, cam, out=out)
                t1 = time.perf_counter()
                vis()
                t2 = time.perf_counter()
                t_render += t1 - t0
                t_vis += t2 - t1
                acc += list(r.timers().values())
            ms = acc / reps
            st = r.stats()
            row = {"kind": "frame", "boids": n, "bounds": bounds, "camera_radius": radius, "res": res, "width": W,
                   "height": H, "state": state, "visible": fl._visible_count, **st,
                   "fragments_per_pixel": st["fragments"] / (W * H), "raster_ms": ms[0], "resolve_ms": ms[2],
                   "copy_ms": ms[3], "device_ms": float(ms.sum()), "render_flock_wall_ms": t_render / reps * 1e3,
                   "visible_vertices_wall_ms": t_vis / reps * 1e3, "visible_vertices_bytes": 144 * fl._visible_count,
                   "wall_ratio_vertices_over_frame": t_vis / t_render,
                   "fragment_gbs": st["fragments"] * 8 / (ms[0] * 1e-3) / 1e9 if ms[0] > 0 else None}
            print(json.dumps(row), flush=True)
            r.close()
    fl.close()


def video_row(n, res, frames):
    from tools import flock_video as fv
    with tempfile.TemporaryDirectory() as tmp:
        args = fv.build_parser().parse_args(["--boids", str(n), "--frames", str(frames), "--resolution", res, "--format",
                                             "raw", "-o", os.path.join(tmp, "bench.rgb"), "--seed", "1"])
        t = fv.run(args, say=lambda *a: None)
    print(json.dumps({"kind": "video", "boids": n, "res": res, "frames": frames, "fps": t["fps"], "wall_s": t["wall_s"],
                      "step_share": t["step_s"] / t["wall_s"], "render_share": t["render_s"] / t["wall_s"],
                      "write_share": t["write_s"] / t["wall_s"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="500k,2m,dense,video",
                    help="comma list of 500k, 2m, dense, video, trace (the 2 M 1080p frame alone, for rocprofv3 --kernel-trace)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--flock-steps", type=int, default=1000)
    ap.add_argument("--dense-bounds", type=float, default=40.0)
    ap.add_argument("--dense-radius", type=float, default=60.0)
    ap.add_argument("--video-frames", type=int, default=300)
    a = ap.parse_args()
    rows = a.rows.split(",")
    b, rad = config.BOIDS["bounds"], config.CAMERA["initial_radius"]
    if "500k" in rows:
        frame_rows(500_000, b, rad, ["720p"], ["t0", "flocked"], a.flock_steps, a.reps, a.warmup)
    if "2m" in rows:
        frame_rows(2_000_000, b, rad, ["1080p", "4k"], ["t0", "flocked"], a.flock_steps, a.reps, a.warmup)
    if "trace" in rows:
        frame_rows(2_000_000, b, rad, ["1080p"], ["t0"], a.flock_steps, a.reps, a.warmup)
    if "dense" in rows:
        frame_rows(2_000_000, a.dense_bounds, a.dense_radius, ["1080p"], ["t0"], a.flock_steps, a.reps, a.warmup)
    if "video" in rows:
        video_row(500_000, "720p", a.video_frames)


if __name__ == "__main__":
    main()
