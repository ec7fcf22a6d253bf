"""Frames or a video of a running flock, rendered headless on the GPU.

The reference shows its boids only in a window; this tool steps a Flock and draws every frame with the device
rasteriser (boids.render.HIPFlockRenderer; image semantics in include/bdmi.h), so a flock can be looked at on a
machine without GL, display or window system.

    python -m tools.flock_video --boids 500k --frames 300                  # ffmpeg if on PATH, else raw rgb24 + JSON
    python -m tools.flock_video --boids 2m --resolution 1080p --camera orbit --format ppm -o frames/
    python -m tools.flock_video --boids 2m --frames 600 --diagnostics 10   # + flock.flock.jsonl: flocks, order parameters
    python -m tools.flock_video --boids 500k --neighbours topological --topological-k 7   # the k nearest within sight
    python -m tools.flock_video --boids 100k --periodic --noise 0.5 --noise-seed 3        # no walls, vectorial noise
    python -m tools.flock_video --boids 100k --periodic --periodic-flocks --diagnostics 10 # + flocks through the faces
    python -m tools.flock_video --boids 100k --periodic --noise 2 --correlations 10        # + flock.correlation.jsonl: C(r)

Each frame: flock.update(dt, substeps), render_flock, sink.  Output formats and sinks are those of tools.export.
With --diagnostics K every K-th frame also appends one JSON line (boids.analysis.jsonl_line) to <output stem>.flock.jsonl:
the whole flock's row, the number of flocks and links at --link, the mean neighbour count and the rows of the 16 largest
flocks of at least --min-members boids, all computed on the device (include/bdmi.h).
With --neighbours topological the flock interacts by the topological rule of include/bdmi.h (--topological-k nearest
neighbours within the perception radius); the clip's metadata and the analysis lines then name the mode.
With --periodic the domain is the periodic box of include/bdmi.h (no walls, neighbours through the faces), with --noise ETA
every update adds a unit vector of amplitude ETA * max_force, drawn from (--noise-seed, update, boid), to each boid's
acceleration; both are set before the warm-up and named in the metadata and the analysis lines.  With --periodic alone
--diagnostics writes the whole flock's row only; --periodic-flocks (which needs --periodic) makes them the full lines of a
walled run, from the flock finder, catalogue and neighbour counts that follow links through the faces of the box
(Flock.periodic_flocks and its siblings), each listed flock with "spans": per axis, whether it occupies every slab.
With --correlations K every K-th frame appends one JSON line (boids.analysis.correlation_line) to
<output stem>.correlation.jsonl, a file of its own: the exact pair counts and heading-fluctuation sums per distance bin of
Flock.velocity_correlation, the correlation function C, its first zero crossing xi and the susceptibility chi.
--correlation-edges lists the bin edges; auto is 17 linear edges from 0 to 4 cell sizes (a convention, not a measured
optimum).  It works with --periodic, --noise and both neighbour modes; the metadata names the file beside "diagnostics".
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

from config import boids as config
from tools.export import (CODECS, FORMATS, QUALITY_PRESETS, RESOLUTION_PRESETS, _FfmpegSink, _PpmSink, _RawSink,
                          ffmpeg_command, format_time, have_ffmpeg)
from tools.record import parse_number

CAMERA_MODES = ("fixed", "orbit")
NEIGHBOUR_MODES = ("metric", "topological")
MAX_DT = 0.05  # the reference application caps a frame's dt (Application._update)


def build_parser():
    cam = config.CAMERA
    ap = argparse.ArgumentParser(prog="python -m tools.flock_video",
                                 description="Run a flock and write its frames, rendered on the GPU")
    ap.add_argument("--boids", type=parse_number, default=config.BOIDS["count"], help="number of boids (500k, 2m, ...)")
    ap.add_argument("--frames", type=int, default=300, help="frames to write (default: 300)")
    ap.add_argument("--fps", type=int, default=30, help="output FPS (default: 30)")
    ap.add_argument("--dt", type=float, default=None, help=f"time per frame (default: 1 / fps, at most {MAX_DT})")
    ap.add_argument("--substeps", type=int, default=1, help="flock updates of dt per frame (default: 1)")
    ap.add_argument("--seed", type=int, default=None, help="seed of the initial state")
    ap.add_argument("--warmup", type=int, default=0, help="updates before the first frame (default: 0)")
    ap.add_argument("--resolution", choices=list(RESOLUTION_PRESETS), default="720p", help="output size (default: 720p)")
    ap.add_argument("--camera", choices=CAMERA_MODES, default="orbit", help="camera animation (default: orbit)")
    ap.add_argument("--camera-speed", type=float, default=0.3, help="orbit speed in degrees/frame (default: 0.3)")
    ap.add_argument("--camera-radius", type=float, default=cam["initial_radius"], help="distance from the centre")
    ap.add_argument("--camera-angle", type=float, default=cam["initial_phi"], help="vertical angle, 0 = horizon")
    ap.add_argument("--camera-theta", type=float, default=cam["initial_theta"], help="horizontal starting angle")
    ap.add_argument("--quality", choices=list(QUALITY_PRESETS), default="balanced", help="ffmpeg quality preset")
    ap.add_argument("--crf", type=int, help="override the CRF value (0-51, lower = better)")
    ap.add_argument("--codec", choices=CODECS, default="h264", help="video codec (default: h264)")
    ap.add_argument("-o", "--output", type=str, help="output file (ffmpeg, raw) or directory (ppm)")
    ap.add_argument("--format", choices=FORMATS, default=None,
                    help="ffmpeg (default when ffmpeg is on PATH), raw rgb24 + JSON sidecar, or one PPM per frame")
    ap.add_argument("--device", type=int, default=0, help="HIP device (default: 0)")
    ap.add_argument("--diagnostics", type=int, default=0, metavar="K",
                    help="every K-th frame, append a flock-analysis JSON line to <output stem>.flock.jsonl (default: off)")
    ap.add_argument("--link", type=float, default=None, metavar="B",
                    help="linking length of the flock finder (default and at most: the perception radius)")
    ap.add_argument("--min-members", type=int, default=20, metavar="M",
                    help="smallest flock listed in the analysis lines (default: 20)")
    ap.add_argument("--neighbours", choices=NEIGHBOUR_MODES, default="metric",
                    help="interaction rule: every boid within the perception radius (metric, the default) or the "
                         "--topological-k nearest of them (topological)")
    ap.add_argument("--topological-k", type=int, default=7, metavar="K",
                    help="neighbours per boid with --neighbours topological, 1..16 (default: 7)")
    ap.add_argument("--periodic", action="store_true",
                    help="periodic box instead of walls; --diagnostics then writes the whole-flock row only, without flocks "
                         "or neighbour counts")
    ap.add_argument("--periodic-flocks", action="store_true",
                    help="with --periodic: --diagnostics writes the full lines (flocks, sizes, neighbour counts), links "
                         "followed through the faces, plus per flock whether it spans each axis")
    ap.add_argument("--noise", type=float, default=0.0, metavar="ETA",
                    help="vectorial noise: ETA * max_force times a random unit vector per boid and update (default: 0, off)")
    ap.add_argument("--noise-seed", type=int, default=0, metavar="S", help="seed of the noise (default: 0)")
    ap.add_argument("--correlations", type=int, default=0, metavar="K",
                    help="every K-th frame append the velocity correlation C(r) of the headings, its correlation length "
                         "and susceptibility to <output stem>.correlation.jsonl (default: 0 = off)")
    ap.add_argument("--correlation-edges", type=str, default="auto", metavar="auto|E0,E1,...",
                    help="bin edges of --correlations: increasing distances, or auto = 17 linear edges from 0 to 4 cell "
                         "sizes (default: auto)")
    return ap


def frame_dt(args) -> float:
    return min(args.dt if args.dt is not None else 1.0 / args.fps, MAX_DT)


def camera_at(args, frame_idx):
    """The camera of frame `frame_idx`: fixed, or orbiting by --camera-speed degrees per frame."""
    from boids.render import OrbitCamera
    theta = args.camera_theta + (frame_idx * args.camera_speed if args.camera == "orbit" else 0.0)
    return OrbitCamera(theta=theta, phi=args.camera_angle, radius=args.camera_radius)


def resolve_format(args, say=print) -> str:
    if args.format is not None:
        return args.format
    if have_ffmpeg():
        return "ffmpeg"
    say("[Flock] ffmpeg not found on PATH: writing raw rgb24 frames + a JSON sidecar instead")
    return "raw"


def default_output(fmt) -> Path:
    suffix = {"ffmpeg": ".mp4", "raw": ".rgb", "ppm": "_frames"}[fmt]
    path = Path(f"flock{suffix}")
    k = 1
    while path.exists():
        path = Path(f"flock ({k}){suffix}")
        k += 1
    return path


def make_sink(args, fmt, output, width, height):
    if fmt == "ffmpeg":
        if not have_ffmpeg():
            raise RuntimeError("--format ffmpeg: ffmpeg is not on PATH (use --format raw or ppm)")
        q = QUALITY_PRESETS[args.quality]
        crf = args.crf if args.crf is not None else q["crf"]
        return _FfmpegSink(ffmpeg_command(width, height, args.fps, args.codec, crf, q["encoding_preset"], output))
    if fmt == "raw":
        output.parent.mkdir(parents=True, exist_ok=True)
        return _RawSink(output, width, height, args.fps)
    return _PpmSink(output, 0)


LARGEST_FLOCKS = 16  # rows per analysis line


def diagnostics_path(output: Path) -> Path:
    """<output stem>.flock.jsonl next to the output (a frame directory keeps its whole name)."""
    return output.with_name((output.stem if output.suffix else output.name) + ".flock.jsonl")


def correlation_path(output: Path) -> Path:
    """<output stem>.correlation.jsonl next to the output (a frame directory keeps its whole name)."""
    return output.with_name((output.stem if output.suffix else output.name) + ".correlation.jsonl")


def correlation_edges(text, cell_size=None) -> np.ndarray:
    """The edges of --correlation-edges: "auto" = 17 linear edges from 0 to 4 cell sizes (a convention, not a measured
    optimum; needs cell_size, None returns None), or 2 to 65 comma-separated distances, finite, not negative and strictly
    increasing."""
    if str(text).strip().lower() == "auto":
        return None if cell_size is None else np.linspace(0.0, 4.0 * float(cell_size), 17)
    try:
        edges = np.array([float(x) for x in str(text).split(",")], dtype=np.float64)
    except ValueError:
        raise ValueError(f"--correlation-edges: {text!r} is neither auto nor a comma-separated list of numbers") from None
    if not 2 <= len(edges) <= 65 or not np.all(np.isfinite(edges)) or edges[0] < 0 or not np.all(np.diff(edges) > 0):
        raise ValueError("--correlation-edges: 2 to 65 finite distances, the first not negative, strictly increasing")
    return edges


def analysis_line(flock, frame, steps, link, min_members, neighbours=None, periodic=False, noise=None,
                  periodic_flocks=False) -> str:
    """One line of the analysis file for the flock's current state (four device calls, no state copied out; on a
    periodic flock one call, the whole flock's row, unless periodic_flocks asks for the four through the faces)."""
    from boids.analysis import global_line, jsonl_line
    if periodic and not periodic_flocks:
        return global_line(frame, steps, flock.diagnostics(), neighbours=neighbours, periodic=True, noise=noise)
    if periodic:
        fl = flock.periodic_flocks(link)
        cat = flock.periodic_flock_catalogue(link, min_members=min_members, capacity=LARGEST_FLOCKS)
        nb = flock.periodic_neighbour_stats(link)
    else:
        fl = flock.flocks(link)
        cat = flock.flock_catalogue(link, min_members=min_members, capacity=LARGEST_FLOCKS)
        nb = flock.neighbour_stats(link)
    count = np.asarray(nb["count"])
    return jsonl_line(frame, steps, flock.diagnostics(), fl["n_flocks"], fl["links"],
                      float(count.mean()) if count.size else 0.0, cat["rows"], flock_labels=cat["label"],
                      link=link, min_members=min_members, qualifying=cat["count"], neighbours=neighbours, noise=noise,
                      flock_spans=cat["spans"] if periodic else None, periodic=periodic)


def run(args, make_flock=None, make_renderer=None, say=print) -> dict:
    """Steps the flock and writes args.frames frames.  make_flock(count, seed, device) and
    make_renderer(width, height, device) default to boids.Flock and boids.render.HIPFlockRenderer."""
    if args.frames <= 0 or args.substeps <= 0 or args.boids <= 0 or args.warmup < 0:
        raise ValueError("--frames, --substeps and --boids must be positive, --warmup not negative")
    every = int(getattr(args, "diagnostics", 0) or 0)
    min_members = int(getattr(args, "min_members", 20))
    if every < 0 or min_members < 1:
        raise ValueError("--diagnostics must not be negative and --min-members at least 1")
    topo_k = int(getattr(args, "topological_k", 7))
    topological = getattr(args, "neighbours", "metric") == "topological"
    if topological and not 1 <= topo_k <= 16:
        raise ValueError("--topological-k must be in 1..16")
    neighbours = {"mode": "topological", "k": topo_k} if topological else None
    periodic = bool(getattr(args, "periodic", False))
    periodic_flocks = bool(getattr(args, "periodic_flocks", False))
    if periodic_flocks and not periodic:
        raise ValueError("--periodic-flocks needs --periodic (a walled run writes the full lines anyway)")
    eta = float(getattr(args, "noise", 0.0) or 0.0)
    if not (0.0 <= eta < float("inf")):
        raise ValueError("--noise must be finite and not negative")
    noise = {"eta": eta, "seed": int(getattr(args, "noise_seed", 0))} if eta > 0 else None
    corr_every = int(getattr(args, "correlations", 0) or 0)
    if corr_every < 0:
        raise ValueError("--correlations must not be negative")
    corr_text = getattr(args, "correlation_edges", "auto") or "auto"
    corr_edges = correlation_edges(corr_text) if corr_every else None  # a bad list is refused before anything is made
    if make_flock is None:
        from boids import Flock
        make_flock = lambda n, seed, device, **kw: Flock(n, seed=seed, device=device, **kw)  # noqa: E731
    if make_renderer is None:
        from boids.render import HIPFlockRenderer
        make_renderer = lambda w, h, device: HIPFlockRenderer(w, h, device=device)  # noqa: E731
    width, height = RESOLUTION_PRESETS[args.resolution]
    fmt = resolve_format(args, say)
    output = Path(args.output) if args.output else default_output(fmt)
    dt = frame_dt(args)
    say(f"[Flock] {args.boids:,} boids, {args.frames} frames, {width}x{height} @ {args.fps} fps, dt {dt:.4f} x "
        f"{args.substeps}, camera {args.camera}, {fmt} -> {output}")
    flock = make_flock(args.boids, args.seed, args.device, periodic=True) if periodic else \
        make_flock(args.boids, args.seed, args.device)
    renderer = make_renderer(width, height, args.device)
    sink = make_sink(args, fmt, output, width, height)
    diag_path = diagnostics_path(output) if every else None
    diag_file = None
    diag_lines = 0
    corr_path = correlation_path(output) if corr_every else None
    corr_file = None
    corr_lines = 0
    t_corr = 0.0
    ok = False
    t_step = t_render = t_write = t_analysis = 0.0
    t0 = time.perf_counter()
    try:
        if topological:
            flock.set_neighbour_mode("topological", topo_k)
        if noise:
            flock.set_noise(noise["eta"], seed=noise["seed"])
        if args.warmup:
            flock.update(dt, args.warmup)
        img = np.empty((height, width, 3), dtype=np.uint8)
        if every:
            diag_path.parent.mkdir(parents=True, exist_ok=True)
            diag_file = open(diag_path, "w")
        if corr_every:
            if corr_edges is None:
                corr_edges = correlation_edges(corr_text, flock.box["cell_size"])
            corr_path.parent.mkdir(parents=True, exist_ok=True)
            corr_file = open(corr_path, "w")
        for i in range(args.frames):
            ts = time.perf_counter()
            flock.update(dt, args.substeps)
            flock.sync()
            tr = time.perf_counter()
            renderer.render_flock(flock, camera_at(args, i), out=img)
            tw = time.perf_counter()
            sink.write(img)
            t_step += tr - ts
            t_render += tw - tr
            t_write += time.perf_counter() - tw
            if every and i % every == 0:
                ta = time.perf_counter()
                steps = args.warmup + (i + 1) * args.substeps
                diag_file.write(analysis_line(flock, i, steps, getattr(args, "link", None), min_members,
                                              neighbours, periodic, noise, periodic_flocks) + "\n")
                diag_lines += 1
                t_analysis += time.perf_counter() - ta
            if corr_every and i % corr_every == 0:
                from boids.analysis import correlation_line
                ta = time.perf_counter()
                corr_file.write(correlation_line(i, args.warmup + (i + 1) * args.substeps,
                                                 flock.velocity_correlation(corr_edges)) + "\n")
                corr_lines += 1
                t_corr += time.perf_counter() - ta
        ok = True
    finally:
        if diag_file is not None:
            diag_file.close()
        if corr_file is not None:
            corr_file.close()
        ok = sink.close(ok) and ok
        renderer.close()
        flock.close()
    wall = time.perf_counter() - t0
    timings = {"ok": ok, "frames": args.frames, "wall_s": wall, "step_s": t_step, "render_s": t_render,
               "write_s": t_write, "fps": args.frames / wall if wall > 0 else 0.0, "output": str(output), "format": fmt}
    if every:
        timings.update({"diagnostics": str(diag_path), "diagnostics_lines": diag_lines, "analysis_s": t_analysis})
    if corr_every:
        timings.update({"correlations": str(corr_path), "correlation_lines": corr_lines, "correlation_s": t_corr})
    if ok and fmt == "raw":  # the sink's sidecar, plus what produced the frames
        meta = json.loads(sink.meta_path.read_text())
        meta["flock"] = {"boids": args.boids, "seed": args.seed, "dt": dt, "substeps": args.substeps,
                         "warmup": args.warmup, "params": {k: float(v) for k, v in config.BOIDS.items()}}
        meta["camera"] = {"mode": args.camera, "speed": args.camera_speed, "radius": args.camera_radius,
                          "angle": args.camera_angle, "theta": args.camera_theta}
        if topological:
            meta["flock"]["neighbours"] = neighbours
        if periodic:
            meta["flock"]["periodic"] = True
        if periodic_flocks:
            meta["flock"]["periodic_flocks"] = True
        if noise:
            meta["flock"]["noise"] = noise
        if every:
            meta["diagnostics"] = {"file": diag_path.name, "every": every, "link": getattr(args, "link", None),
                                   "min_members": min_members, "lines": diag_lines}
        if corr_every:
            meta["correlations"] = {"file": corr_path.name, "every": corr_every, "edges": [float(e) for e in corr_edges],
                                    "lines": corr_lines}
        sink.meta_path.write_text(json.dumps(meta, indent=2))
    say(f"[Flock] {'done' if ok else 'FAILED'}: {output} ({args.frames} frames in {format_time(wall)}, "
        f"{timings['fps']:.1f} fps; step {t_step:.2f}s, render {t_render:.2f}s, write {t_write:.2f}s)")
    if every:
        say(f"[Flock] flock analysis: {diag_lines} lines in {diag_path} ({t_analysis:.2f}s)")
    if corr_every:
        say(f"[Flock] velocity correlation: {corr_lines} lines in {corr_path} ({t_corr:.2f}s)")
    return timings


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    return 0 if run(args)["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
