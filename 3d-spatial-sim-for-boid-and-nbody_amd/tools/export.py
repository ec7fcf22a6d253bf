"""Video export of a recorded session, rendered headless on the GPU (reference tools/export.py, "Video Export").

The reference draws each frame with pygame + fixed-function OpenGL and pipes glReadPixels output to ffmpeg.  Here the
frame is drawn by the device point renderer (nbody.render.HIPPointRenderer; image semantics in include/nbmi.h): no
GL context, window or display is needed, so a session can be exported on the machine that recorded it.

    python -m tools.export <session>                               # ffmpeg if on PATH, else raw rgb24 + JSON
    python -m tools.export <session> --resolution 4k --camera orbit --format ppm
    python -m tools.export --list

Output formats (--format):
    ffmpeg  rgb24 piped to ffmpeg with the reference's codec arguments (h264 / h265 / vp9)
    raw     one .rgb stream of H x W x 3 frames plus a JSON sidecar (ready for ffmpeg -f rawvideo -pix_fmt rgb24)
    ppm     one binary P6 file per frame in a directory

Frames come from tools.record.load_frame with the previous decoded frame passed along (delta .zstd frames decode in
one step); frame k+1 is decoded on a host thread while frame k renders.  The camera modes are the reference's
(fixed / orbit / spiral / zoom / zoomout / zoomin / cinematic / flyby / topdown), driven by the index relative to the
first exported frame.  The reference's interactive menu is not reproduced.
"""
import argparse
import json
import math
import shutil
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Tuple

import numpy as np

from tools.record import PROJECT_ROOT, get_completed_frames, load_frame, load_metadata


@dataclass
class ExportConfig:
    fps: int = 30
    resolution: Tuple[int, int] = (1920, 1080)
    quality_preset: str = "balanced"
    crf: int = 23                      # 0 lossless .. 51; 18 high, 23 balanced, 28 low
    encoding_preset: str = "medium"
    camera_mode: str = "orbit"
    camera_rotation_speed: float = 0.3  # degrees per frame
    camera_initial_theta: float = 45.0
    camera_initial_phi: float = 25.0
    camera_radius: float = 800.0
    point_size: float = 1.5
    background_color: Tuple[float, float, float] = (0.0, 0.0, 0.02)
    fog_density: float = 0.0003
    start_frame: Optional[int] = None
    end_frame: Optional[int] = None
    output_path: Optional[str] = None
    codec: str = "h264"                # h264, h265, vp9
    output_format: Optional[str] = None  # ffmpeg, raw, ppm; None: ffmpeg if it is on PATH, else raw


QUALITY_PRESETS = {
    "fast": {"crf": 28, "encoding_preset": "fast", "description": "Quick export, larger file size"},
    "balanced": {"crf": 23, "encoding_preset": "medium", "description": "Good balance of speed and quality"},
    "high": {"crf": 18, "encoding_preset": "slow", "description": "High quality, smaller file, slower export"},
    "lossless": {"crf": 15, "encoding_preset": "slow", "description": "Visually lossless, best compression"},
}

RESOLUTION_PRESETS = {
    "720p": (1280, 720),
    "1080p": (1920, 1080),
    "1440p": (2560, 1440),
    "4k": (3840, 2160),
    "ultrawide": (2560, 1080),
}

CAMERA_MODES = ("fixed", "orbit", "spiral", "zoom", "zoomout", "zoomin", "cinematic", "flyby", "topdown")
CODECS = ("h264", "h265", "vp9")
FORMATS = ("ffmpeg", "raw", "ppm")


def have_ffmpeg() -> bool:
    return shutil.which("ffmpeg") is not None


def format_time(seconds: float) -> str:
    if seconds < 90:
        return f"{seconds:.0f}s"
    if seconds < 3600:
        return f"{seconds / 60:.1f}m"
    return f"{seconds / 3600:.1f}h"


def format_size(n: int) -> str:
    if n >= 1 << 30:
        return f"{n / (1 << 30):.2f}GB"
    if n >= 1 << 20:
        return f"{n / (1 << 20):.1f}MB"
    if n >= 1 << 10:
        return f"{n / (1 << 10):.1f}KB"
    return f"{n}B"


class ExportCamera:
    """Spherical camera around the origin: theta (horizontal), phi (elevation), radius; animated per mode."""

    def __init__(self, config: ExportConfig):
        self.config = config
        self.radius = config.camera_radius
        self.theta = config.camera_initial_theta
        self.phi = config.camera_initial_phi
        self.target = np.array([0.0, 0.0, 0.0])
        self.frame = 0

    def update(self, frame_idx: int, total_frames: int):
        c = self.config
        self.frame = frame_idx
        t = frame_idx / max(1, total_frames - 1)
        speed = c.camera_rotation_speed
        mode = c.camera_mode
        if mode == "orbit":
            self.theta = c.camera_initial_theta + frame_idx * speed
        elif mode == "spiral":
            self.theta = c.camera_initial_theta + frame_idx * speed
            self.phi = c.camera_initial_phi + 10 * np.sin(t * 2 * np.pi)
        elif mode == "zoom":
            self.theta = c.camera_initial_theta + frame_idx * speed * 0.5
            self.radius = c.camera_radius * (1.0 + 0.3 * np.sin(t * 2 * np.pi))
        elif mode == "zoomout":  # 0.5x -> 2.5x of the radius
            self.theta = c.camera_initial_theta + frame_idx * speed * 0.2
            self.radius = c.camera_radius * (0.5 + 2.0 * t)
        elif mode == "zoomin":  # 2.0x -> 0x of the radius: the reference's formula (2 - 2t)
            self.theta = c.camera_initial_theta + frame_idx * speed * 0.4
            self.radius = c.camera_radius * (2.0 - 2.0 * t)
        elif mode == "cinematic":
            self.theta = c.camera_initial_theta + frame_idx * speed * 0.3
            self.phi = c.camera_initial_phi + 15 * np.sin(t * np.pi)
            self.radius = c.camera_radius * (1.0 - 0.2 * t)
        elif mode == "flyby":
            self.theta = c.camera_initial_theta + 90 * t
            self.phi = c.camera_initial_phi - 20 + 40 * t
            self.radius = c.camera_radius * (1.5 - 0.8 * np.sin(t * np.pi))
        elif mode == "topdown":
            self.theta = c.camera_initial_theta + frame_idx * speed * 0.5
            self.phi = 80
            self.radius = c.camera_radius * 1.2
        # "fixed": nothing moves

    def get_position(self) -> np.ndarray:
        th, ph = math.radians(self.theta), math.radians(self.phi)
        return np.array([self.radius * math.cos(ph) * math.cos(th), self.radius * math.sin(ph),
                         self.radius * math.cos(ph) * math.sin(th)])

    def get_up_vector(self) -> tuple:
        return (0, 1, 0) if math.cos(math.radians(self.phi)) >= 0 else (0, -1, 0)


def ffmpeg_command(width, height, fps, codec, crf, preset, output_path) -> list:
    """rgb24 frames on stdin -> encoded file (the reference exporter's arguments)."""
    cmd = ["ffmpeg", "-y", "-f", "rawvideo", "-vcodec", "rawvideo", "-pix_fmt", "rgb24", "-s", f"{width}x{height}",
           "-r", str(fps), "-i", "-"]
    if codec == "h264":
        cmd += ["-c:v", "libx264", "-preset", preset, "-crf", str(crf), "-pix_fmt", "yuv420p", "-profile:v", "high",
                "-level", "4.2", "-x264-params", "ref=4:bframes=3:b-adapt=2:direct=auto:me=umh:subme=8:trellis=2"]
    elif codec == "h265":
        cmd += ["-c:v", "libx265", "-preset", preset, "-crf", str(crf), "-pix_fmt", "yuv420p", "-tag:v", "hvc1"]
    elif codec == "vp9":
        cmd += ["-c:v", "libvpx-vp9", "-crf", str(crf), "-b:v", "0", "-pix_fmt", "yuv420p"]
    cmd += ["-movflags", "+faststart", str(output_path)]
    return cmd


def ppm_bytes(img: np.ndarray) -> bytes:
    h, w, _ = img.shape
    return f"P6\n{w} {h}\n255\n".encode("ascii") + np.ascontiguousarray(img).tobytes()


def read_ppm(path) -> np.ndarray:
    """Inverse of ppm_bytes (the header this module writes)."""
    data = Path(path).read_bytes()
    parts = data.split(b"\n", 3)
    if parts[0] != b"P6" or parts[2] != b"255":
        raise ValueError(f"{path}: not a binary 8-bit PPM")
    w, h = (int(x) for x in parts[1].split())
    return np.frombuffer(parts[3], dtype=np.uint8, count=w * h * 3).reshape(h, w, 3)


class _FfmpegSink:
    def __init__(self, cmd):
        self.cmd = cmd
        self.proc = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)

    def write(self, img):
        self.proc.stdin.write(img.data if img.flags.c_contiguous else img.tobytes())

    def close(self, ok=True):
        if self.proc.stdin:
            self.proc.stdin.close()
        if not ok:
            self.proc.terminate()
        return self.proc.wait() == 0


class _RawSink:
    def __init__(self, path, width, height, fps):
        self.path = Path(path)
        self.meta_path = self.path.with_name(self.path.name + ".json")
        self.width, self.height, self.fps = width, height, fps
        self.frames = 0
        self.f = open(self.path, "wb")

    def write(self, img):
        self.f.write(img.data if img.flags.c_contiguous else img.tobytes())
        self.frames += 1

    def close(self, ok=True):
        self.f.close()
        meta = {"width": self.width, "height": self.height, "fps": self.fps, "frames": self.frames,
                "pix_fmt": "rgb24",
                "ffmpeg": f"ffmpeg -f rawvideo -pix_fmt rgb24 -s {self.width}x{self.height} -r {self.fps} "
                          f"-i {self.path.name} -c:v libx264 -pix_fmt yuv420p out.mp4"}
        self.meta_path.write_text(json.dumps(meta, indent=2))
        return ok


class _PpmSink:
    def __init__(self, directory, first_index):
        self.dir = Path(directory)
        self.dir.mkdir(parents=True, exist_ok=True)
        self.index = first_index
        self.frames = 0

    def write(self, img):
        (self.dir / f"frame_{self.index:05d}.ppm").write_bytes(ppm_bytes(img))
        self.index += 1
        self.frames += 1

    def close(self, ok=True):
        return ok


def session_dir(session, root=None) -> Path:
    """A session name under <root>/recordings, or a path to a session directory."""
    p = Path(session)
    if (p / "metadata.json").exists():
        return p
    return Path(root or PROJECT_ROOT) / "recordings" / str(session)


class VideoExporter:
    """Renders frames [start, end) of a recorded session on the GPU and writes them out (ffmpeg / raw / ppm)."""

    def __init__(self, session_name, config: ExportConfig, root=None, device=None, quiet=False):
        self.session_name = Path(session_name).name
        self.config = config
        self.device = device
        self.quiet = quiet
        self.rec_dir = session_dir(session_name, root)
        if not (self.rec_dir / "metadata.json").exists():
            raise FileNotFoundError(f"Recording not found: {session_name}")
        self.metadata = load_metadata(self.rec_dir)
        self.total_frames = get_completed_frames(self.rec_dir)
        if self.total_frames == 0:
            raise ValueError(f"No frames found in recording: {session_name}")
        self.start_frame = config.start_frame or 0
        self.end_frame = min(config.end_frame or self.total_frames, self.total_frames)
        self.export_frames = self.end_frame - self.start_frame
        if self.export_frames <= 0:
            raise ValueError(f"empty frame range [{self.start_frame}, {self.end_frame})")
        self.width, self.height = config.resolution
        self.format = config.output_format
        if self.format is None:
            self.format = "ffmpeg" if have_ffmpeg() else "raw"
            if self.format == "raw":
                self._say("[Export] ffmpeg not found on PATH: writing raw rgb24 frames + a JSON sidecar instead")
        if self.format not in FORMATS:
            raise ValueError(f"unknown output format {self.format!r} (have {FORMATS})")
        self.output_path = Path(config.output_path) if config.output_path else self._default_output()
        self.camera = ExportCamera(config)
        self.timings = {}

    def _say(self, *a, **kw):
        if not self.quiet:
            print(*a, **kw)

    def _default_output(self) -> Path:
        base = self.rec_dir.parent
        suffix = {"ffmpeg": ".mp4", "raw": ".rgb", "ppm": "_frames"}[self.format]
        path = base / f"{self.session_name}{suffix}"
        k = 1
        while path.exists():
            path = base / f"{self.session_name} ({k}){suffix}"
            k += 1
        return path

    def ffmpeg_command(self) -> list:
        c = self.config
        return ffmpeg_command(self.width, self.height, c.fps, c.codec, c.crf, c.encoding_preset, self.output_path)

    def _sink(self):
        if self.format == "ffmpeg":
            if not have_ffmpeg():
                raise RuntimeError("--format ffmpeg: ffmpeg is not on PATH (use --format raw or ppm)")
            return _FfmpegSink(self.ffmpeg_command())
        if self.format == "raw":
            self.output_path.parent.mkdir(parents=True, exist_ok=True)
            return _RawSink(self.output_path, self.width, self.height, self.config.fps)
        return _PpmSink(self.output_path, self.start_frame)

    def frame_params(self):
        """Render parameters of the camera's current state."""
        from nbody.render import render_params
        c = self.config
        return render_params(self.camera.get_position(), target=self.camera.target, up=self.camera.get_up_vector(),
                             point_size=c.point_size, fog_density=c.fog_density, bg=c.background_color)

    def export(self) -> bool:
        from nbody.render import HIPPointRenderer
        c = self.config
        self._say(f"[Export] {self.session_name}: {self.metadata.get('num_bodies', '?')} bodies, frames "
                  f"{self.start_frame}-{self.end_frame}, {self.width}x{self.height} @ {c.fps} fps, camera "
                  f"{c.camera_mode}, {self.format} -> {self.output_path}")
        renderer = HIPPointRenderer(self.width, self.height, device=self.device)
        sink = self._sink()
        ok = False
        t_decode = t_render = t_write = 0.0
        t0 = time.perf_counter()

        def decode(idx, prev):
            ts = time.perf_counter()
            p, col = load_frame(self.rec_dir, idx, prev[0], prev[1]) if prev else load_frame(self.rec_dir, idx)
            return p, col, time.perf_counter() - ts

        try:
            with ThreadPoolExecutor(max_workers=1) as pool:
                prev = None
                if self.start_frame > 0:
                    p, col, dt = decode(self.start_frame - 1, None)
                    prev, t_decode = (p, col), t_decode + dt
                pending = pool.submit(decode, self.start_frame, prev)
                img = np.empty((self.height, self.width, 3), dtype=np.uint8)
                for i, idx in enumerate(range(self.start_frame, self.end_frame)):
                    p, col, dt = pending.result()
                    t_decode += dt
                    if idx + 1 < self.end_frame:  # decode the next frame while this one renders
                        pending = pool.submit(decode, idx + 1, (p, col))
                    self.camera.update(i, self.export_frames)
                    ts = time.perf_counter()
                    renderer.render(p, col, params=self.frame_params(), out=img)
                    tw = time.perf_counter()
                    sink.write(img)
                    t_render += tw - ts
                    t_write += time.perf_counter() - tw
                    if not self.quiet and ((i + 1) % 10 == 0 or i == 0 or i + 1 == self.export_frames):
                        el = time.perf_counter() - t0
                        fps = (i + 1) / el if el > 0 else 0.0
                        eta = (self.export_frames - i - 1) / fps if fps > 0 else 0.0
                        print(f"\r[Export] {i + 1}/{self.export_frames} | {fps:.1f} fps | ETA {format_time(eta)}   ",
                              end="", flush=True)
            ok = True
        finally:
            ok = sink.close(ok) and ok
            renderer.close()
        wall = time.perf_counter() - t0
        self.timings = {"frames": self.export_frames, "wall_s": wall, "decode_s": t_decode, "render_s": t_render,
                        "write_s": t_write, "fps": self.export_frames / wall if wall > 0 else 0.0}
        if ok:
            size = sum(f.stat().st_size for f in self.output_path.iterdir()) if self.output_path.is_dir() else (
                self.output_path.stat().st_size if self.output_path.exists() else 0)
            self._say(f"\n[Export] done: {self.output_path} ({format_size(size)}, {self.export_frames} frames in "
                      f"{format_time(wall)}, {self.timings['fps']:.1f} fps)")
        else:
            self._say("\n[Export] ffmpeg failed to encode the video")
        return ok


def list_recordings(root=None):
    recordings = Path(root or PROJECT_ROOT) / "recordings"
    sessions = [d for d in recordings.iterdir() if (d / "metadata.json").exists()] if recordings.is_dir() else []
    if not sessions:
        print("[Export] No recordings found")
        return []
    for d in sorted(sessions, key=lambda x: x.stat().st_mtime, reverse=True):
        meta = load_metadata(d)
        mark = "x" if (recordings / f"{d.name}.mp4").exists() else " "
        print(f"  [{mark}] {d.name:30s} | {meta.get('num_bodies', 0):>10,} bodies | {get_completed_frames(d):>4} frames")
    return sessions


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m tools.export",
                                 description="Export an N-body recording to video, rendered on the GPU")
    ap.add_argument("session", nargs="?", help="recording session name (or path to a session directory)")
    ap.add_argument("--list", action="store_true", help="list available recordings")
    ap.add_argument("--fps", type=int, help="output FPS (default: 30)")
    ap.add_argument("--resolution", choices=list(RESOLUTION_PRESETS), help="output resolution (default: 1080p)")
    ap.add_argument("--quality", choices=list(QUALITY_PRESETS), help="quality preset (default: balanced)")
    ap.add_argument("--crf", type=int, help="override the CRF value (0-51, lower = better)")
    ap.add_argument("--codec", choices=CODECS, help="video codec (default: h264)")
    ap.add_argument("--camera", choices=CAMERA_MODES, help="camera animation mode (default: orbit)")
    ap.add_argument("--camera-speed", type=float, default=0.3, help="rotation speed in degrees/frame (default: 0.3)")
    ap.add_argument("--camera-radius", type=float, default=800.0, help="distance from the centre (default: 800)")
    ap.add_argument("--camera-angle", type=float, default=25.0, help="vertical angle, 0 = horizon (default: 25)")
    ap.add_argument("--camera-theta", type=float, default=45.0, help="horizontal starting angle (default: 45)")
    ap.add_argument("--point-size", type=float, default=1.5, help="point size in pixels, (0, 4] (default: 1.5)")
    ap.add_argument("--start", type=int, help="first frame")
    ap.add_argument("--end", type=int, help="end frame (exclusive)")
    ap.add_argument("-o", "--output", type=str, help="output file (ffmpeg, raw) or directory (ppm)")
    ap.add_argument("--format", choices=FORMATS, default=None,
                    help="ffmpeg (default when ffmpeg is on PATH), raw rgb24 + JSON sidecar, or one PPM per frame")
    ap.add_argument("--device", type=int, default=None, help="HIP device (default: LOCAL_RANK or 0)")
    return ap


def config_from_args(args) -> ExportConfig:
    c = ExportConfig()
    c.fps = args.fps or 30
    c.resolution = RESOLUTION_PRESETS.get(args.resolution, (1920, 1080))
    c.quality_preset = args.quality or "balanced"
    q = QUALITY_PRESETS[c.quality_preset]
    c.crf = args.crf if args.crf is not None else q["crf"]
    c.encoding_preset = q["encoding_preset"]
    c.codec = args.codec or "h264"
    c.camera_mode = args.camera or "orbit"
    c.camera_rotation_speed = args.camera_speed
    c.camera_radius = args.camera_radius
    c.camera_initial_phi = args.camera_angle
    c.camera_initial_theta = args.camera_theta
    c.point_size = args.point_size
    c.start_frame = args.start
    c.end_frame = args.end
    c.output_path = args.output
    c.output_format = args.format
    return c


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if args.list or not args.session:
        list_recordings()
        if not args.list:
            print("\nUsage: python -m tools.export <session_name> [options]   (--help for the options)")
        return 0
    if not (session_dir(args.session) / "metadata.json").exists():
        print(f"[Export] Recording not found: {args.session}")
        list_recordings()
        return 1
    exporter = VideoExporter(args.session, config_from_args(args), device=args.device)
    return 0 if exporter.export() else 1


if __name__ == "__main__":
    sys.exit(main())
