"""Host side of the video exporter and the renderer's image definition (no GPU).

* The NumPy restatement of the image (tests/render_ref.py) against hand-derived pixels: it is the yardstick the GPU
  tests hold the device renderer to, so it is pinned here first.
* tools.export: camera modes against the reference exporter's camera (tests/golden/export_camera.npz, written by
  scripts/gen_export_camera_golden.py), CLI parsing, the raw / ppm writers and the ffmpeg command line (a stand-in
  ffmpeg executable counts the bytes it is sent).
"""
import json
import math
import os
import stat
import sys

import numpy as np
import pytest

from conftest import golden
from render_ref import make_params, render_ref, view_constants

W, H = 64, 48
BG = np.array([0, 0, 5], dtype=np.uint8)  # floor(0.02 * 255 + 0.5)


def _pts(*rows):
    return np.array(rows, dtype=np.float32).reshape(-1, 3)


def _non_bg(img):
    return {(int(r), int(c)): tuple(int(x) for x in img[r, c]) for r, c in zip(*np.nonzero((img != BG).any(axis=2)))}


def _brute_coverage(xw, yw, R, i, j):
    return sum(1 for a in range(4) for b in range(4)
               if ((i + (a + 0.5) / 4.0) - xw) ** 2 + ((j + (b + 0.5) / 4.0) - yw) ** 2 <= R * R)


def test_centre_point_exact_pixels():
    # the origin seen from (0, 0, 100) lands on window (32, 24) exactly: the four pixels around that corner each
    # have 8 of their 16 samples within R = 0.75 (|d| in {1/8, 3/8, 5/8}: all pairs but (5/8, 5/8))
    img, st = render_ref(_pts([0, 0, 0]), _pts([1.0, 0.5, 0.25]), W, H, make_params((0, 0, 100), fog_density=0.0))
    assert st == [1, 4, 4, 4]
    # A = 8 v with v = 4080, 2040, 1020 -> (A + 128) >> 8 = 128, 64, 32 (+ bg 5 on blue); window rows 23, 24 are
    # image rows 24, 23
    want = (128, 64, 37)
    assert _non_bg(img) == {(23, 31): want, (23, 32): want, (24, 31): want, (24, 32): want}
    assert img.dtype == np.uint8 and img.shape == (H, W, 3)


def test_depth_rule_two_points_on_one_pixel():
    p = make_params((0, 0, 100), fog_density=0.0)
    near, far = [0, 0, 0], [0, 0, -10]
    red, green = [1, 0, 0], [0, 1, 0]
    one = (128, 0, 5)
    both = (128, 128, 5)
    img, st = render_ref(_pts(near, far), _pts(red, green), W, H, p)   # near then far: the far one fails
    assert set(_non_bg(img).values()) == {one} and st == [2, 8, 4, 4]
    img, st = render_ref(_pts(far, near), _pts(green, red), W, H, p)   # far then near: both pass, both add
    assert set(_non_bg(img).values()) == {both} and st == [2, 8, 8, 4]
    img, st = render_ref(_pts(near, near), _pts(red, green), W, H, p)  # equal depth: only the first (GL_LESS)
    assert set(_non_bg(img).values()) == {one} and st == [2, 8, 4, 4]


def test_centre_outside_the_frustum_draws_nothing():
    p = make_params((0, 0, 100), fog_density=0.0)
    xs = view_constants(W, H, p)["xs"]
    for eps, drawn in ((1e-4, False), (-1e-4, True)):
        x = np.float32(100.0 / xs * (1.0 + eps))
        xw = (xs * float(x) / 100.0) * (W / 2.0) + W / 2.0
        assert (xw > W) != drawn and _brute_coverage(xw, 24.0, 0.75, W - 1, 24) > 0  # the disk reaches column W-1
        img, st = render_ref(_pts([x, 0, 0]), _pts([1, 1, 1]), W, H, p)
        if drawn:
            assert st[0] == 1 and st[1] > 0 and all(c == W - 1 for _, c in _non_bg(img))
        else:
            assert st == [0, 0, 0, 0] and not _non_bg(img)
    img, st = render_ref(_pts([0, 0, 200]), _pts([1, 1, 1]), W, H, p)  # behind the eye
    assert st == [0, 0, 0, 0] and not _non_bg(img)


def test_viewport_edge_pixels():
    # a centre near the bottom-left corner: the window starts at -1, only pixel (0, 0) is inside
    p = make_params((0, 0, 100), fog_density=0.0)
    v = view_constants(W, H, p)
    x = np.float32((0.2 / (W / 2.0) - 1.0) * 100.0 / v["xs"])
    y = np.float32((0.3 / (H / 2.0) - 1.0) * 100.0 / v["ys"])
    xw = (v["xs"] * float(x) / 100.0) * (W / 2.0) + W / 2.0
    yw = (v["ys"] * float(y) / 100.0) * (H / 2.0) + H / 2.0
    c = _brute_coverage(xw, yw, 0.75, 0, 0)
    img, st = render_ref(_pts([x, y, 0]), _pts([1, 1, 1]), W, H, p)
    a = (c * 4080 + 128) >> 8
    assert st == [1, 1, 1, 1]
    assert _non_bg(img) == {(H - 1, 0): (a, a, min(255, 5 + a))}


def test_fog_off_is_raw_colour_and_fog_on_darkens():
    p0 = make_params((0, 0, 100), fog_density=0.0, bg=(0, 0, 0))
    img, _ = render_ref(_pts([0, 0, 0]), _pts([1, 1, 1]), W, H, p0)
    assert img[23, 32].tolist() == [128, 128, 128]
    # density 0.01 at eye distance 100: fog = exp(-1), v = floor(exp(-1) 4080 + 0.5) = 1501, (8 v + 128) >> 8 = 47
    img, _ = render_ref(_pts([0, 0, 0]), _pts([1, 1, 1]), W, H, make_params((0, 0, 100), fog_density=0.01, bg=(0, 0, 0)))
    assert math.floor(math.exp(-1.0) * 4080 + 0.5) == 1501
    assert img[23, 32].tolist() == [47, 47, 47]


def test_full_coverage_saturates_and_colours_clamp():
    p = make_params((0, 0, 100), fog_density=0.0, point_size=4.0)
    img, _ = render_ref(_pts([0, 0, 0]), _pts([1, 1, 1]), W, H, p)
    assert img[23, 32].tolist() == [255, 255, 255]  # c = 16, v = 4080: (65280 + 128) >> 8 = 255, blue 5 + 255 -> 255
    img2, _ = render_ref(_pts([0, 0, 0]), _pts([2.5, -0.3, np.nan]), W, H, p)
    assert img2[23, 32].tolist() == [255, 0, 5]  # > 1 -> 1, < 0 -> 0, NaN -> 0


def test_empty_input_is_background():
    img, st = render_ref(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 33, 17, make_params((0, 0, 100)))
    assert st == [0, 0, 0, 0] and (img == BG).all()


# ---- tools.export --------------------------------------------------------------------------------------------------
def test_export_camera_matches_reference_camera():
    from tools.export import CAMERA_MODES, ExportCamera, ExportConfig
    g = golden("export_camera")
    assert tuple(str(m) for m in g["modes"]) == CAMERA_MODES
    for r in range(len(g["mode"])):
        speed, radius, phi, theta = g["configs"][g["config"][r]]
        cfg = ExportConfig(camera_mode=CAMERA_MODES[g["mode"][r]], camera_rotation_speed=speed, camera_radius=radius,
                           camera_initial_phi=phi, camera_initial_theta=theta)
        cam = ExportCamera(cfg)
        cam.update(int(g["index"][r]), int(g["total"][r]))
        np.testing.assert_allclose(cam.get_position(), g["eye"][r], rtol=0, atol=1e-9 * max(1.0, radius))
        assert tuple(cam.get_up_vector()) == tuple(g["up"][r])


def test_cli_parsing():
    from tools.export import build_parser, config_from_args
    a = build_parser().parse_args(["sess", "--resolution", "4k", "--quality", "high", "--camera", "flyby", "--fps", "60",
                                   "--camera-speed", "0.7", "--camera-radius", "1200", "--camera-angle", "10",
                                   "--camera-theta", "90", "--point-size", "2.5", "--start", "3", "--end", "9",
                                   "-o", "out_dir", "--format", "ppm", "--codec", "h265"])
    c = config_from_args(a)
    assert a.session == "sess"
    assert c.resolution == (3840, 2160) and c.fps == 60 and c.crf == 18 and c.encoding_preset == "slow"
    assert c.camera_mode == "flyby" and c.camera_rotation_speed == 0.7 and c.camera_radius == 1200.0
    assert c.camera_initial_phi == 10.0 and c.camera_initial_theta == 90.0 and c.point_size == 2.5
    assert (c.start_frame, c.end_frame, c.output_path, c.output_format, c.codec) == (3, 9, "out_dir", "ppm", "h265")
    d = config_from_args(build_parser().parse_args(["sess", "--crf", "30"]))
    assert d.resolution == (1920, 1080) and d.crf == 30 and d.encoding_preset == "medium" and d.camera_mode == "orbit"
    assert d.output_format is None and d.codec == "h264" and d.point_size == 1.5
    with pytest.raises(SystemExit):
        build_parser().parse_args(["sess", "--format", "gif"])


def _session(tmp_path, frames=3, n=5):
    from tools.record import save_frame, save_metadata
    rec = tmp_path / "recordings" / "s1"
    rec.mkdir(parents=True)
    save_metadata(rec, {"session_name": "s1", "num_bodies": n}, 0.0)
    rng = np.random.default_rng(0)
    for k in range(frames):
        save_frame(rec, k, rng.normal(size=(n, 3)).astype(np.float32), rng.random((n, 3)).astype(np.float32))
    return rec


def _fake_ffmpeg(tmp_path):
    bindir = tmp_path / "bin"
    bindir.mkdir()
    exe = bindir / "ffmpeg"
    exe.write_text(f"#!{sys.executable}\nimport sys\nn = len(sys.stdin.buffer.read())\n"
                   "open(sys.argv[-1] + '.count', 'w').write(str(n))\n")
    exe.chmod(exe.stat().st_mode | stat.S_IEXEC)
    return bindir


def test_default_format_follows_ffmpeg_on_path(tmp_path, monkeypatch, capsys):
    from tools.export import ExportConfig, VideoExporter
    _session(tmp_path)
    monkeypatch.setenv("PATH", str(tmp_path / "nothing"))
    e = VideoExporter("s1", ExportConfig(), root=tmp_path)
    assert e.format == "raw" and e.output_path.name == "s1.rgb"
    assert "ffmpeg not found" in capsys.readouterr().out
    monkeypatch.setenv("PATH", str(_fake_ffmpeg(tmp_path)))
    e = VideoExporter("s1", ExportConfig(start_frame=1), root=tmp_path)
    assert e.format == "ffmpeg" and e.output_path.name == "s1.mp4"
    assert (e.start_frame, e.end_frame, e.export_frames) == (1, 3, 2)
    with pytest.raises(FileNotFoundError):
        VideoExporter("missing", ExportConfig(), root=tmp_path)


def test_ffmpeg_command_and_pipe(tmp_path, monkeypatch):
    from tools.export import ExportConfig, VideoExporter, ffmpeg_command
    _session(tmp_path)
    monkeypatch.setenv("PATH", str(_fake_ffmpeg(tmp_path)))
    out = tmp_path / "v.mp4"
    e = VideoExporter("s1", ExportConfig(resolution=(32, 16), fps=24, output_path=str(out), output_format="ffmpeg"),
                      root=tmp_path)
    head = ["ffmpeg", "-y", "-f", "rawvideo", "-vcodec", "rawvideo", "-pix_fmt", "rgb24", "-s", "32x16", "-r", "24",
            "-i", "-"]
    assert e.ffmpeg_command() == head + [
        "-c:v", "libx264", "-preset", "medium", "-crf", "23", "-pix_fmt", "yuv420p", "-profile:v", "high", "-level",
        "4.2", "-x264-params", "ref=4:bframes=3:b-adapt=2:direct=auto:me=umh:subme=8:trellis=2",
        "-movflags", "+faststart", str(out)]
    assert ffmpeg_command(32, 16, 24, "h265", 18, "slow", out) == head + [
        "-c:v", "libx265", "-preset", "slow", "-crf", "18", "-pix_fmt", "yuv420p", "-tag:v", "hvc1",
        "-movflags", "+faststart", str(out)]
    assert ffmpeg_command(32, 16, 24, "vp9", 30, "fast", out) == head + [
        "-c:v", "libvpx-vp9", "-crf", "30", "-b:v", "0", "-pix_fmt", "yuv420p", "-movflags", "+faststart", str(out)]
    sink = e._sink()
    img = np.arange(16 * 32 * 3, dtype=np.uint8).reshape(16, 32, 3)
    for _ in range(3):
        sink.write(img)
    assert sink.close(True)
    assert int((tmp_path / "v.mp4.count").read_text().split()[0]) == 3 * img.size


def test_raw_and_ppm_writers(tmp_path):
    from tools.export import ExportConfig, VideoExporter, read_ppm
    _session(tmp_path)
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, size=(7, 5, 3), dtype=np.uint8) for _ in range(3)]
    raw = tmp_path / "o" / "clip.rgb"
    e = VideoExporter("s1", ExportConfig(resolution=(5, 7), fps=12, output_path=str(raw), output_format="raw"),
                      root=tmp_path)
    sink = e._sink()
    for f in frames:
        sink.write(f)
    sink.close(True)
    data = np.frombuffer(raw.read_bytes(), dtype=np.uint8).reshape(3, 7, 5, 3)
    assert all((data[k] == frames[k]).all() for k in range(3))
    meta = json.loads((tmp_path / "o" / "clip.rgb.json").read_text())
    assert (meta["width"], meta["height"], meta["fps"], meta["frames"], meta["pix_fmt"]) == (5, 7, 12, 3, "rgb24")
    assert "-f rawvideo -pix_fmt rgb24 -s 5x7 -r 12" in meta["ffmpeg"]

    d = tmp_path / "ppm"
    e = VideoExporter("s1", ExportConfig(resolution=(5, 7), start_frame=1, output_path=str(d), output_format="ppm"),
                      root=tmp_path)
    sink = e._sink()
    for f in frames[:2]:
        sink.write(f)
    sink.close(True)
    assert sorted(os.listdir(d)) == ["frame_00001.ppm", "frame_00002.ppm"]
    assert (d / "frame_00001.ppm").read_bytes()[:11] == b"P6\n5 7\n255\n"
    assert (read_ppm(d / "frame_00002.ppm") == frames[1]).all()


def test_list_and_missing_session(tmp_path, monkeypatch, capsys):
    from tools import export
    monkeypatch.setattr(export, "PROJECT_ROOT", tmp_path)
    assert export.main(["--list"]) == 0
    assert "No recordings" in capsys.readouterr().out
    _session(tmp_path)
    assert export.main(["nope"]) == 1
    out = capsys.readouterr().out
    assert "Recording not found" in out and "s1" in out
