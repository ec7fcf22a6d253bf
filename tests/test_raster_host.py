"""Host side of the flock renderer (no GPU): the image definition of include/bdmi.h checked against itself through its
NumPy restatement (tests/raster_ref.py: the yardstick the GPU tests hold the device rasteriser to, so it is pinned
here first), boids.render.OrbitCamera against the reference's camera (tests/golden/flock_camera.npz, written by
scripts/gen_flock_camera_golden.py), and tools.flock_video with a stand-in flock and renderer.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest

from conftest import golden
from raster_ref import NO_FOG, make_params, raster_ref

BG8 = np.array([3, 3, 5], dtype=np.uint8)  # floor((0.01, 0.01, 0.02) 255 + 0.5)


def _tris(*rows):
    return np.array(rows, dtype=np.float32).reshape(-1, 3)


def _flat(colour, n=1):
    return np.tile(np.asarray(colour, dtype=np.float32), (3 * n, 1))


def jittered_mesh(g, sx, sy, jitter, seed):
    """A g x g grid of vertices jittered inside the plane z = 0 (by less than would fold a cell over), every cell two
    triangles with a random diagonal and a random winding."""
    rng = np.random.default_rng(seed)
    xs = np.linspace(-sx, sx, g)[:, None] + rng.uniform(-jitter, jitter, (g, g))
    ys = np.linspace(-sy, sy, g)[None, :] + rng.uniform(-jitter, jitter, (g, g))
    zs = np.zeros((g, g))
    P = np.stack([xs, ys, zs], axis=-1)
    tri = []
    for a in range(g - 1):
        for b in range(g - 1):
            q = [P[a, b], P[a + 1, b], P[a + 1, b + 1], P[a, b + 1]]
            if rng.random() < 0.5:
                tri += [q[0], q[1], q[2], q[0], q[2], q[3]]
            else:
                tri += [q[1], q[0], q[3], q[3], q[2], q[1]]
    v = np.array(tri, dtype=np.float32)
    return v, rng.random((len(v), 3)).astype(np.float32)


def holes(covered):
    """Uncovered pixels that no path of uncovered pixels connects to the border."""
    free = ~covered
    reach = np.zeros_like(free)
    reach[0, :], reach[-1, :], reach[:, 0], reach[:, -1] = free[0, :], free[-1, :], free[:, 0], free[:, -1]
    while True:
        grow = reach.copy()
        grow[1:, :] |= reach[:-1, :]
        grow[:-1, :] |= reach[1:, :]
        grow[:, 1:] |= reach[:, :-1]
        grow[:, :-1] |= reach[:, 1:]
        grow &= free
        if (grow == reach).all():
            return int((free & ~reach).sum())
        reach = grow


@pytest.mark.parametrize("g, size, scale, jitter", [(14, (97, 61), (30, 18), 0.9), (40, (320, 180), (30, 18), 0.3),
                                                    (60, (64, 64), (25, 25), 0.25)])
def test_shared_edges_are_watertight(g, size, scale, jitter):
    W, H = size
    v, c = jittered_mesh(g, scale[0], scale[1], jitter, seed=g)
    img, st, cover = raster_ref(v, c, W, H, make_params((12.0, 9.0, 40.0)))
    n = 2 * (g - 1) ** 2  # a few sub-pixel slivers may snap to zero area: they cover nothing and leave no hole
    assert 0.99 * n <= st[0] <= n and st[1] > 1000
    assert cover.max() == 1, "a pixel centre on a shared edge was hit twice"
    assert st[1] == st[2] == int((cover > 0).sum())
    assert holes(cover > 0) == 0
    if g == 60:  # mostly sub-pixel triangles: most of them cover no centre at all
        assert st[1] < st[0]


def _lattice():
    tri = []
    for a in range(-8, 8, 4):
        for b in range(-8, 8, 4):
            q = [(a + .5, b + .5, 0), (a + 4.5, b + .5, 0), (a + 4.5, b + 4.5, 0), (a + .5, b + 4.5, 0)]
            tri += [q[0], q[1], q[2], q[0], q[2], q[3]]
    return np.array(tri, dtype=np.float32)


def test_edges_through_pixel_centres_hit_once():
    # fovy 90, square viewport, plane at z_e = -W/2: x_w = x + W/2, so every vertex sits on a pixel centre and every
    # quad edge and diagonal runs through centres
    v = _lattice()
    img, st, cover = raster_ref(v, _flat((1, 1, 1), 32), 32, 32, make_params((0, 0, 16.0)))
    assert st == [32, 256, 256]
    assert cover.sum() == 256 and cover.max() == 1
    assert (cover[8:24, 8:24] == 1).all()


def test_equal_depth_first_drawn_wins_and_winding_does_not_matter():
    v = _lattice()[:3]
    p = make_params((0, 0, 16.0), **NO_FOG)
    red, green = _flat((1, 0, 0)), _flat((0, 1, 0))
    img, st, cover = raster_ref(np.concatenate([v, v]), np.concatenate([red, green]), 32, 32, p)
    on = cover[::-1] > 0
    assert st[0] == 2 and st[1] == 2 * st[2] and (cover[cover > 0] == 2).all()
    assert (img[on] == (255, 0, 0)).all() and (img[~on] == BG8).all()
    img2, st2, _ = raster_ref(np.concatenate([v[[0, 2, 1]], v]), np.concatenate([red, green]), 32, 32, p)
    assert (img2 == img).all() and st2 == st


def test_nearer_wins_whatever_the_order():
    near = _tris([-5, -5, 2], [5, -5, 2], [0, 6, 2])
    far = _tris([-12, -10, -3], [12, -10, -3], [0, 14, -3])
    p = make_params((0, 0, 20.0), **NO_FOG)
    a, sa, ca = raster_ref(np.concatenate([near, far]), np.concatenate([_flat((1, 0, 0)), _flat((0, 0, 1))]), 48, 48, p)
    b, sb, cb = raster_ref(np.concatenate([far, near]), np.concatenate([_flat((0, 0, 1)), _flat((1, 0, 0))]), 48, 48, p)
    assert (a == b).all() and sa == sb and (ca == cb).all()
    both = ca[::-1] == 2
    assert both.sum() > 50 and (a[both] == (255, 0, 0)).all()
    assert (a[ca[::-1] == 1] == (0, 0, 255)).all()


def test_row_order_matters_only_where_depths_tie():
    rng = np.random.default_rng(5)
    T = 400
    centre = rng.uniform(-15, 15, (T, 1, 3)) * (1, 1, 0.3)
    v = (centre + rng.normal(0, 2.0, (T, 3, 3))).astype(np.float32)
    v[T // 2:] = v[:T // 2]  # every triangle twice: ties everywhere they are in front
    c = np.repeat(rng.random((T, 1, 3)), 3, axis=1).astype(np.float32)
    p = make_params((3.0, 2.0, 30.0))
    img, st, cover, depth, win = raster_ref(v.reshape(-1, 3), c.reshape(-1, 3), 80, 60, p, buffers=True)
    perm = rng.permutation(T)
    img2, st2, cover2, depth2, win2 = raster_ref(v[perm].reshape(-1, 3), c[perm].reshape(-1, 3), 80, 60, p, buffers=True)
    assert st2 == st and (cover2 == cover).all() and (depth2 == depth).all()
    back = np.where(win2 >= 0, perm[np.maximum(win2, 0)], -1)
    same = back == win
    assert (img2[::-1][same] == img[::-1][same]).all()
    assert (~same).sum() > 0
    twin = np.where(win >= 0, (win + T // 2) % T, -1)
    assert (back[~same] == twin[~same]).all(), "the winner changed to something that is not its equal-depth copy"
    # in the original order the lower row of each pair always wins
    assert (win[win >= 0] < T // 2).all()


def test_discards_draw_nothing():
    p = make_params((0, 0, 20.0), **NO_FOG)
    good = _tris([-5, -5, 0], [5, -5, 0], [0, 6, 0])
    cases = {
        "near rule": _tris([-5, -5, 0], [5, -5, 0], [0, 6, 19.95]),       # w_c = 0.05 < near
        "behind": _tris([-5, -5, 0], [5, -5, 0], [0, 6, 25]),
        "far rule": _tris([-5, -5, 0], [5, -5, 0], [0, 6, -985]),         # w_c = 1005 > far: z_c > w_c
        "nan": _tris([-5, -5, 0], [5, np.nan, 0], [0, 6, 0]),
        "inf": _tris([-5, -5, 0], [5, -5, 0], [np.inf, 6, 0]),
        "zero area": _tris([-5, -5, 0], [0, 0, 0], [5, 5, 0]),
        "one point": _tris([1, 1, 0], [1, 1, 0], [1, 1, 0]),
        "guard": _tris([-5, -5, 0], [5, -5, 0], [4.0e6, 6, 19.0]),       # x_w far beyond 2^20
    }
    for name, v in cases.items():
        img, st, cover = raster_ref(v, _flat((1, 1, 1)), 40, 40, p)
        assert st == [0, 0, 0] and (img == BG8).all() and cover.sum() == 0, name
    allv = np.concatenate(list(cases.values()) + [good])
    img, st, cover = raster_ref(allv, _flat((1, 1, 1), len(cases) + 1), 40, 40, p)
    want, stw, _ = raster_ref(good, _flat((1, 1, 1)), 40, 40, p)
    assert st == stw and stw[0] == 1 and stw[1] > 50 and (img == want).all()
    # a drawn triangle wholly outside the viewport counts as drawn and makes no fragment
    img, st, _ = raster_ref(good + np.float32(200.0) * np.array([1, 0, 0], dtype=np.float32), _flat((1, 1, 1)), 40, 40, p)
    assert st == [1, 0, 0] and (img == BG8).all()


def test_fog_clamp_and_background():
    v = _tris([-200, -100, 0], [200, -100, 0], [0, 300, 0])
    col = _flat((0.2, 0.6, 1.0))
    raw = np.floor(np.array([0.2, 0.6, 1.0], dtype=np.float32).astype(np.float64) * 255 + 0.5).astype(np.uint8)
    # eye depth 40 everywhere: below fog_start -> raw colour; beyond fog_end -> exactly the background bytes
    img, st, cover = raster_ref(v, col, 32, 32, make_params((0, 0, 40.0), fog_start=50.0, fog_end=800.0))
    assert st[1] == 32 * 32 and (img == raw).all()
    img, _, _ = raster_ref(v, col, 32, 32, make_params((0, 0, 40.0), fog_start=10.0, fog_end=40.0))
    assert (img == BG8).all()
    img, _, _ = raster_ref(v, col, 32, 32, make_params((0, 0, 40.0), fog_start=10.0, fog_end=30.0))
    assert (img == BG8).all()
    # half way: fog = 0.5 exactly
    img, _, _ = raster_ref(v, _flat((1, 1, 1)), 32, 32, make_params((0, 0, 40.0), fog_start=20.0, fog_end=60.0, bg=(0, 0, 0)))
    assert set(np.unique(img)) <= {127, 128}  # 0.5 * 255 + 0.5 = 128 up to the rounding of w_f
    # colours clamp, NaN -> 0
    img, _, _ = raster_ref(v, _flat((2.5, -0.3, np.nan)), 32, 32, make_params((0, 0, 40.0), **NO_FOG))
    assert (img == (255, 0, 0)).all()
    # the colour of a triangle is its first row's
    c3 = np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.float32)
    img, _, _ = raster_ref(v, c3, 32, 32, make_params((0, 0, 40.0), **NO_FOG))
    assert (img == (0, 255, 0)).all()


def test_empty_input_and_row_zero_is_the_top():
    p = make_params((0, 0, 20.0), **NO_FOG)
    img, st, cover = raster_ref(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 7, 5, p)
    assert img.shape == (5, 7, 3) and img.dtype == np.uint8 and (img == BG8).all() and st == [0, 0, 0]
    top = _tris([-2, 15, 0], [2, 15, 0], [0, 19, 0])  # high up in the world: the first rows of the image
    img, st, cover = raster_ref(top, _flat((1, 1, 1)), 40, 40, p)
    rows = np.nonzero((img != BG8).any(axis=(1, 2)))[0]
    assert st[1] > 0 and rows.max() < 12
    assert np.nonzero(cover.any(axis=1))[0].min() >= 28  # window rows count from the bottom


def test_large_and_batched_paths_of_the_restatement_agree(monkeypatch):
    import raster_ref as rr
    rng = np.random.default_rng(9)
    v = rng.uniform(-20, 20, (60, 3, 3)).astype(np.float32).reshape(-1, 3)
    c = rng.random((180, 3)).astype(np.float32)
    p = make_params((5.0, 3.0, 45.0))
    a = raster_ref(v, c, 120, 90, p, buffers=True)
    monkeypatch.setattr(rr, "_BATCH_ELEMS", 256)  # every triangle alone, in bands of two rows
    b = raster_ref(v, c, 120, 90, p, buffers=True)
    assert a[1] == b[1] and all((x == y).all() for x, y in zip(a[2:], b[2:])) and (a[0] == b[0]).all()
    assert a[2].max() >= 4


# ---- camera ---------------------------------------------------------------------------------------------------

def test_orbit_camera_against_the_reference():
    from boids.render import OrbitCamera
    g = golden("flock_camera")
    assert len(g["states"]) >= 12 and (g["states"][:, 2] < 0).any() and (np.abs(g["states"][:, 1]) == 89).sum() >= 2
    for k, (theta, phi, radius) in enumerate(g["states"]):
        cam = OrbitCamera(theta, phi, radius)
        f, r, u = cam.get_camera_axes()
        for name, got in (("position", cam.get_position()), ("direction", cam.get_direction()), ("forward", f),
                          ("right", r), ("up", u), ("look_at", cam.look_at())):
            assert np.array_equal(np.asarray(got, dtype=np.float64), g[name][k]), (name, theta, phi, radius)
        view = cam.view()
        assert np.array_equal(view["eye"], g["position"][k]) and tuple(view["up"]) == (0.0, 1.0, 0.0)
    cam = OrbitCamera()
    assert (cam.theta, cam.phi, cam.radius) == tuple(g["initial"])
    for (dt, dp), want in zip(g["rotations"], g["rotated"]):
        cam.rotate(dt, dp)
        assert (cam.theta, cam.phi) == tuple(want)


class _FakeLib:
    def __init__(self):
        self.calls = {}

    def _grab(self, name, cam, *rest):
        arr = np.ctypeslib.as_array(ctypes.cast(cam, ctypes.POINTER(ctypes.c_double)), shape=(12,)).copy()
        self.calls[name] = (arr,) + rest

    def bdmi_visible_vertices(self, h, cam, tan_h, tan_v, fog, cl, cr, ov, oc, cap, cnt):
        self._grab("visible", cam, tan_h, tan_v, fog, cl, cr)
        return 0

    def bdmi_render_flock(self, r, h, cam, tan_h, tan_v, fog, cl, cr, params, out, cnt):
        self._grab("render", cam, tan_h, tan_v, fog, cl, cr)
        self.params = np.ctypeslib.as_array(ctypes.cast(params, ctypes.POINTER(ctypes.c_double)), shape=(17,)).copy()
        ctypes.cast(cnt, ctypes.POINTER(ctypes.c_int64))[0] = 77
        return 0


def test_render_flock_hands_over_what_visible_vertices_computes():
    from boids.flock import Flock
    from boids.render import DEFAULTS, HIPFlockRenderer, OrbitCamera
    lib = _FakeLib()
    flock = Flock.__new__(Flock)
    flock.num_boids, flock.fov_margin, flock.fog_end, flock.verts_per_boid = 10, 1.15, 1000.0, 6
    flock.cone_length, flock.cone_radius = np.float32(1.2), np.float32(1.2 * 0.35)
    flock._lib, flock._h = lib, 1
    r = HIPFlockRenderer.__new__(HIPFlockRenderer)
    r.width, r.height, r._lib, r._h = 1280, 720, lib, None
    for cam in (OrbitCamera(), OrbitCamera(200.0, -89.0, 20.0), OrbitCamera(10.0, 5.0, -40.0)):
        f, right, up = cam.get_camera_axes()
        flock.visible_vertices(cam.get_position(), f, right, up, 90.0, 1280 / 720)
        img = flock.render(r, cam)
        assert img.shape == (720, 1280, 3) and flock._visible_count == 77
        a, b = lib.calls["visible"], lib.calls["render"]
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
        assert np.array_equal(lib.params[0:3], cam.get_position()) and np.array_equal(lib.params[3:6], cam.look_at())
        assert lib.params[9:14].tolist() == [90.0, 0.1, 1000.0, 50.0, 800.0] and lib.params[14:17].tolist() == [0.01, 0.01, 0.02]
    # tan_v of fovy 90 with the 1.15 margin, tan_h through the aspect
    tv = math.tan(math.radians(90.0) / 2 * 1.15)
    assert lib.calls["render"][1:3] == (math.tan(math.atan(tv * 1280 / 720)), tv)
    assert DEFAULTS["bg"] == (0.01, 0.01, 0.02) and DEFAULTS["fog_end"] == 800.0
    with pytest.raises(NotImplementedError):
        flock.draw()
    flock._h = None


def test_flock_render_params_layout():
    from boids.render import flock_render_params
    p = flock_render_params((1, 2, 3), target=(4, 5, 6), up=(0, 0, 1), fovy=60, near=0.5, far=99, fog_start=7, fog_end=8,
                            bg=(0.1, 0.2, 0.3))
    assert p.dtype == np.float64 and p.tolist() == [1, 2, 3, 4, 5, 6, 0, 0, 1, 60, 0.5, 99, 7, 8, 0.1, 0.2, 0.3]
    assert np.array_equal(flock_render_params((1, 2, 3)), make_params((1, 2, 3)))


# ---- command line -----------------------------------------------------------------------------------------------

class _FakeFlock:
    made = []

    def __init__(self, n, seed, device):
        self.n, self.seed, self.device, self.updates, self.closed = n, seed, device, [], False
        _FakeFlock.made.append(self)

    def update(self, dt, substeps=1):
        self.updates.append((dt, substeps))

    def sync(self):
        pass

    def close(self):
        self.closed = True


class _FakeRenderer:
    made = []

    def __init__(self, w, h, device):
        self.size, self.cams, self.closed = (w, h), [], False
        _FakeRenderer.made.append(self)

    def render_flock(self, flock, camera, out=None):
        self.cams.append((camera.theta, camera.phi, camera.radius))
        out[:] = len(self.cams)
        return out

    def close(self):
        self.closed = True


def test_cli_parser_defaults_and_numbers():
    from config import boids as cfg
    from tools import flock_video as fv
    a = fv.build_parser().parse_args([])
    assert (a.boids, a.frames, a.fps, a.dt, a.substeps, a.seed, a.warmup) == (cfg.BOIDS["count"], 300, 30, None, 1, None, 0)
    assert (a.resolution, a.camera, a.camera_speed, a.format, a.output, a.device) == ("720p", "orbit", 0.3, None, None, 0)
    assert (a.camera_radius, a.camera_angle, a.camera_theta) == (120.0, 25.0, 45.0)
    assert (a.quality, a.crf, a.codec) == ("balanced", None, "h264")
    assert fv.build_parser().parse_args(["--boids", "500k"]).boids == 500_000
    assert fv.build_parser().parse_args(["--boids", "2m"]).boids == 2_000_000
    assert fv.frame_dt(a) == 1.0 / 30
    assert fv.frame_dt(fv.build_parser().parse_args(["--fps", "10"])) == 0.05          # 0.1 capped
    assert fv.frame_dt(fv.build_parser().parse_args(["--dt", "0.2"])) == 0.05
    assert fv.frame_dt(fv.build_parser().parse_args(["--dt", "0.01"])) == 0.01
    with pytest.raises(SystemExit):
        fv.build_parser().parse_args(["--camera", "spiral"])
    orbit = fv.build_parser().parse_args(["--camera-speed", "2", "--camera-theta", "10"])
    assert [fv.camera_at(orbit, i).theta for i in (0, 1, 5)] == [10.0, 12.0, 20.0]
    fixed = fv.build_parser().parse_args(["--camera", "fixed", "--camera-radius", "33", "--camera-angle", "-12"])
    cam = fv.camera_at(fixed, 9)
    assert (cam.theta, cam.phi, cam.radius) == (45.0, -12.0, 33.0)


def test_cli_run_ppm_and_raw_with_stand_ins(tmp_path, monkeypatch):
    from tools import flock_video as fv
    from tools.export import read_ppm
    _FakeFlock.made.clear()
    _FakeRenderer.made.clear()
    d = tmp_path / "frames"
    args = fv.build_parser().parse_args(["--boids", "1k", "--frames", "4", "--format", "ppm", "-o", str(d), "--seed", "7",
                                         "--warmup", "3", "--substeps", "2", "--camera-speed", "1.5", "--device", "1"])
    t = fv.run(args, make_flock=_FakeFlock, make_renderer=_FakeRenderer, say=lambda *a: None)
    flock, rend = _FakeFlock.made[-1], _FakeRenderer.made[-1]
    assert t["ok"] and t["frames"] == 4 and t["format"] == "ppm"
    assert (flock.n, flock.seed, flock.device) == (1000, 7, 1) and flock.closed and rend.closed
    assert flock.updates == [(1 / 30, 3)] + [(1 / 30, 2)] * 4
    assert rend.size == (1280, 720) and rend.cams == [(45.0 + 1.5 * i, 25.0, 120.0) for i in range(4)]
    assert sorted(os.listdir(d)) == [f"frame_{i:05d}.ppm" for i in range(4)]
    assert (read_ppm(d / "frame_00002.ppm") == 3).all()

    raw = tmp_path / "o" / "clip.rgb"
    args = fv.build_parser().parse_args(["--boids", "2k", "--frames", "3", "--format", "raw", "-o", str(raw), "--fps", "10",
                                         "--resolution", "1080p", "--camera", "fixed", "--seed", "11"])
    t = fv.run(args, make_flock=_FakeFlock, make_renderer=_FakeRenderer, say=lambda *a: None)
    assert t["ok"] and raw.stat().st_size == 3 * 1920 * 1080 * 3
    assert _FakeFlock.made[-1].updates == [(0.05, 1)] * 3  # 1 / 10 capped
    meta = json.loads((tmp_path / "o" / "clip.rgb.json").read_text())
    assert (meta["width"], meta["height"], meta["fps"], meta["frames"], meta["pix_fmt"]) == (1920, 1080, 10, 3, "rgb24")
    assert meta["flock"]["boids"] == 2000 and meta["flock"]["seed"] == 11 and meta["flock"]["dt"] == 0.05
    assert meta["flock"]["params"]["perception_radius"] == 5.0 and meta["camera"]["mode"] == "fixed"
    with pytest.raises(ValueError):
        fv.run(fv.build_parser().parse_args(["--frames", "0"]), make_flock=_FakeFlock, make_renderer=_FakeRenderer)


def test_cli_format_falls_back_without_ffmpeg(tmp_path, monkeypatch):
    from tools import flock_video as fv
    monkeypatch.setenv("PATH", str(tmp_path / "nothing"))
    monkeypatch.chdir(tmp_path)
    said = []
    args = fv.build_parser().parse_args(["--boids", "10", "--frames", "1"])
    assert fv.resolve_format(args, said.append) == "raw" and "ffmpeg not found" in said[0]
    t = fv.run(args, make_flock=_FakeFlock, make_renderer=_FakeRenderer, say=lambda *a: None)
    assert t["format"] == "raw" and t["output"] == "flock.rgb" and (tmp_path / "flock.rgb.json").exists()
    with pytest.raises(RuntimeError):
        fv.run(fv.build_parser().parse_args(["--boids", "10", "--frames", "1", "--format", "ffmpeg"]),
               make_flock=_FakeFlock, make_renderer=_FakeRenderer, say=lambda *a: None)


def test_new_symbols_are_exported_and_bound():
    import nbmi_native
    lib = ctypes.CDLL(nbmi_native.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bdmi.h")).read()
    for name, nargs in (("bdmi_render_triangles", 6), ("bdmi_render_flock", 11)):
        assert hasattr(lib, name) and name in header
        res, args = nbmi_native.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == nargs
