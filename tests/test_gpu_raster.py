"""The device triangle rasteriser (csrc/raster.hip) against the NumPy restatement of include/bdmi.h
(tests/raster_ref.py): every comparison is byte for byte on the image and equal on the four stats, fog on and off.
Before comparing, each case asserts on the REFERENCE's stats that it exercises what it claims.
"""
import ctypes as C
import math

import numpy as np
import pytest

import boids_cases
from raster_ref import NO_FOG, Setup, make_params, raster_ref

pytestmark = pytest.mark.gpu

FOGS = (dict(), NO_FOG)


def _renderer(W, H, device=None):
    from boids.render import HIPFlockRenderer
    return HIPFlockRenderer(W, H, device=device)


def _check(r, v, c, p, ref=None):
    """Device frame == restatement: image bytes and the four stats.  Returns the restatement's result."""
    ref = ref or raster_ref(v, c, r.width, r.height, p)
    img = r.render_triangles(v, c, params=p)
    st = r.stats()
    print(f"  {r.width}x{r.height} T={len(v) // 3}: ref stats {ref[1]} max count {int(ref[2].max()) if ref[2].size else 0}; "
          f"device {st}; differing bytes {int((img != ref[0]).sum())}")
    assert [st["drawn"], st["fragments"], st["passing"], st["pixels"]] == [ref[1][0], ref[1][1], ref[1][2], ref[1][2]]
    assert np.array_equal(img, ref[0])
    return ref


def soup(rng, T, spread, lo, hi):
    """T triangles around uniformly random centres, vertex offsets of a log-uniform size in [lo, hi]."""
    centre = rng.uniform(-spread, spread, (T, 1, 3))
    size = np.exp(rng.uniform(math.log(lo), math.log(hi), (T, 1, 1)))
    v = (centre + size * rng.normal(0, 1.0, (T, 3, 3))).astype(np.float32).reshape(-1, 3)
    c = np.repeat(rng.random((T, 1, 3)) * 1.2 - 0.1, 3, axis=1).astype(np.float32).reshape(-1, 3)
    return v, c


CAMERAS = (dict(eye=(0.0, 0.0, 60.0)), dict(eye=(40.0, 25.0, 40.0)),
           dict(eye=(5.0, -30.0, 10.0), target=(0.0, 5.0, 0.0), fovy=70.0))


@pytest.mark.parametrize("size, T, lo, hi", [((333, 197), 5000, 0.3, 3.0), ((333, 197), 50000, 0.05, 1.5),
                                             ((1920, 1080), 20000, 0.05, 1.0)])
def test_triangle_soups(gpu, size, T, lo, hi):
    W, H = size
    rng = np.random.default_rng(T + W)
    v, c = soup(rng, T, 22.0, lo, hi)
    with _renderer(W, H) as r:
        for k, cam in enumerate(CAMERAS):
            for fog in FOGS:
                p = make_params(**cam, **fog)
                ref = raster_ref(v, c, W, H, p)
                assert ref[1][1] >= 20000 and ref[2].max() >= 4, (k, ref[1], ref[2].max())
                _check(r, v, c, p, ref)


def _quad(x, y, z, x0=None, y0=None):
    x0, y0 = (-x if x0 is None else x0), (-y if y0 is None else y0)
    return np.array([[x0, y0, z], [x, y0, z], [x, y, z], [x0, y0, z], [x, y, z], [x0, y, z]], dtype=np.float32)


def _fan(n, radius, z_rim):
    a = np.linspace(0, 2 * math.pi, n + 1)
    rim = np.stack([radius * np.cos(a), radius * np.sin(a), np.full(n + 1, z_rim)], axis=1)
    tri = np.zeros((n, 3, 3))
    tri[:, 1], tri[:, 2] = rim[:-1], rim[1:]
    return tri.astype(np.float32).reshape(-1, 3)


def _colours(rng, T):
    return np.repeat(rng.random((T, 1, 3)), 3, axis=1).astype(np.float32).reshape(-1, 3)


@pytest.mark.parametrize("size", [(1920, 1080), (3840, 2160)])
def test_large_triangles(gpu, size):
    W, H = size
    rng = np.random.default_rng(W)
    with _renderer(W, H) as r:
        # two triangles that fill the screen
        v = _quad(100.0, 100.0, 0.0)
        c = np.tile(np.float32([[0.9, 0.4, 0.1]]), (6, 1))
        for fog in FOGS:
            p = make_params((0, 0, 10.0), **fog)
            ref = raster_ref(v, c, W, H, p)
            assert ref[1][2] == W * H and ref[1][1] == W * H
            _check(r, v, c, p, ref)
        # a fan of 64 triangles around one vertex (a shallow cone towards the eye) in front of a farther quad
        v = np.concatenate([_fan(64, 300.0, -40.0), _quad(400.0, 400.0, -60.0)])
        c = _colours(rng, 66)
        p = make_params((3.0, -2.0, 30.0))
        ref = raster_ref(v, c, W, H, p, buffers=True)
        assert ref[2].min() >= 2 and ref[1][2] == W * H and (ref[4] < 64).all()  # the fan is nearer everywhere
        _check(r, v, c, p, ref)
        # boxes of at least 512 x 512 that hang over the viewport's edges
        T = 24
        centre = rng.uniform(-60, 60, (T, 1, 3)) * (1, 1, 0.2)
        v = (centre + rng.normal(0, 45.0, (T, 3, 3)) * (1, 1, 0.1)).astype(np.float32).reshape(-1, 3)
        c = _colours(rng, T)
        for fog in FOGS:
            p = make_params((0, 0, 50.0), fog_start=30.0, fog_end=70.0) if not fog else make_params((0, 0, 50.0), **fog)
            ref = raster_ref(v, c, W, H, p)
            S = Setup(v, W, H, p)
            big = ((S.X.max(axis=1) - S.X.min(axis=1)) >= 512 * 16) & ((S.Y.max(axis=1) - S.Y.min(axis=1)) >= 512 * 16)
            outside = (S.X.min(axis=1) < 0) | (S.X.max(axis=1) > 16 * W) | (S.Y.min(axis=1) < 0) | (S.Y.max(axis=1) > 16 * H)
            assert (big & outside).sum() >= 8 and ref[1][1] > W * H
            _check(r, v, c, p, ref)


def test_sub_pixel_and_huge_triangles_in_one_frame(gpu):
    W, H = 1920, 1080
    rng = np.random.default_rng(77)
    small, cs = soup(rng, 100_000, 25.0, 0.01, 0.05)
    huge = np.concatenate([_quad(90.0, 60.0, z, x0=x0, y0=-70.0) for z, x0 in
                           zip((28.0, 27.0, 26.5, 26.0, -26.0, -27.0, -28.0, -29.0), (10, 20, 30, 40, -90, -60, -30, 0))])
    v = np.concatenate([small[:150_000], huge, small[150_000:]])
    c = np.concatenate([cs[:150_000], _colours(rng, 16), cs[150_000:]])
    with _renderer(W, H) as r:
        for fog in FOGS:
            p = make_params((0.0, 0.0, 60.0), **fog)
            ref = raster_ref(v, c, W, H, p, buffers=True)
            win = ref[4]
            small_wins = ((win >= 0) & ((win < 50_000) | (win >= 50_016))).sum()
            assert ref[1][0] > 20_000 and ref[1][1] > 2 * W * H and small_wins > 1000  # small ones in front of huge ones
            assert ((win >= 50_000) & (win < 50_016)).sum() > W * H // 4
            _check(r, v, c, p, ref[:3])


def test_depth_ties_lowest_row_wins(gpu):
    W, H = 333, 197
    rng = np.random.default_rng(3)
    # 1 000 triangles on the same pixels, each in its own colour
    one = np.array([[-20, -15, 0], [25, -10, 0], [0, 22, 0]], dtype=np.float32)
    v = np.tile(one, (1000, 1))
    c = _colours(rng, 1000)
    p = make_params((0.0, 0.0, 40.0), **NO_FOG)
    with _renderer(W, H) as r:
        ref = raster_ref(v, c, W, H, p, buffers=True)
        assert ref[2].max() == 1000 and ref[1][1] == 1000 * ref[1][2] and (ref[4][ref[4] >= 0] == 0).all()
        _check(r, v, c, p, ref[:3])
        # coplanar duplicates in shuffled row order
        base, _ = soup(rng, 3000, 20.0, 0.5, 3.0)
        rows = rng.permutation(np.repeat(np.arange(3000), 3))
        v = base.reshape(3000, 3, 3)[rows].reshape(-1, 3)
        c = _colours(rng, 9000)
        for fog in FOGS:
            p = make_params((10.0, 5.0, 50.0), **fog)
            ref = raster_ref(v, c, W, H, p, buffers=True)
            win = ref[4][ref[4] >= 0]
            first = np.full(3000, 9000)
            np.minimum.at(first, rows, np.arange(9000))
            assert ref[1][1] >= 20000 and (first[rows[win]] == win).all()  # the lowest row of each triple wins
            _check(r, v, c, p, ref[:3])


def test_discards_sizes_and_empty_input(gpu):
    good = np.array([[-5, -5, 0], [5, -5, 0], [0, 6, 0]], dtype=np.float32)
    bad = np.array([[[-5, -5, 0], [5, -5, 0], [0, 6, 19.95]], [[-5, -5, 0], [5, -5, 0], [0, 6, 25]],
                    [[-5, -5, 0], [5, -5, 0], [0, 6, -985]], [[-5, -5, 0], [5, np.nan, 0], [0, 6, 0]],
                    [[-5, -5, 0], [5, -5, 0], [np.inf, 6, 0]], [[-5, -5, 0], [0, 0, 0], [5, 5, 0]],
                    [[1, 1, 0], [1, 1, 0], [1, 1, 0]], [[-5, -5, 0], [5, -5, 0], [4.0e6, 6, 19.0]]], dtype=np.float32)
    white = np.ones((3 * 9, 3), dtype=np.float32)
    for W, H in ((40, 40), (1, 1), (7, 5), (333, 197), (1, 64), (129, 3)):
        with _renderer(W, H) as r:
            for fog in FOGS:
                p = make_params((0, 0, 20.0), **fog)
                ref = _check(r, bad.reshape(-1, 3), white[:24], p)
                assert ref[1] == [0, 0, 0]
                ref = _check(r, np.concatenate([bad.reshape(-1, 3), good]), white, p)
                assert ref[1][0] == 1 and ref[1][1] >= 1
                ref = _check(r, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), p)
                assert ref[1] == [0, 0, 0] and (ref[0] == np.floor(p[14:17] * 255 + 0.5)).all()
            assert r.timers()["sort_ms"] == 0.0 and r.timers()["project_ms"] > 0.0


def test_argument_errors(gpu):
    import nbmi_native as nat
    lib = nat.load()
    v = np.array([[-5, -5, 0], [5, -5, 0], [0, 6, 0]], dtype=np.float32)
    out = np.zeros((8, 8, 3), dtype=np.uint8)
    with _renderer(8, 8) as r:
        def call(p, n=1, vv=v, cc=v, o=out, h=None):
            return lib.bdmi_render_triangles(r._h if h is None else h, nat.ptr(vv), nat.ptr(cc), n,
                                             None if p is None else nat.ptr(p), nat.ptr(o))
        assert call(make_params((0, 0, 20.0))) == 0
        for bad in (dict(near=0.0), dict(near=-1.0), dict(near=5.0, far=5.0), dict(near=5.0, far=2.0),
                    dict(fog_start=10.0, fog_end=10.0), dict(fog_start=10.0, fog_end=5.0), dict(fovy=0.0), dict(fovy=180.0),
                    dict(bg=(0.0, 1.5, 0.0)), dict(far=float("nan")), dict(target=(0, 0, 20.0)), dict(up=(0, 0, 1.0))):
            assert call(make_params((0, 0, 20.0), **bad)) == -1, bad
            assert nat.last_error()
        assert call(None) == -1 and call(make_params((0, 0, 20.0)), n=-1) == -1
        assert call(make_params((0, 0, 20.0)), vv=None) == -1 and call(make_params((0, 0, 20.0)), o=None) == -1
        assert lib.bdmi_render_triangles(None, nat.ptr(v), nat.ptr(v), 1, nat.ptr(make_params((0, 0, 20.0))), nat.ptr(out)) == -1
        assert lib.bdmi_render_flock(r._h, None, None, 1.0, 1.0, 1000.0, 1.2, 0.42, nat.ptr(make_params((0, 0, 20.0))),
                                     nat.ptr(out), None) == -1
        assert call(make_params((0, 0, 20.0))) == 0  # the renderer is still good


# ---- the flock path -----------------------------------------------------------------------------------------------

def _create(nat, n, seed, bounds):
    from boids.flock import generate_initial_state
    np.random.seed(seed)
    pos, vel, col = generate_initial_state(n, bounds, 25.0)
    prm = boids_cases.params(bounds=bounds)
    h = nat.load().bdmi_create(n, nat.ptr(pos), nat.ptr(vel), nat.ptr(col), nat.ptr(prm), 0)
    assert h, nat.last_error()
    return h


def _frustum(cam, W, H, fovy=90.0, margin=1.15):
    tv = math.tan(math.radians(fovy) / 2 * margin)
    cam12 = np.ascontiguousarray(np.concatenate([cam.get_position(), *cam.get_camera_axes()]))
    return cam12, math.tan(math.atan(tv * W / H)), tv


def _abi_visible(nat, h, n, cam12, th, tv):
    v, c = np.zeros((6 * n, 3), np.float32), np.zeros((6 * n, 3), np.float32)
    cnt = C.c_int64(0)
    nat.check(nat.load().bdmi_visible_vertices(h, nat.ptr(cam12), th, tv, 1000.0, 1.2, 0.42, nat.ptr(v), nat.ptr(c), n,
                                               C.addressof(cnt)), "bdmi_visible_vertices")
    return v[:6 * cnt.value], c[:6 * cnt.value], int(cnt.value)


def _abi_render_flock(nat, r, h, cam12, th, tv, p):
    img = np.zeros((r.height, r.width, 3), np.uint8)
    cnt = C.c_int64(-1)
    nat.check(nat.load().bdmi_render_flock(r._h, h, nat.ptr(cam12), th, tv, 1000.0, 1.2, 0.42, nat.ptr(p), nat.ptr(img),
                                           C.addressof(cnt)), "bdmi_render_flock")
    return img, int(cnt.value)


@pytest.mark.parametrize("radius", [20.0, 5.0])
def test_flock_frame_through_the_c_abi(gpu, radius):
    from boids.render import OrbitCamera, flock_render_params
    nat = gpu
    W, H, n = 320, 180, 20000
    h = _create(nat, n, 1, 30.0)
    nat.check(nat.load().bdmi_step(h, 1.0 / 60.0, 50), "bdmi_step")
    cam = OrbitCamera(45.0, 25.0, radius)
    cam12, th, tv = _frustum(cam, W, H)
    with _renderer(W, H) as r:
        for fog in (dict(), dict(fog_start=5.0, fog_end=60.0), NO_FOG):
            p = flock_render_params(**cam.view(), **fog)
            v, c, count = _abi_visible(nat, h, n, cam12, th, tv)
            ref = raster_ref(v, c, W, H, p)
            share = ref[1][2] / (W * H)
            print(f"  radius {radius}: visible {count}, ref stats {ref[1]}, covered {share:.3f}, max count {ref[2].max()}")
            assert ref[1][1] >= 50_000 and share >= 0.5
            img, vis = _abi_render_flock(nat, r, h, cam12, th, tv, p)
            st = r.stats()
            assert vis == count
            assert [st["drawn"], st["fragments"], st["pixels"]] == ref[1] and st["passing"] == st["pixels"]
            assert np.array_equal(img, ref[0])
            assert np.array_equal(r.render_triangles(v, c, params=p), ref[0])
    nat.load().bdmi_destroy(h)


def _reference_camera_frame(r, flock):
    from boids.render import OrbitCamera
    cam = OrbitCamera()
    img = flock.render(r, cam).copy()
    st = r.stats()
    f, right, up = cam.get_camera_axes()
    v, c = flock.visible_vertices(cam.get_position(), f, right, up, 90.0, r.width / r.height)
    assert flock._visible_count * 6 == len(v)
    by_hand = r.render_triangles(v, c, **cam.view())
    assert r.stats() == st and st["drawn"] > 0 and st["fragments"] > 0
    assert np.array_equal(img, by_hand)
    return img, st


def test_reference_box_200k_boids_720p(gpu):
    from boids import Flock
    fl = Flock(200_000, seed=1)
    fl.update(1.0 / 60.0, 20)
    with _renderer(1280, 720) as r:
        img, st = _reference_camera_frame(r, fl)
        print(f"  200k boids 720p: visible {fl._visible_count}, stats {st}")
        assert 0 < fl._visible_count < 200_000 and (img != img[0, 0]).any()
    fl.close()


def test_two_million_boids_1080p_and_determinism(gpu):
    from boids import Flock
    from boids.render import OrbitCamera
    fl = Flock(2_000_000, seed=2)
    fl.update(1.0 / 60.0, 5)
    with _renderer(1920, 1080) as r:
        img, st = _reference_camera_frame(r, fl)
        print(f"  2M boids 1080p: visible {fl._visible_count}, stats {st}, timers {r.timers()}")
        for _ in range(3):
            assert np.array_equal(fl.render(r, OrbitCamera()), img) and r.stats() == st
    fl.close()


def test_rendering_does_not_disturb_the_flock(gpu):
    from boids import Flock
    from boids.render import OrbitCamera
    a, b = Flock(30_000, seed=5), Flock(30_000, seed=5)
    cam = OrbitCamera(radius=300.0)
    with _renderer(320, 180) as r:
        for k in range(30):
            a.update(1.0 / 60.0)
            b.update(1.0 / 60.0)
            cam.rotate(2.0, 0.5)
            img = a.render(r, cam).copy()
            f, right, up = cam.get_camera_axes()
            v, c = a.visible_vertices(cam.get_position(), f, right, up, 90.0, 320 / 180)
            assert np.array_equal(r.render_triangles(v, c, **cam.view()), img)
    for name in ("positions", "velocities", "colors"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    a.close()
    b.close()


def test_slab_handles_and_other_devices_are_refused(gpu):
    from boids.render import OrbitCamera, flock_render_params
    nat = gpu
    lib = nat.load()
    n = 1000
    rng = np.random.default_rng(0)
    pos = rng.uniform(-20, 20, (n, 3))
    vel, col = rng.uniform(-5, 5, (n, 3)), rng.random((n, 3))
    ids = np.arange(n, dtype=np.int32)
    prm = boids_cases.params(bounds=30.0)
    slab = lib.bdmi_create_slab(n, nat.ptr(pos), nat.ptr(vel), nat.ptr(col), nat.ptr(ids), 2 * n, nat.ptr(prm), -35.0, 35.0,
                                0, 0, 0)
    assert slab, nat.last_error()
    cam = OrbitCamera(45.0, 25.0, 20.0)
    cam12, th, tv = _frustum(cam, 64, 48)
    p = flock_render_params(**cam.view())
    img = np.zeros((48, 64, 3), np.uint8)
    with _renderer(64, 48) as r:
        rc = lib.bdmi_render_flock(r._h, slab, nat.ptr(cam12), th, tv, 1000.0, 1.2, 0.42, nat.ptr(p), nat.ptr(img), None)
        assert rc == -1 and "slab" in nat.last_error()
    lib.bdmi_destroy(slab)
    h = _create(nat, n, 1, 30.0)
    if nat.device_count() >= 2:
        with _renderer(64, 48, device=1) as r1:
            rc = lib.bdmi_render_flock(r1._h, h, nat.ptr(cam12), th, tv, 1000.0, 1.2, 0.42, nat.ptr(p), nat.ptr(img), None)
            assert rc == -1 and "device" in nat.last_error()
    else:  # one device: a renderer elsewhere cannot exist
        assert not lib.nbmi_render_create(64, 48, 1)
    with _renderer(64, 48) as r:  # and the plain handle renders
        im, vis = _abi_render_flock(nat, r, h, cam12, th, tv, p)
        assert vis > 0 and r.stats()["fragments"] > 0
    lib.bdmi_destroy(h)


def test_flock_video_end_to_end(gpu, tmp_path):
    from boids import Flock
    from tools import flock_video as fv
    from tools.export import read_ppm
    d = tmp_path / "frames"
    argv = ["--boids", "50000", "--frames", "5", "--format", "ppm", "-o", str(d), "--seed", "3", "--camera-speed", "2.0"]
    assert fv.main(argv) == 0
    frames = sorted(x.name for x in d.iterdir())
    assert frames == [f"frame_{i:05d}.ppm" for i in range(5)]
    args = fv.build_parser().parse_args(argv)
    fl = Flock(50_000, seed=3)
    with _renderer(1280, 720) as r:
        for i in range(4):
            fl.update(fv.frame_dt(args), 1)
        want = fl.render(r, fv.camera_at(args, 3))
        assert r.stats()["fragments"] > 0
    got = read_ppm(d / "frame_00003.ppm")
    assert np.array_equal(got, want)
    assert not np.array_equal(read_ppm(d / "frame_00002.ppm"), got)
    fl.close()
