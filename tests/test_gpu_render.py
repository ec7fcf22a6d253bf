"""The device point renderer (csrc/render.hip, nbmi_render_*) and the video exporter on the MI355X, against the NumPy
restatement of the image in tests/render_ref.py (include/nbmi.h, "headless point renderer").

Without fog the image is compared byte for byte; with fog the device exp may differ from the C library's by an ulp,
which can move a channel by one: at most 1e-5 of the channels may differ by 1 (the count is reported).  The four
stats (points drawn, fragments, passing fragments, pixels touched) must always be equal.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from render_ref import compare, make_params, render_ref

pytestmark = pytest.mark.gpu

CAMERAS = [  # (eye, up)
    ((800.0 * np.cos(np.radians(25)) * np.cos(np.radians(45)), 800.0 * np.sin(np.radians(25)),
      800.0 * np.cos(np.radians(25)) * np.sin(np.radians(45))), (0, 1, 0)),
    ((0.0, 900.0, 1e-3), (0, 0, 1)),
    ((-150.0, 40.0, 260.0), (0, 1, 0)),
]


def _check(r, pos, col, W, H, params, label):
    img = r.render(pos, col, params=params)
    ref, st = render_ref(pos, col, W, H, params)
    got = r.stats()
    assert [got["drawn"], got["fragments"], got["passing"], got["pixels"]] == st, (label, got, st)
    if params[13] == 0.0:
        assert np.array_equal(img, ref), (label, int((img != ref).sum()))
    else:
        ok, n1, nbig = compare(img, ref)
        print(f"{label}: {n1} channels differ by 1 (of {img.size}), {nbig} by more")
        assert ok, (label, n1, nbig)
    return img, st


@pytest.fixture(scope="module")
def bodies(gpu):
    """Seeded galaxy / collision frames with the colours a handle computes (compute_colors(15), as record() does)."""
    from nbody.gpu_backend import HIPBarnesHutSimulation
    from tools.presets import generate_distribution
    out = {}
    for name, n in (("galaxy", 200_000), ("collision", 200_000), ("galaxy", 1_000_000)):
        np.random.seed(11)
        p, v, m = generate_distribution(name, n, 500.0, 1.0)
        sim = HIPBarnesHutSimulation(p, v, m, 1.0, 0.5, 1.0, 0.5)
        sim.compute_colors(15.0)
        out[(name, n)] = (sim.get_positions(), sim.get_colors())
        sim.close()
    return out


def test_tiny_golden_frames(gpu):
    from nbody.render import HIPPointRenderer
    frames = [np.load(os.path.join(GOLDEN, "frames", f"frame_000{k}.npz")) for k in (0, 1)]
    for W, H in ((333, 197), (1920, 1080)):
        with HIPPointRenderer(W, H) as r:
            for f in frames:
                pos, col = f["positions"], f["colors"]
                scale = float(np.abs(pos).max()) or 1.0
                for eye, up in CAMERAS:
                    for ps in (0.5, 1.5, 4.0):
                        for fog in (0.0, 0.0003):
                            e = np.asarray(eye) * (scale / 300.0)
                            p = make_params(e, up=up, point_size=ps, fog_density=fog)
                            _check(r, pos, col, W, H, p, f"tiny {W}x{H} ps {ps} fog {fog}")


@pytest.mark.parametrize("name,n", [("galaxy", 200_000), ("collision", 200_000)])
def test_200k_frames(bodies, name, n):
    from nbody.render import HIPPointRenderer
    pos, col = bodies[(name, n)]
    with HIPPointRenderer(1920, 1080) as r:
        for k, (eye, up) in enumerate(CAMERAS):
            _check(r, pos, col, 1920, 1080, make_params(eye, up=up, fog_density=0.0), f"{name} 1080p cam {k}")
        _check(r, pos, col, 1920, 1080, make_params(CAMERAS[0][0]), f"{name} 1080p fog")
    with HIPPointRenderer(333, 197) as r:
        for ps in (0.5, 4.0):
            _check(r, pos, col, 333, 197, make_params(CAMERAS[2][0], point_size=ps, fog_density=0.0),
                   f"{name} 333x197 ps {ps}")
        _check(r, pos, col, 333, 197, make_params(CAMERAS[0][0], point_size=4.0), f"{name} 333x197 ps 4 fog")


def test_1m_galaxy_and_repeatability(bodies):
    from nbody.render import HIPPointRenderer
    pos, col = bodies[("galaxy", 1_000_000)]
    with HIPPointRenderer(1920, 1080) as r:
        img, st = _check(r, pos, col, 1920, 1080, make_params(CAMERAS[0][0], fog_density=0.0), "1M 1080p")
        assert st[1] > 1_000_000 and st[2] < st[1]
        again = r.render(pos, col, params=make_params(CAMERAS[0][0], fog_density=0.0))
        assert np.array_equal(img, again)
        _check(r, pos, col, 1920, 1080, make_params(CAMERAS[2][0], point_size=4.0), "1M 1080p ps 4 fog")


def test_one_pixel_stack_spans_many_tiles(gpu):
    """300 k points on the same pixels (one pixel run spans ~150 resolve tiles): shuffled depths with repeats, and a
    strictly approaching sequence in which every fragment passes."""
    from nbody.render import HIPPointRenderer
    rng = np.random.default_rng(5)
    n = 300_000
    z = np.round(rng.uniform(-50.0, 50.0, n), 1)  # ~1 000 distinct depths, shuffled
    pos = np.zeros((n, 3), dtype=np.float32)
    pos[:, 2] = z
    col = rng.random((n, 3)).astype(np.float32)
    W, H = 333, 197
    with HIPPointRenderer(W, H) as r:
        # eye on the axis: every point lands on the same window position
        _check(r, pos, col, W, H, make_params((0, 0, 100), fog_density=0.0), "stack shuffled")
        _check(r, pos, col, W, H, make_params((0, 0, 100), point_size=4.0), "stack shuffled fog ps 4")
        pos2 = np.zeros((n, 3), dtype=np.float32)
        pos2[:, 2] = np.linspace(-60.0, 99.0, n, dtype=np.float32)  # far to near in draw order
        col2 = np.full((n, 3), 1e-4, dtype=np.float32)
        _, st = _check(r, pos2, col2, W, H, make_params((0, 0, 100), fog_density=0.0), "stack approaching")
        assert st[2] > n  # a third of the 1.5 M fragments pass (the rest tie in 24-bit depth)


@pytest.mark.parametrize("n", [262_144, 262_145])
def test_tile_scan_round_edge(gpu, n):
    """1 024 and 1 025 tiles of 256 points (one full round of the tile scan, and one entry carried into the next):
    everything behind the eye except one point in the first tile and one in the last."""
    from nbody.render import HIPPointRenderer
    rng = np.random.default_rng(n)
    pos = rng.uniform(-50.0, 50.0, (n, 3)).astype(np.float32)
    pos[:, 2] += 500.0  # eye at z = 300 looking down -z: all behind it
    pos[3] = (-20.0, 10.0, 0.0)
    pos[n - 1] = (25.0, -15.0, 40.0)
    col = rng.random((n, 3)).astype(np.float32)
    W, H = 333, 197
    with HIPPointRenderer(W, H) as r:
        for ps in (1.5, 4.0):
            _, st = _check(r, pos, col, W, H, make_params((0, 0, 300), point_size=ps, fog_density=0.0), f"{n} points ps {ps}")
            assert st[0] == 2 and st[1] >= 2


def test_everything_clipped_and_empty(gpu):
    from nbody.render import HIPPointRenderer
    rng = np.random.default_rng(9)
    n = 1_000_000
    pos = rng.uniform(-100.0, 100.0, (n, 3)).astype(np.float32)
    pos[:, 2] += 500.0  # all behind the eye at z = 100 looking at -z
    col = rng.random((n, 3)).astype(np.float32)
    bg = np.array([0, 0, 5], dtype=np.uint8)
    with HIPPointRenderer(1920, 1080) as r:
        img = r.render(pos, col, eye=(0, 0, 100))
        assert (img == bg).all() and r.stats() == {"drawn": 0, "fragments": 0, "passing": 0, "pixels": 0}
        img = r.render(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), eye=(0, 0, 100))
        assert (img == bg).all() and r.stats()["drawn"] == 0
        img = r.render(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), eye=(0, 0, 100), bg=(1, 0.5, 0))
        assert (img == np.array([255, 128, 0], dtype=np.uint8)).all()


def test_render_sim_equals_host_arrays(gpu):
    from nbody.gpu_backend import HIPBarnesHutSimulation, HIPDirectSimulation
    from nbody.render import HIPPointRenderer
    from tools.presets import generate_distribution
    np.random.seed(3)
    p, v, m = generate_distribution("collision", 50_000, 300.0, 1.0)
    with HIPPointRenderer(640, 360) as r:
        for cls in (HIPBarnesHutSimulation, HIPDirectSimulation):
            sim = cls(p[:20_000] if cls is HIPDirectSimulation else p, v[:20_000] if cls is HIPDirectSimulation else v,
                      m[:20_000] if cls is HIPDirectSimulation else m, 1.0, 0.5, 1.0, 0.5)
            sim.step_many(0.05, 3)  # Barnes-Hut bodies now sit in key order on the device
            sim.compute_colors(15.0)
            params = make_params((300.0, 200.0, 400.0), point_size=2.0)
            a = r.render_sim(sim, params=params)
            sa = r.stats()
            b = r.render(sim.get_positions(), sim.get_colors(), params=params)
            assert np.array_equal(a, b) and sa == r.stats() and sa["drawn"] > 0
            c = sim.render(r, params=params)
            assert np.array_equal(a, c)
            sim.close()


def test_export_ppm_end_to_end(gpu, tmp_path):
    from tools import export
    from tools import record as rec
    from tools.presets import get_preset_config
    cfg = get_preset_config("quick_galaxy")
    cfg.update(num_bodies=20_000, theta=0.5, total_frames=6, substeps=1)
    sessions = [rec.record(dict(cfg, session_name="e_npz"), root=tmp_path, quiet=True, seed=4)]
    try:
        rec._load_zstd()
        sessions.append(rec.record(dict(cfg, session_name="e_zstd", zstd=True), root=tmp_path, quiet=True, seed=4))
    except RuntimeError:
        print("no libzstd: .zstd session skipped")
    for d in sessions:
        out = tmp_path / f"{d.name}_ppm"
        assert export.main([str(d), "--format", "ppm", "--resolution", "720p", "--camera", "orbit", "--start", "1",
                            "-o", str(out)]) == 0
        files = sorted(os.listdir(out))
        assert files == [f"frame_{k:05d}.ppm" for k in range(1, 6)]
        conf = export.config_from_args(export.build_parser().parse_args([str(d), "--resolution", "720p"]))
        cam = export.ExportCamera(conf)
        for i, k in enumerate(range(1, 6)):
            pos, col = rec.load_frame(d, k)
            cam.update(i, 5)
            params = make_params(cam.get_position(), up=cam.get_up_vector())
            ref, _ = render_ref(pos, col, 1280, 720, params)
            img = export.read_ppm(out / f"frame_{k:05d}.ppm")
            ok, n1, nbig = compare(img, ref)
            assert ok, (d.name, k, n1, nbig)


def test_argument_errors(gpu):
    import nbmi_native
    from nbody.gpu_backend import HIPOwnerSimulation
    from nbody.render import HIPPointRenderer
    lib = nbmi_native.load()
    for w, h in ((0, 10), (10, -1), (20000, 10)):
        assert not lib.nbmi_render_create(w, h, 0)
        assert "size" in nbmi_native.last_error()
    r = HIPPointRenderer(64, 48)
    pos = np.zeros((4, 3), np.float32)
    col = np.ones((4, 3), np.float32)
    img = np.zeros((48, 64, 3), np.uint8)
    good = make_params((0, 0, 100))
    P = nbmi_native.ptr
    for ps in (0.0, -1.0, 4.5, np.nan):
        bad = good.copy()
        bad[12] = ps
        assert lib.nbmi_render_points(r._h, P(pos), P(col), 4, P(bad), P(img)) == -1
    for k, val in ((3, 0.0), (10, 0.0), (11, 0.05), (13, -1.0), (14, 2.0), (9, 180.0)):
        bad = good.copy()
        bad[:3] = (0, 0, 0) if k == 3 else bad[:3]
        bad[k] = val
        assert lib.nbmi_render_points(r._h, P(pos), P(col), 4, P(bad), P(img)) == -1, k
    up_parallel = make_params((0, 0, 100), up=(0, 0, 1))
    assert lib.nbmi_render_points(r._h, P(pos), P(col), 4, P(up_parallel), P(img)) == -1
    assert lib.nbmi_render_points(r._h, None, P(col), 4, P(good), P(img)) == -1
    assert lib.nbmi_render_points(r._h, P(pos), P(col), 4, None, P(img)) == -1
    assert lib.nbmi_render_points(r._h, P(pos), P(col), 4, P(good), None) == -1
    assert lib.nbmi_render_points(r._h, P(pos), P(col), -1, P(good), P(img)) == -1
    assert lib.nbmi_render_points(r._h, P(pos), P(col), 1 << 27, P(good), P(img)) == -1
    assert lib.nbmi_render_points(None, P(pos), P(col), 4, P(good), P(img)) == -1
    assert lib.nbmi_render_stats(r._h, None) == -1
    assert lib.nbmi_render_sim(r._h, None, P(good), P(img)) == -1
    rng = np.random.default_rng(1)
    n = 1000
    own = HIPOwnerSimulation(rng.normal(size=(n, 3)) * 50, np.zeros((n, 3)), np.ones(n), np.arange(n, dtype=np.int32),
                             n, 4096, 1, 0, 1.0, 0.5, 1.0, 0.5)
    assert lib.nbmi_render_sim(r._h, own._h, P(good), P(img)) == -1
    assert "owner" in nbmi_native.last_error()
    own.close()
    with pytest.raises(RuntimeError):
        r.render(pos, col, eye=(0, 0, 100), point_size=8.0)
    # the renderer still works after the refusals
    out = r.render(pos, col, params=good)
    ref, st = render_ref(pos, col, 64, 48, good)
    assert compare(out, ref)[0] and r.stats()["drawn"] == st[0] == 4
    r.close()
    lib.nbmi_render_destroy(None)
