"""Host side of the massless tracers (include/nbmi.h nbmi_set_tracers), no device: the header and the
library's exports, the NumPy replay (tests/tracer_ref.py) on a Kepler orbit, nbody/field.py's seeds and energies over a
point-mass stand-in, and the recorder's --tracers with the stand-in handle of test_record_streams_host.py."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import tracer_ref as tr
from test_record_streams_host import Handle, World, _config, _files

CALLS = {"nbmi_set_tracers": 4, "nbmi_tracer_count": 1, "nbmi_get_tracers_f64": 3, "nbmi_get_tracer_positions_f32": 2}


def test_header_declares_and_library_exports_the_four_calls():
    import nbmi_native
    text = open(os.path.join(ROOT, "include", "nbmi.h")).read()
    assert re.search(r"^int nbmi_set_tracers\(nbmi_sim \*sim, int64_t m, const double \*positions_xyz", text, re.M)
    assert re.search(r"^int64_t nbmi_tracer_count\(nbmi_sim \*sim\);", text, re.M)
    assert re.search(r"^int nbmi_get_tracers_f64\(nbmi_sim \*sim, double \*positions_xyz", text, re.M)
    assert re.search(r"^int nbmi_get_tracer_positions_f32\(nbmi_sim \*sim, float \*positions_xyz", text, re.M)
    assert "67 108 864" in text  # the largest m accepted is stated, and is at least 2^24
    lib = ctypes.CDLL(nbmi_native.LIB_PATH)
    for name, nargs in CALLS.items():
        assert len(nbmi_native.PROTOTYPES[name][1]) == nargs, name
        assert hasattr(lib, name), name
    assert nbmi_native.PROTOTYPES["nbmi_tracer_count"][0] is ctypes.c_int64


# ---- the replay on a Kepler orbit ----
GM, R0 = 2.0, 1.5
PERIOD = 2.0 * np.pi * np.sqrt(R0 ** 3 / GM)
ORDER = {"kick_drift": 1, "leapfrog": 2}  # of the radius; the phase of both is second order


def _orbit(integrator, steps):
    """(largest |r - R0| / R0 over one nominal period of a circular orbit, |angle swept - 2 pi| / 2 pi)"""
    dt = PERIOD / steps
    rep = tr.TracerReplay([[R0, 0.0, 0.0]], [[0.0, np.sqrt(GM / R0), 0.0]], integrator)
    force = tr.point_mass_field([0.0, 0.0, 0.0], GM)
    worst, swept, prev = 0.0, 0.0, 0.0
    for _ in range(steps):
        rep.step(dt, force)
        worst = max(worst, abs(np.sqrt((rep.p ** 2).sum()) - R0) / R0)
        angle = np.arctan2(rep.p[0, 1], rep.p[0, 0])
        swept += (angle - prev + np.pi) % (2.0 * np.pi) - np.pi
        prev = angle
    assert rep.p[0, 2] == 0.0 and rep.v[0, 2] == 0.0
    return worst, abs(swept - 2.0 * np.pi) / (2.0 * np.pi)


@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
def test_replay_keeps_radius_and_period_to_the_integrators_order(integrator):
    """No fixed tolerance: the errors at dt, dt / 2 and dt / 4 must shrink by the integrator's order, and the bound on
    the finest run is the middle run's error scaled by that order."""
    p = ORDER[integrator]
    coarse, middle, fine = (_orbit(integrator, n) for n in (200, 400, 800))
    for k, order in ((0, p), (1, 2)):  # radius, phase
        seen = [np.log2(a[k] / b[k]) for a, b in ((coarse, middle), (middle, fine))]
        print(integrator, ("radius", "phase")[k], [c[k] for c in (coarse, middle, fine)], "orders", seen)
        assert all(abs(s - order) < 0.15 for s in seen), (integrator, k, seen)
        assert fine[k] <= middle[k] * 2.0 ** -(order - 0.15)


def test_replay_is_reversible_only_for_leapfrog_and_retires():
    force = tr.point_mass_field([0.0, 0.0, 0.0], GM, 0.05)
    rng = np.random.default_rng(3)
    p0, v0 = rng.normal(size=(20, 3)) * 2.0, rng.normal(size=(20, 3)) * 0.3
    back = {}
    for integrator in ORDER:
        rep = tr.TracerReplay(p0, v0, integrator)
        for _ in range(50):
            rep.step(0.01, force)
        rep.v = -rep.v
        for _ in range(50):
            rep.step(0.01, force)
        back[integrator] = np.abs(rep.p - p0).max()
    assert back["leapfrog"] < 1e-12 < back["kick_drift"]
    # beyond 1e18 a row stays as it is; the others go on
    p = np.array([[9e17, 0.0, 0.0], [1.0, 0.0, 0.0]])
    rep = tr.TracerReplay(p, [[1e18, 0.0, 0.0], [0.0, 1.0, 0.0]])
    rep.step(0.5, force)
    frozen, other = (rep.p[0].copy(), rep.v[0].copy()), rep.p[1].copy()
    assert frozen[0][0] > 1e18
    rep.step(0.5, force)
    assert np.array_equal(rep.p[0], frozen[0]) and np.array_equal(rep.v[0], frozen[1])
    assert not np.array_equal(rep.p[1], other)


# ---- nbody/field.py over a point mass ----
class PointMass:
    def __init__(self, center, gm):
        self.c, self.gm, self.tracers = np.asarray(center, np.float64), gm, None

    def field_at(self, points, potential=True, terms=False):
        d = self.c[None, :] - np.asarray(points, np.float64)
        r = np.sqrt((d * d).sum(axis=1))
        acc = d * (self.gm / r ** 3)[:, None]
        return (acc, -self.gm / r) if potential else acc

    def set_tracers(self, p, v=None):
        self.tracers = (np.array(p, np.float64), np.zeros_like(p) if v is None else np.array(v, np.float64))

    def get_tracers(self):
        return self.tracers


@pytest.mark.parametrize("normal", [(0, 0, 1), (0, 0, -1), (1, 2, -0.5)])
def test_circular_tracers_and_energies_about_a_point_mass(normal):
    from nbody.field import circular_tracers, ring_points, tracer_energies
    c, radii = np.array([3.0, -1.0, 2.0]), np.array([0.5, 2.0, 40.0])
    sim = PointMass(c, GM)
    p, v = circular_tracers(sim, radii, c, per_ring=12, normal=normal)
    assert p.shape == v.shape == (36, 3) and np.array_equal(p, ring_points(c, radii, 12, normal))
    r = p - c
    dist = np.sqrt((r * r).sum(axis=1))
    n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    assert np.allclose(dist, np.repeat(radii, 12), rtol=1e-14)
    assert np.allclose(np.sqrt((v * v).sum(axis=1)), np.sqrt(GM / dist), rtol=1e-13)
    assert np.abs((r * v).sum(axis=1)).max() < 1e-13 * np.sqrt(GM * radii.max())  # along the ring ...
    assert np.allclose(np.cross(r, v), (dist * np.sqrt(GM / dist))[:, None] * n, rtol=0, atol=1e-12)  # ... counter-clockwise
    sim.set_tracers(p, v)
    assert np.allclose(tracer_energies(sim), -GM / (2.0 * dist), rtol=1e-12)  # a circular orbit's 0.5 v^2 + phi
    sim.set_tracers(np.zeros((0, 3)))
    assert tracer_energies(sim).shape == (0,)
    # and they stay on their rings under the replay (leapfrog, 400 steps per period of the innermost ring)
    rep = tr.TracerReplay(p, v, "leapfrog")
    dt = 2.0 * np.pi * np.sqrt(radii[0] ** 3 / GM) / 400
    for _ in range(100):
        rep.step(dt, lambda pts: sim.field_at(pts, potential=False))
    now = np.sqrt(((rep.p - c) ** 2).sum(axis=1))
    assert np.abs(now / dist - 1.0).max() < 4.0 * _orbit("leapfrog", 400)[0]


# ---- the recorder ----
class TracerHandle(Handle):
    """test_record_streams_host's stand-in with tracers that move on straight lines with the steps"""

    def set_tracers(self, p, v=None):
        self.tp = np.array(p, np.float64)
        self.tv = np.zeros_like(self.tp) if v is None else np.array(v, np.float64)
        self.set_calls = getattr(self, "set_calls", 0) + 1

    @property
    def tracer_count(self):
        return len(self.tp)

    def step_many(self, dt, substeps):
        super().step_many(dt, substeps)
        for _ in range(substeps):
            self.tp = self.tp + self.tv * dt

    def get_tracers(self):
        return self.tp.copy(), self.tv.copy()

    def tracer_positions_f32(self):
        return self.tp.astype(np.float32)


class TracerWorld(World):
    def create(self, positions, velocities, masses, G, softening, damping, **kw):
        self.handles.append(TracerHandle(self, positions, velocities, masses))
        return self.handles[-1]


FRAMES, EVERY, M = 57, 4, 9


def _tracer_config(tmp_path, name, pipeline=False, frames=FRAMES, every=EVERY, cols=6):
    seeds = np.random.default_rng(1).normal(size=(M, cols))
    path = tmp_path / f"seeds{cols}.npy"
    np.save(path, seeds)
    cfg = _config(name, False, pipeline, frames)
    cfg["tracers"] = {"file": str(path), "every": every}
    return cfg, seeds


def _tracer_frames(d):
    return [int(p.stem.split("_")[1]) for p in sorted(d.glob("tracers_*.npy"))]


@pytest.mark.parametrize("pipeline", [False, True], ids=["sequential", "pipelined"])
def test_recorder_files_period_metadata_and_checkpoint(tmp_path, monkeypatch, pipeline):
    from tools import record as rec
    world = TracerWorld(monkeypatch)
    cfg, seeds = _tracer_config(tmp_path, "tr", pipeline)
    d = rec.record(cfg, root=tmp_path, quiet=True)
    assert _tracer_frames(d) == [f for f in range(FRAMES) if (f + 1) % EVERY == 0]
    assert [p.name for p in d.glob("tracers_*")][0].startswith("tracers_0000") and not list(d.glob(".*.part"))
    dt = cfg["dt_per_frame"]
    for f in (3, 55):
        a = np.load(d / f"tracers_{f:06d}.npy")
        assert a.dtype == np.float32 and a.shape == (M, 3)
        assert np.allclose(a, seeds[:, :3] + seeds[:, 3:] * dt * (f + 1), rtol=1e-6, atol=1e-6)
    assert rec.load_metadata(d)["tracers"] == cfg["tracers"]
    with np.load(d / "state_0049.npz") as st:
        assert sorted(st.files) == ["masses", "positions", "tracer_positions", "tracer_velocities", "velocities"]
        assert st["tracer_positions"].dtype == np.float64 and np.array_equal(st["tracer_velocities"], seeds[:, 3:])
    assert world.handles[0].set_calls == 1 and world.handles[0].closed == 1
    assert rec.get_completed_frames(d) == FRAMES  # the tracer files are no frames


def test_seeds_without_velocities_and_no_files(tmp_path, monkeypatch):
    from tools import record as rec
    world = TracerWorld(monkeypatch)
    cfg, seeds = _tracer_config(tmp_path, "rest", frames=6, every=0, cols=3)
    d = rec.record(cfg, root=tmp_path, quiet=True)
    assert _tracer_frames(d) == [] and world.handles[0].tracer_count == M
    assert np.array_equal(world.handles[0].tp, seeds) and not world.handles[0].tv.any()
    np.save(tmp_path / "bad.npy", np.zeros((4, 5)))
    cfg["tracers"]["file"] = str(tmp_path / "bad.npy")
    with pytest.raises(ValueError, match=r"\(m, 3\) or \(m, 6\)"):
        rec.record(dict(cfg, session_name="bad"), root=tmp_path, quiet=True)
    assert world.handles[-1].closed == 1


@pytest.mark.parametrize("pipeline", [False, True], ids=["sequential", "pipelined"])
@pytest.mark.parametrize("at", [2, 50, 52])
def test_interrupt_then_resume_restores_the_tracers(tmp_path, monkeypatch, pipeline, at):
    from tools import record as rec
    TracerWorld(monkeypatch)
    cfg, _ = _tracer_config(tmp_path, "whole", pipeline)
    want = _files(rec.record(cfg, root=tmp_path, quiet=True), "tracers_*")
    world = TracerWorld(monkeypatch)
    world.interrupt_at = at
    cfg, _ = _tracer_config(tmp_path, "cut", pipeline)
    with pytest.raises(KeyboardInterrupt):
        rec.record(cfg, root=tmp_path, quiet=True)
    d = rec.get_recording_dir("cut", tmp_path)
    with np.load(d / f"state_{at - 1:04d}.npz") as st:
        assert "tracer_positions" in st.files
    os.remove(cfg["tracers"]["file"])  # the resume takes the tracers from the checkpoint, not from the seeds
    rec.record(rec.load_metadata(d), resume=True, root=tmp_path, quiet=True)
    assert _files(d, "tracers_*") == want and len(world.handles) == 2


def test_extend_and_status(tmp_path, monkeypatch, capsys):
    from tools import record as rec
    TracerWorld(monkeypatch)
    cfg, _ = _tracer_config(tmp_path, "short")
    d = rec.record(cfg, root=tmp_path, quiet=True)
    assert rec.extend_recording("short", 7, root=tmp_path) == d
    longer = rec.record(_tracer_config(tmp_path, "longer", frames=FRAMES + 7)[0], root=tmp_path, quiet=True)
    assert _files(d, "tracers_*") == _files(longer, "tracers_*") and _tracer_frames(d)[-1] == 63
    capsys.readouterr()
    assert rec.show_status("short", root=tmp_path)
    out = capsys.readouterr().out
    assert f"Tracers: {M} from" in out and f"a file every {EVERY} frames" in out and "last file: tracers_000063.npy" in out


def test_command_line_stores_both_settings(tmp_path):
    from tools import record as rec
    np.save(tmp_path / "s.npy", np.zeros((3, 6)))
    parse = rec.build_parser().parse_args
    cfg = rec.build_config(parse(["--preset", "quick_galaxy", "--tracers", str(tmp_path / "s.npy"), "--tracers-every", "5"]))
    assert cfg["tracers"] == {"file": str((tmp_path / "s.npy").resolve()), "every": 5}
    assert rec.tracers_config(cfg) == (cfg["tracers"]["file"], 5)
    assert rec.build_config(parse(["--preset", "quick_galaxy", "--tracers", str(tmp_path / "s.npy")]))["tracers"]["every"] == 0
    assert "tracers" not in rec.build_config(parse(["--preset", "quick_galaxy"]))
    with pytest.raises(ValueError, match="needs --tracers"):
        rec.build_config(parse(["--preset", "quick_galaxy", "--tracers-every", "5"]))
    with pytest.raises(ValueError, match="must be positive"):
        rec.build_config(parse(["--preset", "quick_galaxy", "--tracers", "x.npy", "--tracers-every", "0"]))


def test_a_session_without_tracers_has_no_new_keys_or_files(tmp_path, monkeypatch, capsys):
    """the stand-in here has no tracer method at all: a session without the key never asks for one"""
    from tools import record as rec
    world = World(monkeypatch)
    d = rec.record(_config("plain", False), root=tmp_path, quiet=True)
    assert not hasattr(world.handles[0], "set_tracers")
    assert "tracers" not in json.loads((d / "metadata.json").read_text())
    assert not list(d.glob("tracers_*"))
    with np.load(d / "state_0049.npz") as st:
        assert sorted(st.files) == ["masses", "positions", "velocities"]
    capsys.readouterr()
    assert rec.show_status("plain", root=tmp_path) and "Tracers" not in capsys.readouterr().out
