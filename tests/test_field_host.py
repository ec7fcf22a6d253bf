"""Field evaluation at arbitrary points, host side: the NumPy restatement against the direct sum and against the
potential's restatement, the C ABI's declaration, the Python classes' refusals, the derived quantities of nbody/field.py
against a point mass, and the recorder's options, metadata, rotation.jsonl and --status with a stand-in backend (no
device)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import field_ref as fr
import potential_ref as pr
from conftest import ROOT, golden


def _points(pos, rng, extra=200):
    span = np.abs(pos).max()
    mid = 0.5 * (pos[rng.integers(0, len(pos), extra)] + pos[rng.integers(0, len(pos), extra)])
    far = rng.normal(size=(20, 3)) * 3.0 * span
    return np.concatenate([pos[:100], mid, far, np.zeros((1, 3))])


def test_restatement_with_every_cell_opened_is_the_direct_sum(oracle):
    g = golden("tree_galaxy_2048")
    pos, mass, G, eps = g["pos"][:600], g["mass"][:600], float(g["G"]), float(g["eps"])
    pts = _points(pos, np.random.default_rng(1))
    for e in (eps, 0.0):
        t = fr.tree_field(oracle, pts, pos, mass, G, e, 1e-9)
        acc, phi, terms, mag_a, mag_p = fr.direct_field(pts, pos, mass, G, e)
        assert np.array_equal(t["terms"], terms)  # every applied node is a leaf: one term per body off the point
        assert terms[0] == len(pos) - 1 and terms[-1] == len(pos)
        assert np.all(np.abs(t["phi"] - phi) <= 1e-12 * mag_p)
        assert np.all(np.abs(t["acc"] - acc).max(axis=1) <= 1e-12 * mag_a)
        assert np.all(t["bound_acc"] == 0.0) and np.all(t["bound_phi"] == 0.0)  # no cell term, nothing to bound


@pytest.mark.parametrize("name", ["tree_galaxy_2048", "tree_cluster_2048"])
def test_restatement_at_the_bodies_is_the_potential_restatement(oracle, name):
    g = golden(name)
    pos, mass, G, eps = g["pos"], g["mass"], float(g["G"]), float(g["eps"])
    tree = pr.build_tree(oracle, pos, mass)
    for theta in (0.5, 1.3):
        phi, terms, bound = pr.tree_potential(oracle, pos, mass, G, eps, theta, tree=tree)
        t = fr.tree_field(oracle, pos, pos, mass, G, eps, theta, tree=tree)
        assert np.array_equal(t["phi"], phi) and int(t["terms"].sum()) == terms
        assert np.array_equal(t["bound_phi"], bound)
        assert np.isfinite(t["margin"]) and t["margin"] >= 0.0


def test_quadrupole_restatement_is_closer_to_the_direct_sum(oracle):
    g = golden("tree_collision_2048")
    pos, mass, G, eps = g["pos"], g["mass"], float(g["G"]), float(g["eps"])
    pts = _points(pos, np.random.default_rng(2))
    acc, phi, _, _, _ = fr.direct_field(pts, pos, mass, G, eps)
    tree = pr.build_tree(oracle, pos, mass)
    mono = fr.tree_field(oracle, pts, pos, mass, G, eps, 0.5, tree=tree)
    quad = fr.tree_field(oracle, pts, pos, mass, G, eps, 0.5, tree=tree, multipole="quadrupole")
    assert np.array_equal(mono["terms"], quad["terms"])
    for key, ref in (("acc", acc), ("phi", phi)):
        em, eq = np.abs(mono[key] - ref).sum(), np.abs(quad[key] - ref).sum()
        assert eq < 0.5 * em, (key, em, eq)


def test_header_declares_and_library_exports_the_call():
    import nbmi_native
    text = open(os.path.join(ROOT, "include", "nbmi.h")).read()
    assert re.search(r"^int nbmi_field_at\(nbmi_sim \*sim, int64_t m, const double \*points_xyz", text, re.M)
    assert len(nbmi_native.PROTOTYPES["nbmi_field_at"][1]) == 6
    assert hasattr(ctypes.CDLL(nbmi_native.LIB_PATH), "nbmi_field_at")
    for word in ("NBMI_FIELD_SORT", "There is no own-leaf rule", "chunks of at most 1 048 576", "108 bytes per point",
                 "phi equals nbmi_get_potentials_f64", "the message names the first bad row"):
        assert word in text, word


def test_python_classes_refuse_without_a_device():
    from nbody.gpu_backend import HIPBarnesHutSimulation, HIPDirectSimulation, HIPOwnerSimulation
    sim = HIPOwnerSimulation.__new__(HIPOwnerSimulation)  # no handle: the refusal must come before any library call
    sim._h = None
    for call in (lambda: sim.field_at(np.zeros((2, 3))), lambda: sim.field_at(np.zeros((2, 3)), terms=True)):
        with pytest.raises(ValueError, match="owner"):
            call()
    for cls in (HIPBarnesHutSimulation, HIPDirectSimulation):
        sim = cls.__new__(cls)
        sim._h = None
        for bad in (np.zeros(3), np.zeros((4, 2)), np.zeros((2, 3, 1)), [[1.0, 2.0]], 5.0):
            with pytest.raises(ValueError, match=r"\(m, 3\)"):
                sim.field_at(bad)


# ---- nbody/field.py against a point mass ---------------------------------------------------------------------------
class PointMass:
    """field_at of a point mass G M at `at`, softening 0"""

    def __init__(self, gm=2.5, at=(1.0, -2.0, 0.5)):
        self.gm, self.at, self.calls = gm, np.asarray(at, dtype=np.float64), []

    def field_at(self, points, potential=True, terms=False):
        p = np.asarray(points, dtype=np.float64)
        self.calls.append(p.shape)
        d = self.at - p
        r = np.sqrt((d * d).sum(1))
        acc, phi = d * (self.gm / r ** 3)[:, None], -self.gm / r
        return (acc, phi) if potential else acc


def test_ring_points_and_rotation_curve_of_a_point_mass():
    from nbody.field import ring_points, rotation_curve
    sim = PointMass()
    radii = np.array([0.5, 1.0, 3.0, 40.0])
    for normal in ((0, 0, 1), (0, 0, -2), (1, 0, 0), (1, 2, 3)):
        pts = ring_points(sim.at, radii, azimuths=16, normal=normal)
        assert pts.shape == (64, 3) and pts.dtype == np.float64
        d = pts - sim.at
        assert np.allclose(np.sqrt((d * d).sum(1)), np.repeat(radii, 16), rtol=1e-14)
        assert np.abs(d @ (np.asarray(normal, dtype=np.float64) / np.linalg.norm(normal))).max() <= 1e-13 * 40.0
        assert np.abs(d.reshape(4, 16, 3).sum(1)).max() <= 1e-12 * 40.0  # equally spaced: the ring's mean is its centre
        c = rotation_curve(sim, radii, sim.at, azimuths=16, normal=normal)
        assert sorted(c) == ["a_radial", "phi", "radii", "v_circ"] and all(c[k].shape == (4,) for k in c)
        assert np.all(np.abs(c["v_circ"] ** 2 * radii - sim.gm) <= 1e-12 * sim.gm)
        assert np.all(np.abs(c["a_radial"] * radii ** 2 - sim.gm) <= 1e-12 * sim.gm)
        assert np.all(np.abs(c["phi"] * radii + sim.gm) <= 1e-12 * sim.gm)
    z = ring_points((0, 0, 0), [2.0], azimuths=4)
    assert np.allclose(z, [[2, 0, 0], [0, 2, 0], [-2, 0, 0], [0, -2, 0]], atol=1e-15)
    # a repulsive mean field has no circular orbit
    assert rotation_curve(PointMass(gm=-1.0), [1.0, 2.0], (1.0, -2.0, 0.5))["v_circ"].tolist() == [0.0, 0.0]
    for bad in (lambda: ring_points((0, 0, 0), [1.0, -1.0]), lambda: ring_points((0, 0, 0), [np.nan]),
                lambda: ring_points((0, 0, 0), [1.0], azimuths=0), lambda: ring_points((0, 0, 0), [1.0], normal=(0, 0, 0))):
        with pytest.raises(ValueError):
            bad()


def test_potential_slice_and_escape_speed_of_a_point_mass():
    from nbody.field import escape_speed, potential_slice
    sim = PointMass(at=(0.0, 0.0, 0.0))
    img = potential_slice(sim, (0.0, 0.0, 0.3), 2.0, 8)
    assert img.shape == (8, 8) and img.dtype == np.float64 and sim.calls == [(64, 3)]
    assert np.array_equal(img, img.T) and np.array_equal(img, img[::-1]) and np.array_equal(img, img[:, ::-1])
    u = (np.arange(8) + 0.5) * 0.5 - 2.0
    assert abs(img[2, 5] + sim.gm / np.sqrt(u[5] ** 2 + u[2] ** 2 + 0.09)) <= 1e-15 * sim.gm * 10
    # other axes: the image's columns run along axes[0], its rows along axes[1]
    off = PointMass(at=(0.0, 0.0, 1.0))
    xz = potential_slice(off, (0.0, 0.0, 0.0), 2.0, 8, axes=(0, 2))
    assert np.array_equal(xz, xz[:, ::-1]) and not np.array_equal(xz, xz[::-1])
    assert np.argmin(xz) // 8 == 5  # the row whose z is closest to the mass
    for bad in (lambda: potential_slice(sim, (0, 0, 0), 2.0, 0), lambda: potential_slice(sim, (0, 0, 0), 0.0, 4),
                lambda: potential_slice(sim, (0, 0, 0), 1.0, 4, axes=(1, 1)), lambda: potential_slice(sim, (0, 0, 0), 1.0, 4, axes=(0, 3))):
        with pytest.raises(ValueError):
            bad()
    assert escape_speed([-2.0, 0.0, 3.0, -0.5]).tolist() == [2.0, 0.0, 0.0, 1.0]
    assert escape_speed(-8.0) == 4.0


# ---- the recorder ----------------------------------------------------------------------------------------------------
def _args(*extra):
    from tools import record as rec
    return rec.build_parser().parse_args(["--preset", "quick_galaxy", *extra])


def test_recorder_options():
    from tools import record as rec
    assert "rotation_curve" not in rec.build_config(_args())  # the default writes no key
    assert rec.rotation_config({}) is None
    assert rec.LINE_STREAMS[-1] is rec.ROTATION and rec.LINE_STREAMS[-2] is rec.PAIRS
    cfg = rec.build_config(_args("--rotation-curve", "5"))
    r = cfg["spawn_radius"]
    assert cfg["rotation_curve"] == {"every": 5, "radii": [r * k / 16 for k in range(1, 17)]}
    assert rec.rotation_config(cfg) == (5, cfg["rotation_curve"]["radii"])
    assert rec.build_config(_args("--rotation-curve", "5", "--curve-radii", "AUTO")) == cfg
    cfg = rec.build_config(_args("--rotation-curve", "2", "--curve-radii", "1.5,3,6"))
    assert cfg["rotation_curve"] == {"every": 2, "radii": [1.5, 3.0, 6.0]} and rec.rotation_config(cfg) == (2, [1.5, 3.0, 6.0])
    assert rec.build_config(_args("--rotation-curve", "2", "--pairs", "3"))["pairs"]["every"] == 3
    assert len(rec.build_config(_args("--rotation-curve", "1", "--curve-radii", ",".join(str(k) for k in range(1, 257))))
               ["rotation_curve"]["radii"]) == 256
    for bad, word in ((("--curve-radii", "1,2"), "needs --rotation-curve"), (("--curve-radii", "auto"), "needs --rotation-curve"),
                      (("--rotation-curve", "0"), "--rotation-curve"), (("--rotation-curve", "-2"), "--rotation-curve"),
                      (("--rotation-curve", "2", "--curve-radii", "2,1"), "--curve-radii"),
                      (("--rotation-curve", "2", "--curve-radii", "1,1"), "--curve-radii"),
                      (("--rotation-curve", "2", "--curve-radii", "0,1"), "--curve-radii"),
                      (("--rotation-curve", "2", "--curve-radii=-1,1"), "--curve-radii"),
                      (("--rotation-curve", "2", "--curve-radii", "1,inf"), "--curve-radii"),
                      (("--rotation-curve", "2", "--curve-radii", "1,nan"), "--curve-radii"),
                      (("--rotation-curve", "2", "--curve-radii", "1,wide"), "--curve-radii"),
                      (("--rotation-curve", "2", "--curve-radii", ",".join(str(k) for k in range(1, 258))), "--curve-radii")):
        with pytest.raises(ValueError, match=word):
            rec.build_config(_args(*bad))
    with pytest.raises(ValueError, match="--curve-radii"):
        rec.rotation_config({"rotation_curve": {"every": 2, "radii": [3.0, 2.0]}})


class FakeSim(PointMass):
    """the backend object's diagnostics and field_at: a point mass at the centre of mass"""

    class _D:
        center_of_mass = (1.0, -2.0, 0.5)

    def diagnostics(self, potential=True):
        assert potential is False  # the line needs the centre of mass only
        return self._D()


def test_recorder_metadata_round_trip_line_and_status(tmp_path, capsys):
    from tools import record as rec
    cfg = rec.build_config(_args("--rotation-curve", "4", "--curve-radii", "1,2,4"))
    d = rec.get_recording_dir("rot", tmp_path)
    rec.save_metadata(d, cfg, 0.0)
    sim = FakeSim()
    assert rec.ROTATION.apply(sim, cfg, d) == cfg and sim.calls == []  # nothing is taken from the state
    meta = rec.load_metadata(d)
    assert meta["rotation_curve"] == {"every": 4, "radii": [1.0, 2.0, 4.0]} and rec.rotation_config(meta) == (4, [1.0, 2.0, 4.0])
    line = rec.rotation_line(sim, 7, [1.0, 2.0, 4.0])
    assert line.endswith("\n") and sim.calls == [(48, 3)]
    row = json.loads(line)
    assert sorted(row) == ["a_radial", "center", "frame", "phi", "radii", "v_circ"]
    assert row["frame"] == 7 and row["center"] == [1.0, -2.0, 0.5] and row["radii"] == [1.0, 2.0, 4.0]
    assert np.allclose(np.square(row["v_circ"]) * row["radii"], sim.gm, rtol=1e-12)
    assert np.allclose(np.multiply(row["phi"], row["radii"]), -sim.gm, rtol=1e-12)
    assert np.allclose(np.multiply(row["a_radial"], np.square(row["radii"])), sim.gm, rtol=1e-12)
    rec.append_line(d / rec.ROTATION_FILE, line)
    capsys.readouterr()
    assert rec.show_status("rot", root=tmp_path)
    text = capsys.readouterr().out
    assert "Rotation curve: every 4 frames, 3 radii from 1 to 4" in text
    assert f"frame 7: peak v_circ = {row['v_circ'][0]:.6g} at R = 1" in text
    rec.save_metadata(rec.get_recording_dir("plain", tmp_path), rec.build_config(_args()), 0.0)
    assert rec.show_status("plain", root=tmp_path) and "Rotation" not in capsys.readouterr().out


def test_rotation_file_truncation_on_resume(tmp_path):
    from tools import record as rec
    path = tmp_path / rec.ROTATION_FILE
    sim = FakeSim()
    for frame in (1, 3, 5, 7):
        rec.append_line(path, rec.rotation_line(sim, frame, [1.0, 2.0]))
    with open(path, "a") as f:
        f.write('{"frame": 9, "center": [1.0, 2.')  # a killed process left a torn line
    assert [r["frame"] for r in rec.read_diagnostics(path)] == [1, 3, 5, 7]
    before = path.read_text().splitlines(keepends=True)
    kept = rec.truncate_diagnostics(path, 4)  # a resume after the checkpoint of frame 4
    assert [r["frame"] for r in kept] == [1, 3] and path.read_text() == "".join(before[:2])
    rec.append_line(path, rec.rotation_line(sim, 5, [1.0, 2.0]))
    assert [r["frame"] for r in rec.read_diagnostics(path)] == [1, 3, 5] and path.read_text() == "".join(before[:3])
