"""The tidal tensor, host side (include/nbmi.h nbmi_tidal_at / nbmi_get_tidal_f64): the NumPy restatement's
terms against minus the symbolic Hessian of the potentials field_ref sums, the restatement against the direct sum and
against field_ref's accepted sets, the C ABI's declaration, the Python classes' refusals, nbody/field.py against a point
mass, and the recorder's options, metadata, timestep.jsonl and --status with a stand-in backend (no device)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import field_ref as fr
import potential_ref as pr
import tidal_ref as tr
from conftest import ROOT, golden

IDX = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))  # the six components of a row


def _hessians():
    """minus the Hessians, as mpmath functions of (dx, dy, dz, gm, eps, Pxx, Pyy, Pzz, Pxy, Pxz, Pyz), of the two
    potentials field_ref sums: -gm u^-1/2, and quadrupole_ref.term's 1/2 [tr P u^-3/2 - 3 (d^T P d) u^-5/2]; d = c - p, so
    the Hessian in p is the Hessian in d"""
    import sympy as sp
    dx, dy, dz, gm, eps, pxx, pyy, pzz, pxy, pxz, pyz = syms = sp.symbols("dx dy dz gm eps pxx pyy pzz pxy pxz pyz", real=True)
    d = sp.Matrix([dx, dy, dz])
    P = sp.Matrix([[pxx, pxy, pxz], [pxy, pyy, pyz], [pxz, pyz, pzz]])
    u = dx * dx + dy * dy + dz * dz + eps * eps
    mono = -gm / sp.sqrt(u)
    quad = sp.Rational(1, 2) * (P.trace() * u ** sp.Rational(-3, 2) - 3 * (d.T * P * d)[0, 0] * u ** sp.Rational(-5, 2))
    out = []
    for phi in (mono, quad):
        H = sp.hessian(phi, (dx, dy, dz))
        out.append(sp.lambdify(syms, [-H[i, j] for i, j in IDX], modules="mpmath"))
    return out


def test_terms_are_minus_the_hessian_of_the_potentials():
    import mpmath
    rng = np.random.default_rng(11)
    k = 200
    d = rng.normal(size=(k, 3)) * 10.0 ** rng.uniform(-1, 2, (k, 1))
    a = rng.normal(size=(k, 3, 3))
    Pm = np.einsum("kij,klj->kil", a, a) * rng.uniform(0.1, 5.0, (k, 1, 1))  # A A^T: positive semi-definite
    Pm[:20] = np.einsum("ki,kj->kij", a[:20, 0], a[:20, 0])  # rank one: on the edge of the cone
    P6 = np.stack([Pm[:, i, j] for i, j in IDX], axis=1)
    gm = rng.uniform(0.1, 50.0, k)
    eps = np.where(np.arange(k) % 4 == 0, 0.0, rng.uniform(0.01, 3.0, k))  # eps = 0 included
    u = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + eps * eps
    tm, mag_m = tr.mono_term(d, u, gm)
    tq, mag_q = tr.quad_term(d, u, P6)
    f_mono, f_quad = _hessians()
    with mpmath.workdps(50):
        for i in range(k):
            args = [mpmath.mpf(float(x)) for x in (*d[i], gm[i], eps[i], *P6[i])]
            for f, t, mag in ((f_mono, tm, mag_m), (f_quad, tq, mag_q)):
                e = [mpmath.mpf(float(t[i, c])) - h for c, h in enumerate(f(*args))]
                err = mpmath.sqrt(e[0] ** 2 + e[1] ** 2 + e[2] ** 2 + 2 * (e[3] ** 2 + e[4] ** 2 + e[5] ** 2))
                assert err <= 1e-12 * mag[i], (i, float(err), mag[i])
    # the trace of the monopole term is -3 G M eps^2 u^-5/2
    assert np.all(np.abs(tr.trace(tm) + 3.0 * gm * eps * eps * u ** -2.5) <= 1e-12 * mag_m)


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
        for multipole in ("monopole", "quadrupole"):  # (no cell is applied: the second-order term never appears)
            t = tr.tree_tidal(oracle, pts, pos, mass, G, e, 1e-9, multipole=multipole)
            t6, terms, mag = tr.direct_tidal(pts, pos, mass, G, e)
            assert np.array_equal(t["terms"], terms)
            assert terms[0] == len(pos) - 1 and terms[-1] == len(pos)
            assert np.all(tr.error(t["t6"], t6) <= 1e-12 * mag)
            assert np.all(np.abs(t["mag"] - mag) <= 1e-12 * mag)
            assert np.all(t["bound"] == 0.0)  # no cell term, nothing to bound


@pytest.mark.parametrize("name", ["tree_galaxy_2048", "tree_cluster_2048"])
def test_accepted_sets_are_the_field_restatements(oracle, name):
    g = golden(name)
    pos, mass, G, eps = g["pos"], g["mass"], float(g["G"]), float(g["eps"])
    tree = pr.build_tree(oracle, pos, mass)
    pts = np.concatenate([_points(pos, np.random.default_rng(3)), pos[100:400]])
    for theta in (0.5, 1.3):
        for multipole in ("monopole", "quadrupole"):
            f = fr.tree_field(oracle, pts, pos, mass, G, eps, theta, tree=tree, multipole=multipole)
            t = tr.tree_tidal(oracle, pts, pos, mass, G, eps, theta, tree=tree, multipole=multipole)
            assert np.array_equal(t["terms"], f["terms"]) and t["margin"] == f["margin"]
            assert np.all(t["bound"] >= 0.0) and np.all(t["mag"] > 0.0)


def test_trace_is_zero_without_softening_and_negative_with(oracle):
    g = golden("tree_collision_2048")
    pos, mass, G, eps = g["pos"], g["mass"], float(g["G"]), float(g["eps"])
    assert eps > 0.0
    pts = _points(pos, np.random.default_rng(4))
    tree = pr.build_tree(oracle, pos, mass)
    for multipole in ("monopole", "quadrupole"):
        t = tr.tree_tidal(oracle, pts, pos, mass, G, 0.0, 0.5, tree=tree, multipole=multipole)
        assert np.all(np.abs(tr.trace(t["t6"])) <= 1e-12 * t["mag"])
    t6, _, mag = tr.direct_tidal(pts, pos, mass, G, 0.0)
    assert np.all(np.abs(tr.trace(t6)) <= 1e-12 * mag)
    assert np.all(tr.trace(tr.direct_tidal(pts, pos, mass, G, eps)[0]) < 0.0)
    assert np.all(tr.trace(tr.tree_tidal(oracle, pts, pos, mass, G, eps, 0.5, tree=tree)["t6"]) < 0.0)


def test_quadrupole_restatement_is_closer_to_the_direct_sum(oracle):
    g = golden("tree_collision_2048")
    pos, mass, G, eps = g["pos"], g["mass"], float(g["G"]), float(g["eps"])
    pts = _points(pos, np.random.default_rng(2))
    t6, _, _ = tr.direct_tidal(pts, pos, mass, G, eps)
    tree = pr.build_tree(oracle, pos, mass)
    mono = tr.tree_tidal(oracle, pts, pos, mass, G, eps, 0.5, tree=tree)
    quad = tr.tree_tidal(oracle, pts, pos, mass, G, eps, 0.5, tree=tree, multipole="quadrupole")
    assert np.array_equal(mono["terms"], quad["terms"])
    em, eq = tr.error(mono["t6"], t6).sum(), tr.error(quad["t6"], t6).sum()
    assert eq < 0.5 * em, (em, eq)


def test_header_declares_and_library_exports_the_calls():
    import nbmi_native
    text = open(os.path.join(ROOT, "include", "nbmi.h")).read()
    assert re.search(r"^int nbmi_tidal_at\(nbmi_sim \*sim, int64_t m, const double \*points_xyz", text, re.M)
    assert re.search(r"^int nbmi_get_tidal_f64\(nbmi_sim \*sim, double \*tidal6", text, re.M)
    assert len(nbmi_native.PROTOTYPES["nbmi_tidal_at"][1]) == 5 and len(nbmi_native.PROTOTYPES["nbmi_get_tidal_f64"][1]) == 3
    lib = ctypes.CDLL(nbmi_native.LIB_PATH)
    assert hasattr(lib, "nbmi_tidal_at") and hasattr(lib, "nbmi_get_tidal_f64")
    for word in ("the same accepted set as nbmi_field_at", "{Txx, Tyy, Tzz, Txy, Txz, Tyz}", "48 bytes per row", "56 bytes per body",
                 "w5 = (3.0 * w) / u", "the message names the first bad row", "2.0 * ((Txy^2 + Txz^2) + Tyz^2)"):
        assert word in text, word


def test_python_classes_refuse_without_a_device():
    from nbody.gpu_backend import HIPBarnesHutSimulation, HIPDirectSimulation, HIPOwnerSimulation
    sim = HIPOwnerSimulation.__new__(HIPOwnerSimulation)  # no handle: the refusal must come before any library call
    sim._h = None
    for call in (lambda: sim.tidal_at(np.zeros((2, 3))), lambda: sim.tidal_at(np.zeros((2, 3)), terms=True), sim.tidal,
                 lambda: sim.tidal(norm=True), sim.tidal_norm):
        with pytest.raises(ValueError, match="owner"):
            call()
    for cls in (HIPBarnesHutSimulation, HIPDirectSimulation):
        sim = cls.__new__(cls)
        sim._h = None
        for bad in (np.zeros(3), np.zeros((4, 2)), np.zeros((2, 3, 1)), [[1.0, 2.0]], 5.0):
            with pytest.raises(ValueError, match=r"\(m, 3\)"):
                sim.tidal_at(bad)


# ---- nbody/field.py against a point mass ---------------------------------------------------------------------------
GM, AT = 2.5, np.array([1.0, -2.0, 0.5])


def _point_mass_rows(points):
    d = AT - np.asarray(points, dtype=np.float64)
    return tr.mono_term(d, (d * d).sum(1), np.full(len(d), GM))[0]


def test_field_helpers_against_a_point_mass():
    from nbody import field as fl
    rng = np.random.default_rng(6)
    pts = AT + rng.normal(size=(50, 3)) * 10.0 ** rng.uniform(-1, 2, (50, 1))
    r = np.sqrt(((pts - AT) ** 2).sum(1))
    t6 = _point_mass_rows(pts)
    M = fl.tidal_matrix(t6)
    assert M.shape == (50, 3, 3) and np.array_equal(M, M.transpose(0, 2, 1))
    assert np.array_equal(M[:, 0, 1], t6[:, 3]) and np.array_equal(M[:, 0, 2], t6[:, 4]) and np.array_equal(M[:, 1, 2], t6[:, 5])
    assert np.array_equal(np.stack([M[:, 0, 0], M[:, 1, 1], M[:, 2, 2]], axis=1), t6[:, :3])
    lam = fl.tidal_eigenvalues(t6)
    scale = GM / r ** 3
    assert lam.shape == (50, 3) and np.all(np.abs(lam - scale[:, None] * np.array([2.0, -1.0, -1.0])) <= 1e-12 * scale[:, None])
    norm = fl.tidal_norm(t6)
    assert np.all(np.abs(norm - np.sqrt(6.0) * scale) <= 1e-12 * scale)
    assert np.all(np.abs(norm - np.sqrt((M * M).sum((1, 2)))) <= 1e-14 * norm)
    dt = 0.37
    omega = np.sqrt(GM / r ** 3)  # the angular speed of a circular Kepler orbit
    assert np.all(np.abs(fl.phase_per_step(norm, dt) - omega * dt) <= 1e-12 * omega * dt)
    assert fl.phase_per_step(np.sqrt(6.0) * 4.0, 0.5) == 1.0
    # a point mass stretches along one axis and compresses along two: -T has two positive eigenvalues (a filament)
    assert np.all(fl.web_type(t6) == 2) and np.all(fl.web_type(t6, threshold=1.5 * scale.max()) == 0)
    assert fl.web_type(-t6).tolist() == [1] * 50
    iso = np.array([[-1.0, -1.0, -1.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 0.0, 0.0, 0.0], [-1.0, -2.0, 3.0, 0.0, 0.0, 0.0]])
    assert fl.web_type(iso).tolist() == [3, 0, 2] and fl.web_type(iso, threshold=1.5).tolist() == [0, 0, 1]
    # static tidal limit of a satellite G m in the field of the point mass: cbrt(gm / (2 G M / r^3)) = r cbrt(gm / (2 G M))
    rt = fl.tidal_radius(0.01, t6)
    assert np.all(np.abs(rt - r * np.cbrt(0.01 / (2.0 * GM))) <= 1e-12 * r)
    assert fl.tidal_radius(1.0, iso).tolist() == [np.inf, 1.0, float(np.cbrt(1.0 / 3.0))]
    assert fl.tidal_radius(1.0, np.zeros((2, 6))).tolist() == [np.inf, np.inf]
    assert "centrifugal" in fl.tidal_radius.__doc__
    for bad in (np.zeros(6), np.zeros((3, 5))):
        with pytest.raises(ValueError, match=r"\(m, 6\)"):
            fl.tidal_matrix(bad)


# ---- the recorder ----------------------------------------------------------------------------------------------------
def _args(*extra):
    from tools import record as rec
    return rec.build_parser().parse_args(["--preset", "quick_galaxy", *extra])


def test_recorder_options():
    from tools import record as rec
    assert "timestep_check" not in rec.build_config(_args())  # the default writes no key
    assert rec.timestep_config({}) is None
    ls = rec.LINE_STREAMS
    assert ls.index(rec.TIMESTEP) == ls.index(rec.DIAGNOSTICS) + 1 and ls[-1] is rec.ROTATION and ls[-2] is rec.PAIRS
    assert ls.index(rec.PROFILE) == ls.index(rec.GROUPS) + 1 == ls.index(rec.PAIRS) - 1
    cfg = rec.build_config(_args("--timestep-check", "5"))
    assert cfg["timestep_check"] == {"every": 5, "levels": [0.1, 0.5, 2.0]}
    assert rec.timestep_config(cfg) == (5, cfg["dt_per_frame"] / cfg["substeps"], [0.1, 0.5, 2.0])
    cfg = rec.build_config(_args("--timestep-check", "2", "--chi-levels", "0.25,1,2,4", "--dt", "0.4"))
    assert cfg["timestep_check"] == {"every": 2, "levels": [0.25, 1.0, 2.0, 4.0]}
    assert rec.timestep_config(cfg) == (2, 0.4 / cfg["substeps"], [0.25, 1.0, 2.0, 4.0])
    assert rec.timestep_config({**cfg, "substeps": 4})[1] == 0.1  # dt of a step, not of a frame
    assert rec.build_config(_args("--timestep-check", "2", "--pairs", "3"))["pairs"]["every"] == 3
    assert len(rec.build_config(_args("--timestep-check", "1", "--chi-levels", ",".join(str(k) for k in range(1, 17))))
               ["timestep_check"]["levels"]) == 16
    for bad, word in ((("--chi-levels", "1,2"), "needs --timestep-check"),
                      (("--timestep-check", "0"), "--timestep-check"), (("--timestep-check", "-2"), "--timestep-check"),
                      (("--timestep-check", "2", "--chi-levels", "2,1"), "--chi-levels"),
                      (("--timestep-check", "2", "--chi-levels", "1,1"), "--chi-levels"),
                      (("--timestep-check", "2", "--chi-levels", "0,1"), "--chi-levels"),
                      (("--timestep-check", "2", "--chi-levels=-1,1"), "--chi-levels"),
                      (("--timestep-check", "2", "--chi-levels", "1,inf"), "--chi-levels"),
                      (("--timestep-check", "2", "--chi-levels", "1,nan"), "--chi-levels"),
                      (("--timestep-check", "2", "--chi-levels", "1,wide"), "--chi-levels"),
                      (("--timestep-check", "2", "--chi-levels", ""), "--chi-levels"),
                      (("--timestep-check", "2", "--chi-levels", ",".join(str(k) for k in range(1, 18))), "--chi-levels")):
        with pytest.raises(ValueError, match=word):
            rec.build_config(_args(*bad))
    with pytest.raises(ValueError, match="--chi-levels"):
        rec.timestep_config({"timestep_check": {"every": 2, "levels": [3.0, 2.0]}, "dt_per_frame": 1.0, "substeps": 1})


class FakeSim:
    """the backend object's tidal_norm: bodies on circular orbits about a point mass, Omega = 0.01 .. 10"""

    def __init__(self, n=1000):
        self.omega = np.geomspace(0.01, 10.0, n)
        self.calls = 0

    def tidal_norm(self):
        self.calls += 1
        return np.sqrt(6.0) * self.omega ** 2


def test_recorder_metadata_round_trip_line_and_status(tmp_path, capsys):
    from tools import record as rec
    cfg = rec.build_config(_args("--timestep-check", "4", "--chi-levels", "0.1,0.5,2,30", "--dt", "1.0"))
    cfg["substeps"] = 2
    d = rec.get_recording_dir("ts", tmp_path)
    rec.save_metadata(d, cfg, 0.0)
    sim = FakeSim()
    assert rec.TIMESTEP.apply(sim, cfg, d) == cfg and sim.calls == 0  # nothing is taken from the state
    meta = rec.load_metadata(d)
    assert meta["timestep_check"] == {"every": 4, "levels": [0.1, 0.5, 2.0, 30.0]}
    every, dt, levels = rec.timestep_config(meta)
    assert (every, dt, levels) == (4, 0.5, [0.1, 0.5, 2.0, 30.0])
    line = rec.timestep_line(sim, 7, dt, levels)
    assert line.endswith("\n") and sim.calls == 1
    row = json.loads(line)
    assert sorted(row) == ["above", "bodies", "chi_quantiles", "dt", "frame", "levels"]
    assert sorted(row["chi_quantiles"]) == ["0.5", "0.9", "0.99", "1.0"]
    chi = sim.omega * 0.5
    assert row["frame"] == 7 and row["dt"] == 0.5 and row["bodies"] == 1000 and row["levels"] == levels
    assert row["above"] == [int((chi > c).sum()) for c in levels] and row["above"][2] > 0 and row["above"][3] == 0
    assert np.allclose([row["chi_quantiles"][k] for k in ("0.5", "0.9", "0.99", "1.0")], np.quantile(chi, [0.5, 0.9, 0.99, 1.0]),
                       rtol=1e-12)
    assert abs(row["chi_quantiles"]["1.0"] - 5.0) <= 1e-12
    rec.append_line(d / rec.TIMESTEP_FILE, line)
    capsys.readouterr()
    assert rec.show_status("ts", root=tmp_path)
    text = capsys.readouterr().out
    assert "Time-step check: every 4 frames, levels 0.1, 0.5, 2, 30" in text
    assert f"frame 7: dt = 0.5, phase per step median {row['chi_quantiles']['0.5']:.3g}" in text
    assert text.count("WARNING") == 1 and f"WARNING: {row['above'][2]:,} of 1,000 bodies advance more than 2 rad per step" in text
    # a resolved run warns of nothing; a recording without the key says nothing
    calm = rec.get_recording_dir("calm", tmp_path)
    rec.save_metadata(calm, cfg, 0.0)
    rec.append_line(calm / rec.TIMESTEP_FILE, rec.timestep_line(sim, 3, 0.01, levels))
    capsys.readouterr()
    assert rec.show_status("calm", root=tmp_path)
    text = capsys.readouterr().out
    assert "Time-step check" in text and "frame 3" in text and "WARNING" not in text
    rec.save_metadata(rec.get_recording_dir("plain", tmp_path), rec.build_config(_args()), 0.0)
    assert rec.show_status("plain", root=tmp_path) and "Time-step" not in capsys.readouterr().out


def test_timestep_file_truncation_on_resume(tmp_path):
    from tools import record as rec
    path = tmp_path / rec.TIMESTEP_FILE
    sim = FakeSim(10)
    for frame in (1, 3, 5, 7):
        rec.append_line(path, rec.timestep_line(sim, frame, 0.1, [0.5, 2.0]))
    with open(path, "a") as f:
        f.write('{"frame": 9, "dt": 0.1, "chi_quan')  # a killed process left a torn line
    assert [r["frame"] for r in rec.read_diagnostics(path)] == [1, 3, 5, 7]
    before = path.read_text().splitlines(keepends=True)
    kept = rec.truncate_diagnostics(path, 4)  # a resume after the checkpoint of frame 4
    assert [r["frame"] for r in kept] == [1, 3] and path.read_text() == "".join(before[:2])
    rec.append_line(path, rec.timestep_line(sim, 5, 0.1, [0.5, 2.0]))
    assert [r["frame"] for r in rec.read_diagnostics(path)] == [1, 3, 5] and path.read_text() == "".join(before[:3])
