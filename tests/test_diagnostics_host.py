"""Host side of the conservation diagnostics: the NumPy restatement of the potential (tests/potential_ref.py)
against analytic values and the oracle's walk, and the recorder's diagnostics.jsonl handling on synthetic files."""
import json
import math

import numpy as np
import pytest

import potential_ref as pr
from conftest import golden

TREES = ["tree_galaxy_2048", "tree_collision_2048", "tree_cluster_2048"]


def test_two_and_three_bodies_analytic(oracle):
    G, eps = 0.5, 0.1
    pos = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]])
    mass = np.array([2.0, 3.0])
    r = math.sqrt(25.0 + eps * eps)
    want = np.array([-G * 3.0 / r, -G * 2.0 / r])
    phi, terms = pr.direct_potential(pos, mass, G, eps)
    assert np.allclose(phi, want, rtol=1e-15, atol=0) and terms == 2
    tphi, tterms, bound = pr.tree_potential(oracle, pos, mass, G, eps, 0.5)
    assert np.allclose(tphi, want, rtol=1e-15, atol=0) and tterms == 2 and not bound.any()
    pos3 = np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 2.0]])
    m3 = np.array([1.0, 2.0, 4.0])
    d = np.sqrt(((pos3[:, None] - pos3[None]) ** 2).sum(-1) + eps * eps)
    want3 = np.array([-G * sum(m3[j] / d[i, j] for j in range(3) if j != i) for i in range(3)])
    for theta in (0.0, 0.5):  # the root cell (half size ~12) is opened: only leaf terms
        tphi, _, _ = pr.tree_potential(oracle, pos3, m3, G, eps, theta)
        assert np.allclose(tphi, want3, rtol=1e-14, atol=0), theta
    assert np.allclose(pr.direct_potential(pos3, m3, G, eps)[0], want3, rtol=1e-14, atol=0)
    # W of the pair: -G m1 m2 / r
    assert np.isclose(0.5 * np.sum(mass * phi), -G * 6.0 / r, rtol=1e-15)


def test_coincident_and_eps0_direct():
    pos = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [2.0, 1.0, 1.0]])
    mass = np.ones(3)
    phi, terms = pr.direct_potential(pos, mass, 1.0, 0.0)
    assert np.array_equal(phi, [-1.0, -1.0, -2.0]) and terms == 4  # the zero-distance pair is skipped
    phi, terms = pr.direct_potential(pos, mass, 1.0, 0.5)
    assert terms == 6 and np.isclose(phi[0], -(1 / 0.5) - 1 / math.sqrt(1.25), rtol=1e-15)


@pytest.mark.parametrize("name", TREES)
def test_small_theta_equals_guarded_pair_sum(oracle, name):
    g = golden(name)
    pos, mass, G, eps = g["pos"], g["mass"], float(g["G"]), float(g["eps"])
    phi, terms, bound = pr.tree_potential(oracle, pos, mass, G, eps, 1e-9)  # below every cell's opening threshold
    ref, rterms = pr.direct_potential(pos, mass, G, eps)
    assert terms == rterms and not bound.any()
    assert np.all(np.abs(phi - ref) <= 1e-13 * np.abs(ref))


@pytest.mark.parametrize("name", TREES)
@pytest.mark.parametrize("theta", [0.3, 0.5, 0.95, 1.3])
def test_terms_equal_oracle_accepted(oracle, name, theta):
    g = golden(name)
    pos, mass, G, eps = g["pos"], g["mass"], float(g["G"]), float(g["eps"])
    tree = pr.build_tree(oracle, pos, mass)
    _, st = oracle.compute_forces_barnes_hut(pos, mass, tree[0], tree[1], theta, G, eps, stats=True)
    phi, terms, bound = pr.tree_potential(oracle, pos, mass, G, eps, theta, tree=tree)
    assert terms == st["accepted"]
    assert np.all(phi < 0) and np.all(bound >= 0)


def test_terms_edge_cases(oracle):
    g = golden("tree_edge_cases")
    for tag in ["n1", "n2", "lattice", "close_pairs", "heavy"]:
        pos, mass = g[tag + "_pos"], g[tag + "_mass"]
        tree = pr.build_tree(oracle, pos, mass)
        for theta in (0.5, 1.3):
            _, st = oracle.compute_forces_barnes_hut(pos, mass, tree[0], tree[1], theta, 1.0, 0.1, stats=True)
            _, terms, _ = pr.tree_potential(oracle, pos, mass, 1.0, 0.1, theta, tree=tree)
            assert terms == st["accepted"], (tag, theta)


# ---- recorder: diagnostics.jsonl --------------------------------------------------------------------------------
def _row(frame, E, P=(0.0, 0.0, 0.0), L=(0.0, 0.0, 1.0), **extra):
    r = {"frame": frame, "steps": frame + 1, "time": 0.1 * (frame + 1), "mass": 1.0, "center_of_mass": [0.0, 0.0, 0.0],
         "momentum": list(P), "angular_momentum": list(L), "kinetic": 1.0, "potential": E - 1.0, "total": E, "terms": 7,
         "force_precision_share": 0.5, "all_float64": False}
    r.update(extra)
    return r


def _write(path, rows, tail=""):
    path.write_text("".join(json.dumps(r) + "\n" for r in rows) + tail)


def test_jsonl_roundtrip_and_torn_line(tmp_path):
    from tools import record as rec
    p = tmp_path / "diagnostics.jsonl"
    rows = [_row(-1, -1.2345678901234567, abs_momentum=3.0), _row(4, -1.2345678901234e0 + 1e-16)]
    _write(p, rows, tail='{"frame": 9, "ste')
    got = rec.read_diagnostics(p)
    assert got == rows  # repr floats come back bit for bit; the torn line is left out
    assert rec.read_diagnostics(tmp_path / "missing.jsonl") == []
    _write(p, rows, tail="not json\n")
    assert rec.read_diagnostics(p) == rows


def test_resume_truncation_and_restart(tmp_path):
    from tools import record as rec
    p = tmp_path / "diagnostics.jsonl"
    rows = [_row(-1, -1.0)] + [_row(f, -1.0) for f in range(4, 60, 5)]
    _write(p, rows, tail='{"frame": 64')
    keep = rec.truncate_diagnostics(p, 49)
    assert [r["frame"] for r in keep] == [-1, 4, 9, 14, 19, 24, 29, 34, 39, 44, 49]
    assert rec.read_diagnostics(p) == keep and p.read_text().endswith("\n")
    assert not list(tmp_path.glob(".*.part"))
    rec.truncate_diagnostics(p, -1)  # nothing but the initial state survives a restart point before frame 0
    assert [r["frame"] for r in rec.read_diagnostics(p)] == [-1]
    rec.append_line(p, json.dumps(_row(4, -1.0)) + "\n")
    assert [r["frame"] for r in rec.read_diagnostics(p)] == [-1, 4]


def test_drift_and_status_text(tmp_path, capsys):
    from tools import record as rec
    d = tmp_path / "recordings" / "s1"
    d.mkdir(parents=True)
    (d / "metadata.json").write_text(json.dumps({"num_bodies": 10, "theta": 0.5, "distribution": "galaxy",
                                                 "total_frames": 20, "diagnostics_every": 5}))
    rows = [_row(-1, -2.0, P=(0.0, 0.0, 0.0), L=(0.0, 0.0, 4.0), abs_momentum=10.0),
            _row(4, -2.5, P=(0.0, 0.0, 0.0), L=(0.0, 0.0, 4.0)),
            _row(9, -2.002, P=(0.3, 0.4, 0.0), L=(0.0, 0.0, 4.4))]
    _write(d / "diagnostics.jsonl", rows)
    de, dp, dl = rec.diagnostics_drift(rec.read_diagnostics(d / "diagnostics.jsonl"))
    assert math.isclose(de, 0.001, rel_tol=1e-9) and math.isclose(dp, 0.05, rel_tol=1e-12)
    assert math.isclose(dl, 0.1, rel_tol=1e-9)
    assert rec.show_status("s1", root=tmp_path)
    out = capsys.readouterr().out
    assert "|E - E0| / |E0|:        1.000e-03" in out
    assert "|P - P0| / sum m|v|_0:  5.000e-02" in out
    assert "|L - L0| / |L0|:        1.000e-01" in out
    assert "frame -1 -> 9 (3 lines)" in out
    (d / "diagnostics.jsonl").unlink()
    rec.show_status("s1", root=tmp_path)
    assert "Diagnostics" not in capsys.readouterr().out


def test_cli_flag_into_config():
    from tools import record as rec
    ap = rec.build_parser()
    cfg = rec.build_config(ap.parse_args(["s", "--preset", "quick_galaxy", "--diagnostics", "5", "--seed", "3"]))
    assert cfg["diagnostics_every"] == 5
    cfg = rec.build_config(ap.parse_args(["s", "--preset", "quick_galaxy"]))
    assert "diagnostics_every" not in cfg
    with pytest.raises(ValueError):
        rec.build_config(ap.parse_args(["s", "--preset", "quick_galaxy", "--diagnostics", "0"]))
