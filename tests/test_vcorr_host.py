"""Host checks for bdmi_velocity_correlation (include/bdmi.h): the NumPy restatement tests/vcorr_ref.py against a plain
double loop, its quantisation at ties and with velocities that are not finite, the identity that ties the pair sums to the
moments, the inputs of tests/vcorr_cases.py (the candidate mask removes no pair in range, except on the one input built
for it), boids.analysis on hand-made results, the binding and tools.flock_video --correlations with stand-ins.  No GPU.
"""
import json
import os

import numpy as np
import pytest

import vcorr_cases as VC
import vcorr_ref as VR
from test_flockstats_host import _FakeFlock, _FakeRenderer


@pytest.mark.parametrize("periodic", (False, True))
def test_restatement_equals_a_double_loop(periodic):
    c = VC.periodic_box(5) if periodic else VC.sizes(200)
    pos, vel = c["pos"][:200], c["vel"][:200]
    table = VR.PairTable(pos, c["params"], periodic)
    for edges in (np.linspace(0.0, 5.0, 7), np.geomspace(0.3, 10.0, 9), np.array([2.0, 2.5])):
        mean = VC.mean_heading(vel)
        a = VR.correlate(pos, vel, c["params"], edges, mean, periodic, table=table)
        b = VR.double_loop(pos, vel, c["params"], edges, mean, periodic)
        assert [int(x) for x in a["pairs"]] == b["pairs"] and a["dot"] == b["dot"] and a["evals"] == b["evals"]
        assert a["cut"] == 0 and sum(b["pairs"]) > 0
    assert VR.correlate(pos, vel, c["params"], np.geomspace(0.3, 10.0, 9), np.zeros(3), periodic, table=table)["reach"] == 2


def test_quantisation_at_ties_and_with_values_that_are_not_finite():
    # headings along x: u = (1, 0, 0) exactly, so d = 1 - mean; mean chosen so that d 2^24 = k + 1/2
    vel = np.array([[2.0, 0.0, 0.0]] * 4)
    for k, want in ((0, 0), (1, 2), (2, 2), (3, 4), (-1, 0), (-2, -2), (-3, -2)):
        mean = np.array([1.0 - (k + 0.5) * 2.0 ** -24, 0.0, 0.0])
        assert (mean[0] - 1.0) * 2.0 ** 24 == -(k + 0.5)  # exact
        q = VR.quantise(vel, mean)
        assert q[:, 0].tolist() == [want] * 4 and not q[:, 1:].any(), (k, q[0])
    v = np.array([[np.nan, 1.0, 2.0], [np.inf, 1.0, 2.0], [0.0, 0.0, 0.0], [0.0, -3.0, 4.0], [1e-200, 0.0, 0.0]])
    q = VR.quantise(v, [0.5, 0.0, -0.25])
    assert q[0].tolist() == [0, 0, 0]                      # s is NaN: every component is
    assert q[1].tolist() == [0, 0, 1 << 22]                # u = (NaN, 0, 0)
    assert q[2].tolist() == [-(1 << 23), 0, 1 << 22]       # at rest: u = 0
    assert q[3].tolist() == [-(1 << 23), int(np.rint(-0.6 * 2 ** 24)), int(np.rint((0.8 + 0.25) * 2 ** 24))]
    assert q[4].tolist() == [-(1 << 23), 0, 1 << 22]       # the square underflows: s == 0 and u = 0, as for a boid at rest
    assert np.abs(VR.quantise(np.random.default_rng(0).normal(size=(100, 3)), [1.0, -1.0, 1.0])).max() <= 1 << 25
    assert VR.hi_lo(-1) == (-1, 0xFFFFFFFF) and VR.from_hi_lo(*VR.hi_lo(-(3 << 70) + 5)) == -(3 << 70) + 5


def test_identity_between_the_pair_sums_and_the_moments():
    for c in (VC.sizes(257), VC.periodic_box(3)):
        n = len(c["pos"])
        last = VC.WHOLE_GRID if not c["periodic"] else 5.0  # dim 3, reach 1: all 27 cells, but only d <= 5 is in range
        for mean in (np.zeros(3), VC.mean_heading(c["vel"])):
            w = VR.correlate(c["pos"], c["vel"], c["params"], np.linspace(0.0, last, 9), mean, c["periodic"])
            if not c["periodic"]:
                assert int(w["pairs"].sum()) == n * (n - 1) // 2 == w["evals"]
                assert 2 * sum(w["dot"]) == sum(x * x for x in w["qsum"]) - w["qsq"]
            else:
                assert w["evals"] == n * (n - 1) // 2 and int(w["pairs"].sum()) < w["evals"]


def test_inputs_are_what_they_claim():
    for n in (2049, 4097):
        c = VC.uniform(n)
        assert len(c["pos"]) == n and np.abs(c["pos"]).max() > 17.5 and np.abs(c["pos"]).max() <= 22.5
        sets = VC.edge_sets(n)
        assert len(sets) == 20 and {1, 64} <= {len(e) - 1 for e in sets} and any(e[0] == 0 for e in sets) and any(e[0] > 0 for e in sets)
        assert all(1 <= VR.reach(e, c["params"], False) <= 3 for e in sets)
    assert VR.reach([0.0, VC.WHOLE_GRID], VC.WALLED, False) == 16 and 45.0 * np.sqrt(3.0) < VC.WHOLE_GRID
    for dim, ok, bad in ((3, 1, 2), (5, 2, 3), (6, 2, 3), (7, 3, 4)):
        prm = VC.periodic_box(dim)["params"]
        assert VR.grid_of(prm, True) == (5.0, dim) and VR.admissible(ok, prm, True) and not VR.admissible(bad, prm, True)
    assert len(VC.LATTICE_EDGES) == 16 and np.all(np.diff(VC.LATTICE_EDGES) > 0)
    for m in (1, 2, 3):
        c = VC.boundary(m)
        w = VR.correlate(c["pos"], c["vel"], c["params"], [0.0, 1.0, 5.0 * m], np.zeros(3))
        assert w["pairs"].tolist() == [0, 1, 1] and w["evals"] == 2 and w["cut"] == 0
    c = VC.boundary_face(2)
    w = VR.correlate(c["pos"], c["vel"], c["params"], [0.0, 1.0, 10.0], np.zeros(3), True)
    assert w["pairs"].tolist() == [0, 1, 1] and w["evals"] == 2 and w["cut"] == 1  # the one input the mask cuts
    for kind in ("face_pair", "face", "edge", "corner"):
        for c, reaches in ((VC.torus_pair(kind), (1,)), (VC.wide_pair(kind), (1, 2))):
            for m in reaches:
                assert VR.admissible(m, c["params"], True)
                w = VR.correlate(c["pos"], c["vel"], c["params"], [0.0, 5.0 * m], np.zeros(3), True)
                assert w["cut"] == 0 and int(w["pairs"].sum()) >= 1
    t = VC.twins()
    assert VR.correlate(t["pos"], t["vel"], t["params"], [0.0, 1.0], np.zeros(3))["pairs"][0] == 40


def test_binding_and_header():
    import ctypes
    import nbmi_native
    res, args = nbmi_native.PROTOTYPES["bdmi_velocity_correlation"]
    assert res is ctypes.c_int and len(args) == 8
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bdmi.h")).read()
    for words in ("bdmi_velocity_correlation", "rint(d_c 2^24)", "CANDIDATE", "2 m + 1 <= dim", "hi 2^32 + lo", "bytes per boid"):
        assert words in header, words


# ---- boids.analysis on hand-made results -------------------------------------------------------------------------------
def _res(edges, pairs, dot, qsq, n, qsum=(0, 0, 0)):
    return dict(edges=np.asarray(edges, float), pairs=np.asarray(pairs, np.int64), dot=list(dot), qsq=qsq, n=n, qsum=list(qsum),
                mean=[0.0, 0.0, 0.0], quantum=2.0 ** -24, reach=1, evals=sum(pairs))


def test_analysis_functions():
    from boids import analysis as A
    one = 1 << 48
    # 4 boids with |q|^2 = 2^48 each: C0 = 1.  C = 0.5, 0.25, -0.25, (empty), -0.125
    res = _res([1, 2, 3, 4, 5, 6], [0, 2, 4, 2, 0, 8], [0, one, one, -one // 2, 0, -one], 4 * one, 4)
    r, c = A.velocity_correlation_function(res)
    assert r.tolist() == [0.5, 1.5, 2.5, 3.5, 4.5, 5.5]
    assert np.isnan(c[0]) and np.isnan(c[4]) and c[[1, 2, 3, 5]].tolist() == [0.5, 0.25, -0.25, -0.125]
    assert A.correlation_length(res) == 3.0  # between the centres 2.5 (0.25) and 3.5 (-0.25)
    chi = A.susceptibility(res)
    assert chi == {"chi": 2 * 2 / 4, "r": 3.0}  # the cumulated sum peaks at 2 * 2^48 behind slot 2, whose edge is 3
    # the crossing skips an empty slot; a zero is a crossing at its own centre
    gap = _res([1, 2, 3, 4], [0, 1, 0, 1], [0, one, 0, -one], one, 1)
    assert A.correlation_length(gap) == 2.5
    zero = _res([1, 2, 3], [0, 1, 1], [0, one, 0], one, 1)
    assert A.correlation_length(zero) == 2.5
    # no crossing: all positive, all negative, nothing at all
    assert A.correlation_length(_res([1, 2, 3], [0, 1, 1], [0, one, one], one, 1)) is None
    assert A.correlation_length(_res([1, 2, 3], [0, 1, 1], [0, -one, -one], one, 1)) is None
    assert A.correlation_length(_res([1, 2, 3], [0, 0, 0], [0, 0, 0], one, 1)) is None
    assert np.isnan(A.velocity_correlation_function(_res([1, 2], [3, 3], [5, 5], 0, 7))[1]).all()  # C0 == 0
    assert A.susceptibility(_res([1, 2], [1, 1], [-one, -one], one, 2)) == {"chi": -1.0, "r": 1.0}
    assert A.susceptibility(_res([1, 2], [0, 0], [0, 0], 0, 0)) == {"chi": 0.0, "r": None}
    # sums beyond 2^63 stay exact integers until the one division
    big = _res([0, 1], [0, 1 << 40], [0, 1 << 90], 1 << 60, 1 << 20)
    assert A.velocity_correlation_function(big)[1][1] == float(1 << 10)
    # g(r): an ideal gas has g = 1
    n, L = 1000, 10.0
    edges = np.array([0.0, 1.0, 2.0])
    vol = 4.0 / 3.0 * np.pi * np.array([1.0, 7.0])
    ideal = np.rint(0.5 * n * (n - 1) * vol / L ** 3).astype(np.int64)
    r, g = A.radial_distribution(_res(edges, [0, *ideal], [0, 0, 0], one, n), dict(length=L))
    assert np.isnan(g[0]) and np.allclose(g[1:], 1.0, rtol=1e-3) and r.tolist() == [0.0, 0.5, 1.5]
    assert np.allclose(A.radial_distribution(_res(edges, [0, *ideal], [0, 0, 0], one, n), L)[1][1:], g[1:])
    with pytest.raises(ValueError):
        A.velocity_correlation_function(_res([1, 2, 3], [1, 1], [1, 1], 1, 1))
    line = A.correlation_line(4, 9, res)
    rec = json.loads(line)
    assert "\n" not in line and set(rec) == {"frame", "steps", "edges", "pairs", "dot", "mean", "C", "xi", "chi"}
    assert rec["C"][0] is None and rec["C"][1] == 0.5 and rec["xi"] == 3.0 and rec["chi"] == 1.0 and rec["pairs"][5] == 8
    assert json.loads(A.correlation_line(0, 0, big))["dot"][1] == str(1 << 90)


# ---- tools.flock_video --correlations ------------------------------------------------------------------------------------
class _CorrFlock(_FakeFlock):
    def __init__(self, n, seed, device, periodic=False):
        super().__init__(n, seed, device)
        self.box = dict(periodic=periodic, length=60.0, cell_size=6.0 if periodic else 5.0)

    def set_noise(self, eta, seed=0, step=None):
        pass

    def set_neighbour_mode(self, mode, k=7):
        pass

    def velocity_correlation(self, edges, mean=None):
        self.calls.append(("correlation", tuple(float(e) for e in edges), mean))
        nb = len(edges) - 1
        return _res(edges, [0] + [2] * nb, [0] + [1 << 48] * nb, 8 << 48, 8)


def test_flock_video_correlation_arguments(tmp_path):
    from tools import flock_video as fv
    a = fv.build_parser().parse_args([])
    assert (a.correlations, a.correlation_edges) == (0, "auto")
    assert fv.correlation_edges("auto") is None and np.array_equal(fv.correlation_edges("auto", 5.0), np.linspace(0.0, 20.0, 17))
    assert fv.correlation_edges("0,1.5,4").tolist() == [0.0, 1.5, 4.0]
    for bad in ("1", "1,1", "2,1", "-1,2", "0,nan", "0,inf", "a,b", "", ",".join(str(k) for k in range(66))):
        with pytest.raises(ValueError, match="--correlation-edges"):
            fv.correlation_edges(bad)
    assert fv.correlation_path(tmp_path / "clip.rgb").name == "clip.correlation.jsonl"
    assert fv.correlation_path(tmp_path / "frames").name == "frames.correlation.jsonl"
    quiet = lambda *x: None  # noqa: E731
    made = len(_FakeFlock.made)
    for flags in (["--correlations", "-1"], ["--correlations", "2", "--correlation-edges", "3,2"]):
        with pytest.raises(ValueError):
            fv.run(fv.build_parser().parse_args(["--frames", "1", *flags]), make_flock=_CorrFlock, make_renderer=_FakeRenderer, say=quiet)
    assert len(_FakeFlock.made) == made  # refused before a flock is made
    for flags, cell in (([], 5.0), (["--periodic", "--noise", "0.5", "--neighbours", "topological"], 6.0)):
        raw = tmp_path / ("p" if flags else "w") / "clip.rgb"
        said = []
        args = fv.build_parser().parse_args(["--boids", "8", "--frames", "5", "--format", "raw", "-o", str(raw), "--warmup", "3",
                                             "--correlations", "2", *flags])
        t = fv.run(args, make_flock=_CorrFlock, make_renderer=_FakeRenderer, say=said.append)
        flock = _FakeFlock.made[-1]
        path = raw.with_name("clip.correlation.jsonl")
        assert t["ok"] and t["correlations"] == str(path) and t["correlation_lines"] == 3 and "diagnostics" not in t
        recs = [json.loads(x) for x in path.read_text().splitlines()]
        assert [r["frame"] for r in recs] == [0, 2, 4] and [r["steps"] for r in recs] == [4, 6, 8]
        assert all(np.array_equal(r["edges"], np.linspace(0.0, 4.0 * cell, 17)) and r["C"][1] == 0.5 and r["xi"] is None for r in recs)
        assert [c[0] for c in flock.calls] == ["correlation"] * 3 and flock.calls[0][2] is None
        meta = json.loads(raw.with_name("clip.rgb.json").read_text())
        assert meta["correlations"]["file"] == "clip.correlation.jsonl" and meta["correlations"]["every"] == 2
        assert meta["correlations"]["lines"] == 3 and len(meta["correlations"]["edges"]) == 17 and "diagnostics" not in meta
        assert any("clip.correlation.jsonl" in s for s in said)
    # explicit edges, together with --diagnostics: two files
    raw = tmp_path / "both" / "clip.rgb"
    args = fv.build_parser().parse_args(["--boids", "8", "--frames", "2", "--format", "raw", "-o", str(raw), "--diagnostics", "1",
                                         "--correlations", "1", "--correlation-edges", "0.5,1,2"])
    t = fv.run(args, make_flock=_CorrFlock, make_renderer=_FakeRenderer, say=quiet)
    assert t["ok"] and sorted(os.listdir(raw.parent)) == ["clip.correlation.jsonl", "clip.flock.jsonl", "clip.rgb", "clip.rgb.json"]
    assert _FakeFlock.made[-1].calls[-1][:2] == ("correlation", (0.5, 1.0, 2.0))
    meta = json.loads(raw.with_name("clip.rgb.json").read_text())
    assert meta["correlations"]["edges"] == [0.5, 1.0, 2.0] and meta["diagnostics"]["file"] == "clip.flock.jsonl"
