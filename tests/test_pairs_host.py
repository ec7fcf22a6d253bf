"""Binned pair counts, host side: the NumPy restatement against the definition as a double loop, the derived quantities
(correlation dimension, the natural estimator of xi), the C ABI's declaration, the Python classes' refusals and the
recorder's options, metadata and pairs.jsonl with a stand-in backend (no device)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import pairs_ref as pr
from conftest import ROOT


def test_restatement_against_the_double_loop():
    rng = np.random.RandomState(0)
    for n, span, edges in ((300, 5.0, (0.0, 0.5, 1.0, 2.0, 4.0)), (257, 1e-3, (5e-5, 2e-4, 1e-3)), (64, 1e6, (1e5, 4e5)),
                           (2, 1.0, (0.1, 10.0)), (1, 1.0, (0.1, 10.0)), (0, 1.0, (0.1, 10.0))):
        p = rng.uniform(-span, span, (n, 3))
        got, want = pr.pair_counts(p, edges), pr.pair_counts_naive(p, edges)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1], (n, span)
        assert got[0].dtype == np.int64 and len(got[0]) == len(edges) - 1
    # lattice points: edges that equal occurring distances - the upper edge belongs to the bin
    # (spacing 33: no float64 squares to 2, 3 or 5, but 33^2 m has an exact root for every m used here)
    assert [pr.exact_root(m) for m in (1.0, 2.0, 3.0, 4.0, 5.0)] == [1.0, None, None, 2.0, None]
    g = 33.0 * np.arange(6, dtype=np.float64)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(216)]
    edges = np.array([pr.exact_root(1089.0 * m) for m in (1, 2, 3, 4, 5)])
    assert (edges * edges == 1089.0 * np.arange(1, 6)).all()
    got, want = pr.pair_counts(p, edges), pr.pair_counts_naive(p, edges)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    assert got[1] == 3 * 5 * 36 and got[0][0] == 3 * 2 * 25 * 6  # the axis neighbours are `below`, the face diagonals bin 0
    low = np.nextafter(edges, 0.0)
    shifted = pr.pair_counts(p, low)
    assert shifted[1] == 0 and shifted[0][0] == got[1] and shifted[0][1] == got[0][0]  # one ulp lower: every count moves up a bin
    assert np.array_equal(shifted[0], pr.pair_counts_naive(p, low)[0])
    # coincident points: with edges[0] == 0 `below` is the number of coincident pairs
    base = rng.uniform(-1.0, 1.0, (100, 3))
    p = np.concatenate([base, base, base[:10]])
    got, want = pr.pair_counts(p, (0.0, 0.5, 1.0)), pr.pair_counts_naive(p, (0.0, 0.5, 1.0))
    assert got[1] == want[1] == 90 + 3 * 10 and np.array_equal(got[0], want[0])
    # several sets in one pass, and everything is somewhere
    many = pr.pair_counts_multi(p, [(0.0, 0.5, 1.0), (0.3, 9.0)])
    assert np.array_equal(many[0][0], got[0]) and many[0][1] == got[1]
    for c, below, beyond in many:
        assert c.sum() + below + beyond == 210 * 209 // 2
    d = base[1:] - base[0]
    assert pr.nearest_d2(base)[0] == ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).min()
    assert (pr.nearest_d2(p)[:110] == 0.0).all()


def test_correlation_dimension():
    from nbody.pairs import correlation_dimension, cumulative
    edges = np.array([0.5, 1.0, 2.0, 4.0, 8.0, 16.0])
    below, counts = 3, [5, 40, 300, 2500, 20000]
    c = cumulative(below, counts)
    assert c == [3, 8, 48, 348, 2848, 22848]
    slope, used = correlation_dimension(edges, below, counts)
    want = np.polyfit(np.log(edges[1:]), np.log(np.array(c[1:], dtype=np.float64)), 1)[0]
    assert used == 5 and abs(slope - want) <= 1e-12
    slope, used = correlation_dimension(edges, below, counts, lo=2.0, hi=8.0)
    want = np.polyfit(np.log(edges[2:5]), np.log(np.array(c[2:5], dtype=np.float64)), 1)[0]
    assert used == 3 and abs(slope - want) <= 1e-12
    # edges without a pair within them are left out (C > 0), the first edge always is
    slope, used = correlation_dimension([1.0, 2.0, 4.0, 8.0], 0, [0, 7, 21])
    assert used == 2 and abs(slope - np.log(28.0 / 7.0) / np.log(2.0)) <= 1e-12
    for args in (([1.0, 2.0], 5, [7]), ([1.0, 2.0, 4.0], 0, [0, 9]), ([1.0, 2.0, 4.0, 8.0], 1, [1, 1], ),
                 ([0.5, 1.0, 2.0, 4.0], 3, [5, 40, 300], 3.0, 5.0)):
        with pytest.raises(ValueError):
            correlation_dimension(*args)


def test_correlation_dimension_of_a_line():
    """4 096 points at unit spacing on a line: C(r) = sum over d <= r of (n - d), whose slope against r is at least
    1 - r / (2 n) >= 0.97 up to r = 256"""
    from nbody.pairs import correlation_dimension
    n = 4096
    p = np.zeros((n, 3))
    p[:, 0] = np.arange(n)
    edges = 2.0 ** np.arange(2, 9)
    counts, below = pr.pair_counts(p, edges)
    c = [sum(n - d for d in range(1, int(r) + 1)) for r in edges]
    assert below == c[0] and (np.cumsum(counts) + below).tolist() == c[1:]
    slope, used = correlation_dimension(edges, below, counts)
    print(f"line of {n}: D2 = {slope:.4f} over {used} edges")
    assert used == 6 and 0.9 < slope < 1.1


def test_xi_natural():
    from nbody.pairs import xi_natural
    xi = xi_natural([10, 0, 6, 5], [5, 4, 0, 10], 11, 21)
    norm = 21.0 * 20.0 / (11.0 * 10.0)
    assert xi.dtype == np.float64 and np.isnan(xi[2])
    assert xi[0] == 2.0 * norm - 1.0 and xi[1] == -1.0 and xi[3] == 0.5 * norm - 1.0
    assert xi_natural([4], [4], 7, 7)[0] == 0.0  # the data are the randoms
    assert np.isnan(xi_natural([0], [0], 5, 5)[0])


def test_check_edges_and_auto_edges():
    from nbody.pairs import AUTO_EDGES, auto_pair_edges, check_edges
    assert check_edges([0, 1, 2]).dtype == np.float64
    for bad in ([1.0], [], [1.0, 1.0], [2.0, 1.0], [-1.0, 1.0], [0.0, np.inf], [0.0, np.nan], list(range(67)),
                [1e-200, 2e-200], [1e200, 1e201]):  # (squares that collide at 0, squares that overflow)
        with pytest.raises(ValueError):
            check_edges(bad)
    assert len(check_edges(np.arange(65.0))) == 65
    r2 = np.arange(1, 1002, dtype=np.float64) ** 2  # nearest-neighbour distances 1 .. 1001: the median is 501
    e = auto_pair_edges(r2)
    assert len(e) == AUTO_EDGES == 13 and e[0] == 0.5 * 501.0 and e[12] == 0.5 * 501.0 * 64.0 and e[2] == 501.0
    assert np.allclose(np.diff(np.log2(e)), 0.5)
    with pytest.raises(ValueError, match="median nearest-neighbour"):
        auto_pair_edges(np.zeros(5))


def test_header_declares_and_library_exports_the_call():
    import nbmi_native
    text = open(os.path.join(ROOT, "include", "nbmi.h")).read()
    assert re.search(r"^int nbmi_pair_counts\(nbmi_sim \*sim, int nb, const double \*edges,", text, re.M)
    assert len(nbmi_native.PROTOTYPES["nbmi_pair_counts"][1]) == 7
    assert hasattr(ctypes.CDLL(nbmi_native.LIB_PATH), "nbmi_pair_counts")
    for word in ("NBMI_PAIRS_CELLS", "cell_pairs", "The first call allocates 4 bytes per node row"):
        assert word in text


def test_python_classes_refuse_without_a_device():
    from nbody.gpu_backend import HIPDirectSimulation, HIPOwnerSimulation
    for cls, word in ((HIPDirectSimulation, "direct"), (HIPOwnerSimulation, "owner")):
        sim = cls.__new__(cls)  # no handle: the refusal must come before any library call
        sim._h = None
        for call in (lambda: sim.pair_counts([1.0, 2.0]), lambda: sim.pair_counts([1.0, 2.0], evals=True),
                     lambda: sim.correlation_function([1.0, 2.0], np.zeros((5, 3)))):
            with pytest.raises(ValueError, match=word):
                call()


# ---- the recorder ----------------------------------------------------------------------------------------------------
def _args(*extra):
    from tools import record as rec
    return rec.build_parser().parse_args(["--preset", "quick_galaxy", *extra])


def test_recorder_options():
    from tools import record as rec
    assert "pairs" not in rec.build_config(_args())  # the default writes no key
    assert rec.pairs_config({}) is None
    cfg = rec.build_config(_args("--pairs", "5"))
    assert cfg["pairs"] == {"every": 5, "edges": "auto"} and rec.pairs_config(cfg) == (5, None)
    assert rec.build_config(_args("--pairs", "5", "--pair-edges", "AUTO"))["pairs"]["edges"] == "auto"
    cfg = rec.build_config(_args("--pairs", "2", "--pair-edges", "0,1.5,3,6"))
    assert cfg["pairs"] == {"every": 2, "edges": [0.0, 1.5, 3.0, 6.0]} and rec.pairs_config(cfg) == (2, [0.0, 1.5, 3.0, 6.0])
    assert rec.build_config(_args("--pairs", "2", "--groups", "3"))["groups"]["every"] == 3
    for bad, word in ((("--pair-edges", "1,2"), "needs --pairs"), (("--pair-edges", "auto"), "needs --pairs"),
                      (("--pairs", "0"), "--pairs"), (("--pairs", "-2"), "--pairs"),
                      (("--pairs", "2", "--pair-edges", "1"), "--pair-edges"),
                      (("--pairs", "2", "--pair-edges", "2,1"), "--pair-edges"),
                      (("--pairs", "2", "--pair-edges", "1,1"), "--pair-edges"),
                      (("--pairs", "2", "--pair-edges=-1,1"), "--pair-edges"),
                      (("--pairs", "2", "--pair-edges", "1,inf"), "--pair-edges"),
                      (("--pairs", "2", "--pair-edges", "1,nan"), "--pair-edges"),
                      (("--pairs", "2", "--pair-edges", "1,wide"), "--pair-edges"),
                      (("--pairs", "2", "--pair-edges", ",".join(str(k) for k in range(67))), "--pair-edges")):
        with pytest.raises(ValueError, match=word):
            rec.build_config(_args(*bad))
    with pytest.raises(ValueError, match="--pair-edges"):
        rec.pairs_config({"pairs": {"every": 2, "edges": [3.0, 2.0]}})


class FakeSim:
    """knn / pair_counts of the backend object: nearest-neighbour distances 1 .. n, counts that grow as r^2"""

    def __init__(self, n=1001):
        self.n = n
        self.r2 = np.arange(1, n + 1, dtype=np.float64) ** 2
        self.calls = []

    def knn(self, k, evals=False):
        self.calls.append(("knn", k))
        return self.r2.copy(), np.ones(self.n)

    def pair_counts(self, edges, evals=False):
        self.calls.append(("pair_counts", [float(e) for e in edges]))
        c = [int(round(e * e)) for e in edges]  # C(e) = e^2
        return np.array([b - a for a, b in zip(c[:-1], c[1:])], dtype=np.int64), c[0]


def test_recorder_metadata_round_trip_line_and_status(tmp_path, capsys):
    from tools import record as rec
    cfg = rec.build_config(_args("--pairs", "4"))
    d = rec.get_recording_dir("prs", tmp_path)
    rec.save_metadata(d, cfg, 0.0)
    sim = FakeSim()
    out = rec.apply_pairs(sim, cfg, d)
    want = [0.5 * 501.0 * 2.0 ** (k / 2.0) for k in range(13)]
    assert out["pairs"] == {"every": 4, "edges": want} and sim.calls == [("knn", 1)]
    meta = rec.load_metadata(d)
    assert meta["pairs"] == out["pairs"] and meta["start_time"] == 0.0 and meta["num_bodies"] == cfg["num_bodies"]
    # --resume / --extend: the edges come from metadata.json, the state is not asked again
    again = FakeSim()
    again.r2 *= 9.0
    assert rec.apply_pairs(again, meta, d)["pairs"] == meta["pairs"] and again.calls == []
    assert rec.load_metadata(d) == meta
    # given edges are used as given; a session without pairs touches nothing
    given = FakeSim()
    assert rec.apply_pairs(given, rec.build_config(_args("--pairs", "1", "--pair-edges", "1,2,4")), None)["pairs"]["edges"] == [1.0, 2.0, 4.0]
    assert rec.apply_pairs(given, rec.build_config(_args()), None) == rec.build_config(_args()) and given.calls == []
    flat = FakeSim()
    flat.r2[:] = 0.0
    with pytest.raises(ValueError, match="median nearest-neighbour"):
        rec.apply_pairs(flat, cfg, None)
    # the line
    edges = [1.0, 2.0, 4.0, 8.0]
    line = rec.pairs_line(sim, 7, edges)
    assert line.endswith("\n") and sim.calls[1:] == [("pair_counts", edges)]
    row = json.loads(line)
    assert sorted(row) == ["below", "counts", "d2", "d2_points", "edges", "frame"]
    assert row["frame"] == 7 and row["edges"] == edges and row["below"] == 1 and row["counts"] == [3, 12, 48]
    assert abs(row["d2"] - 2.0) <= 1e-12 and row["d2_points"] == 3
    empty = json.loads(rec.pairs_line(sim, 8, [0.1, 0.2]))  # C = 0 everywhere: no dimension
    assert empty["d2"] is None and empty["d2_points"] == 0 and empty["counts"] == [0] and empty["below"] == 0
    # --status: the last line's dimension and the pairs within the last edge
    rec.append_line(d / rec.PAIRS_FILE, line)
    capsys.readouterr()
    assert rec.show_status("prs", root=tmp_path)
    text = capsys.readouterr().out
    assert f"Pairs: every 4 frames, 12 bins from {want[0]:.6g} to {want[-1]:.6g}" in text
    assert "frame 7: D2 = 2.000 over 3 edges, 64 pairs within 8" in text
    rec.save_metadata(rec.get_recording_dir("plain", tmp_path), rec.build_config(_args()), 0.0)
    assert rec.show_status("plain", root=tmp_path) and "Pairs" not in capsys.readouterr().out
    rec.save_metadata(rec.get_recording_dir("untaken", tmp_path), cfg, 0.0)
    assert rec.show_status("untaken", root=tmp_path) and "edges auto (not taken yet)" in capsys.readouterr().out


def test_pairs_file_truncation_on_resume(tmp_path):
    from tools import record as rec
    path = tmp_path / rec.PAIRS_FILE
    sim = FakeSim()
    for frame in (1, 3, 5, 7):
        rec.append_line(path, rec.pairs_line(sim, frame, [1.0, 2.0]))
    with open(path, "a") as f:
        f.write('{"frame": 9, "edges": [1.0, 2.')  # a killed process left a torn line
    assert [r["frame"] for r in rec.read_diagnostics(path)] == [1, 3, 5, 7]
    before = path.read_text().splitlines(keepends=True)
    kept = rec.truncate_diagnostics(path, 4)  # a resume after the checkpoint of frame 4
    assert [r["frame"] for r in kept] == [1, 3] and path.read_text() == "".join(before[:2])
    rec.append_line(path, rec.pairs_line(sim, 5, [1.0, 2.0]))
    assert [r["frame"] for r in rec.read_diagnostics(path)] == [1, 3, 5] and path.read_text() == "".join(before[:3])


def test_pipelined_loop_finishes_the_frame_before_a_line_of_either_period(tmp_path):
    """record_pipelined with a predicate over two periods (groups and pairs): the writer is called where either is due,
    after the frame's file; one period alone and none work too"""
    from tools import record as rec
    import test_record_pipeline_host as tp
    for also, want in (((3, 2), [1, 2, 3, 5]), ((0, 2), [1, 3, 5]), (3, [2, 5]), ((0, 0), [])):
        d = rec.get_recording_dir(f"piped{also}", tmp_path)
        sim = tp.FakeSim(rec)
        seen = []

        def write_lines(frame):
            assert any(q.exists() for q in rec._frame_paths(d, frame)) and not sim.frames_pending()
            seen.append(frame)
        periods = also if isinstance(also, tuple) else (also,)
        rec.record_pipelined(sim, d, 0, 7, 2, 0.01, False, lambda frame: any(rec.line_due(frame, k) for k in periods),
                             write_lines, lambda frame, compressed=False: None)
        assert seen == want and not sim.slots and rec.get_completed_frames(d) == 7
