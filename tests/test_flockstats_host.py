"""Host side of the flock analysis (include/bdmi.h): the NumPy restatement against brute force,
the constructed cases' own claims, the bindings, boids.analysis and tools.flock_video --diagnostics with stand-ins.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import boids_cases as BC
import flockstats_cases as FC
import flockstats_ref as FR
import fof_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"bdmi_flocks": 6, "bdmi_flock_catalogue": 8, "bdmi_diagnostics": 2, "bdmi_neighbour_stats": 5}


def _small_inputs():
    rng = np.random.default_rng(0)
    th = BC.thresholds()["pos"]
    yield "thresholds_head", th[:300], 5.0
    yield "thresholds_below", th[:300], 5.0 - 2.0 ** -16
    yield "clumps", BC.R.lattice(rng.normal(0, 3.0, (250, 3)), 16), 2.0
    yield "coincident", np.zeros((7, 3)), 1.0
    yield "chain", FC.chain(200)[0]["pos"], 1.0


@pytest.mark.parametrize("name,pos,link", list(_small_inputs()), ids=[x[0] for x in _small_inputs()])
def test_restatement_agrees_with_brute_force(name, pos, link):
    a = FR.analyse(pos, link)
    lab, ng = fof_ref.fof_naive(pos, link)
    assert np.array_equal(a["labels"], lab) and a["n_flocks"] == ng
    assert a["links"] == FR.all_pairs_links(pos, link)
    n = len(pos)
    d2 = fof_ref.d2_pairs(pos, np.repeat(np.arange(n), n), np.tile(np.arange(n), n)).reshape(n, n)
    near = (d2 <= link * link) & ~np.eye(n, dtype=bool)
    assert np.array_equal(a["count"], near.sum(axis=1)) and int(a["count"].sum()) == 2 * a["links"]
    assert np.array_equal(a["nn_d2"], np.where(near, d2, np.inf).min(axis=1))


def test_equality_links_and_coincident_boids_form_one_flock():
    p = np.array([[0, 0, 0], [5, 0, 0], [5, 0, 0], [5, 3, 4 + 2.0 ** -16], [20, 0, 0]], dtype=np.float64)
    a = FR.analyse(p, 5.0)
    assert a["labels"].tolist() == [0, 0, 0, 3, 4] and a["links"] == 3 and a["n_flocks"] == 3
    assert a["count"].tolist() == [2, 2, 2, 0, 0] and a["nn_d2"].tolist() == [25.0, 0.0, 0.0, np.inf, np.inf]


def test_rows_follow_the_header():
    # four boids on a circle around the origin, flying tangentially: a perfect mill, no net heading
    p = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], dtype=np.float64)
    v = np.array([[0, 2, 0], [-2, 0, 0], [0, -2, 0], [2, 0, 0]], dtype=np.float64)
    r, smax = FR.row(p, v)
    assert r.tolist() == [4, 0, 0, 0, 0, 0, 0, 0, 2, 1, -1, -1, 0, 1, 1, 0] and smax == 2.0
    # the same boids flying one way: polarisation 1, milling 0; a boid at rest counts in m only
    r, _ = FR.row(np.concatenate([p, [[0, 0, 0]]]), np.concatenate([np.tile([0, 0, 3.0], (4, 1)), [[0, 0, 0]]]))
    assert r[0] == 5 and r[7] == 0.8 and r[8] == 2.4 and r[9] == 0.0 and r[4:7].tolist() == [0, 0, 2.4]
    assert FR.row(np.zeros((0, 3)), np.zeros((0, 3)))[0].tolist() == [0.0] * 16
    cat = FR.catalogue(np.concatenate([p, p + 50, [[9, 9, 9]]]), np.concatenate([v, v, [[1, 0, 0]]]),
                       np.array([4, 4, 4, 4, 0, 0, 0, 0, 8]), min_members=2)
    assert cat["count"] == 2 and cat["label"].tolist() == [0, 4] and cat["members"].tolist() == [4, 4]
    assert cat["rows"][0][1:4].tolist() == [50, 50, 50] and cat["rows"][1][9] == 1.0
    b = FR.row_bounds(cat["rows"][0], 2.0)
    assert b[7] == b[9] == 8 * FR.U and b[8] == 8 * FR.U and not b[list(FR.EXACT)].any()


def test_constructed_cases_are_what_they_claim():
    c, perm = FC.chain(6000)
    a = FR.analyse(c["pos"], 1.0)
    assert a["n_flocks"] == 1 and a["links"] == 5999 and set(a["count"].tolist()) == {1, 2}
    g, perm = FC.chain(6000, gap_at=3000 + 20)
    a = FR.analyse(g["pos"], 1.0)
    sizes = sorted(np.bincount(np.unique(a["labels"], return_inverse=True)[1]).tolist())
    assert a["n_flocks"] == 2 and a["links"] == 5998 and sizes == [2979, 3021]
    cells = np.unique(BC.R.cell_index(c["pos"], c["params"]))
    assert len(cells) > 3000  # through many cells
    for k in (2047, 2048, 2049):
        pc = FC.isolated_pairs(k)
        a = FR.analyse(pc["pos"], 1.0)
        m = np.bincount(np.unique(a["labels"], return_inverse=True)[1])
        assert (m == 2).sum() == k and (m == 1).sum() == 500 and a["links"] == k


def test_blobs_are_pairwise_linked():
    c = FC.blobs(sizes=(300, 301))
    a = FR.analyse(c["pos"], c["link"])
    assert a["n_flocks"] == 2 and a["links"] == 300 * 299 // 2 + 301 * 300 // 2
    full = FC.blobs()
    assert len(np.unique(full["pos"], axis=0)) == len(full["pos"]) == 4095 + 4096 + 4097 + 8193


def test_header_declares_and_table_binds_the_calls():
    import nbmi_native
    header = open(os.path.join(ROOT, "include", "bdmi.h")).read()
    lib = ctypes.CDLL(nbmi_native.LIB_PATH)
    for name, nargs in CALLS.items():
        assert f"int {name}(bdmi_flock *f" in header
        assert hasattr(lib, name)
        res, args = nbmi_native.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == nargs
    for words in ("d2(i, j) <= b2", "NOT the sweep's window", "clamped", "bytes per boid", "4096"):
        assert words in header


def test_analysis_helpers():
    from boids import analysis as A
    r = np.arange(16, dtype=np.float64)
    d = A.row_dict(r)
    assert d == {"members": 0, "center": [1, 2, 3], "velocity": [4, 5, 6], "polarisation": 7.0, "mean_speed": 8.0,
                 "milling": 9.0, "lo": [10, 11, 12], "hi": [13, 14, 15]}
    with pytest.raises(ValueError):
        A.row_dict(np.zeros(15))
    assert A.size_histogram([1, 1, 2, 3, 4, 7, 8, 4095, 4096, 1 << 40]) == {1: 2, 2: 2, 4: 2, 8: 1, 2048: 1, 4096: 1,
                                                                           1 << 40: 1}
    assert A.size_histogram([]) == {}
    with pytest.raises(ValueError):
        A.size_histogram([0])
    line = A.jsonl_line(3, 40, r, 5, 17, 2.5, np.stack([r, r + 1]), flock_labels=[0, 9], link=5.0, min_members=20,
                        qualifying=7)
    rec = json.loads(line)
    assert "\n" not in line and rec["frame"] == 3 and rec["steps"] == 40 and rec["n_flocks"] == 5 and rec["links"] == 17
    assert rec["mean_neighbours"] == 2.5 and rec["global"] == d and len(rec["flocks"]) == 2
    assert rec["flocks"][1]["label"] == 9 and rec["flocks"][1]["members"] == 1 and rec["qualifying_flocks"] == 7
    assert json.loads(A.jsonl_line(0, 0, r, 0, 0, 0.0, np.zeros((0, 16))))["flocks"] == []


class _FakeFlock:
    """What tools.flock_video needs of a Flock, with an analysis that names its arguments."""
    made = []

    def __init__(self, n, seed, device):
        self.n, self.updates, self.calls, self.closed = n, [], [], False
        _FakeFlock.made.append(self)

    def update(self, dt, substeps=1):
        self.updates.append((dt, substeps))

    def sync(self):
        pass

    def close(self):
        self.closed = True

    def flocks(self, link=None):
        self.calls.append(("flocks", link))
        return dict(labels=np.zeros(self.n, np.int32), n_flocks=3, links=11, evals=99)

    def flock_catalogue(self, link=None, min_members=1, capacity=64):
        self.calls.append(("catalogue", link, min_members, capacity))
        rows = np.zeros((2, 16))
        rows[:, 0] = (40, 25)
        return dict(count=2, label=np.array([0, 7], np.int32), members=np.array([40, 25]), rows=rows)

    def diagnostics(self):
        self.calls.append(("diagnostics",))
        r = np.zeros(16)
        r[0] = self.n
        r[7] = 0.5 + len(self.updates)
        return r

    def neighbour_stats(self, radius=None):
        self.calls.append(("neighbours", radius))
        return dict(count=np.arange(self.n, dtype=np.int32) % 4, nn_d2=np.zeros(self.n), evals=5)


class _FakeRenderer:
    def __init__(self, w, h, device):
        self.closed = False

    def render_flock(self, flock, camera, out=None):
        out[:] = 1
        return out

    def close(self):
        self.closed = True


def test_flock_video_writes_analysis_lines(tmp_path):
    from tools import flock_video as fv
    a = fv.build_parser().parse_args([])
    assert (a.diagnostics, a.link, a.min_members) == (0, None, 20)
    raw = tmp_path / "o" / "clip.rgb"
    said = []
    args = fv.build_parser().parse_args(["--boids", "8", "--frames", "7", "--format", "raw", "-o", str(raw), "--warmup", "4",
                                         "--substeps", "2", "--diagnostics", "3", "--link", "2.5", "--min-members", "9"])
    t = fv.run(args, make_flock=_FakeFlock, make_renderer=_FakeRenderer, say=said.append)
    flock = _FakeFlock.made[-1]
    path = tmp_path / "o" / "clip.flock.jsonl"
    assert t["ok"] and t["diagnostics"] == str(path) and t["diagnostics_lines"] == 3 and flock.closed
    recs = [json.loads(x) for x in path.read_text().splitlines()]
    assert [r["frame"] for r in recs] == [0, 3, 6] and [r["steps"] for r in recs] == [6, 12, 18]
    assert all(r["n_flocks"] == 3 and r["links"] == 11 and r["mean_neighbours"] == 1.5 for r in recs)
    assert [r["global"]["polarisation"] for r in recs] == [2.5, 5.5, 8.5] and recs[0]["global"]["members"] == 8
    assert [f["members"] for f in recs[0]["flocks"]] == [40, 25] and recs[0]["flocks"][1]["label"] == 7
    assert recs[0]["link"] == 2.5 and recs[0]["min_members"] == 9 and recs[0]["qualifying_flocks"] == 2
    assert flock.calls[:4] == [("flocks", 2.5), ("catalogue", 2.5, 9, 16), ("neighbours", 2.5), ("diagnostics",)]
    assert len(flock.calls) == 12
    meta = json.loads((tmp_path / "o" / "clip.rgb.json").read_text())
    assert meta["diagnostics"] == {"file": "clip.flock.jsonl", "every": 3, "link": 2.5, "min_members": 9, "lines": 3}
    assert any("clip.flock.jsonl" in s for s in said)
    # a frame directory keeps its name
    assert fv.diagnostics_path(tmp_path / "frames").name == "frames.flock.jsonl"
    with pytest.raises(ValueError):
        fv.run(fv.build_parser().parse_args(["--frames", "1", "--diagnostics", "-1"]), make_flock=_FakeFlock,
               make_renderer=_FakeRenderer, say=lambda *x: None)


def test_flock_video_without_diagnostics_makes_no_new_call(tmp_path):
    from tools import flock_video as fv
    raw = tmp_path / "clip.rgb"
    args = fv.build_parser().parse_args(["--boids", "8", "--frames", "3", "--format", "raw", "-o", str(raw)])
    t = fv.run(args, make_flock=_FakeFlock, make_renderer=_FakeRenderer, say=lambda *x: None)
    assert t["ok"] and "diagnostics" not in t and _FakeFlock.made[-1].calls == []
    assert sorted(os.listdir(tmp_path)) == ["clip.rgb", "clip.rgb.json"]
    assert "diagnostics" not in json.loads((tmp_path / "clip.rgb.json").read_text())
