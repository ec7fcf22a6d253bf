"""The restatement of the flock analysis on periodic handles (tests/torus_ref.py) against scalar loops and rows written
out by hand, the cases of tests/torus_cases.py against what their names say, the bindings of the three new calls, and
boids.analysis / tools.flock_video --periodic-flocks with stand-ins.  No GPU.
"""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

import boids_ref as R
import periodic_ref as PR
import torus_cases as TC
import torus_ref as TR
from conftest import ROOT
from test_flockstats_host import _FakeFlock, _FakeRenderer


# ---- the distance ------------------------------------------------------------------------------------------------------
def _scalar_d2(p, q, B, L):
    t = []
    for a in range(3):
        d = float(q[a]) - float(p[a])
        if d > B:
            d = d - L
        elif d < -B:
            d = d + L
        t.append(d * d)
    return (t[0] + t[1]) + t[2]


@pytest.mark.parametrize("kind", ["face", "edge", "corner"])
def test_d2_is_symmetric_bit_for_bit(kind):
    """Off the lattice, where the differences round: pairs on either side of a face, an edge and a corner."""
    B, L = 10.0, 20.0
    rng = np.random.default_rng({"face": 1, "edge": 2, "corner": 3}[kind])
    axes = {"face": 1, "edge": 2, "corner": 3}[kind]
    n = 400
    a, b = rng.uniform(-B, B, (n, 3)), rng.uniform(-B, B, (n, 3))
    a[:, :axes] = B - rng.uniform(0, 2.5, (n, axes))
    b[:, :axes] = -B + rng.uniform(0, 2.5, (n, axes))
    pos = np.concatenate([a, b])
    i, j = np.arange(n), np.arange(n) + n
    fwd, back = TR.d2_pairs(pos, i, j, B, L), TR.d2_pairs(pos, j, i, B, L)
    assert R.same_bits(fwd, back)
    assert all(fwd[k] == _scalar_d2(pos[k], pos[k + n], B, L) == _scalar_d2(pos[k + n], pos[k], B, L) for k in range(n))
    shifted = np.abs(pos[j] - pos[i]) > B
    assert shifted[:, :axes].all() and (np.abs(TR.diff_pairs(pos, i, j, B, L)) <= [5.0] * axes + [B] * (3 - axes)).all()
    # the constructed pairs of the GPU test: linked through the face, the edge, the corner
    c = TC.through(kind)
    got = TR.analyse(c["pos"], c["params"], c["link"])
    assert got["links"] == 1 and got["n_flocks"] == 1 and (np.abs(c["pos"][1] - c["pos"][0]) > 10.0).sum() == axes


def test_face_pair_at_the_link_and_just_below():
    c = TC.face_pair()
    B, L, dim, _ = PR.box(c["params"])
    assert (B, L, dim) == (7.5, 15.0, 3)
    d = TR.diff_pairs(c["pos"], np.array([0, 1, 2, 3]), np.array([1, 0, 3, 2]), B, L)
    assert d[0].tolist() == [1.0, 0.0, 0.0] and d[1].tolist() == [-1.0, 0.0, 0.0]  # -14 + 15 and 14 - 15
    assert d[2].tolist() == [-7.5, 0.0, 0.0] and d[3].tolist() == [7.5, 0.0, 0.0]  # |dx| == B: equality does not shift
    at = TR.analyse(c["pos"], c["params"], 1.0)
    assert at["links"] == 1 and at["labels"].tolist() == [0, 0, 2, 3] and at["nn_d2"][:2].tolist() == [1.0, 1.0]
    below = TR.analyse(c["pos"], c["params"], np.nextafter(1.0, 0.0))
    assert below["links"] == 0 and below["labels"].tolist() == [0, 1, 2, 3] and np.isinf(below["nn_d2"]).all()


# ---- the restatement against scalar loops ------------------------------------------------------------------------------
def _scalar_analysis(pos, params, link):
    B, L, dim, cell = PR.box(params)
    n = len(pos)
    b2 = link * link
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    count, nn, links, evals = [0] * n, [math.inf] * n, 0, 0
    cc = [[min(max(int((float(x) + B) / cell), 0), dim - 1) for x in p] for p in pos]
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            if all((cc[i][a] - cc[j][a]) % dim in (0, 1, dim - 1) for a in range(3)):
                evals += 1
            d2 = _scalar_d2(pos[i], pos[j], B, L)
            if d2 <= b2:
                count[i] += 1
                nn[i] = min(nn[i], d2)
                if i < j:
                    links += 1
                    a, b = find(i), find(j)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    return dict(labels=[find(i) for i in range(n)], links=links, count=count, nn_d2=nn, evals=evals // 2, nb_evals=evals)


@pytest.mark.parametrize("case", [TC.sizes(0), TC.sizes(1), TC.sizes(2), TC.sizes(255), TC.chain(), TC.chain((2, 3)),
                                  TC.face_blob(+1), TC.crowded_cell()], ids=lambda c: c["name"])
def test_analyse_against_scalar_loops(case):
    got = TR.analyse(case["pos"], case["params"], case["link"])
    want = _scalar_analysis(case["pos"], case["params"], case["link"])
    assert got["labels"].tolist() == want["labels"] and got["n_flocks"] == len(set(want["labels"]))
    assert (got["links"], got["evals"], got["nb_evals"]) == (want["links"], want["evals"], want["nb_evals"])
    assert got["count"].tolist() == want["count"] and R.same_bits(got["nn_d2"], np.array(want["nn_d2"], dtype=np.float64))
    assert int(got["count"].sum()) == 2 * got["links"]


def _scalar_ordered_sum(vals):
    """The header's order for one column, one float at a time."""
    total = None
    for c0 in range(0, len(vals), 4096):
        chunk = vals[c0:c0 + 4096]
        acc = [0.0] * 256
        for k, v in enumerate(chunk):
            acc[k % 256] = acc[k % 256] + float(v)
        waves = []
        for w in range(4):
            lane = acc[64 * w:64 * w + 64]
            o = 32
            while o:
                lane = [lane[x] + lane[x ^ o] for x in range(64)]
                o >>= 1
            waves.append(lane[0])
        part = ((waves[0] + waves[1]) + waves[2]) + waves[3]
        total = part if total is None else total + part
    return total


def test_ordered_sum_is_the_header_order():
    rng = np.random.default_rng(12)
    for m in (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 9000):
        t = rng.normal(0, 1, (m, 2)) * 10.0 ** rng.integers(-6, 6, (m, 2))
        got = TR.ordered_sum(t)
        assert [float(x).hex() for x in got] == [_scalar_ordered_sum(t[:, k]).hex() for k in range(2)], m
    assert TR.ordered_sum(t)[0] != math.fsum(t[:, 0])  # (this seed's 9 000 terms:) an order, not the exactly rounded sum


# ---- rows by hand ------------------------------------------------------------------------------------------------------
def test_wrap_of():
    assert TR.wrap_of([0, 1, 2, 3], 4) == -1
    assert TR.wrap_of([3, 0], 4) == 3 and TR.wrap_of([0, 2], 3) == 2 and TR.wrap_of([0], 3) == 0
    assert TR.wrap_of([1, 2], 4) == 1 and TR.wrap_of([0, 1, 3], 4) == 3 and TR.wrap_of([0, 2], 4) == 0
    assert TR.wrap_of([5, 6, 40, 41, 0], 42) == 5  # the smallest start, whatever the arcs


def test_pair_through_the_face_by_hand():
    c = TC.face_pair()
    vel = np.array([[3.0, 0.0, 4.0], [0.0, 5.0, 0.0]])
    row, wrap = TR.row(c["pos"][:2], vel, c["params"])
    # cells: x = 7 -> int(14.5 / 5) = 2, x = -7 -> 0: O_x = {0, 2}, the cut is 2 (its predecessor 1 is free): -7 -> 8
    assert wrap.tolist() == [2, 1, 1]
    assert row[0] == 2.0 and row[1:4].tolist() == [7.5, 1.0, 1.0]  # (7 + 8) / 2 = 7.5 == B: not brought back
    assert row[10:13].tolist() == [7.0, 1.0, 1.0] and row[13:16].tolist() == [8.0, 1.0, 1.0]
    assert row[4:7].tolist() == [1.5, 2.5, 2.0] and row[8] == 5.0
    su = np.array([0.6 + 0.0, 0.0 + 1.0, 0.8 + 0.0])
    assert row[7] == math.sqrt((su[0] * su[0] + su[1] * su[1]) + su[2] * su[2]) / 2.0
    # r = (-0.5, 0, 0) and (0.5, 0, 0): rhat = (-1, 0, 0), (1, 0, 0); w = rhat x u = (0, 0.8, -0.0) + (0, -0.0, 1)
    w = np.array([0.0, 0.8, 1.0])
    assert row[9] == math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) / 2.0


def _exact_row_fields(c, ids, shift):
    """c~, lo, hi of the members `ids` with `shift` (m, 3) added: exact on the lattice, so any order gives these bits."""
    y = c["pos"][ids] + shift
    ct = np.array([math.fsum(y[:, a]) for a in range(3)]) / float(len(ids))
    return ct, y.min(axis=0), y.max(axis=0)


@pytest.mark.parametrize("heavy", [+1, -1])
def test_blob_across_the_face(heavy):
    c = TC.face_blob(heavy)
    B, L, dim, _ = PR.box(c["params"])
    got = TR.analyse(c["pos"], c["params"], c["link"])
    assert got["n_flocks"] == 1 and got["links"] == 300 * 299 // 2
    cat = TR.catalogue(c["pos"], c["vel"], got["labels"], c["params"])
    assert cat["count"] == 1 and cat["members"].tolist() == [300]
    assert cat["wrap"][0].tolist() == [dim - 1, 1, 1]
    ids = cat["idx"][0]
    shift = np.zeros((300, 3))
    shift[c["pos"][ids, 0] < 0, 0] = L  # by hand: the members beyond the face come back next to the others
    ct, lo, hi = _exact_row_fields(c, ids, shift)
    row = cat["rows"][0]
    assert (ct[0] > B) == (heavy > 0)  # the heavy side decides where the unwrapped centre lies
    assert row[1] == (ct[0] - L if ct[0] > B else ct[0]) and row[2:4].tolist() == ct[1:].tolist()
    assert R.same_bits(row[10:13], lo) and R.same_bits(row[13:16], hi)
    assert row[13] > B and row[13] - row[10] <= 2.5 and abs(row[1]) >= B - 1.25


def test_blob_round_the_corner():
    c = TC.corner_blob()
    B, L, dim, _ = PR.box(c["params"])
    got = TR.analyse(c["pos"], c["params"], c["link"])
    cat = TR.catalogue(c["pos"], c["vel"], got["labels"], c["params"])
    assert got["n_flocks"] == 1 and cat["wrap"][0].tolist() == [dim - 1] * 3
    ids = cat["idx"][0]
    ct, lo, hi = _exact_row_fields(c, ids, np.where(c["pos"][ids] < 0, L, 0.0))
    row = cat["rows"][0]
    assert R.same_bits(row[1:4], np.where(ct > B, ct - L, ct)) and R.same_bits(row[10:13], lo) and R.same_bits(row[13:16], hi)
    assert (hi > B).all() and (hi - lo <= 2.5).all()


def test_single_boid():
    c = TC.single()
    got = TR.analyse(c["pos"], c["params"], c["link"])
    assert got["labels"].tolist() == [0] and (got["links"], got["evals"], got["count"].tolist()) == (0, 0, [0])
    cat = TR.catalogue(c["pos"], c["vel"], got["labels"], c["params"])
    assert cat["wrap"][0].tolist() == PR.cell_coords(c["pos"], c["params"])[0].tolist() == [3, 1, 2]
    row = cat["rows"][0]
    assert row[0] == 1 and row[1:4].tolist() == c["pos"][0].tolist() == row[10:13].tolist() == row[13:16].tolist()
    assert row[7] == 1.0 and row[9] == 0.0 and R.same_bits(row[4:7], c["vel"][0])


def test_chain_spans_and_so_does_the_c():
    """The ring along x spans x; the C (two boids taken out, a gap of 3 > link) is one open flock that still has a member
    in every x slab: it spans as well.  The rule is conservative, and this pins it."""
    for gap, members in (((), 20), ((2, 3), 18)):
        c = TC.chain(gap)
        got = TR.analyse(c["pos"], c["params"], c["link"])
        assert got["n_flocks"] == 1 and got["links"] == (20 if not gap else 17)
        cat = TR.catalogue(c["pos"], c["vel"], got["labels"], c["params"])
        assert cat["members"].tolist() == [members]
        cy, cz = PR.cell_coords(c["pos"], c["params"])[0, 1:]
        assert cat["wrap"][0].tolist() == [-1, cy, cz]
        row = cat["rows"][0]
        assert (row[10], row[13]) == (-10.0, 9.0)  # taken as they stand
        assert row[1] == math.fsum(c["pos"][:, 0]) / members
    open_chain = TC.chain((2, 3, 4, 5, 6))  # slab [5, 10) still has 7, 8, 9 ...
    assert TR.catalogue(open_chain["pos"], open_chain["vel"], np.zeros(15, np.int32), open_chain["params"])["wrap"][0, 0] == -1
    short = TC.chain((0, 1, 2, 3, 4))  # ... slab [0, 5) is now empty: cut at 5, the members below come behind
    got = TR.analyse(short["pos"], short["params"], 1.0)
    cat = TR.catalogue(short["pos"], short["vel"], got["labels"], short["params"])
    assert got["n_flocks"] == 1 and cat["wrap"][0, 0] == 3 and (cat["rows"][0, 10], cat["rows"][0, 13]) == (5.0, 19.0)


def test_catalogue_order_and_member_order():
    c = TC.mixed()
    got = TR.analyse(c["pos"], c["params"], c["link"])
    cat = TR.catalogue(c["pos"], c["vel"], got["labels"], c["params"], min_members=2)
    m = cat["members"]
    assert cat["count"] > 50 and (m >= 2).all() and (np.diff(m) <= 0).all()
    ties = np.flatnonzero(np.diff(m) == 0)
    assert len(ties) and (np.diff(cat["label"])[ties] > 0).all()
    # near the percolation threshold: the largest flock spans, most do not, several reach through a face
    assert (cat["wrap"][0] == -1).all() and (cat["wrap"][5:] >= 0).all() and (cat["rows"][5:, 13:16] > 18.75).any()
    cells = PR.cell_index(c["pos"], c["params"])
    for ids, lab in zip(cat["idx"][:5], cat["label"][:5]):
        assert (got["labels"][ids] == lab).all() and ids.min() == lab
        key = cells[ids] * len(cells) + ids
        assert (np.diff(key) > 0).all()  # by cell, then by row


# ---- bindings ----------------------------------------------------------------------------------------------------------
NEW_CALLS = {"bdmi_periodic_flocks": 6, "bdmi_periodic_flock_catalogue": 9, "bdmi_periodic_neighbour_stats": 5}


def test_header_declares_and_table_binds_the_calls():
    import nbmi_native
    text = open(os.path.join(ROOT, "include", "bdmi.h")).read()
    lib = ctypes.CDLL(nbmi_native.LIB_PATH)
    for name, arity in NEW_CALLS.items():
        m = re.search(r"\b" + name + r"\(([^;]*)\);", text)
        assert m, name
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == arity == len(nbmi_native.PROTOTYPES[name][1]), name
        getattr(lib, name)
    for phrase in ("acts on the DIFFERENCE", "may differ in the last bit", "|O_a| == dim", "necessary for a flock that winds",
                   "(c - 1 + dim) mod dim", "c~_a - L if c~_a > B", "r_j = y_j - c~", "hi may exceed B",
                   "12 * ceil(dim / 32) bytes"):
        assert phrase in text, phrase


# ---- boids.analysis ----------------------------------------------------------------------------------------------------
def test_percolation_summary_and_spans_in_the_line():
    from boids.analysis import jsonl_line, percolation_summary
    cat = dict(members=np.array([600, 30, 5]), spans=np.array([[True, False, False], [False, False, False], [False, True, True]]))
    assert percolation_summary(cat, 1000) == {"largest_fraction": 0.6, "spanning_flocks": 2, "largest_spans": [True, False, False]}
    empty = dict(members=np.zeros(0, np.int64), spans=np.zeros((0, 3), bool))
    assert percolation_summary(empty, 0) == {"largest_fraction": 0.0, "spanning_flocks": 0, "largest_spans": [False] * 3}
    with pytest.raises(ValueError):
        percolation_summary(cat, 500)
    with pytest.raises(ValueError):
        percolation_summary(dict(members=cat["members"], spans=cat["spans"][:2]), 1000)
    rows = np.zeros((3, 16))
    rows[:, 0] = cat["members"]
    rec = json.loads(jsonl_line(1, 2, np.zeros(16), 3, 4, 1.5, rows, flock_spans=cat["spans"], periodic=True))
    assert [f["spans"] for f in rec["flocks"]] == cat["spans"].tolist() and rec["periodic"] is True
    rec = json.loads(jsonl_line(1, 2, np.zeros(16), 3, 4, 1.5, rows))
    assert all("spans" not in f for f in rec["flocks"]) and "periodic" not in rec
    with pytest.raises(ValueError):
        jsonl_line(1, 2, np.zeros(16), 3, 4, 1.5, rows, flock_spans=cat["spans"][:2])


# ---- tools.flock_video --periodic-flocks -------------------------------------------------------------------------------
class _TorusFlock(_FakeFlock):
    def __init__(self, n, seed, device, periodic=False):
        super().__init__(n, seed, device)
        self.periodic = periodic

    def flocks(self, link=None):
        raise AssertionError("the walled flock finder on a periodic flock")

    flock_catalogue = neighbour_stats = flocks

    def periodic_flocks(self, link=None):
        self.calls.append(("periodic_flocks", link))
        return dict(labels=np.zeros(self.n, np.int32), n_flocks=5, links=13, evals=99)

    def periodic_flock_catalogue(self, link=None, min_members=1, capacity=64):
        self.calls.append(("periodic_catalogue", link, min_members, capacity))
        rows = np.zeros((2, 16))
        rows[:, 0] = (40, 25)
        wrap = np.array([[-1, 2, 0], [3, 3, 1]], np.int32)
        return dict(count=2, label=np.array([0, 7], np.int32), members=np.array([40, 25]), rows=rows, wrap=wrap,
                    spans=wrap == -1)

    def periodic_neighbour_stats(self, radius=None):
        self.calls.append(("periodic_neighbours", radius))
        return dict(count=np.arange(self.n, dtype=np.int32) % 4, nn_d2=np.zeros(self.n), evals=5)


def test_flock_video_periodic_flocks(tmp_path):
    import tools.flock_video as fv
    out = tmp_path / "clip.rgb"
    args = fv.build_parser().parse_args(["--boids", "64", "--frames", "4", "--format", "raw", "--diagnostics", "2", "--link", "2.5",
                                         "--min-members", "9", "--periodic", "--periodic-flocks", "-o", str(out)])
    t = fv.run(args, make_flock=_TorusFlock, make_renderer=_FakeRenderer, say=lambda *x: None)
    assert t["ok"]
    flock = _FakeFlock.made[-1]
    assert flock.periodic and flock.calls[:4] == [("periodic_flocks", 2.5), ("periodic_catalogue", 2.5, 9, 16),
                                                  ("periodic_neighbours", 2.5), ("diagnostics",)]
    lines = [json.loads(l) for l in open(t["diagnostics"])]
    assert len(lines) == 2
    for l in lines:  # the full line of a walled run, plus spans
        assert l["periodic"] is True and l["n_flocks"] == 5 and l["links"] == 13 and l["mean_neighbours"] == 1.5
        assert l["qualifying_flocks"] == 2 and "global" in l
        assert [f["members"] for f in l["flocks"]] == [40, 25] and [f["label"] for f in l["flocks"]] == [0, 7]
        assert [f["spans"] for f in l["flocks"]] == [[True, False, False], [False, False, False]]
    assert json.loads((tmp_path / "clip.rgb.json").read_text())["flock"]["periodic_flocks"] is True
    with pytest.raises(ValueError, match="--periodic-flocks needs --periodic"):
        fv.run(fv.build_parser().parse_args(["--frames", "1", "--periodic-flocks"]), make_flock=_TorusFlock,
               make_renderer=_FakeRenderer, say=lambda *x: None)
    assert "--periodic-flocks" in fv.build_parser().format_help() and "--periodic-flocks" in fv.__doc__
