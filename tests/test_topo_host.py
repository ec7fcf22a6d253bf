"""Host side of the topological interaction (include/bdmi.h): the NumPy restatement
(tests/topo_ref.py) against a plain triple-loop brute force and against rows written out by hand, its agreement with
the metric reference where k covers every neighbour, the bindings, tools.flock_video's flags with stand-ins and
boids.analysis.neighbour_rank_profile.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import boids_cases as BC
import boids_ref as R
import topo_ref as T
from test_flockstats_host import _FakeFlock, _FakeRenderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"bdmi_set_neighbour_mode": 3, "bdmi_get_neighbour_mode": 3, "bdmi_topological_neighbours": 5}
K = 7


def _state(pos, seed=0):
    rng = np.random.default_rng(seed)
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    return pos, R.lattice(rng.uniform(-12.5, 12.5, pos.shape), BC.VB), R.id_colours(len(pos))


def brute(pos, vel, col, prm, k):
    """The header, loop by loop: the rows (ids, d2, count) and the four force arrays."""
    P = R.unpack(prm)
    n = len(pos)
    ps, ss = P["perception_radius"] ** 2, P["separation_radius"] ** 2
    ids = np.full((n, k), -1, dtype=np.int32)
    d2o = np.full((n, k), np.inf)
    count = np.zeros(n, dtype=np.int32)
    out = [np.zeros((n, 3)) for _ in range(3)] + [np.array(col, dtype=np.float64)]

    def steer(x, v, w):
        mag = math.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
        if not mag > 0:
            return [0.0, 0.0, 0.0]
        y = [(x[c] / mag) * P["max_speed"] - v[c] for c in range(3)]
        m2 = math.sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2])
        if m2 > P["max_force"]:
            y = [(y[c] / m2) * P["max_force"] for c in range(3)]
        return [y[c] * w for c in range(3)]

    for i in range(n):
        found = []
        for j in range(n):
            if j == i:
                continue
            dx, dy, dz = (float(pos[i, c]) - float(pos[j, c]) for c in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            if 0.0001 < d2 < ps:
                found.append((d2, j))
        found.sort()
        found = found[:k]
        count[i] = len(found)
        s, a, q, cl = ([0.0, 0.0, 0.0] for _ in range(4))
        nsep = 0
        for rank, (d2, j) in enumerate(found):
            ids[i, rank], d2o[i, rank] = j, d2
            if d2 < ss:
                dist = math.sqrt(d2)
                inv = 1.0 / dist
                for c in range(3):
                    s[c] += (float(pos[i, c]) - float(pos[j, c])) * inv / dist
                nsep += 1
            for c in range(3):
                a[c] += float(vel[j, c])
                q[c] += float(pos[j, c])
                cl[c] += float(col[j, c])
        v = [float(x) for x in vel[i]]
        if nsep:
            out[0][i] = steer([s[c] / nsep for c in range(3)], v, P["separation_weight"])
        m = len(found)
        if m:
            out[1][i] = steer([a[c] / m for c in range(3)], v, P["alignment_weight"])
            out[2][i] = steer([q[c] / m - float(pos[i, c]) for c in range(3)], v, P["cohesion_weight"])
            out[3][i] = [(cl[c] + float(col[i, c])) / (m + 1) for c in range(3)]
    return ids, d2o, count, out


def _small_inputs():
    rng = np.random.default_rng(0)
    yield "thresholds_head", BC.thresholds()["pos"][:300], K
    yield "clumps", R.lattice(rng.normal(0, 3.0, (250, 3)), 16), K
    yield "clumps_k16", R.lattice(rng.normal(0, 2.0, (250, 3)), 16), 16
    yield "coincident", np.zeros((7, 3)), K
    for n in (1, 2, K, K + 1):
        yield f"n_{n}", R.lattice(rng.normal(0, 1.5, (n, 3)), 16), K


@pytest.mark.parametrize("name,pos,k", list(_small_inputs()), ids=[x[0] for x in _small_inputs()])
def test_restatement_agrees_with_brute_force(name, pos, k):
    prm = BC.params(bounds=100.0)
    pos, vel, col = _state(pos)
    ids, d2, count, forces = brute(pos, vel, col, prm, k)
    F = T.flocking(pos, vel, col, prm, k)
    assert np.array_equal(F.rows["ids"], ids) and R.same_bits(F.rows["d2"], d2) and np.array_equal(F.rows["count"], count)
    for got, want in zip((F.sep, F.ali, F.coh, F.avg), forces):
        assert R.same_bits(got, want), name
    if name == "coincident":
        assert count.sum() == 0 and not np.any(F.sep) and R.same_bits(F.avg, col)
    if name.startswith("clumps"):
        assert count.max() == k and (F.rows["metric"] > k).any()
    if name in ("n_1", "n_2", f"n_{K}"):
        assert count.max() < k  # fewer than k in sight


def test_rows_written_out_by_hand():
    prm = BC.params(bounds=100.0)  # perception 5, separation 3
    inf = np.inf
    # boid 0 has one neighbour at d2 = 1 (id 3) and two at equal d2 = 4 (ids 1 and 2): with k = 2 the lower id of the
    # tied pair wins
    pos = np.array([[0, 0, 0], [0, 2, 0], [2, 0, 0], [0, 0, 1]], dtype=np.float64)
    r = T.neighbours(pos, prm, 2)
    assert r["ids"][0].tolist() == [3, 1] and r["d2"][0].tolist() == [1.0, 4.0] and r["count"][0] == 2
    assert r["metric"][0] == 3
    # ... and the order of the tied pair is by id whatever k is
    assert T.neighbours(pos, prm, 3)["ids"][0].tolist() == [3, 1, 2]
    # a neighbour at exactly perception^2 = 25 is excluded; a pair at d2 = 2^-14 < 1e-4 is excluded; 2^-13 counts
    pos = np.array([[0, 0, 0], [5, 0, 0], [0, 3, 4], [0, 2.0 ** -7, 0], [2.0 ** -7, 2.0 ** -7, 0], [40, 0, 0]],
                   dtype=np.float64)
    r = T.neighbours(pos, prm, 3)
    assert r["ids"][0].tolist() == [4, -1, -1] and r["d2"][0].tolist() == [2.0 ** -13, inf, inf] and r["count"][0] == 1
    # boid 3: 0 and 4 are 2^-7 away (d2 = 2^-14: excluded), 1 is at 25 + 2^-14 (out), 2 at (3 - 2^-7)^2 + 16 < 25
    assert r["ids"][3].tolist() == [2, -1, -1] and r["count"][3] == 1
    assert r["d2"][3].tolist() == [25.0 - 6 * 2.0 ** -7 + 2.0 ** -14, inf, inf]
    # fewer than k in sight: padded with -1 / +inf, and a boid alone has an empty row
    assert r["ids"][5].tolist() == [-1, -1, -1] and r["count"][5] == 0 and np.all(np.isinf(r["d2"][5]))
    # boid 1 at (5, 0, 0): 0 is at exactly 25 (out), 3 at 25 + 2^-14 (out), 2 at 50, 4 at (5 - 2^-7)^2 + 2^-14 < 25
    assert r["ids"][1].tolist() == [4, -1, -1] and r["d2"][1, 0] == 25.0 - 10 * 2.0 ** -7 + 2.0 ** -13
    with pytest.raises(ValueError):
        T.neighbours(pos, prm, 0)
    with pytest.raises(ValueError):
        T.neighbours(pos, prm, 17)


@pytest.mark.parametrize("name", ["thresholds", "lattice_random"])
def test_k_above_every_neighbour_count_gives_the_metric_reference(name):
    """With k >= max |N_i| the set is the metric one, and on the lattice ali, coh, avg and nb are exact in any order."""
    if name == "thresholds":
        c = BC.thresholds()
        pos, vel, col, prm = c["pos"], c["vel"], c["col"], c["params"]
    else:
        rng = np.random.default_rng(5)
        prm = BC.params(bounds=28.0)
        pos = R.lattice(rng.uniform(-28, 28, (900, 3)), BC.PB)
        _, vel, col = _state(pos, 5)
    M = R.flocking(pos, vel, col, prm)
    assert 1 <= M.nb.max() <= 16
    F = T.flocking(pos, vel, col, prm, 16)
    assert np.array_equal(F.nb, M.nb) and np.array_equal(F.nsep, M.nsep)
    assert R.same_bits(F.ali, M.ali) and R.same_bits(F.coh, M.coh) and R.same_bits(F.avg, M.avg)
    R.check_sep(F.sep, M, vel, prm, name)


def test_distinct_d2_sees_a_tie():
    prm = BC.params(bounds=100.0)
    pos = np.array([[0, 0, 0], [0, 2, 0], [2, 0, 0], [0, 0, 1]], dtype=np.float64)
    assert T.distinct_d2(T.neighbours(pos, prm, 3)).tolist() == [False, True, True, False]


def test_header_declares_and_table_binds_the_calls():
    import nbmi_native
    header = open(os.path.join(ROOT, "include", "bdmi.h")).read()
    lib = ctypes.CDLL(nbmi_native.LIB_PATH)
    for name, nargs in CALLS.items():
        assert f"int {name}(bdmi_flock *f" in header
        assert hasattr(lib, name)
        res, args = nbmi_native.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == nargs
    for words in ("#define BDMI_NEIGHBOURS_METRIC 0", "#define BDMI_NEIGHBOURS_TOPOLOGICAL 1", "(d2(i, j), id_j)",
                  "STILL BOUNDED BY PERCEPTION", "starts at +0.0", "1 <= k <= 16", "BDMI_NEIGHBOURS", "GLOBAL id"):
        assert words in header
    from boids import flock
    assert flock.NEIGHBOUR_MODES == ("metric", "topological")


class _TopoFlock(_FakeFlock):
    """The stand-in of test_flockstats_host with the new method."""

    def set_neighbour_mode(self, mode, k=7):
        self.calls.append(("mode", mode, k))


def test_flock_video_topological_flags(tmp_path):
    from tools import flock_video as fv
    a = fv.build_parser().parse_args([])
    assert (a.neighbours, a.topological_k) == ("metric", 7)
    with pytest.raises(SystemExit):
        fv.build_parser().parse_args(["--neighbours", "nearest"])
    raw = tmp_path / "clip.rgb"
    args = fv.build_parser().parse_args(["--boids", "8", "--frames", "4", "--format", "raw", "-o", str(raw), "--warmup", "2",
                                         "--diagnostics", "2", "--neighbours", "topological", "--topological-k", "5"])
    t = fv.run(args, make_flock=_TopoFlock, make_renderer=_FakeRenderer, say=lambda *x: None)
    flock = _FakeFlock.made[-1]
    assert t["ok"] and flock.calls[0] == ("mode", "topological", 5) and flock.updates[0][1] == 2  # set before the warm-up
    assert sum(1 for c in flock.calls if c[0] == "mode") == 1
    meta = json.loads((tmp_path / "clip.rgb.json").read_text())
    assert meta["flock"]["neighbours"] == {"mode": "topological", "k": 5}
    recs = [json.loads(x) for x in (tmp_path / "clip.flock.jsonl").read_text().splitlines()]
    assert len(recs) == 2 and all(r["neighbours"] == {"mode": "topological", "k": 5} for r in recs)
    # metric (the default, or spelled out): no call, no key - with a stand-in that has no such method
    raw2 = tmp_path / "m" / "clip.rgb"
    args = fv.build_parser().parse_args(["--boids", "8", "--frames", "2", "--format", "raw", "-o", str(raw2),
                                         "--diagnostics", "1", "--neighbours", "metric", "--topological-k", "3"])
    fv.run(args, make_flock=_FakeFlock, make_renderer=_FakeRenderer, say=lambda *x: None)
    assert "neighbours" not in json.loads((tmp_path / "m" / "clip.rgb.json").read_text())["flock"]
    assert all("neighbours" not in json.loads(x) for x in (tmp_path / "m" / "clip.flock.jsonl").read_text().splitlines())
    for bad in ("0", "17"):
        with pytest.raises(ValueError, match="topological-k"):
            fv.run(fv.build_parser().parse_args(["--frames", "1", "--neighbours", "topological", "--topological-k", bad]),
                   make_flock=_TopoFlock, make_renderer=_FakeRenderer, say=lambda *x: None)


def test_neighbour_rank_profile():
    from boids import analysis as A
    inf = np.inf
    d2 = np.array([[1.0, 4.0, 9.0], [4.0, 16.0, inf], [inf, inf, inf], [9.0, inf, inf]])
    p = A.neighbour_rank_profile(d2)
    assert p.tolist() == [2.0, 3.0, 3.0]
    p = A.neighbour_rank_profile(np.array([[1.0, inf], [0.25, inf]]))
    assert p[0] == 0.75 and np.isnan(p[1])
    assert A.neighbour_rank_profile(np.zeros((0, 4))).shape == (4,)
    with pytest.raises(ValueError):
        A.neighbour_rank_profile(np.zeros(5))
    # on a restatement's rows: non-decreasing over the ranks every boid has
    rng = np.random.default_rng(1)
    pos = R.lattice(rng.normal(0, 1.0, (200, 3)), 16)
    r = T.neighbours(pos, BC.params(bounds=100.0), 5)
    assert (r["count"] == 5).all()
    assert np.all(np.diff(A.neighbour_rank_profile(r["d2"])) >= 0)
