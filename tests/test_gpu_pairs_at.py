"""nbmi_pair_counts_at on the GPU against the NumPy brute force of tests/pairs_at_ref.py (include/nbmi.h; DESIGN.md section
4.28).

Per-point rows and totals are compared EXACTLY in every case: a pair's column is a function of the float64 value
d2(i, j), which the kernel and NumPy form with the same three products and two sums, of the E[k] = edges[k] * edges[k],
one product each on both sides, and of comparisons; the sums are integers.  Every case first checks on the reference that
its input has the property the case is there for.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import pairs_at_ref as par
import pairs_ref as pr
import query_cases as qc
from query_cases import bh as _bh
from conftest import ROOT

pytestmark = pytest.mark.gpu

NBMI_ERR_ARG = -1
NBMI_ERR_CAPACITY = -4
M = 4097  # a partial last wave and more than 64 waves
CHUNK = 1048576  # the header's chunk
LIMIT = 1e18


def _twins():
    rng = np.random.RandomState(9)  # test_gpu_pairs' coincident twins: every position held twice
    base = rng.uniform(-1e-9, 1e-9, (2048, 3))
    return np.concatenate([base, base])


def _lattice_edges(spacing):
    """section 4.16's edge set: sqrt(1, 2, 3, 4, 5, 6, 8, 9) lattice spacings, exact roots where there are any"""
    s2 = spacing * spacing
    return np.array([pr.exact_root(s2 * m) or np.sqrt(s2 * m) for m in (1, 2, 3, 4, 5, 6, 8, 9)])


# name -> (bodies, eps of the handle, edge sets): a set near the bodies' own scale and one that reaches the far points
SYSTEMS = {
    "n2049": lambda: (qc.system("n2049")[0], 1.5, [np.array([0.0, 5.0, 10.0, 20.0, 40.0, 80.0, 160.0, 400.0]),
                                                   np.array([30.0, 300.0, 3000.0, 3.0e4, 1.0e18])]),
    "n4097": lambda: (qc.system("n4097")[0], 1.5, [np.linspace(0.0, 352.0, 65), np.array([1.0, 1.0e3, 1.0e17, 8.0e17])]),
    "trap": lambda: (qc.system("trap")[0], 1.5, [np.array([0.0, 1e-4, 5e-4, 2e-3, 50.0, 400.0]), np.array([1e-3, 1.0e4, 1.0e18])]),
    "far": lambda: (qc.system("far")[0], 1.5, [np.array([1.0, 5.0, 25.0, 100.0, 2.0e6]), np.array([0.0, 50.0, 3.0e7, 1.0e18])]),
    "twins": lambda: (_twins(), 0.0, [np.array([0.0, 1e-12, 1e-10, 1e-9, 4e-9]), np.array([0.0, 1e-8, 1e-7, 1.0])]),
    "lattice1": lambda: (qc.lattice(1.0)[0], 1.5, [_lattice_edges(1.0), np.nextafter(_lattice_edges(1.0), 0.0)]),
    "lattice33": lambda: (qc.lattice(33.0)[0], 1.5, [_lattice_edges(33.0), np.nextafter(_lattice_edges(33.0), 0.0)]),
}


def _points(p, seed, m=M, spacing=None):
    """m points of every kind the header speaks of, shuffled into one array: inside the bodies' box, outside it by 1, 10
    and 1e15 times its size (the last held to the limit of 1e18 per coordinate), exactly at bodies, between bodies, a
    body's position 64 times and one other point 65 times; ``spacing``: lattice sites, beyond the lattice too, and the
    midpoints of its edges, faces and cells"""
    rng = np.random.RandomState(seed)
    n = len(p)
    lo, hi = p.min(0), p.max(0)
    centre, size = 0.5 * (lo + hi), float((hi - lo).max())
    u = rng.normal(size=(300, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    parts = [p[rng.choice(n, min(n, 600), replace=False)], 0.5 * (p[rng.randint(0, n, 300)] + p[rng.randint(0, n, 300)])]
    for k, scale in enumerate((1.0, 10.0, 1.0e15)):
        parts.append(np.clip(centre + scale * size * u[100 * k:100 * k + 100], -0.9 * LIMIT, 0.9 * LIMIT))
    parts.append(np.repeat(p[rng.randint(0, n)][None, :], 64, axis=0))
    parts.append(np.repeat(rng.uniform(lo, hi, (1, 3)), 65, axis=0))
    if spacing is not None:
        sites = spacing * rng.randint(-2, 18, (500, 3)).astype(np.float64)
        half = spacing * (rng.randint(0, 15, (500, 3)) + 0.5 * rng.randint(0, 2, (500, 3)))
        parts += [sites, half]
    have = sum(len(x) for x in parts)
    parts.append(rng.uniform(lo, hi, (m - have, 3)))
    pts = np.concatenate(parts)
    assert pts.shape == (m, 3) and np.abs(pts).max() <= LIMIT
    pts = np.ascontiguousarray(pts[rng.permutation(m)])
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _case(name):
    """(bodies, eps, edge sets, points, [reference rows per edge set]) of a system, made once and never written to"""
    p, eps, sets = SYSTEMS[name]()
    spacing = {"lattice1": 1.0, "lattice33": 33.0}.get(name)
    pts = _points(p, 17 + len(name), spacing=spacing)
    refs = [par.per_point(pts, p, e) for e in sets]
    for r in refs:
        r.setflags(write=False)
    return p, eps, sets, pts, refs


def _check(tag, got, ref_rows):
    counts, below, rows = got[0], got[1], got[2]
    want_counts, want_below = par.totals(ref_rows)
    wrong = int((rows != ref_rows).any(axis=1).sum())
    print(f"{tag}: below {below} (reference {want_below}), counts {counts.tolist()} (reference {want_counts.tolist()}), "
          f"rows that differ {wrong} of {len(ref_rows)}")
    assert rows.dtype == np.int32 and rows.shape == ref_rows.shape and wrong == 0, tag
    assert counts.dtype == np.int64 and below == want_below and np.array_equal(counts, want_counts), tag


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_points_of_every_kind_exact(gpu, name):
    p, eps, sets, pts, refs = _case(name)
    n = len(p)
    outside = np.abs(pts).max(axis=1) > 1e3 * np.abs(p).max()
    assert outside.sum() >= 100  # the points at 1e15 sizes are there
    if name.startswith("lattice"):  # lowering the edges by one ulp moves pairs: many sit exactly at an edge
        within = [np.cumsum(r.sum(0, dtype=np.int64)) for r in refs]  # the pairs within each edge
        moved = within[0] - within[1]
        print(f"{name}: (point, body) pairs that leave each edge when it is lowered by one ulp: {moved.tolist()}")
        assert moved.sum() > 10_000 and (moved[[0, 3, 7]] > 500).all()  # (1, 2 and 3 spacings have exact squares on both lattices)
    else:
        assert refs[0].sum() > 10 * M, "the case lost its point: the near edges reach nothing"
    if name == "n2049":
        assert (refs[1][outside].sum(axis=1) == n).all()  # the far set reaches from the farthest points to every body
    sim = _bh(p, eps=eps)
    try:
        for k, (e, ref) in enumerate(zip(sets, refs)):
            got = sim.pair_counts_at(pts, e, per_point=True, evals=True)
            _check(f"{name} set {k} (nb = {len(e) - 1})", got, ref)
            print(f"    evals / point {got[3] / M:.1f}, cell pairs / point {got[4] / M:.1f}")
            assert got[3] + got[4] >= int(ref.sum())  # every counted pair was evaluated or came through a whole cell
            plain = sim.pair_counts_at(pts, e)  # without per_point: the same totals
            assert len(plain) == 2 and plain[1] == got[1] and np.array_equal(plain[0], got[0])
        # duplicated points give identical rows (the reference has them identical: compared above); a row of the call
        # does not depend on the call: a slice of the points gives the slice of the rows
        part = sim.pair_counts_at(pts[1000:1131], sets[0], per_point=True)
        assert np.array_equal(part[2], refs[0][1000:1131])
    finally:
        sim.close()


def test_all_points_equal(gpu):
    p = qc.system("n2049")[0]
    e = np.array([0.0, 20.0, 60.0, 120.0, 400.0])
    sim = _bh(p)
    try:
        for q in (p[77], np.array([13.0, -7.5, 2.25]), np.array([4.0e17, -9.0e17, 1.0])):
            pts = np.repeat(q[None, :], M, axis=0)
            one = par.per_point(pts[:1], p, e)
            assert one[0, 0] == int((q == p[77]).all()) and (one.sum() > 100) == (abs(q[0]) < 100.0)
            _check(f"all points at {q.tolist()}", sim.pair_counts_at(pts, e, per_point=True), np.repeat(one, M, axis=0))
    finally:
        sim.close()


def test_at_the_bodies_it_is_twice_the_pair_counts(gpu):
    """the tie to nbmi_pair_counts, on the device: every unordered pair is seen from both ends, and every body sees itself
    at d2 = 0"""
    from nbody.pairs import auto_pair_edges
    p = qc.system("galaxy")[0]
    n = len(p)
    assert n == 20_000
    sim = _bh(p)
    try:
        edges = np.array(auto_pair_edges(sim.knn(1)[0]))
        dd, below_dd = sim.pair_counts(edges)
        counts, below, rows, ev, cp = sim.pair_counts_at(sim.get_positions_f64(), edges, per_point=True, evals=True)
        print(f"galaxy 20 000 at the bodies: evals / point {ev / n:.1f}, cell pairs / point {cp / n:.1f}")
        assert dd.sum() > 10 * n and (dd > 0).all()
        assert np.array_equal(counts, 2 * dd) and below == 2 * below_dd + n
        assert np.array_equal(rows.sum(0, dtype=np.int64), np.concatenate([[below], counts])) and (rows[:, 0] >= 1).all()
        nc = sim.neighbour_counts(edges)
        assert np.array_equal(nc[:, 1:], rows[:, 1:]) and np.array_equal(nc[:, 0], rows[:, 0] - 1)
    finally:
        sim.close()


def test_small_sizes(gpu):
    rng = np.random.RandomState(4)
    edges = np.array([0.0, 20.0, 60.0, 120.0, 400.0])
    for n in (0, 1, 2, 64, 65):
        p = rng.uniform(-100.0, 100.0, (n, 3))
        sim = _bh(p)
        try:
            for m in (0, 1, 63, 64, 65, 129):
                pts = rng.uniform(-150.0, 150.0, (m, 3))
                if n and m:
                    pts[0] = p[n - 1]
                ref = par.per_point(pts, p, edges)
                if n and m:
                    assert ref[0, 0] == 1
                if n >= 64 and m >= 63:
                    assert (ref.sum(0)[1:] > 0).all()
                got = sim.pair_counts_at(pts, edges, per_point=True, evals=True)
                _check(f"N {n} M {m}", got, ref)
                if n == 0 or m == 0:
                    assert got[3] == 0 and got[4] == 0
        finally:
            sim.close()


def test_m_zero_touches_only_the_totals(gpu):
    lib = gpu.load()
    sim = _bh(qc.system("n65")[0])
    try:
        edges = np.array([1.0, 2.0, 3.0])
        counts, below, ev, cp = np.full(4, 7, np.int64), np.full(1, 7, np.int64), np.full(1, 7, np.int64), np.full(1, 7, np.int64)
        rows = np.full((2, 3), 7, np.int32)
        rc = lib.nbmi_pair_counts_at(sim._h, 0, None, 2, gpu.ptr(edges), gpu.ptr(counts), gpu.ptr(below), gpu.ptr(rows), gpu.ptr(ev),
                                     gpu.ptr(cp))
        assert rc == 0, gpu.last_error()
        assert counts.tolist() == [0, 0, 7, 7] and below[0] == 0 and ev[0] == 0 and cp[0] == 0 and (rows == 7).all()
        assert lib.nbmi_pair_counts_at(sim._h, 0, None, 2, gpu.ptr(edges), None, None, None, None, None) == 0
        pts = np.ones((3, 3))
        assert lib.nbmi_pair_counts_at(sim._h, 3, gpu.ptr(pts), 2, gpu.ptr(edges), None, None, None, None, None) == 0  # all NULL
    finally:
        sim.close()


def test_extremes_of_nb_and_edges(gpu):
    p, _, _, pts, _ = _case("n4097")
    pts = pts[:1025]
    n, m = len(p), len(pts)
    inside = np.abs(pts).max(axis=1) <= 100.0
    sets = {"nb1": np.array([10.0, 30.0]), "nb64": np.linspace(0.0, 352.0, 65),  # (the box's diameter is 346.4)
            "last edge beyond everything": np.array([0.0, 1.0, 100.0, 3.0e18]),
            "first edge beyond everything": np.array([3.0e18, 4.0e18, 5.0e18]),
            "edges that reach nothing": np.array([1e-9, 1e-8, 1e-7])}
    refs = {tag: par.per_point(pts, p, e) for tag, e in sets.items()}
    assert (refs["last edge beyond everything"].sum(1) == n).all()  # every row sums to N, the far points' too
    assert (refs["first edge beyond everything"][:, 0] == n).all() and not refs["first edge beyond everything"][:, 1:].any()
    on_a_body = (refs["edges that reach nothing"][:, 0] > 0)
    assert refs["edges that reach nothing"].sum() == on_a_body.sum() > 0  # nothing but the bodies the points sit on
    assert (refs["nb64"][inside].sum(1) == n).all() and (refs["nb64"].sum(0) > 0).sum() >= 60 and refs["nb1"][:, 1].sum() > 0
    sim = _bh(p)
    try:
        for tag, e in sets.items():
            _check(tag, sim.pair_counts_at(pts, e, per_point=True), refs[tag])
    finally:
        sim.close()


def test_chunk_boundary(gpu):
    """CHUNK + 1 points - the call's second chunk is one point - made of 4 097 distinct points tiled: the rows are the
    brute force's of the distinct points, tiled, and the totals their sum over both chunks"""
    p = qc.system("n65")[0]
    distinct = _points(p, 5)
    edges = np.array([40.0, 90.0, 180.0])
    one = par.per_point(distinct, p, edges)
    assert (one.sum(0) > 1000).all()
    reps = -(-(CHUNK + 1) // M)
    pts = np.tile(distinct, (reps, 1))[:CHUNK + 1]
    want = np.tile(one, (reps, 1))[:CHUNK + 1]
    sim = _bh(p)
    try:
        counts, below, rows = sim.pair_counts_at(pts, edges, per_point=True)
        assert np.array_equal(rows, want)
        tot = want.sum(0, dtype=np.int64)
        assert below == tot[0] and np.array_equal(counts, tot[1:])
        last = sim.pair_counts_at(pts[CHUNK:], edges, per_point=True)  # the second chunk's point on its own
        assert np.array_equal(last[2], want[CHUNK:])
        again = sim.pair_counts_at(pts[:M], edges, per_point=True)  # a small call after the large one
        assert np.array_equal(again[2], one)
    finally:
        sim.close()


def test_a_permutation_of_the_points_permutes_the_rows(gpu):
    p, _, sets, pts, refs = _case("n2049")
    perm = np.random.RandomState(8).permutation(M)
    sim = _bh(p)
    try:
        a = sim.pair_counts_at(pts, sets[0], per_point=True)
        b = sim.pair_counts_at(pts[perm], sets[0], per_point=True)
        c = sim.pair_counts_at(pts[::-1], sets[0], per_point=True)
    finally:
        sim.close()
    _check("as given", a, refs[0])
    assert np.array_equal(b[2], a[2][perm]) and np.array_equal(c[2], a[2][::-1])
    assert b[1] == a[1] == c[1] and np.array_equal(b[0], a[0]) and np.array_equal(c[0], a[0])


_CHILD = ("import sys, numpy as np; sys.path.insert(0, %r); import __graft_entry__ as g; g._import_package();"
          "from nbody.gpu_backend import HIPBarnesHutSimulation as H;"
          "d = np.load(sys.argv[2]); p = d['p'];"
          "s = H(p, np.zeros_like(p), np.ones(len(p)), 0.07, 1.5, 1.0, 0.5);"
          "c, b, rows, ev, cp = s.pair_counts_at(d['pts'], d['edges'], per_point=True, evals=True); s.close();"
          "np.savez(sys.argv[1], c=c, rows=rows, x=np.array([b, ev, cp], dtype=np.int64))") % ROOT


@functools.lru_cache(maxsize=None)
def _knob_reference():
    p, _, _, pts, _ = _case("n4097")
    ref = par.per_point(pts, p, np.array([0.0, 20.0, 60.0, 120.0, 400.0]))
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("knob", ["NBMI_FIELD_SORT", "NBMI_PAIRS_CELLS"])
def test_knobs_give_the_same_numbers(gpu, tmp_path, knob):
    """both knobs are read when the handle is created: a fresh child process with the knob at 0 counts the same input -
    in the caller's order, or without ever accepting a cell whole - and gives the same numbers"""
    p, _, _, pts, _ = _case("n4097")
    edges = np.array([0.0, 20.0, 60.0, 120.0, 400.0])
    ref = _knob_reference()
    f, out = str(tmp_path / "case.npz"), str(tmp_path / "out.npz")
    np.savez(f, p=p, pts=pts, edges=edges)
    subprocess.run([sys.executable, "-c", _CHILD, out, f], env=dict(os.environ, **{knob: "0"}), check=True, timeout=300)
    child = np.load(out)
    b, ev, cp = (int(x) for x in child["x"])
    sim = _bh(p)
    try:
        got = sim.pair_counts_at(pts, edges, per_point=True, evals=True)
    finally:
        sim.close()
    _check("default", got, ref)
    _check(f"{knob}=0", (child["c"], b, child["rows"]), ref)
    print(f"    evals {got[3]} and {got[4]} pairs through whole cells by default; {ev} and {cp} with {knob}=0")
    assert got[4] > 0
    if knob == "NBMI_PAIRS_CELLS":
        assert cp == 0 and ev > got[3]
    else:
        assert cp > 0


def test_work_is_actually_saved(gpu):
    """Conditions, not measurements.  Uniform 4 097 in the cube of side 200, points inside the cube.

    1. One bin that holds everything.  The root cube's half size is 1.1 x 100 + 10 = 120, so for a point and an anchor
       inside +-100 the root's query_upper is at most 3 (200 + 240)^2 (1 + 2^-40) < 5.9e5.  With edges [1e3, 1e6] that is
       below E[0] = 1e6: p = pair_bin(query_lower = 0) = 0 and the root is accepted whole into column 0 - no distance at
       all, evals == 0 and cell_pairs == m N.
       With edges [0, 1e6] - the set the existing test of nbmi_pair_counts uses - the same bound is below E[1] = 1e12,
       but the root is NOT accepted: a point inside the cube has query_lower = 0, whose counter is column 0 (d2 <= 0, a
       body ON the point), while query_upper falls into bin 0, and a cell that spans two counters cannot be counted
       whole by an exact count.  The lane descends along the cells that contain it and accepts their siblings; what
       holds exactly is evals + cell_pairs == m N, and the existing test's cap for this set, an eighth of the pairs.
    2. A last edge of 2 d1, d1 the median nearest-neighbour distance: pruning keeps evals below m N / 4."""
    p = qc.system("n4097")[0]
    n = len(p)
    pts = np.random.RandomState(31).uniform(-100.0, 100.0, (M, 3))
    pts[:50] = p[:50]
    d1 = float(np.sqrt(np.median(pr.nearest_d2(p))))
    e = np.array([0.0, 2.0 * d1])
    ref = par.per_point(pts, p, e)
    assert ref[:50, 0].min() == 1 and ref[50:, 0].max() == 0 and M / 4 < ref[:, 1].sum() < M * 40
    sim = _bh(p)
    try:
        c, below, ev, cp = sim.pair_counts_at(pts, [1.0e3, 1.0e6], evals=True)
        print(f"one column that holds everything: {ev} distances, {cp} pairs through whole cells of {M * n}")
        assert below == M * n and c[0] == 0 and ev == 0 and cp == M * n
        c, below, ev, cp = sim.pair_counts_at(pts, [0.0, 1.0e6], evals=True)
        print(f"one bin [0, 1e6]: {ev} distances ({ev / M:.1f} per point), {cp} pairs through whole cells")
        assert below == 50 and c[0] == M * n - 50 and ev + cp == M * n
        assert ev < M * n / 8
        got = sim.pair_counts_at(pts, e, per_point=True, evals=True)
        print(f"last edge 2 d1 = {2.0 * d1:.3f}: {got[3]} distances ({got[3] / M:.1f} per point), {got[0][0]} pairs")
        _check("2 d1", got, ref)
        assert 0 < got[3] < M * n / 4
    finally:
        sim.close()


def test_other_handle_states_and_repeat_calls(gpu):
    p, v, m = qc.preset("galaxy", 4096, 3, 800.0, 0.07, scale_masses=False)
    edges = np.array([0.0, 3.0, 6.0, 12.0, 24.0, 48.0, 200.0])
    pts = _points(p, 23)
    ref = par.per_point(pts, p, edges)
    assert (ref.sum(0)[1:] > 0).all()
    for kw in ({}, {"multipole": "quadrupole"}, {"integrator": "leapfrog"}):
        sim = _bh(p, v, m, **kw)
        try:
            a = sim.pair_counts_at(pts, edges, per_point=True, evals=True)
            b = sim.pair_counts_at(pts, edges, per_point=True, evals=True)
            _check(str(kw), a, ref)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and a[1] == b[1] and a[3:] == b[3:], "two calls differ"
        finally:
            sim.close()


@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
def test_calls_do_not_disturb_the_run_and_see_the_current_state(gpu, integrator):
    p, v, m = qc.preset("galaxy", 20_000, 7, 800.0, 0.07, scale_masses=False)
    rng = np.random.RandomState(6)
    tp, tv = rng.uniform(-500.0, 500.0, (300, 3)), rng.normal(size=(300, 3))
    edges = np.array([0.0, 10.0, 40.0, 160.0])
    pts = _points(p, 29)

    def run(query):
        sim = _bh(p, v, m, integrator=integrator)
        try:
            sim.set_force_precision("auto")
            sim.set_tracers(tp, tv)
            shares = []
            for i in range(12):
                if query and i % 3 == 0:
                    sim.pair_counts_at(pts, edges, per_point=True)
                sim.step(0.2)
                shares.append(sim.force_precision_share())
            state = (sim.get_positions_f64(), sim.get_velocities(), *sim.get_tracers())
            steps = sim.step_count()
            after = sim.pair_counts_at(pts, edges, per_point=True) if query else None
            moved = None
            if query:  # after a set_state too: a fresh handle's numbers
                sim.set_state(p, v)
                moved = sim.pair_counts_at(pts, edges, per_point=True)
            return state, steps, shares, after, moved
        finally:
            sim.close()
    a, b = run(False), run(True)
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    assert a[1] == b[1] == 12 and a[2] == b[2], (a[2], b[2])
    for x, got in ((a[0][0], b[3]), (p, b[4])):  # the same positions on a fresh handle
        fresh = _bh(x)
        try:
            want = fresh.pair_counts_at(pts, edges, per_point=True)
        finally:
            fresh.close()
        assert want[2].sum() > 10 * M
        assert np.array_equal(got[2], want[2]) and got[1] == want[1] and np.array_equal(got[0], want[0])


def test_capacity_error_is_a_steps_and_the_handle_goes_on(gpu):
    """DESIGN 4.14's capacity input: one position held by 70 bodies at +-50 needs more node rows than 4 N"""
    lib = gpu.load()
    rng = np.random.RandomState(9)
    base = rng.uniform(-50.0, 50.0, (2048, 3))
    p = np.concatenate([base, base])
    p[2049:2049 + 68] = p[0]
    pts = rng.uniform(-60.0, 60.0, (200, 3))
    sim = _bh(p, eps=0.0)
    try:
        edges = np.array([0.0, 1.0, 8.0])
        counts, below, rows = np.zeros(2, np.int64), np.zeros(1, np.int64), np.full((200, 3), -5, np.int32)
        rc = lib.nbmi_pair_counts_at(sim._h, 200, gpu.ptr(pts), 2, gpu.ptr(edges), gpu.ptr(counts), gpu.ptr(below), gpu.ptr(rows),
                                     None, None)
        msg = gpu.last_error()
        assert rc == NBMI_ERR_CAPACITY and "octree needs" in msg and "rows allocated" in msg, (rc, msg)
        assert (rows == -5).all()  # nothing walked
        good = rng.uniform(-50.0, 50.0, (4096, 3))
        sim.set_state(good, np.zeros_like(good))
        _check("after the capacity error", sim.pair_counts_at(pts, edges, per_point=True), par.per_point(pts, good, edges))
    finally:
        sim.close()


def test_refusals_leave_outputs_handle_and_state_untouched(gpu):
    from nbody.gpu_backend import HIPBarnesHutSimulation, HIPDirectSimulation, HIPOwnerSimulation
    from nbody.sharded import let_capacities
    lib = gpu.load()
    rng = np.random.RandomState(1)
    n = 256
    p, v, m = rng.uniform(-10, 10, (n, 3)), np.zeros((n, 3)), np.ones(n)
    pts = rng.uniform(-12, 12, (70, 3))
    good = np.array([0.0, 2.0, 4.0])
    outs = [np.full(64, 7, np.int64), np.full(1, 7, np.int64), np.full((70, 65), 7, np.int32), np.full(1, 7, np.int64),
            np.full(1, 7, np.int64)]

    def refused(sim, mm, points, nb, edges, *needles):
        rc = lib.nbmi_pair_counts_at(sim._h, mm, gpu.ptr(points) if points is not None else None, nb,
                                     gpu.ptr(edges) if edges is not None else None, gpu.ptr(outs[0]), gpu.ptr(outs[1]),
                                     gpu.ptr(outs[2]), gpu.ptr(outs[3]), gpu.ptr(outs[4]))
        msg = gpu.last_error()
        assert rc == NBMI_ERR_ARG and msg.startswith("nbmi_pair_counts_at: "), (rc, msg)
        for s in needles:
            assert s in msg, (s, msg)
        assert all((o == 7).all() for o in outs), msg  # every output as it was

    direct = HIPDirectSimulation(p, v, m, 0.07, 1.5, 1.0)
    cap, let_cap = let_capacities(n, 1)
    owner = HIPOwnerSimulation(p, v, m, np.arange(n, dtype=np.int32), cap, let_cap, 1, 0, 0.07, 1.5, 1.0)
    shard = HIPBarnesHutSimulation(p, v, m, 0.07, 1.5, 1.0, 0.5)
    bh = HIPBarnesHutSimulation(p, v, m, 0.07, 1.5, 1.0, 0.5)
    try:
        shard.set_shard(0, n // 2)
        for sim, needle in ((direct, "direct N^2"), (owner, "owner-mode"), (shard, "sharded")):
            refused(sim, 70, pts, 2, good, needle)
        for sim in (direct, owner):  # the Python classes refuse on their own
            with pytest.raises(ValueError):
                sim.pair_counts_at(pts, good)
            with pytest.raises(ValueError):
                sim.neighbour_counts(good)
        with pytest.raises(ValueError, match="sharded"):
            shard.pair_counts_at(pts, good)
        bh.compute_colors(15.0)
        bh.set_tracers(pts[:5], pts[5:10])
        before = (bh.get_positions_f64(), bh.get_velocities(), bh.get_colors(), *bh.get_tracers(), bh.step_count())
        refused(bh, -1, pts, 2, good, "negative")
        refused(bh, 70, None, 2, good, "null points_xyz")
        for bad, row in ((np.nan, 0), (np.inf, 33), (-np.inf, 69), (1.0000001e18, 5), (-2e18, 68)):
            q = pts.copy()
            q[row, row % 3] = bad
            q[69, 2] = bad if row != 69 else q[69, 2]  # (a later bad row too: the first is named)
            refused(bh, 70, q, 2, good, f"row {row} ")
            with pytest.raises(ValueError, match="nbmi_pair_counts_at"):
                bh.pair_counts_at(q, good)
        refused(bh, 70, pts, 0, good, "nb = 0")
        refused(bh, 70, pts, 65, np.arange(66.0), "nb = 65")
        refused(bh, 70, pts, -1, good, "nb = -1")
        refused(bh, 70, pts, 2, None, "null edges")
        refused(bh, 0, None, 2, None, "null edges")  # m == 0 does not excuse the edges
        for bad in ([0.0, np.inf, 4.0], [0.0, np.nan, 4.0], [-1.0, 2.0, 4.0], [0.0, 2.0, 2.0], [0.0, 3.0, 2.0],
                    [0.0, 1e200, 2e200], [1e-200, 2e-200, 1.0]):
            refused(bh, 70, pts, 2, np.array(bad), "edges[")
            with pytest.raises(ValueError, match="edges"):
                bh.pair_counts_at(pts, bad)
        with pytest.raises(ValueError, match="shape"):
            bh.pair_counts_at(pts[:, :2], good)
        after = (bh.get_positions_f64(), bh.get_velocities(), bh.get_colors(), *bh.get_tracers(), bh.step_count())
        for a, c in zip(before[:5], after[:5]):
            assert a.tobytes() == c.tobytes()
        assert before[5] == after[5] == 0
        # every handle goes on working
        direct.step(0.1)
        direct.sync()
        shard.set_shard(0, n)
        ref = par.per_point(pts, p, good)
        for sim in (shard, bh):
            _check("after refusals", sim.pair_counts_at(pts, good, per_point=True), ref)
            sim.step(0.1)
            sim.sync()
    finally:
        for sim in (direct, owner, shard, bh):
            sim.close()


def test_estimators_against_three_reference_counts(gpu):
    from nbody.pairs import xi_davis_peebles, xi_landy_szalay, xi_natural
    p = qc.preset("galaxy", 4096, 3, 800.0, 0.07, scale_masses=False)[0]
    rnd = np.random.RandomState(12).uniform(-400.0, 400.0, (3000, 3))
    edges = np.array([5.0, 10.0, 20.0, 40.0, 80.0, 160.0])
    dd, rr = pr.pair_counts(p, edges)[0], pr.pair_counts(rnd, edges)[0]
    dr = par.pair_counts_at(rnd, p, edges)[0]
    assert (dd > 0).all() and (rr > 0).all() and (dr > 0).all()
    want = xi_landy_szalay(dd, dr, rr, len(p), len(rnd))
    assert want[0] > 1.0  # the galaxy is clustered on small scales
    sim = _bh(p)
    try:
        got = sim.correlation_function(edges, rnd, estimator="landy-szalay")
        print(f"xi (Landy-Szalay) = {got.tolist()}")
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
        got = sim.correlation_function(edges, rnd, estimator="davis-peebles")
        assert np.array_equal(got.view(np.uint64), xi_davis_peebles(dd, dr, len(p), len(rnd)).view(np.uint64))
        nat = xi_natural(dd, rr, len(p), len(rnd))
        for kw in ({}, {"estimator": "natural"}):  # the default keeps its bits
            assert np.array_equal(sim.correlation_function(edges, rnd, **kw).view(np.uint64), nat.view(np.uint64))
        assert np.isnan(sim.correlation_function([1e-9, 1e-8], rnd, estimator="landy-szalay")).all()
        with pytest.raises(ValueError, match="estimator"):
            sim.correlation_function(edges, rnd, estimator="hamilton")
    finally:
        sim.close()


def test_neighbour_counts_against_the_restatement(gpu):
    from nbody.pairs import counts_within
    p = qc.system("n2049")[0].copy()
    p[100:110] = p[5]  # ten coincident twins of body 5
    edges = np.array([0.0, 5.0, 10.0, 20.0])
    ref = par.per_point(p, p, edges)
    ref[:, 0] -= 1
    assert ref[5, 0] == 10 and ref[:, 0].sum() == 11 * 10 and ref[:, 1:].sum() > 1000
    sim = _bh(p, eps=0.0)
    try:
        got = sim.neighbour_counts(edges)
    finally:
        sim.close()
    assert got.dtype == np.int32 and np.array_equal(got, ref)
    assert np.array_equal(counts_within(got)[:, -1], ref.sum(1, dtype=np.int64))
