"""nbmi_tidal_at and nbmi_get_tidal_f64 on the device (include/nbmi.h) against the NumPy restatement
(tests/tidal_ref.py): the bit pins between the two calls and against the field's term counts, points of every kind, edge
sizes and the chunk boundary, order independence, the direct handle, non-interference with the steps and the tracers,
the refusals and the recorder's timestep.jsonl.

Limits, the project's: |T - ref| (Frobenius) <= 1e-12 mag + bound on tree handles, <= 1e-11 mag on direct handles, with
mag and bound as tidal_ref derives them."""
import functools
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden
import potential_ref as pr
import quadrupole_ref as qr
import tidal_ref as tr

pytestmark = pytest.mark.gpu

PINS = ["tree_galaxy_2048", "tree_collision_2048", "tree_cluster_2048"]
THETAS = (0.3, 0.5, 1.3)
CHUNK = 1048576  # the header's chunk
M = 4097


def _bh(pos, mass, G, eps, theta, vel=None, **kw):
    from nbody.gpu_backend import HIPBarnesHutSimulation
    return HIPBarnesHutSimulation(pos, np.zeros_like(pos) if vel is None else vel, mass, G, eps, 1.0, theta, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _norm(t6):
    """the header's expression of norm, operation by operation"""
    return np.sqrt(((t6[:, 0] * t6[:, 0] + t6[:, 1] * t6[:, 1]) + t6[:, 2] * t6[:, 2])
                   + 2.0 * ((t6[:, 3] * t6[:, 3] + t6[:, 4] * t6[:, 4]) + t6[:, 5] * t6[:, 5]))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(pos, mass, G, eps, the oracle's tree, its cell moments) of a golden, built once and never written to"""
    from oracle import pyref
    pyref.lib()
    g = golden(name)
    pos, mass, G = np.ascontiguousarray(g["pos"], np.float64), np.ascontiguousarray(g["mass"], np.float64), float(g["G"])
    tree = pr.build_tree(pyref, pos, mass)
    P = qr.cell_moments(tree[0], tree[1], pos, mass, G)
    for a in (pos, mass, P):
        a.setflags(write=False)
    return pos, mass, G, float(g["eps"]), tree, P


def _probe_points(pos, seed, m=M):
    """m points of every kind the header speaks of, in one array: test_gpu_field's generator"""
    rng = np.random.default_rng(seed)
    n = len(pos)
    bounds = np.abs(pos).max() * 1.1 + 10.0  # the root cube's half size
    own = pos[rng.choice(n, min(n, 1000), replace=False)]
    mid = 0.5 * (pos[rng.integers(0, n, 1000)] + pos[rng.integers(0, n, 1000)])
    corners = bounds * np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64)
    faces = rng.uniform(-bounds, bounds, (60, 3))
    faces[np.arange(60), np.arange(60) % 3] = np.where(np.arange(60) % 2 == 0, bounds, -bounds)
    faces[:6] = bounds * np.concatenate([np.eye(3), -np.eye(3)])
    u = rng.normal(size=(200, 3))
    u /= np.sqrt((u * u).sum(1))[:, None]
    outside = np.concatenate([3.0 * bounds * u[:100], 100.0 * bounds * u[100:]])
    copies = np.repeat(pos[rng.integers(0, n)][None, :], 64, axis=0)
    dup = np.repeat(rng.uniform(-0.5 * bounds, 0.5 * bounds, (1, 3)), 65, axis=0)
    parts = [own, mid, np.zeros((1, 3)), corners, faces, outside, copies, dup]
    have = sum(len(p) for p in parts)
    parts.append(rng.uniform(-bounds, bounds, (m - have, 3)))
    pts = np.concatenate(parts)
    assert pts.shape == (m, 3)
    return pts[rng.permutation(m)]


def _check(tag, got, ref, min_margin=1e-9):
    t6, terms = got
    # a condition on the input, not on the device: no opening test of the restatement is near a tie (at the bodies' own
    # positions, whose terms the potential's tests already pin, -1: no condition)
    assert ref["margin"] > min_margin, (tag, ref["margin"])
    lim = 1e-12 * ref["mag"] + ref["bound"]
    err = tr.error(t6, ref["t6"])
    ratio = float((err / np.where(lim > 0, lim, 1e-300)).max()) if len(err) else 0.0
    wrong = int((terms != ref["terms"]).sum())
    print(f"{tag}: margin {ref['margin']:.3g}, points with other terms {wrong}, largest |dT| / limit {ratio:.3g}")
    assert wrong == 0, tag
    assert np.all(err <= lim), (tag, ratio)


@pytest.mark.parametrize("multipole", ["monopole", "quadrupole"])
@pytest.mark.parametrize("name", PINS)
def test_at_the_bodies_both_calls_agree_bit_for_bit(gpu, oracle, name, multipole):
    pos, mass, G, eps, tree, P = _case(name)
    for theta in THETAS:
        sim = _bh(pos, mass, G, eps, theta, multipole=multipole)
        try:
            x = sim.get_positions_f64()
            t6, terms = sim.tidal_at(x, terms=True)
            rows, norm = sim.tidal(norm=True)
            assert _same([t6], [rows]), (name, theta)
            assert _same([norm], [_norm(rows)]) and _same([norm], [sim.tidal_norm()]) and _same([rows], [sim.tidal()])
            assert int(terms.sum()) == sim.diagnostics().terms, (name, theta)
        finally:
            sim.close()
        ref = tr.tree_tidal(oracle, pos, pos, mass, G, eps, theta, tree=tree, multipole=multipole, P=P)
        _check(f"{name} {multipole} theta {theta}", (t6, terms), ref, min_margin=-1.0)
        _check(f"{name} {multipole} theta {theta} tidal()", (rows, terms), ref, min_margin=-1.0)


@pytest.mark.parametrize("multipole", ["monopole", "quadrupole"])
@pytest.mark.parametrize("name", PINS)
def test_points_of_every_kind_against_the_restatement(gpu, oracle, name, multipole):
    pos, mass, G, eps, tree, P = _case(name)
    pts = _probe_points(pos, 7)
    for e in (eps, 0.0):  # eps = 0: the copies of a body take the guard path
        ref = tr.tree_tidal(oracle, pts, pos, mass, G, e, 0.5, tree=tree, multipole=multipole, P=P)
        sim = _bh(pos, mass, G, e, 0.5, multipole=multipole)
        try:
            got = sim.tidal_at(pts, terms=True)
            field_terms = sim.field_at(pts, terms=True)[2]
        finally:
            sim.close()
        _check(f"{name} {multipole} eps {e}", got, ref)
        assert np.array_equal(got[1], field_terms)
        if e == 0.0:
            assert np.all(np.abs(tr.trace(got[0])) <= 1e-12 * ref["mag"] + ref["bound"])
        _, inv, cnt = np.unique(pts, axis=0, return_inverse=True, return_counts=True)
        groups = np.nonzero(cnt >= 64)[0]  # the copies of a body and the duplicated point: identical rows
        assert len(groups) == 2
        for k in groups:
            rows = np.nonzero(inv.reshape(-1) == k)[0]
            assert _same([a[rows] for a in got], [np.repeat(a[rows[:1]], len(rows), axis=0) for a in got])


def test_edge_sizes_and_no_points(gpu, oracle):
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 64, 65):
        pos = rng.normal(size=(n, 3)) * 20.0
        mass = rng.uniform(0.5, 2.0, n)
        for multipole in ("monopole", "quadrupole"):
            sim = _bh(pos, mass, 0.7, 0.1, 0.5, multipole=multipole)
            try:
                for m in (1, 63, 64, 65):
                    pts = rng.normal(size=(m, 3)) * 30.0
                    pts[0] = pos[0]
                    got = sim.tidal_at(pts, terms=True)
                    ref = tr.tree_tidal(oracle, pts, pos, mass, 0.7, 0.1, 0.5, multipole=multipole)
                    _check(f"N {n} M {m} {multipole}", got, ref)
                    assert got[1][0] == ref["terms"][0]
                t6, terms = sim.tidal_at(np.zeros((0, 3)), terms=True)
                assert t6.shape == (0, 6) and t6.dtype == np.float64 and terms.shape == (0,) and terms.dtype == np.int32
                lib = gpu.load()
                assert lib.nbmi_tidal_at(sim._h, 0, None, None, None) == 0
                three = np.zeros((3, 3))
                assert lib.nbmi_tidal_at(sim._h, 3, gpu.ptr(three), None, None) == 0  # the all-NULL call
                assert lib.nbmi_get_tidal_f64(sim._h, None, None) == 0
                rows, norm = sim.tidal(norm=True)
                assert _same([rows], [sim.tidal_at(pos)]) and _same([norm], [_norm(rows)])
                if n == 1:
                    assert not rows.any() and not norm.any()  # its own leaf is dropped by the guard
            finally:
                sim.close()


def test_no_bodies_gives_zeros(gpu):
    sim = _bh(np.zeros((0, 3)), np.zeros(0), 1.0, 0.1, 0.5)
    try:
        t6, terms = sim.tidal_at(np.ones((5, 3)), terms=True)
        assert t6.shape == (5, 6) and not t6.any() and not terms.any()
        rows, norm = sim.tidal(norm=True)
        assert rows.shape == (0, 6) and norm.shape == (0,) and sim.tidal_norm().shape == (0,)
    finally:
        sim.close()


def test_chunk_boundary(gpu):
    """CHUNK + 1 points: the call's second chunk is one point.  A point's row does not depend on the call it is in."""
    pos, mass, G, eps, _, _ = _case("tree_galaxy_2048")
    rng = np.random.default_rng(3)
    pts = rng.uniform(-600.0, 600.0, (CHUNK + 1, 3))
    sim = _bh(pos, mass, G, eps, 0.5)
    try:
        whole = sim.tidal_at(pts, terms=True)
        cut = 400001
        a, b = sim.tidal_at(pts[:cut], terms=True), sim.tidal_at(pts[cut:], terms=True)
        last = sim.tidal_at(pts[CHUNK:], terms=True)
        few = sim.tidal_at(pts[CHUNK - 40:CHUNK + 1], terms=True)
    finally:
        sim.close()
    assert _same(whole, [np.concatenate([x, y]) for x, y in zip(a, b)])
    assert _same([x[CHUNK:] for x in whole], last) and _same([x[CHUNK - 40:] for x in whole], few)
    assert whole[1].min() > 0 and np.isfinite(whole[0]).all()


@pytest.mark.parametrize("multipole", ["monopole", "quadrupole"])
def test_order_independence(gpu, monkeypatch, multipole):
    pos, mass, G, eps, _, _ = _case("tree_collision_2048")
    pts = _probe_points(pos, 19)
    perm = np.random.default_rng(0).permutation(M)
    sim = _bh(pos, mass, G, eps, 0.5, multipole=multipole)
    try:
        one = sim.tidal_at(pts, terms=True)
        assert _same(one, sim.tidal_at(pts, terms=True))  # a repeat
        shuffled = sim.tidal_at(pts[perm], terms=True)
        assert _same([x[perm] for x in one], shuffled)
        h1, h2 = sim.tidal_at(pts[:2000], terms=True), sim.tidal_at(pts[2000:], terms=True)
        assert _same(one, [np.concatenate([x, y]) for x, y in zip(h1, h2)])
        assert _same(one[:1], [sim.tidal_at(pts)])  # tidal6 alone
    finally:
        sim.close()
    monkeypatch.setenv("NBMI_FIELD_SORT", "0")  # read when the handle is created
    plain = _bh(pos, mass, G, eps, 0.5, multipole=multipole)
    try:
        assert _same(one, plain.tidal_at(pts, terms=True))
    finally:
        plain.close()


@pytest.mark.parametrize("eps", [0.1, 0.0])
@pytest.mark.parametrize("n", [1, 3, 65, 4097])
def test_direct_handle(gpu, n, eps):
    from nbody.gpu_backend import HIPDirectSimulation
    rng = np.random.default_rng(n)
    pos = rng.normal(size=(n, 3)) * 20.0
    mass = rng.uniform(0.5, 2.0, n)
    pts = np.concatenate([pos[: min(n, 40)], rng.normal(size=(260, 3)) * 30.0, rng.normal(size=(3, 3)) * 5000.0])
    sim = HIPDirectSimulation(pos, np.zeros_like(pos), mass, 0.7, eps, 1.0)
    try:
        t6, terms = sim.tidal_at(pts, terms=True)
        again = sim.tidal_at(pts, terms=True)
        rows, norm = sim.tidal(norm=True)
        at_bodies = sim.tidal_at(sim.get_positions_f64())
    finally:
        sim.close()
    rt, rterms, mag = tr.direct_tidal(pts, pos, mass, 0.7, eps)
    assert np.array_equal(terms, rterms) and terms[0] == n - 1 and terms[-1] == n
    assert np.all(tr.error(t6, rt) <= 1e-11 * mag), (n, eps)
    assert _same((t6, terms), again)
    assert _same([rows], [at_bodies]) and _same([norm], [_norm(rows)])
    if eps == 0.0:
        assert np.all(np.abs(tr.trace(t6)) <= 1e-11 * mag)
    else:
        assert np.all(tr.trace(t6)[terms > 0] < 0.0)


@pytest.mark.parametrize("integrator,precision", [("kick_drift", "auto"), ("leapfrog", "auto"), ("kick_drift", "f32")])
def test_tidal_calls_do_not_disturb_the_run(gpu, integrator, precision):
    pos, mass, G, eps, _, _ = _case("tree_galaxy_2048")
    rng = np.random.default_rng(4)
    vel = rng.normal(size=pos.shape) * 0.3
    pts = _probe_points(pos, 23)[:300]
    tp, tv = _probe_points(pos, 29)[:200], rng.normal(size=(200, 3)) * 0.3

    def run(query):
        sim = _bh(pos, mass, G, eps, 0.5, vel=vel, integrator=integrator)
        try:
            sim.set_force_precision(precision)
            sim.set_tracers(tp, tv)
            shares, rows = [], []
            for _ in range(4):
                if query:
                    rows.append((sim.tidal_at(pts, terms=True), sim.tidal(norm=True)))
                sim.step(0.2)
                shares.append(sim.force_precision_share())
            state = (sim.get_positions_f64(), sim.get_velocities(), *sim.get_tracers())
            after = None
            if query:  # after that history, and after a set_state: a fresh handle's bits at the same state
                after = [sim.tidal_at(pts, terms=True)]
                sim.set_state(pos, vel)
                after.append(sim.tidal_at(pts, terms=True))
            return state, sim.step_count(), shares, rows, after
        finally:
            sim.close()
    a, b = run(False), run(True)
    assert _same(a[0], b[0]) and a[1] == b[1] == 4
    assert a[2] == b[2], (a[2], b[2])
    # a leapfrog handle returns a plain handle's bits for the same state (the first call: the initial state)
    plain = _bh(pos, mass, G, eps, 0.5, vel=vel)
    try:
        first = plain.tidal_at(pts, terms=True)
        assert _same(b[3][0][0], first) and _same(b[3][0][1], plain.tidal(norm=True))
        assert _same(b[4][1], first)
        plain.set_state(b[0][0], b[0][1])
        assert _same(b[4][0], plain.tidal_at(pts, terms=True))
    finally:
        plain.close()


def test_refusals(gpu):
    pos, mass, G, eps, _, _ = _case("tree_cluster_2048")
    sim = _bh(pos, mass, G, eps, 0.5)
    try:
        good = np.zeros((5, 3))
        for bad in (np.nan, np.inf, -np.inf, 1e19, -1e19):
            pts = good.copy()
            pts[3, 1] = bad
            with pytest.raises(ValueError, match="row 3"):
                sim.tidal_at(pts)
        pts = good.copy()
        pts[2, 0], pts[4, 2] = np.nan, np.inf
        with pytest.raises(ValueError, match="row 2"):  # the first bad row
            sim.tidal_at(pts)
        assert np.isfinite(sim.tidal_at(np.full((1, 3), 1e18))).all()
        for shape in ((3,), (4, 2), (2, 3, 1)):
            with pytest.raises(ValueError, match=r"\(m, 3\)"):
                sim.tidal_at(np.zeros(shape))
        lib = gpu.load()
        assert lib.nbmi_tidal_at(sim._h, -1, gpu.ptr(good), None, None) == -1
        assert "nbmi_tidal_at: " in gpu.last_error() and "negative" in gpu.last_error()
        assert lib.nbmi_tidal_at(sim._h, 5, None, None, None) == -1 and "nbmi_tidal_at: null points_xyz" in gpu.last_error()
        before = sim.tidal_at(good, terms=True), sim.tidal(norm=True)
        sim.set_shard(0, len(pos) // 2)
        with pytest.raises(ValueError, match="sharded"):
            sim.tidal_at(good)
        with pytest.raises(ValueError, match="sharded"):
            sim.tidal()
        assert lib.nbmi_get_tidal_f64(sim._h, None, None) == -1 and "nbmi_get_tidal_f64: " in gpu.last_error()
        sim.set_shard(0, len(pos))
        assert _same(before[0], sim.tidal_at(good, terms=True)) and _same(before[1], sim.tidal(norm=True))
    finally:
        sim.close()


def test_recorder_writes_the_timestep_check(gpu, tmp_path):
    """quick_galaxy cut to 4 096 bodies x 5 frames with --timestep-check 2, in a process of its own: lines after the
    frames 1 and 3"""
    code = ("import sys; sys.path.insert(0, %r); import __graft_entry__ as g; g._import_package();"
            "from tools import record; sys.exit(record.main(sys.argv[1:]))") % ROOT
    argv = ["ts", "--preset", "quick_galaxy", "--bodies", "4096", "--frames", "5", "--root", str(tmp_path),
            "--timestep-check", "2"]
    subprocess.run([sys.executable, "-c", code, *argv], check=True, timeout=300)
    from tools import record as rec
    d = rec.get_recording_dir("ts", tmp_path)
    meta = rec.load_metadata(d)
    assert meta["timestep_check"] == {"every": 2, "levels": [0.1, 0.5, 2.0]}
    rows = [json.loads(line) for line in (d / rec.TIMESTEP_FILE).read_text().splitlines()]
    assert [r["frame"] for r in rows] == [1, 3]
    for r in rows:
        assert sorted(r) == ["above", "bodies", "chi_quantiles", "dt", "frame", "levels"]
        assert r["bodies"] == 4096 and r["levels"] == [0.1, 0.5, 2.0] and r["dt"] == meta["dt_per_frame"] / meta["substeps"]
        q = [r["chi_quantiles"][k] for k in ("0.5", "0.9", "0.99", "1.0")]
        assert np.isfinite(q).all() and q[0] > 0.0 and np.all(np.diff(q) >= 0.0)
        above = r["above"]
        assert all(0 <= k <= 4096 for k in above) and np.all(np.diff(above) <= 0)
        for c, k in zip(r["levels"], above):  # consistent with the quantiles
            assert (k > 0) == (q[3] > c)
            for f, v in zip((0.5, 0.9, 0.99), q[:3]):
                if v > c:
                    assert k >= int(np.floor((1.0 - f) * 4096))  # at least the bodies above that quantile
                else:
                    assert k <= int(np.ceil((1.0 - f) * 4096))
    assert rec.show_status("ts", root=tmp_path)
