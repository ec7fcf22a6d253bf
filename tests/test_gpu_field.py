"""nbmi_field_at on the device (include/nbmi.h) against the NumPy restatement (tests/field_ref.py): the bit
pins against the potential and the diagnostics, points of every kind, edge sizes and the chunk boundary, order
independence, the direct handle, non-interference with the steps, the refusals and the recorder's rotation.jsonl."""
import functools
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden
import field_ref as fr
import potential_ref as pr
import quadrupole_ref as qr

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
    """m points of every kind the header speaks of, in one array (the test compares every one of them)"""
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
    acc, phi, terms = got
    # a condition on the input, not on the device: no opening test of the restatement is near a tie (the bit pins at
    # the bodies' own positions, whose terms the potential's tests already pin, pass -1: no condition)
    assert ref["margin"] > min_margin, (tag, ref["margin"])
    lim_a = 1e-12 * ref["mag_acc"] + ref["bound_acc"]
    lim_p = 1e-12 * ref["mag_phi"] + ref["bound_phi"]
    err_a = np.sqrt(((acc - ref["acc"]) ** 2).sum(1))
    err_p = np.abs(phi - ref["phi"])
    ra = float((err_a / np.where(lim_a > 0, lim_a, 1e-300)).max()) if len(phi) else 0.0
    rp = float((err_p / np.where(lim_p > 0, lim_p, 1e-300)).max()) if len(phi) else 0.0
    wrong = int((terms != ref["terms"]).sum())
    print(f"{tag}: margin {ref['margin']:.3g}, points with other terms {wrong}, largest |dacc| / bound {ra:.3g}, "
          f"|dphi| / bound {rp:.3g}")
    assert wrong == 0, tag
    assert np.all(err_a <= lim_a), (tag, ra)
    assert np.all(err_p <= lim_p), (tag, rp)


@pytest.mark.parametrize("multipole", ["monopole", "quadrupole"])
@pytest.mark.parametrize("name", PINS)
def test_at_the_bodies_it_is_the_potential_bit_for_bit(gpu, oracle, name, multipole):
    pos, mass, G, eps, tree, P = _case(name)
    for theta in THETAS:
        sim = _bh(pos, mass, G, eps, theta, multipole=multipole)
        try:
            x = sim.get_positions_f64()
            acc, phi, terms = sim.field_at(x, terms=True)
            assert np.array_equal(_bits(phi), _bits(sim.potentials())), (name, theta)
            assert int(terms.sum()) == sim.diagnostics().terms, (name, theta)
        finally:
            sim.close()
        ref = fr.tree_field(oracle, pos, pos, mass, G, eps, theta, tree=tree, multipole=multipole, P=P)
        _check(f"{name} {multipole} theta {theta}", (acc, phi, terms), ref, min_margin=-1.0)


@pytest.mark.parametrize("multipole", ["monopole", "quadrupole"])
@pytest.mark.parametrize("name", PINS)
def test_points_of_every_kind_against_the_restatement(gpu, oracle, name, multipole):
    pos, mass, G, eps, tree, P = _case(name)
    pts = _probe_points(pos, 7)
    for e in (eps, 0.0):  # eps = 0: the copies of a body take the guard path
        ref = fr.tree_field(oracle, pts, pos, mass, G, e, 0.5, tree=tree, multipole=multipole, P=P)
        sim = _bh(pos, mass, G, e, 0.5, multipole=multipole)
        try:
            got = sim.field_at(pts, terms=True)
        finally:
            sim.close()
        _check(f"{name} {multipole} eps {e}", got, ref)
        _, inv, cnt = np.unique(pts, axis=0, return_inverse=True, return_counts=True)
        groups = np.nonzero(cnt >= 64)[0]  # the copies of a body and the duplicated point: identical rows
        assert len(groups) == 2
        for k in groups:
            rows = np.nonzero(inv.reshape(-1) == k)[0]
            assert _same([a[rows] for a in got], [np.repeat(a[rows[:1]], len(rows), axis=0) for a in got])


def test_points_of_every_kind_at_20000_bodies(gpu, oracle):
    from tools.presets import generate_distribution
    np.random.seed(123)
    p, _, m = generate_distribution("galaxy", 20000, 500.0, 0.15)
    pos, mass = p.astype(np.float64), m.astype(np.float64)
    pts = _probe_points(pos, 11)
    tree = pr.build_tree(oracle, pos, mass)
    ref = fr.tree_field(oracle, pts, pos, mass, 0.15, 3.0, 0.5, tree=tree)
    sim = _bh(pos, mass, 0.15, 3.0, 0.5)
    try:
        got = sim.field_at(pts, terms=True)
    finally:
        sim.close()
    _check("galaxy 20000", got, ref)


def test_edge_sizes_and_no_points(gpu, oracle):
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 64, 65):
        pos = rng.normal(size=(n, 3)) * 20.0
        mass = rng.uniform(0.5, 2.0, n)
        sim = _bh(pos, mass, 0.7, 0.1, 0.5)
        try:
            for m in (1, 63, 64, 65):
                pts = rng.normal(size=(m, 3)) * 30.0
                pts[0] = pos[0]
                got = sim.field_at(pts, terms=True)
                ref = fr.tree_field(oracle, pts, pos, mass, 0.7, 0.1, 0.5)
                _check(f"N {n} M {m}", got, ref)
                assert got[2][0] == ref["terms"][0]
            acc, phi, terms = sim.field_at(np.zeros((0, 3)), terms=True)
            assert acc.shape == (0, 3) and phi.shape == (0,) and terms.shape == (0,) and terms.dtype == np.int32
            assert gpu.load().nbmi_field_at(sim._h, 0, None, None, None, None) == 0
        finally:
            sim.close()


def test_no_bodies_gives_zeros(gpu):
    sim = _bh(np.zeros((0, 3)), np.zeros(0), 1.0, 0.1, 0.5)
    try:
        acc, phi, terms = sim.field_at(np.ones((5, 3)), terms=True)
        assert not acc.any() and not phi.any() and not terms.any()
    finally:
        sim.close()


def test_chunk_boundary(gpu):
    """CHUNK + 1 points: the call's second chunk is one point.  A point's row does not depend on the call it is in."""
    pos, mass, G, eps, _, _ = _case("tree_galaxy_2048")
    rng = np.random.default_rng(3)
    pts = rng.uniform(-600.0, 600.0, (CHUNK + 1, 3))
    sim = _bh(pos, mass, G, eps, 0.5)
    try:
        whole = sim.field_at(pts, terms=True)
        cut = 400001
        a, b = sim.field_at(pts[:cut], terms=True), sim.field_at(pts[cut:], terms=True)
        last = sim.field_at(pts[CHUNK:], terms=True)
        few = sim.field_at(pts[CHUNK - 40:CHUNK + 1], terms=True)
    finally:
        sim.close()
    assert _same(whole, [np.concatenate([x, y]) for x, y in zip(a, b)])
    assert _same([x[CHUNK:] for x in whole], last) and _same([x[CHUNK - 40:] for x in whole], few)
    assert whole[2].min() > 0 and np.isfinite(whole[0]).all()


@pytest.mark.parametrize("multipole", ["monopole", "quadrupole"])
def test_order_independence(gpu, monkeypatch, multipole):
    pos, mass, G, eps, _, _ = _case("tree_collision_2048")
    pts = _probe_points(pos, 19)
    perm = np.random.default_rng(0).permutation(M)
    sim = _bh(pos, mass, G, eps, 0.5, multipole=multipole)
    try:
        one = sim.field_at(pts, terms=True)
        assert _same(one, sim.field_at(pts, terms=True))  # a repeat
        shuffled = sim.field_at(pts[perm], terms=True)
        assert _same([x[perm] for x in one], shuffled)
        h1, h2 = sim.field_at(pts[:2000], terms=True), sim.field_at(pts[2000:], terms=True)
        assert _same(one, [np.concatenate([x, y]) for x, y in zip(h1, h2)])
        assert _same(one[:1], [sim.field_at(pts, potential=False)]) and _same(one[:2], sim.field_at(pts))
    finally:
        sim.close()
    monkeypatch.setenv("NBMI_FIELD_SORT", "0")  # read when the handle is created
    plain = _bh(pos, mass, G, eps, 0.5, multipole=multipole)
    try:
        assert _same(one, plain.field_at(pts, terms=True))
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
        acc, phi, terms = sim.field_at(pts, terms=True)
        again = sim.field_at(pts, terms=True)
    finally:
        sim.close()
    ra, rp, rt, _, _ = fr.direct_field(pts, pos, mass, 0.7, eps)
    assert np.array_equal(terms, rt) and terms[0] == n - 1 and terms[-1] == n
    assert np.all(np.abs(phi - rp) <= 1e-11 * np.abs(rp) + 1e-300)
    norm = np.sqrt((ra * ra).sum(1))
    assert np.all(np.sqrt(((acc - ra) ** 2).sum(1)) <= 1e-11 * norm + 1e-300), (n, eps)
    assert _same((acc, phi, terms), again)


@pytest.mark.parametrize("integrator,precision", [("kick_drift", "auto"), ("leapfrog", "auto"), ("kick_drift", "f32")])
def test_field_at_does_not_disturb_the_run(gpu, integrator, precision):
    pos, mass, G, eps, _, _ = _case("tree_galaxy_2048")
    vel = np.random.default_rng(4).normal(size=pos.shape) * 0.3
    pts = _probe_points(pos, 23)[:300]

    def run(query):
        sim = _bh(pos, mass, G, eps, 0.5, vel=vel, integrator=integrator)
        try:
            sim.set_force_precision(precision)
            shares, fields = [], []
            for _ in range(4):
                if query:
                    fields.append(sim.field_at(pts, terms=True))
                sim.step(0.2)
                shares.append(sim.force_precision_share())
            return sim.get_positions_f64(), sim.get_velocities(), sim.step_count(), shares, fields
        finally:
            sim.close()
    a, b = run(False), run(True)
    assert _same(a[:2], b[:2]) and a[2] == b[2] == 4
    assert a[3] == b[3], (a[3], b[3])
    # a leapfrog handle returns a plain handle's bits for the same state (the first call: the initial state)
    plain = _bh(pos, mass, G, eps, 0.5, vel=vel)
    try:
        assert _same(b[4][0], plain.field_at(pts, terms=True))
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
                sim.field_at(pts)
        pts = good.copy()
        pts[2, 0], pts[4, 2] = np.nan, np.inf
        with pytest.raises(ValueError, match="row 2"):  # the first bad row
            sim.field_at(pts)
        assert np.isfinite(sim.field_at(np.full((1, 3), 1e18))[1]).all()
        for shape in ((3,), (4, 2), (2, 3, 1)):
            with pytest.raises(ValueError, match=r"\(m, 3\)"):
                sim.field_at(np.zeros(shape))
        lib = gpu.load()
        assert lib.nbmi_field_at(sim._h, -1, gpu.ptr(good), None, None, None) == -1 and "negative" in gpu.last_error()
        assert lib.nbmi_field_at(sim._h, 5, None, None, None, None) == -1 and "null points_xyz" in gpu.last_error()
        before = sim.field_at(good, terms=True)
        sim.set_shard(0, len(pos) // 2)
        with pytest.raises(ValueError, match="sharded"):
            sim.field_at(good)
        sim.set_shard(0, len(pos))
        assert _same(before, sim.field_at(good, terms=True))
    finally:
        sim.close()


def test_recorder_writes_the_rotation_curve(gpu, tmp_path):
    """quick_galaxy cut to 4 096 bodies x 5 frames with --rotation-curve 2, in a process of its own: lines after the
    frames 1 and 3, each the curve of nbody/field.py about the line's own centre"""
    code = ("import sys; sys.path.insert(0, %r); import __graft_entry__ as g; g._import_package();"
            "from tools import record; sys.exit(record.main(sys.argv[1:]))") % ROOT
    argv = ["rot", "--preset", "quick_galaxy", "--bodies", "4096", "--frames", "5", "--root", str(tmp_path),
            "--rotation-curve", "2", "--curve-radii", "5,20,80,320"]
    subprocess.run([sys.executable, "-c", code, *argv], check=True, timeout=300)
    from tools import record as rec
    d = rec.get_recording_dir("rot", tmp_path)
    assert rec.load_metadata(d)["rotation_curve"] == {"every": 2, "radii": [5.0, 20.0, 80.0, 320.0]}
    rows = [json.loads(line) for line in (d / rec.ROTATION_FILE).read_text().splitlines()]
    assert [r["frame"] for r in rows] == [1, 3]
    for r in rows:
        assert sorted(r) == ["a_radial", "center", "frame", "phi", "radii", "v_circ"]
        assert r["radii"] == [5.0, 20.0, 80.0, 320.0] and len(r["center"]) == 3
        a, v, phi = (np.array(r[k]) for k in ("a_radial", "v_circ", "phi"))
        assert np.isfinite(a).all() and np.all(phi < 0.0) and np.all(np.diff(phi) > 0.0)
        assert np.array_equal(v, np.sqrt(np.array(r["radii"]) * np.maximum(a, 0.0))) and v[1] > 0.0
    assert rec.show_status("rot", root=tmp_path)
