"""Massless tracers on the device (include/nbmi.h nbmi_set_tracers) against the NumPy replay
(tests/tracer_ref.py), bit for bit: the replay takes its accelerations from nbmi_field_at of a twin handle that carries
no tracers, or - one body - from the header's closed form.  Also: the bodies are untouched, edge sizes, the chunk
boundary, the direct handle, interleaved queries, the growing pmax, retirement, the capacity error, the refusals and a
recorder session."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden
import tracer_ref as tr
from test_gpu_field import _probe_points

pytestmark = pytest.mark.gpu

PINS = ["tree_galaxy_2048", "tree_collision_2048", "tree_cluster_2048"]
CHUNK = 1048576  # the header's chunk
M = 4097
DT = 0.2


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _case(name):
    g = golden(name)
    pos, mass = np.ascontiguousarray(g["pos"], np.float64), np.ascontiguousarray(g["mass"], np.float64)
    vel = np.random.default_rng(4).normal(size=pos.shape) * 0.3
    for a in (pos, mass, vel):
        a.setflags(write=False)
    return pos, vel, mass, float(g["G"]), float(g["eps"])


def _bh(pos, vel, mass, G, eps, damping=1.0, theta=0.5, **kw):
    from nbody.gpu_backend import HIPBarnesHutSimulation
    return HIPBarnesHutSimulation(pos, vel, mass, G, eps, damping, theta, **kw)


def _direct(pos, vel, mass, G, eps, damping=1.0, **kw):
    from nbody.gpu_backend import HIPDirectSimulation
    return HIPDirectSimulation(pos, vel, mass, G, eps, damping, **kw)


def _replay_steps(A, B, rep, steps, dt=DT):
    """A carries the tracers, its twin B none: B's field before and after each of its steps drives the replay."""
    force = lambda pts: B.field_at(pts, potential=False)
    for _ in range(steps):
        rep.begin(dt, force)
        A.step(dt)
        B.step(dt)
        rep.end(dt, force)


def _bodies(sim):
    return sim.get_positions_f64(), sim.get_velocities()


def _tracer_seeds(pos, seed, m=M):
    """test_gpu_field's mixture of points (its fixed parts are about 2 400 of them) with random velocities"""
    pts = _probe_points(pos, seed, m)
    return pts, np.random.default_rng(seed + 1).normal(size=pts.shape) * 2.0


# ---- 1, 2: the replay through nbmi_field_at; the bodies are a plain handle's ----
@pytest.mark.parametrize("multipole", ["monopole", "quadrupole"])
@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
@pytest.mark.parametrize("name", PINS)
def test_replay_through_field_at_bit_for_bit(gpu, name, integrator, multipole):
    pos, vel, mass, G, eps = _case(name)
    p0, v0 = _tracer_seeds(pos, 7)
    for damping in (1.0, 0.99):
        for precision in ("auto", "f32"):
            A = _bh(pos, vel, mass, G, eps, damping, integrator=integrator, multipole=multipole)
            B = _bh(pos, vel, mass, G, eps, damping, integrator=integrator, multipole=multipole)
            try:
                for s in (A, B):
                    s.set_force_precision(precision)
                A.set_tracers(p0, v0)
                assert A.tracer_count == M and B.tracer_count == 0
                assert _same(A.get_tracers(), (p0, v0))
                rep = tr.TracerReplay(p0, v0, integrator, damping)
                _replay_steps(A, B, rep, 4)  # (leapfrog: the first of them primes)
                got = A.get_tracers()
                tag = (name, integrator, multipole, damping, precision)
                assert _same(got, (rep.p, rep.v)), (tag, int((_bits(got[0]) != _bits(rep.p)).any(axis=1).sum()))
                assert np.array_equal(A.tracer_positions_f32(), rep.p.astype(np.float32)), tag
                assert not np.array_equal(got[0], p0)
                # the bodies: B was asked for its field between the steps, which changes nothing
                assert _same(_bodies(A), _bodies(B)), tag
                assert A.force_precision_share() == B.force_precision_share(), tag
                assert A.diagnostics() == B.diagnostics(), tag
            finally:
                A.close()
                B.close()


@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
def test_bodies_untouched(gpu, integrator):
    """against a handle that never saw a tracer or a query: state, precision shares step by step, diagnostics, walk
    counters; tracers set in the middle of the run too"""
    pos, vel, mass, G, eps = _case("tree_galaxy_2048")
    p0, v0 = _tracer_seeds(pos, 9)

    def run(tracers):
        sim = _bh(pos, vel, mass, G, eps, integrator=integrator)
        try:
            shares = []
            if tracers:
                sim.set_tracers(p0, v0)
            for k in range(5):
                sim.step(DT)
                shares.append(sim.force_precision_share())
                if tracers and k == 2:
                    sim.set_tracers(p0[:100])
            return _bodies(sim), shares, sim.diagnostics(), sim.walk_counters(), sim.step_count()
        finally:
            sim.close()
    a, b = run(False), run(True)
    assert _same(a[0], b[0])
    assert a[1:] == b[1:]


# ---- 3: one body, the closed form ----
@pytest.mark.parametrize("eps", [0.0, 0.05])
@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
@pytest.mark.parametrize("method", ["tree", "direct"])
def test_one_body_is_the_closed_form(gpu, method, integrator, eps):
    c = np.array([[3.0, -2.0, 0.5]])
    G, m = 0.7, np.array([5.0])
    rng = np.random.default_rng(1)
    p0 = np.concatenate([c, c + rng.normal(size=(130, 3)) * 4.0, c + rng.normal(size=(3, 3)) * 1e4])
    v0 = rng.normal(size=p0.shape)
    v0[0] = [0.25, -0.5, 1.0]  # the tracer on the body: dist_sq = eps^2, no term
    make = _bh if method == "tree" else _direct
    for damping in (1.0, 0.97):
        sim = make(c, np.zeros_like(c), m, G, eps, damping, integrator=integrator)
        try:
            sim.set_tracers(p0, v0)
            rep = tr.TracerReplay(p0, v0, integrator, damping)
            force = tr.point_mass_field(c[0], G * m[0], eps)
            for k in range(5):
                sim.step(0.05)
                rep.step(0.05, force)
                if k == 0:  # on the body: no term, so the first drift is a straight line (kick-drift damps before it)
                    v1 = (v0[0] + 0.0) * damping if integrator == "kick_drift" else v0[0]
                    assert np.array_equal(sim.get_tracers()[0][0], p0[0] + v1 * 0.05)
            assert np.array_equal(sim.get_positions_f64(), c)
            assert _same(sim.get_tracers(), (rep.p, rep.v)), (method, integrator, eps, damping)
        finally:
            sim.close()


# ---- 4: edge sizes ----
@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
def test_edge_sizes(gpu, integrator):
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 64, 65):
        pos = rng.normal(size=(n, 3)) * 20.0
        vel = rng.normal(size=(n, 3)) * 0.5
        mass = rng.uniform(0.5, 2.0, n)
        A, B = (_bh(pos, vel, mass, 0.7, 0.1, integrator=integrator) for _ in range(2))
        try:
            for m in (1, 63, 64, 65):  # (every set_tracers replaces the last set, with another m)
                p0 = rng.normal(size=(m, 3)) * 30.0
                p0[0] = B.get_positions_f64()[0]
                v0 = rng.normal(size=(m, 3))
                A.set_tracers(p0, v0)
                assert A.tracer_count == m
                rep = tr.TracerReplay(p0, v0, integrator)
                _replay_steps(A, B, rep, 3)
                assert _same(A.get_tracers(), (rep.p, rep.v)), (n, m)
            assert _same(_bodies(A), _bodies(B))
        finally:
            A.close()
            B.close()


@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
@pytest.mark.parametrize("method", ["tree", "direct"])
def test_no_bodies_no_tracers_and_replacement(gpu, method, integrator):
    make = _bh if method == "tree" else _direct
    rng = np.random.default_rng(8)
    p0, v0 = rng.normal(size=(70, 3)), rng.normal(size=(70, 3))
    sim = make(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), 1.0, 0.1, 0.98, integrator=integrator)
    try:  # N == 0: straight lines
        sim.set_tracers(p0, v0)
        sim.step(0.1)
        sim.step_many(0.1, 2)
        rep = tr.TracerReplay(p0, v0, integrator, 0.98)
        for _ in range(3):
            rep.step(0.1, lambda pts: np.zeros_like(pts))
        assert _same(sim.get_tracers(), (rep.p, rep.v))
    finally:
        sim.close()
    pos, vel, mass, G, eps = _case("tree_cluster_2048")
    sim = make(pos, vel, mass, G, eps, integrator=integrator)
    try:
        assert sim.tracer_count == 0
        p, v = sim.get_tracers()
        assert p.shape == v.shape == (0, 3) and sim.tracer_positions_f32().shape == (0, 3)
        sim.set_tracers(p0)  # no velocities: at rest
        assert _same(sim.get_tracers(), (p0, np.zeros_like(p0)))
        sim.step(DT)
        sim.set_tracers(p0[:5], v0[:5])
        assert sim.tracer_count == 5 and _same(sim.get_tracers(), (p0[:5], v0[:5]))
        sim.set_tracers(np.zeros((0, 3)))  # m == 0 removes them
        assert sim.tracer_count == 0 and sim.get_tracers()[0].shape == (0, 3)
        sim.step(DT)
        sim.set_tracers(p0, v0)
        sim.step(DT)
        assert sim.tracer_count == 70 and np.isfinite(sim.get_tracers()[0]).all()
        lib = gpu.load()
        assert lib.nbmi_tracer_count(None) == -1
        only_v = np.empty((70, 3))
        assert lib.nbmi_get_tracers_f64(sim._h, None, gpu.ptr(only_v)) == 0  # either pointer may be NULL
        assert np.array_equal(only_v, sim.get_tracers()[1])
    finally:
        sim.close()


# ---- 5: the chunk boundary ----
_CHILD = """
import sys
sys.path.insert(0, {root!r})
import __graft_entry__ as g
g._import_package()
import numpy as np
from nbody.gpu_backend import HIPBarnesHutSimulation
d = np.load(sys.argv[1])
sim = HIPBarnesHutSimulation(d["pos"], d["vel"], d["mass"], 0.7, 0.1, 1.0, 0.5, integrator=sys.argv[3])
sim.set_tracers(d["p0"], d["v0"])
sim.step_many({dt!r}, 2)
p, v = sim.get_tracers()
sim.close()
np.savez(sys.argv[2], p=p, v=v)
"""


@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
def test_chunk_boundary(gpu, tmp_path, integrator):
    """CHUNK + 1 tracers over 65 bodies: the second chunk is one tracer.  A tracer's row does not depend on the others."""
    rng = np.random.default_rng(3)
    pos, vel, mass = rng.normal(size=(65, 3)) * 20.0, rng.normal(size=(65, 3)) * 0.5, rng.uniform(0.5, 2.0, 65)
    m = CHUNK + 1
    p0, v0 = rng.uniform(-60.0, 60.0, (m, 3)), rng.normal(size=(m, 3))
    perm = rng.permutation(m)
    cut = 400001

    def run(p, v):
        sim = _bh(pos, vel, mass, 0.7, 0.1, integrator=integrator)
        try:
            sim.set_tracers(p, v)
            sim.step_many(DT, 2)
            return sim.get_tracers()
        finally:
            sim.close()
    whole = run(p0, v0)
    halves = [run(p0[:cut], v0[:cut]), run(p0[cut:], v0[cut:])]
    assert _same(whole, [np.concatenate([a, b]) for a, b in zip(*halves)])
    assert _same([x[perm] for x in whole], run(p0[perm], v0[perm]))
    assert np.isfinite(whole[0]).all() and not np.array_equal(whole[1], v0)
    np.savez(tmp_path / "in.npz", pos=pos, vel=vel, mass=mass, p0=p0, v0=v0)
    env = dict(os.environ, NBMI_FIELD_SORT="0")  # read when the handle is created
    subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, dt=DT), str(tmp_path / "in.npz"), str(tmp_path / "out.npz"),
                    integrator], check=True, timeout=120, env=env)
    out = np.load(tmp_path / "out.npz")
    assert _same(whole, (out["p"], out["v"]))


# ---- 6: the direct handle ----
@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
def test_direct_handle(gpu, integrator):
    g = golden("direct_galaxy_2048")
    pos, mass = np.ascontiguousarray(g["pos"], np.float64), np.ascontiguousarray(g["mass"], np.float64)
    assert len(pos) == 2048
    G, eps = float(g["G"]), float(g["eps"])
    vel = np.random.default_rng(4).normal(size=pos.shape) * 0.3
    p0, v0 = _tracer_seeds(pos, 13, 2500)
    A, B = (_direct(pos, vel, mass, G, eps, 0.99, integrator=integrator) for _ in range(2))
    try:
        A.set_tracers(p0, v0)
        rep = tr.TracerReplay(p0, v0, integrator, 0.99)
        _replay_steps(A, B, rep, 4)
        assert _same(A.get_tracers(), (rep.p, rep.v))
        assert _same(_bodies(A), _bodies(B))
    finally:
        A.close()
        B.close()


# ---- 7: interleaving ----
@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
def test_queries_between_the_steps_change_nothing(gpu, integrator):
    pos, vel, mass, G, eps = _case("tree_collision_2048")
    p0, v0 = _tracer_seeds(pos, 17)

    def run(apart):
        sim = _bh(pos, vel, mass, G, eps, integrator=integrator)
        try:
            sim.set_tracers(p0, v0)
            if not apart:
                sim.step_many(DT, 4)
            for _ in range(4 if apart else 0):
                sim.step_many(DT, 1)
                sim.get_tracers()
                sim.field_at(p0[:300])
                sim.knn(8)
                sim.potentials()
            return sim.get_tracers() + _bodies(sim)
        finally:
            sim.close()
    assert _same(run(False), run(True))


# ---- 8: pmax grows on the device ----
@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
def test_a_tracer_that_leaves_the_root_cube_fast(gpu, integrator):
    pos, vel, mass, G, eps = _case("tree_galaxy_2048")
    bounds = np.abs(pos).max() * 1.1 + 10.0
    p0, v0 = _tracer_seeds(pos, 21, 2500)
    p0[5], v0[5] = pos[10], [60.0 * bounds / DT, -45.0 * bounds / DT, 0.0]  # 100 root cubes within two steps
    A, B = (_bh(pos, vel, mass, G, eps, integrator=integrator) for _ in range(2))
    try:
        A.set_tracers(p0, v0)
        rep = tr.TracerReplay(p0, v0, integrator)
        _replay_steps(A, B, rep, 4)
        got = A.get_tracers()
        assert np.abs(got[0][5]).max() > 100.0 * bounds
        assert _same(got, (rep.p, rep.v))
    finally:
        A.close()
        B.close()


# ---- 9: retirement ----
@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
def test_a_tracer_beyond_1e18_retires(gpu, integrator):
    pos, vel, mass, G, eps = _case("tree_cluster_2048")
    p0, v0 = _tracer_seeds(pos, 25, 2500)
    p0[3], v0[3] = [9e17, 0.0, 0.0], [3e17 / DT, 0.0, 0.0]  # past 1e18 with the first drift
    p0[130], v0[130] = [0.0, -9e17, 1.0], [0.0, -1e308, 0.0]  # as far as a finite velocity takes it
    A, B = (_bh(pos, vel, mass, G, eps, integrator=integrator) for _ in range(2))
    try:
        A.set_tracers(p0, v0)
        rep = tr.TracerReplay(p0, v0, integrator)
        _replay_steps(A, B, rep, 1)
        first = A.get_tracers()
        assert _same(first, (rep.p, rep.v))
        assert first[0][3, 0] > 1e18 and first[0][130, 1] < -1e300
        _replay_steps(A, B, rep, 3)
        last = A.get_tracers()
        assert _same(last, (rep.p, rep.v))
        for k in (3, 130):  # retired: the rows stay as they are
            assert _same([x[k] for x in last], [x[k] for x in first])
        others = np.setdiff1d(np.arange(2500), [3, 130])
        assert not np.array_equal(last[0][others], first[0][others]) and np.isfinite(last[0][others]).all()
    finally:
        A.close()
        B.close()


# ---- 10: a substep whose octree does not fit ----
@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
def test_capacity_error_freezes_tracers_and_bodies(gpu, integrator):
    """test_gpu_nbody's construction: G = 0, 1 500 pairs that meet to within 1e-9 after exactly one step, where the
    octree no longer fits.  Kick-drift builds before it moves: substep 1 completes, 2 and 3 freeze.  Leapfrog drifts
    first: substep 1 freezes already."""
    n_pairs, dt, sep = 1500, 0.1, 1.0
    rng = np.random.RandomState(7)
    base = rng.uniform(-50, 50, (n_pairs, 3))
    pos = np.concatenate([base, base + [sep, 0.0, 0.0]])
    vv = (sep - 1e-9) / (2 * dt)
    vel = np.concatenate([np.tile([vv, 0.0, 0.0], (n_pairs, 1)), np.tile([-vv, 0.0, 0.0], (n_pairs, 1))])
    p0, v0 = rng.uniform(-60, 60, (300, 3)), rng.normal(size=(300, 3))
    sim = _bh(pos, vel, np.ones(2 * n_pairs), 0.0, 0.1, integrator=integrator)
    try:
        sim.set_tracers(p0, v0)
        sim.step_many(dt, 3)
        with pytest.raises(RuntimeError, match="octree needs"):
            sim.sync()
        done = 1 if integrator == "kick_drift" else 0
        p, v = sim.get_tracers()  # reported once
        assert np.array_equal(sim.get_positions_f64(), pos + vel * dt * done)
        assert np.array_equal(p, p0 + v0 * dt * done) and np.array_equal(v, v0)
        sim.set_state(pos, -vel)  # moving apart: the handle steps again, the tracers from where they are
        sim.step(dt)
        sim.sync()
        assert np.array_equal(sim.get_tracers()[0], p + v0 * dt)
    finally:
        sim.close()


# ---- 11: refusals ----
def test_refusals(gpu):
    pos, vel, mass, G, eps = _case("tree_cluster_2048")
    sim = _bh(pos, vel, mass, G, eps)
    try:
        good = np.random.default_rng(2).normal(size=(5, 3))
        sim.set_tracers(good, good)
        for bad in (np.nan, np.inf, -np.inf, 1e19, -1e19):
            pts = good.copy()
            pts[3, 1] = bad
            with pytest.raises(ValueError, match="positions_xyz row 3"):
                sim.set_tracers(pts)
            if not np.isfinite(bad):
                with pytest.raises(ValueError, match="velocities_xyz row 3"):
                    sim.set_tracers(good, pts)
        sim.set_tracers(good, np.full((5, 3), 1e19))  # a velocity only has to be finite
        pts = good.copy()
        pts[2, 0], pts[4, 2] = np.nan, np.inf
        with pytest.raises(ValueError, match="row 2"):  # the first bad row
            sim.set_tracers(pts)
        for shape in ((3,), (4, 2), (2, 3, 1)):
            with pytest.raises(ValueError, match=r"\(m, 3\)"):
                sim.set_tracers(np.zeros(shape))
        with pytest.raises(ValueError, match="velocities of shape"):
            sim.set_tracers(good, np.zeros((4, 3)))
        lib = gpu.load()
        assert lib.nbmi_set_tracers(sim._h, -1, gpu.ptr(good), None) == -1 and "negative" in gpu.last_error()
        assert lib.nbmi_set_tracers(sim._h, 5, None, None) == -1 and "null positions_xyz" in gpu.last_error()
        assert lib.nbmi_set_tracers(sim._h, 2 ** 26 + 1, gpu.ptr(good), None) == -1 and "largest" in gpu.last_error()
        sim.set_tracers(good, good)
        assert sim.tracer_count == 5  # a refused call leaves the tracers as they were
        with pytest.raises(ValueError, match="tracers"):  # a proper shard, in both orders of the calls
            sim.set_shard(0, len(pos) // 2)
        sim.set_shard(0, len(pos))
        sim.set_tracers(np.zeros((0, 3)))
        sim.set_shard(0, len(pos) // 2)
        with pytest.raises(ValueError, match="sharded"):
            sim.set_tracers(good)
        assert sim.tracer_count == 0
    finally:
        sim.close()


def test_owner_mode_refuses(gpu):
    from nbody.gpu_backend import HIPOwnerSimulation
    called = []

    class NoLibrary:
        def __getattr__(self, name):
            called.append(name)
            raise AssertionError(name)
    owner = HIPOwnerSimulation.__new__(HIPOwnerSimulation)  # refused before the library is called
    owner._lib, owner._h = NoLibrary(), None
    with pytest.raises(ValueError, match="owner-mode"):
        owner.set_tracers(np.zeros((2, 3)))
    assert not called
    # the library's own refusal, through diag_refuse
    rng = np.random.default_rng(0)
    pos, mass = rng.normal(size=(256, 3)) * 10.0, np.ones(256)
    from nbody.sharded import let_capacities
    cap, let = let_capacities(256, 1)
    real = HIPOwnerSimulation(pos, np.zeros_like(pos), mass, np.arange(256), cap, let, 1, 0, 1.0, 0.1, 1.0)
    try:
        assert gpu.load().nbmi_set_tracers(real._h, 2, gpu.ptr(pos), None) == -1
        assert "nbmi_set_tracers: owner-mode" in gpu.last_error()
    finally:
        real.close()


# ---- 12: a recorder session ----
def test_recorder_session_with_tracers_resumed_once(gpu, tmp_path):
    """quick_galaxy cut to 4 096 bodies with --tracers / --tracers-every 2, each run in a process of its own and with a
    state checkpoint every 3 frames: 4 frames extended by 4 (the resume starts from the checkpoint after frame 2, tracers
    included) against 8 frames in one go."""
    import json
    code = ("import sys; sys.path.insert(0, %r); import __graft_entry__ as g; g._import_package();"
            "from tools import record; record.STATE_EVERY = 3; sys.exit(record.main(sys.argv[1:]))") % ROOT
    rng = np.random.default_rng(12)
    seeds = np.concatenate([rng.normal(size=(300, 3)) * 120.0, rng.normal(size=(300, 3)) * 3.0], axis=1)
    np.save(tmp_path / "seeds.npy", seeds)
    common = ["--preset", "quick_galaxy", "--bodies", "4096", "--root", str(tmp_path), "--seed", "5",
              "--tracers", str(tmp_path / "seeds.npy"), "--tracers-every", "2"]

    def run(*argv):
        subprocess.run([sys.executable, "-c", code, *argv], check=True, timeout=300)
    run("whole", "--frames", "8", *common)
    run("cut", "--frames", "4", *common)
    run("cut", "--extend", "4", "--root", str(tmp_path))
    from tools import record as rec
    whole, cut = rec.get_recording_dir("whole", tmp_path), rec.get_recording_dir("cut", tmp_path)
    names = [f"tracers_{f:06d}.npy" for f in (1, 3, 5, 7)]
    assert sorted(p.name for p in cut.glob("tracers_*.npy")) == names == sorted(p.name for p in whole.glob("tracers_*.npy"))
    for name in names:
        a, b = np.load(whole / name), np.load(cut / name)
        assert a.dtype == np.float32 and a.shape == (300, 3) and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    assert not np.array_equal(np.load(whole / names[0]), np.load(whole / names[-1]))
    meta = json.loads((cut / "metadata.json").read_text())
    assert meta["tracers"] == {"file": str((tmp_path / "seeds.npy").resolve()), "every": 2} and meta["total_frames"] == 8
    with np.load(cut / "state_0005.npz") as st, np.load(whole / "state_0005.npz") as sw:
        assert sorted(st.files) == ["masses", "positions", "tracer_positions", "tracer_velocities", "velocities"]
        for k in st.files:
            assert np.array_equal(st[k], sw[k]), k
        assert st["tracer_positions"].shape == (300, 3) and st["tracer_positions"].dtype == np.float64
    assert rec.show_status("cut", root=tmp_path)
