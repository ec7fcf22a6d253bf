"""The topological interaction (include/bdmi.h: the k nearest neighbours within sight; csrc/bdmi.hip `k_flock_topo`)
against its NumPy restatement (tests/topo_ref.py).  The specification fixes the neighbour order and the summation
order, so every comparison here is bit for bit, the separation force included.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import boids_cases as BC
import boids_ref as R
import topo_ref as T
from test_gpu_boids import RawFlock

pytestmark = pytest.mark.gpu

METRIC, TOPOLOGICAL = 0, 1
KS = (1, 7, 8, 9, 16)
CASES = ("thresholds", "hit_list", "run_length_4097", "mixed_lanes", "grid_3", "grid_33", "grid_64", "perception_2.5",
         "perception_7.25")


# ---- raw calls ------------------------------------------------------------------------------------------------------
def set_mode(f, mode, k=7):
    return f.lib.bdmi_set_neighbour_mode(f.h, mode, k)


def get_mode(f):
    mode, k = C.c_int(-5), C.c_int(-5)
    assert f.lib.bdmi_get_neighbour_mode(f.h, C.addressof(mode), C.addressof(k)) == 0, f.nat.last_error()
    return int(mode.value), int(k.value)


def hook(f, k):
    ids = np.full((f.n, k), -7, dtype=np.int32)
    d2 = np.full((f.n, k), -7.0)
    count = np.full(f.n, -7, dtype=np.int32)
    f.nat.check(f.lib.bdmi_topological_neighbours(f.h, k, f.nat.ptr(ids), f.nat.ptr(d2), f.nat.ptr(count)), "hook")
    return ids, d2, count


def topo_flock(nat, pos, vel, col, prm, k):
    f = RawFlock(nat, pos, vel, col, prm)
    assert set_mode(f, TOPOLOGICAL, k) == 0, nat.last_error()
    return f


def same_state(a, b):
    return all(R.same_bits(x, y) for x, y in zip(a, b))


# ---- the constructed cases --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    """The case and its rows at k = 16, computed once: the rows of a smaller k are their prefix."""
    if name.startswith("run_length_"):
        c = BC.run_length(int(name.rsplit("_", 1)[1]))
    elif name.startswith("grid_"):
        c = BC.grid_dims(int(name.split("_")[1]))
    elif name in ("mixed_lanes", "hit_list", "thresholds"):
        c = getattr(BC, name)()
    else:
        c = next(x for x in BC.parameter_cases() if x["name"] == name)
    return c, T.neighbours(c["pos"], c["params"], T.K_MAX)


def _check(nat, pos, vel, col, prm, dt, k, rows, what):
    """Hook rows, bdmi_get_forces and one bdmi_step against the restatement."""
    F = T.flocking(pos, vel, col, prm, k, nb=rows)
    f = RawFlock(nat, pos, vel, col, prm)
    try:
        ids, d2, count = hook(f, k)  # in metric mode: the hook takes its own k
        bad = np.flatnonzero(np.any(ids != rows["ids"], axis=1))
        assert len(bad) == 0, (what, "ids", len(bad), bad[:5], ids[bad[:3]], rows["ids"][bad[:3]])
        assert R.same_bits(d2, rows["d2"]) and np.array_equal(count, rows["count"]), what
        assert set_mode(f, TOPOLOGICAL, k) == 0, nat.last_error()
        got = f.forces()
        for g, w, name in zip(got, (F.sep, F.ali, F.coh, F.avg), ("sep", "ali", "coh", "avg")):
            bad = np.flatnonzero(np.any(g != w, axis=1))
            assert R.same_bits(g, w), (what, name, len(bad), bad[:5], F.nb[bad[:5]])
        f.step(dt)
        want = R.physics(pos, vel, col, (F.sep, F.ali, F.coh, F.avg), prm, dt)
        assert same_state(f.state(), want), what
    finally:
        f.close()
    return F


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", CASES)
def test_cases_match_restatement(gpu, name, k):
    c, rows16 = _case(name)
    rows = T.first_k(rows16, k)
    F = _check(gpu, c["pos"], c["vel"], c["col"], c["params"], c["dt"], k, rows, (name, k))
    print(f"{name} k={k}: n={len(c['pos'])} metric neighbours up to {rows['metric'].max()}, lists full for "
          f"{(F.nb == k).mean():.0%}, never filled for {(rows['metric'] < k).mean():.0%}")
    if name == "hit_list":  # lists that never fill, just fill and overflow many times
        assert (rows["metric"] < k).any() and (rows["metric"] == k).any() and (rows["metric"] > 4 * k).any()
    if name in ("run_length_4097", "mixed_lanes"):  # runs above 4095, thousands of candidates on the lattice
        assert BC.grid_facts(c["pos"], c["params"])["big"].any()
        print(f"  boids with an exact d2 tie among their first 16: {(~T.distinct_d2(rows16)).sum()}")


@pytest.mark.parametrize("k", KS)
def test_ties_break_by_id(gpu, k):
    """A cubic lattice of spacing 1 in shuffled id order: 6 neighbours at d2 = 1, 12 at 2, 8 at 3, 6 at 4, ... - every
    list is cut inside a group of equal d2, where only the ids decide."""
    rng = np.random.default_rng(k)
    g = np.stack(np.meshgrid(*[np.arange(7.0)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) - 3.0
    pos = np.ascontiguousarray(g[rng.permutation(len(g))])
    prm = BC.params(bounds=8.0)
    _, vel, col = _random_state(len(pos), k, 8.0)
    rows = T.neighbours(pos, prm, k)
    assert (~T.distinct_d2(T.neighbours(pos, prm, min(k + 1, T.K_MAX)))).all() or k == 16
    assert (rows["metric"] > k).all()
    _check(gpu, pos, vel, col, prm, BC.DT, k, rows, ("ties", k))


def _random_state(n, seed, bounds, lattice=True):
    rng = np.random.default_rng(seed)
    pos, vel = rng.uniform(-bounds, bounds, (n, 3)), rng.uniform(-12.5, 12.5, (n, 3))
    if lattice:
        pos, vel = R.lattice(pos, BC.PB), R.lattice(vel, BC.VB)
    return pos, vel, (R.id_colours(n) if lattice else rng.random((n, 3)))


@pytest.mark.parametrize("k", [7, 16])
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257])
def test_sizes(gpu, n, k):
    """Block edges of both tiers (256 and 128 threads per block), and the empty and single-boid flocks."""
    prm = BC.params(bounds=6.0)
    pos, vel, col = _random_state(n, 100 + n, 6.0)
    F = _check(gpu, pos, vel, col, prm, BC.DT, k, T.neighbours(pos, prm, k), (n, k))
    if n <= 1:
        assert not F.nb.any() and not np.any(F.sep) and not np.any(F.ali) and not np.any(F.coh)
    if n >= 255:
        assert (F.nb == k).any()


def test_trajectory(gpu):
    """2 000 boids at about 20 metric neighbours each, k = 7: ten steps against the replay, step by step."""
    n, k, bounds = 2000, 7, 18.7
    prm = BC.params(bounds=bounds)
    pos, vel, col = _random_state(n, 11, bounds)
    assert 15 < T.neighbours(pos, prm, k)["metric"].mean() < 25
    f = topo_flock(gpu, pos, vel, col, prm, k)
    try:
        for s in range(10):
            f.step(BC.DT)
            pos, vel, col = T.step(pos, vel, col, prm, k, BC.DT)
            assert same_state(f.state(), (pos, vel, col)), s
    finally:
        f.close()


def test_order_independence(gpu, monkeypatch):
    """A permutation of the caller order gives the permuted forces and the permuted state after 5 steps, and the
    hardware block order (BDMI_XCD=0) the same bits as the default one."""
    n, k, bounds = 3000, 7, 21.5
    prm = BC.params(bounds=bounds)
    for seed in range(20, 30):  # a seed without two equal d2 among any boid's first k + 1: no tie for the ids to break
        pos, vel, col = _random_state(n, seed, bounds, lattice=False)
        if T.distinct_d2(T.neighbours(pos, prm, k + 1)).all():
            break
    else:
        raise AssertionError("no tie-free seed")
    perm = np.random.default_rng(1).permutation(n)

    def run(p, v, c):
        f = topo_flock(gpu, np.ascontiguousarray(p), np.ascontiguousarray(v), np.ascontiguousarray(c), prm, k)
        try:
            forces = f.forces()
            f.step(BC.DT, 5)
            return forces, f.state()
        finally:
            f.close()

    monkeypatch.delenv("BDMI_XCD", raising=False)
    forces, state = run(pos, vel, col)
    F = T.flocking(pos, vel, col, prm, k)
    assert same_state(forces, (F.sep, F.ali, F.coh, F.avg))
    forces_p, state_p = run(pos[perm], vel[perm], col[perm])
    assert same_state(forces_p, [a[perm] for a in forces]) and same_state(state_p, [a[perm] for a in state])
    monkeypatch.setenv("BDMI_XCD", "0")
    forces_x, state_x = run(pos, vel, col)
    assert same_state(forces_x, forces) and same_state(state_x, state)


# ---- mode hygiene -----------------------------------------------------------------------------------------------------
def _metric_run(nat, pos, vel, col, prm, steps=5, before=None):
    f = RawFlock(nat, pos, vel, col, prm)
    try:
        if before:
            before(f)
        f.step(BC.DT, steps)
        return f.state()
    finally:
        f.close()


def test_default_mode_and_round_trip(gpu, monkeypatch):
    monkeypatch.delenv("BDMI_NEIGHBOURS", raising=False)
    prm = BC.params(bounds=12.0)
    pos, vel, col = _random_state(1500, 3, 12.0)
    fresh = _metric_run(gpu, pos, vel, col, prm)

    def there_and_back(f):
        assert get_mode(f) == (METRIC, 7)
        assert set_mode(f, TOPOLOGICAL, 7) == 0 and get_mode(f) == (TOPOLOGICAL, 7)
        assert set_mode(f, TOPOLOGICAL, 12) == 0 and get_mode(f) == (TOPOLOGICAL, 12)
        assert set_mode(f, METRIC, 99) == 0 and get_mode(f) == (METRIC, 12)  # k ignored, and kept
        # either output of the getter may be null
        k = C.c_int(0)
        assert f.lib.bdmi_get_neighbour_mode(f.h, None, C.addressof(k)) == 0 and k.value == 12
        assert f.lib.bdmi_get_neighbour_mode(f.h, None, None) == 0

    assert same_state(_metric_run(gpu, pos, vel, col, prm, before=there_and_back), fresh)

    def hooked(f):  # the hook in metric mode works and leaves the next step's bits alone
        ids, d2, count = hook(f, 7)
        rows = T.neighbours(pos, prm, 7)
        assert np.array_equal(ids, rows["ids"]) and R.same_bits(d2, rows["d2"]) and np.array_equal(count, rows["count"])
        assert f.lib.bdmi_topological_neighbours(f.h, 3, None, None, None) == 0  # each output may be null
        assert get_mode(f) == (METRIC, 7)

    assert same_state(_metric_run(gpu, pos, vel, col, prm, before=hooked), fresh)
    # and metric mode is not the topological one: the two rules differ on this state
    f = topo_flock(gpu, pos, vel, col, prm, 7)
    f.step(BC.DT, 5)
    assert not same_state(f.state(), fresh)
    f.close()


def test_analysis_calls_between_topological_steps_change_nothing(gpu):
    prm = BC.params(bounds=12.0)
    pos, vel, col = _random_state(1500, 4, 12.0)
    out = []
    for with_calls in (False, True):
        f = topo_flock(gpu, pos, vel, col, prm, 7)
        try:
            for _ in range(3):
                f.step(BC.DT)
                if with_calls:
                    lib, nat = f.lib, gpu
                    row = np.empty(16)
                    cnt, nn = np.empty(f.n, np.int32), np.empty(f.n)
                    labels = np.empty(f.n, np.int32)
                    nat.check(lib.bdmi_flocks(f.h, 5.0, nat.ptr(labels), None, None, None), "bdmi_flocks")
                    nat.check(lib.bdmi_diagnostics(f.h, nat.ptr(row)), "bdmi_diagnostics")
                    nat.check(lib.bdmi_neighbour_stats(f.h, 5.0, nat.ptr(cnt), nat.ptr(nn), None), "bdmi_neighbour_stats")
                    hook(f, 16)
                    hook(f, 3)
                    f.forces()
            out.append(f.state())
        finally:
            f.close()
    assert same_state(out[0], out[1])


@pytest.mark.parametrize("value,want", [("topological:5", (TOPOLOGICAL, 5)), ("topological", (TOPOLOGICAL, 7)),
                                        ("topological:16", (TOPOLOGICAL, 16)), ("topological:17", (METRIC, 7)),
                                        ("topological:0", (METRIC, 7)), ("topological:5x", (METRIC, 7)),
                                        ("metric", (METRIC, 7)), ("", (METRIC, 7))])
def test_environment_sets_the_initial_mode(gpu, monkeypatch, value, want):
    monkeypatch.setenv("BDMI_NEIGHBOURS", value)
    prm = BC.params(bounds=12.0)
    pos, vel, col = _random_state(64, 5, 12.0)
    f = RawFlock(gpu, pos, vel, col, prm)
    try:
        assert get_mode(f) == want
        if want == (TOPOLOGICAL, 5):  # and the handle sweeps in that mode
            F = T.flocking(pos, vel, col, prm, 5)
            assert same_state(f.forces(), (F.sep, F.ali, F.coh, F.avg))
    finally:
        f.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _refused(nat, rc, call):
    assert rc == -1 and nat.last_error().startswith(call + ": "), (rc, nat.last_error())
    return nat.last_error()


def test_refusals(gpu, monkeypatch):
    monkeypatch.setenv("BDMI_NEIGHBOURS", "topological:5")  # a slab handle does not take it
    lib = gpu.load()
    prm = BC.params(bounds=30.0)
    n = 64
    pos, vel, col = _random_state(n, 6, 20.0)
    f = RawFlock(gpu, pos, vel, col, prm)
    ids = np.arange(n, dtype=np.int32)
    slab = lib.bdmi_create_slab(n, gpu.ptr(pos), gpu.ptr(vel), gpu.ptr(col), gpu.ptr(ids), 2 * n, gpu.ptr(prm), -35.0, 35.0,
                                0, 0, 0)
    assert slab, gpu.last_error()
    try:
        assert get_mode(f) == (TOPOLOGICAL, 5)
        for mode in (-1, 2, 7):
            assert "mode" in _refused(gpu, set_mode(f, mode, 7), "bdmi_set_neighbour_mode")
        for k in (0, -3, 17, 1 << 20):
            assert f"k = {k}" in _refused(gpu, set_mode(f, TOPOLOGICAL, k), "bdmi_set_neighbour_mode")
        assert get_mode(f) == (TOPOLOGICAL, 5)
        out = np.full((n, 17), -7, dtype=np.int32), np.full((n, 17), -7.0), np.full(n, -7, dtype=np.int32)
        for k in (0, -1, 17):
            rc = lib.bdmi_topological_neighbours(f.h, k, *[gpu.ptr(a) for a in out])
            assert f"k = {k}" in _refused(gpu, rc, "bdmi_topological_neighbours")
        # null handles
        _refused(gpu, lib.bdmi_set_neighbour_mode(None, TOPOLOGICAL, 7), "bdmi_set_neighbour_mode")
        _refused(gpu, lib.bdmi_get_neighbour_mode(None, None, None), "bdmi_get_neighbour_mode")
        _refused(gpu, lib.bdmi_topological_neighbours(None, 7, *[gpu.ptr(a) for a in out]), "bdmi_topological_neighbours")
        # a slab handle: metric whatever the environment says, and it stays so
        sf = RawFlock.__new__(RawFlock)
        sf.lib, sf.nat, sf.n, sf.h = lib, gpu, n, slab
        assert get_mode(sf) == (METRIC, 7)
        assert "slab" in _refused(gpu, set_mode(sf, TOPOLOGICAL, 7), "bdmi_set_neighbour_mode")
        assert "slab" in _refused(gpu, set_mode(sf, METRIC, 7), "bdmi_set_neighbour_mode")
        rc = lib.bdmi_topological_neighbours(slab, 7, *[gpu.ptr(a) for a in out])
        assert "slab" in _refused(gpu, rc, "bdmi_topological_neighbours")
        assert get_mode(sf) == (METRIC, 7)
        assert all((a == -7).all() for a in out)  # outputs untouched by every refusal
        gpu.check(lib.bdmi_step(slab, BC.DT, 1), "bdmi_step")  # the slab handle still steps (metric)
        gpu.check(lib.bdmi_sync(slab), "bdmi_sync")
    finally:
        f.close()
        lib.bdmi_destroy(slab)


def test_flock_class(gpu, monkeypatch):
    """boids.Flock: set_neighbour_mode, neighbour_mode, topological_neighbours and their errors."""
    import config.boids as bcfg
    from boids import Flock
    from boids.analysis import neighbour_rank_profile
    monkeypatch.delenv("BDMI_NEIGHBOURS", raising=False)
    saved = dict(bcfg.BOIDS)
    bcfg.BOIDS["bounds"] = 15.0
    try:
        fl = Flock(2048, seed=7)
        prm = np.array([float(bcfg.BOIDS[key]) for key in bcfg.PARAM_ORDER], dtype=np.float64)
    finally:
        bcfg.BOIDS.clear()
        bcfg.BOIDS.update(saved)
    try:
        assert fl.neighbour_mode == ("metric", 7)
        fl.set_neighbour_mode("topological", k=9)
        assert fl.neighbour_mode == ("topological", 9)
        pos, vel, col = fl.positions.copy(), fl.velocities.copy(), fl.colors.copy()
        rows = T.neighbours(pos, prm, 9)
        got = fl.topological_neighbours()
        assert got["ids"].shape == (2048, 9) and np.array_equal(got["ids"], rows["ids"])
        assert R.same_bits(got["d2"], rows["d2"]) and np.array_equal(got["count"], rows["count"])
        assert fl.topological_neighbours(k=2)["ids"].shape == (2048, 2)
        prof = neighbour_rank_profile(got["d2"])
        assert prof.shape == (9,) and np.all(np.diff(prof) >= 0)
        fl.update(BC.DT)
        assert same_state((fl.positions, fl.velocities, fl.colors), T.step(pos, vel, col, prm, 9, BC.DT))
        with pytest.raises(ValueError, match="bdmi_set_neighbour_mode: .*k = 17"):
            fl.set_neighbour_mode("topological", k=17)
        with pytest.raises(ValueError, match="mode must be one of"):
            fl.set_neighbour_mode("nearest")
        with pytest.raises(ValueError, match="bdmi_topological_neighbours: .*k = 0"):
            fl.topological_neighbours(k=0)
        assert fl.neighbour_mode == ("topological", 9)
        fl.set_neighbour_mode("metric")
        assert fl.neighbour_mode == ("metric", 9)
    finally:
        fl.close()
