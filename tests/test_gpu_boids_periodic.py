"""Periodic handles (include/bdmi.h "Periodic handles"; csrc/bdmi.hip, the GridPer instances) against the NumPy
restatement (tests/periodic_ref.py) on the constructed cases of tests/periodic_cases.py.  In topological mode everything
is compared bit for bit; in metric mode everything but the separation force, which has boids_ref.check_sep's bound.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import boids_cases as BC
import boids_ref as R
import periodic_cases as PC
import periodic_ref as PR
import topo_ref as T
from test_gpu_boids import RawFlock
from test_gpu_boids_topological import METRIC, TOPOLOGICAL, KS, get_mode, hook, same_state, set_mode

pytestmark = pytest.mark.gpu

CASES = ("box_3", "box_4", "box_33", "face_waves", "long_run_2100", "long_run_4200")
SIZES = (0, 1, 2, 255, 256, 257)  # the empty and single-boid flocks, and the block edges of every tier


class PeriodicFlock(RawFlock):
    def __init__(self, nat, pos, vel, col, params, k=None):
        self.lib = nat.load()
        self.nat = nat
        self.n = len(pos)
        pos, vel, col = (np.ascontiguousarray(a, dtype=np.float64) for a in (pos, vel, col))
        self.h = self.lib.bdmi_create_periodic(self.n, nat.ptr(pos), nat.ptr(vel), nat.ptr(col), nat.ptr(params), 0)
        assert self.h, nat.last_error()
        if k is not None:
            assert set_mode(self, TOPOLOGICAL, k) == 0, nat.last_error()


def get_box(f):
    per, length, cell = C.c_int(-5), C.c_double(-5), C.c_double(-5)
    assert f.lib.bdmi_get_box(f.h, C.addressof(per), C.addressof(length), C.addressof(cell)) == 0, f.nat.last_error()
    return int(per.value), float(length.value), float(cell.value)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case and its rows at k = 16, computed once: the rows of a smaller k are their prefix."""
    c = next(x for x in PC.gpu_cases() if x["name"] == name) if name in CASES else PC.sizes(int(name.split("_")[1]))
    return c, (PR.neighbours(c["pos"], c["params"], T.K_MAX) if len(c["pos"]) else None)


def _rows(name, k):
    c, rows16 = _case(name)
    return c, (T.first_k(rows16, k) if rows16 is not None else PR.neighbours(c["pos"], c["params"], k))


def _check_topological(nat, c, k, rows, what):
    """Hook rows, the four force arrays and one stepped state, bit for bit."""
    pos, vel, col, prm, dt = c["pos"], c["vel"], c["col"], c["params"], c["dt"]
    F = PR.flocking(pos, vel, col, prm, k, nb=rows)
    f = PeriodicFlock(nat, pos, vel, col, prm)
    try:
        ids, d2, count = hook(f, k)  # in metric mode: the hook takes its own k
        bad = np.flatnonzero(np.any(ids != rows["ids"], axis=1))
        assert len(bad) == 0, (what, "ids", len(bad), bad[:5], ids[bad[:3]], rows["ids"][bad[:3]])
        assert R.same_bits(d2, rows["d2"]) and np.array_equal(count, rows["count"]), what
        assert set_mode(f, TOPOLOGICAL, k) == 0, nat.last_error()
        for g, w, name in zip(f.forces(), (F.sep, F.ali, F.coh, F.avg), ("sep", "ali", "coh", "avg")):
            bad = np.flatnonzero(np.any(g != w, axis=1))
            assert R.same_bits(g, w), (what, name, len(bad), bad[:5], F.nb[bad[:5]])
        f.step(dt)
        want = PR.physics(pos, vel, col, (F.sep, F.ali, F.coh, F.avg), prm, dt)
        assert same_state(f.state(), want), what
    finally:
        f.close()
    return F


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", CASES)
def test_topological_cases_match_restatement(gpu, name, k):
    c, rows = _rows(name, k)
    F = _check_topological(gpu, c, k, rows, (name, k))
    print(f"{name} k={k}: n={len(c['pos'])} metric neighbours up to {rows['metric'].max()}, lists full for "
          f"{(F.nb == k).mean():.0%}")


@pytest.mark.parametrize("name", CASES + tuple(f"n_{n}" for n in SIZES))
def test_metric_cases_match_restatement(gpu, name):
    """The same cases in metric mode, the sizes included (n = 0 is the empty-handle path of every call)."""
    c, _ = _case(name)
    pos, vel, col, prm = c["pos"], c["vel"], c["col"], c["params"]
    F = PR.metric(pos, vel, col, prm)
    f = PeriodicFlock(gpu, pos, vel, col, prm)
    try:
        assert get_mode(f)[0] == METRIC
        assert np.array_equal(f.cells(), PR.cell_index(pos, prm))
        sep, ali, coh, avg = f.forces()
        assert R.same_bits(ali, F.ali) and R.same_bits(coh, F.coh) and R.same_bits(avg, F.avg), name
        diff, worst = R.check_sep(sep, F, vel, prm, name)
        print(f"{name}: n={len(pos)} neighbours up to {F.nb.max(initial=0)}, sep differs by up to {diff:.3g} (bound {worst:.3g})")
        f.step(c["dt"])
        p, v, cl = f.state()
        want = PR.physics(pos, vel, col, (sep, F.ali, F.coh, F.avg), prm, c["dt"])  # the device's own separation sum
        assert same_state((p, v, cl), want) and np.all(np.abs(p) <= PR.box(prm)[0])
    finally:
        f.close()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes(gpu, n, k):
    c, rows = _rows(f"n_{n}", k)
    F = _check_topological(gpu, c, k, rows, (n, k))
    if n <= 1:
        assert not F.nb.any() and not np.any(F.sep) and not np.any(F.ali) and not np.any(F.coh)
    if n >= 255:
        assert (F.nb == k).any()


def test_trajectory(gpu):
    """2 000 boids at about 20 metric neighbours each, k = 7: ten steps against the replay, step by step, with dozens of
    boids crossing a face."""
    c = PC.trajectory()
    prm, k = c["params"], 7
    B = PR.box(prm)[0]
    pos, vel, col = c["pos"], c["vel"], c["col"]
    f = PeriodicFlock(gpu, pos, vel, col, prm, k)
    crossed = np.zeros(len(pos), dtype=bool)
    try:
        for s in range(10):
            f.step(c["dt"])
            new = PR.step(pos, vel, col, prm, k, c["dt"])
            crossed |= PR.crossings(pos, new[0], prm)
            pos, vel, col = new
            got = f.state()
            assert same_state(got, (pos, vel, col)), s
            assert np.all(np.abs(got[0]) <= B)
    finally:
        f.close()
    assert crossed.sum() >= 50, crossed.sum()


def test_order_independence(gpu, monkeypatch):
    """A permutation of the caller's order gives the permuted forces and the permuted state after five steps, and the
    hardware block order (BDMI_XCD=0) the same bits as the default one.  Off the lattice, on a seed without two equal d2
    among any boid's first k + 1, so that no tie is left for the (permuted) ids to break."""
    prm, k, n = BC.params(bounds=18.75), 7, 3000
    for seed in range(20, 30):
        rng = np.random.default_rng(seed)
        pos, vel, col = rng.uniform(-18.75, 18.75, (n, 3)), rng.uniform(-12.5, 12.5, (n, 3)), rng.random((n, 3))
        if T.distinct_d2(PR.neighbours(pos, prm, k + 1)).all():
            break
    else:
        raise AssertionError("no tie-free seed")
    perm = np.random.default_rng(2).permutation(n)

    def run(order):
        f = PeriodicFlock(gpu, pos[order], vel[order], col[order], prm, k)
        try:
            forces = f.forces()
            f.step(BC.DT, 5)
            return forces, f.state()
        finally:
            f.close()

    monkeypatch.delenv("BDMI_XCD", raising=False)
    forces, state = run(np.arange(n))
    F = PR.flocking(pos, vel, col, prm, k)
    assert same_state(forces, (F.sep, F.ali, F.coh, F.avg))
    want = pos, vel, col
    for _ in range(5):
        want = PR.step(*want, prm, k, BC.DT)
    assert same_state(state, want)
    forces_p, state_p = run(perm)
    assert same_state(forces_p, [a[perm] for a in forces]) and same_state(state_p, [a[perm] for a in state])
    monkeypatch.setenv("BDMI_XCD", "0")
    forces_x, state_x = run(np.arange(n))
    assert same_state(forces_x, forces) and same_state(state_x, state)


def test_translation(gpu):
    """All positions shifted by a lattice vector and wrapped: the same neighbours at the same d2, and the forces that do
    not see absolute coordinates (cohesion rounds them once) are the same bits."""
    c, rows = _rows("box_4", 9)
    prm = c["params"]
    B = PR.box(prm)[0]
    shift = np.array([3.0 + 2.0 ** -3, -7.0 - 2.0 ** -10, 2.0 ** -16])
    moved = PC.wrapped(c["pos"] + shift, B)
    assert R.same_bits(moved, R.lattice(moved, BC.PB)) and PR.crossings(c["pos"] + shift, moved, prm).mean() > 0.2
    out = []
    for pos in (c["pos"], moved):
        f = PeriodicFlock(gpu, pos, c["vel"], c["col"], prm, 9)
        try:
            out.append((hook(f, 9), f.forces()))
        finally:
            f.close()
    (ids0, d20, cnt0), (sep0, ali0, _, avg0) = out[0]
    (ids1, d21, cnt1), (sep1, ali1, _, avg1) = out[1]
    assert np.array_equal(ids0, rows["ids"])
    assert np.array_equal(ids0, ids1) and R.same_bits(d20, d21) and np.array_equal(cnt0, cnt1)
    assert R.same_bits(sep0, sep1) and R.same_bits(ali0, ali1) and R.same_bits(avg0, avg1)


# ---- hygiene ----------------------------------------------------------------------------------------------------------
def test_interior_flock_equals_a_walled_handle(gpu):
    """Further than one cell from every face no image is shifted: the topological forces of a periodic handle are the bits
    of a walled handle on the same state.  The grids differ (12 cells of 5 against 14), the function does not."""
    c = PC.interior_cluster()
    got = []
    for cls in (PeriodicFlock, RawFlock):
        f = cls(gpu, c["pos"], c["vel"], c["col"], c["params"])
        try:
            assert set_mode(f, TOPOLOGICAL, 7) == 0
            dim = C.c_int32(0)
            assert f.lib.bdmi_grid_info(f.h, C.addressof(dim), None, None) == 0
            got.append((f.forces(), dim.value))
        finally:
            f.close()
    assert (got[0][1], got[1][1]) == (12, 14)
    assert same_state(got[0][0], got[1][0])


def test_environment_and_box(gpu, monkeypatch):
    monkeypatch.setenv("BDMI_NEIGHBOURS", "topological:5")
    c = PC.sizes(257)
    f = PeriodicFlock(gpu, c["pos"], c["vel"], c["col"], c["params"])
    w = RawFlock(gpu, c["pos"], c["vel"], c["col"], c["params"])
    try:
        assert get_mode(f) == (TOPOLOGICAL, 5)
        F = PR.flocking(c["pos"], c["vel"], c["col"], c["params"], 5)
        assert same_state(f.forces(), (F.sep, F.ali, F.coh, F.avg))
        assert get_box(f) == (1, 15.0, 5.0) and get_box(w) == (0, 15.0, 5.0)
        assert f.lib.bdmi_get_box(f.h, None, None, None) == 0
        length = C.c_double(0)
        assert f.lib.bdmi_get_box(f.h, None, C.addressof(length), None) == 0 and length.value == 15.0
        assert np.array_equal(f.cells(), PR.cell_index(c["pos"], c["params"]))
    finally:
        f.close()
        w.close()
    prm = BC.params(bounds=18.75)
    f = PeriodicFlock(gpu, np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 3)), prm)
    try:
        assert get_box(f) == (1, 37.5, 37.5 / 7)
        row = np.empty(16)
        gpu.check(f.lib.bdmi_diagnostics(f.h, gpu.ptr(row)), "bdmi_diagnostics")  # works on a periodic handle
        assert row[0] == 1
    finally:
        f.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _refused(nat, rc, call):
    assert rc == -1 and nat.last_error().startswith(call + ": "), (rc, nat.last_error())
    return nat.last_error()


def test_refusals(gpu):
    lib = gpu.load()
    n = 64
    rng = np.random.default_rng(6)
    pos, vel, col = R.lattice(rng.uniform(-7.5, 7.5, (n, 3)), BC.PB), R.lattice(rng.uniform(-5, 5, (n, 3)), BC.VB), R.id_colours(n)

    def create(p, prm):
        p = np.ascontiguousarray(p)
        return lib.bdmi_create_periodic(n, gpu.ptr(p), gpu.ptr(vel), gpu.ptr(col), gpu.ptr(prm), 0)

    # dim < 3 (and a wall margin of 0 alone is no reason)
    assert not create(pos * 0.5, BC.params(bounds=7.0)) and "dimension" in gpu.last_error()
    assert gpu.last_error().startswith("bdmi_create_periodic: ")
    h = create(pos, BC.params(bounds=7.5, wall_margin=0.0, wall_weight=0.0))
    assert h, gpu.last_error()
    lib.bdmi_destroy(h)
    # a position outside the box, or not finite, at create: the message names the first offending row
    for value in (7.5 + 2.0 ** -16, -8.0, np.nan, np.inf):
        bad = pos.copy()
        bad[41, 1] = value
        bad[50, 0] = 99.0
        assert not create(bad, PC.box_params(3))
        assert gpu.last_error().startswith("bdmi_create_periodic: ") and "row 41" in gpu.last_error(), gpu.last_error()
    f = PeriodicFlock(gpu, pos, vel, col, PC.box_params(3))
    try:
        before = f.state()
        # ... and at bdmi_set_state: nothing is uploaded
        bad = pos.copy()
        bad[7, 2] = -7.5 - 2.0 ** -16
        other = np.ascontiguousarray(vel + 1.0)
        rc = lib.bdmi_set_state(f.h, gpu.ptr(bad), gpu.ptr(other), None)
        assert "row 7" in _refused(gpu, rc, "bdmi_set_state")
        assert same_state(f.state(), before)
        edge = pos.copy()
        edge[7] = (7.5, -7.5, 7.5)  # the faces themselves are inside
        gpu.check(lib.bdmi_set_state(f.h, gpu.ptr(edge), None, None), "bdmi_set_state")
        assert R.same_bits(f.state()[0], edge)
        gpu.check(lib.bdmi_set_state(f.h, gpu.ptr(pos), None, None), "bdmi_set_state")
        # max_speed * |dt| >= L: nothing is run
        for dt in (15.0 / 25.0, -15.0 / 25.0, 1.0):
            assert "box length" in _refused(gpu, lib.bdmi_step(f.h, dt, 1), "bdmi_step")
        assert same_state(f.state(), before)
        gpu.check(lib.bdmi_step(f.h, np.nextafter(15.0 / 25.0, 0), 0), "bdmi_step")
        # the flock finder, the catalogue and the neighbour statistics
        labels = np.full(n, -7, dtype=np.int32)
        cnt, nn = np.full(n, -7, dtype=np.int32), np.full(n, -7.0)
        lab16, mem16, rows16 = np.full(16, -7, dtype=np.int32), np.full(16, -7, dtype=np.int64), np.full((16, 16), -7.0)
        nf = C.c_int64(-7)
        rc = lib.bdmi_flocks(f.h, 5.0, gpu.ptr(labels), C.addressof(nf), None, None)
        assert "periodic" in _refused(gpu, rc, "bdmi_flocks")
        rc = lib.bdmi_flock_catalogue(f.h, 5.0, 1, 16, gpu.ptr(lab16), gpu.ptr(mem16), gpu.ptr(rows16), C.addressof(nf))
        assert "periodic" in _refused(gpu, rc, "bdmi_flock_catalogue")
        rc = lib.bdmi_neighbour_stats(f.h, 5.0, gpu.ptr(cnt), gpu.ptr(nn), C.addressof(nf))
        assert "periodic" in _refused(gpu, rc, "bdmi_neighbour_stats")
        assert nf.value == -7 and all((a == -7).all() for a in (labels, cnt, nn, lab16, mem16, rows16))
        assert same_state(f.state(), before)
    finally:
        f.close()
    _refused(gpu, lib.bdmi_get_box(None, None, None, None), "bdmi_get_box")
    assert not lib.bdmi_create_periodic(n, None, None, None, None, 0)
    # a slab handle has no box call
    ids = np.arange(n, dtype=np.int32)
    prm = BC.params(bounds=30.0)
    slab = lib.bdmi_create_slab(n, gpu.ptr(pos), gpu.ptr(vel), gpu.ptr(col), gpu.ptr(ids), 2 * n, gpu.ptr(prm), -35.0, 35.0,
                                0, 0, 0)
    assert slab, gpu.last_error()
    try:
        per = C.c_int(-7)
        assert "slab" in _refused(gpu, lib.bdmi_get_box(slab, C.addressof(per), None, None), "bdmi_get_box")
        assert per.value == -7
    finally:
        lib.bdmi_destroy(slab)
