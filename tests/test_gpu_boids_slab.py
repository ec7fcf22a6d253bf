"""Slab-mode boids (bdmi_create_slab / bdmi_slab_export / bdmi_slab_import / bdmi_slab_get / bdmi_slab_count, the
ghost branch of `k_flock`, boids.sharded.HipSlabEngine) at the slab faces, against references that share nothing
with the library: tests/slab_ref.py (the protocol in NumPy), tests/boids_ref.py (all-pairs float64) and the CPU
oracle.  The states are those of tests/slab_cases.py, whose claims tests/test_slab_cases_host.py checks.

One thread plays all ranks in turn: export on every handle, the rows to the neighbours with device copies, import,
step.  HipSlabEngine where its plane split is wanted, the raw C ABI (RawSlabEngine, same interface) where a test
sets x_lo, x_hi, the capacity or a NULL id array itself.

Bounds.  Lattice positions and velocities with id colours make the alignment, cohesion and colour sums exact in
any order, so wherever the reference has no separation term the new state must equal it bit for bit; with
separation terms the order of their sum differs: 1e-9 absolute, the project's bound for that (header of
tests/test_gpu_boids.py).  The 25-step runs use the bounds of test_flock_vs_reference.
"""
import ctypes as C

import numpy as np
import pytest

import boids_ref as R
import slab_cases as SC
import slab_ref as S

pytestmark = pytest.mark.gpu

ROW = 10
SENTINEL = -7.25


class RawSlabEngine:
    """boids.sharded.HipSlabEngine's interface over bdmi_create_slab with the caller's own slab, capacity and rows."""

    def __init__(self, nat, rows, prm, x_lo, x_hi, cap, rank, world, has_left=None, has_right=None):
        import torch
        self.torch, self.nat, self.lib = torch, nat, nat.load()
        self.rank, self.world, self.cap = rank, world, cap
        self.x_lo, self.x_hi = x_lo, x_hi
        n = len(rows)
        a = [np.ascontiguousarray(rows[:, k:k + 3]) for k in (0, 3, 6)] if n else [None] * 3
        ids = np.ascontiguousarray(rows[:, 9].astype(np.int32)) if n else None  # n = 0: NULL arrays
        prm = np.ascontiguousarray(prm, dtype=np.float64)
        self._h = self.lib.bdmi_create_slab(n, nat.ptr(a[0]), nat.ptr(a[1]), nat.ptr(a[2]), nat.ptr(ids), cap, nat.ptr(prm),
                                            x_lo, x_hi, int(rank > 0 if has_left is None else has_left),
                                            int(rank < world - 1 if has_right is None else has_right), 0)
        assert self._h, nat.last_error()
        z = lambda k: torch.zeros((k, ROW), dtype=torch.float64, device="cuda")  # noqa: E731
        self.left, self.right, self.send, self.recv = z(cap), z(cap), z(2 * cap), z(2 * cap)
        torch.cuda.synchronize()

    def op_export(self):
        nl, nr = C.c_int64(0), C.c_int64(0)
        self.nat.check(self.lib.bdmi_slab_export(self._h, self.left.data_ptr(), C.addressof(nl), self.right.data_ptr(),
                                                 C.addressof(nr)), "bdmi_slab_export")
        self.nat.check(self.lib.bdmi_sync(self._h), "bdmi_sync")
        nl, nr = int(nl.value), int(nr.value)
        counts = np.zeros(self.world, dtype=np.int64)
        if nl:
            counts[self.rank - 1] = nl
            self.send[:nl].copy_(self.left[:nl])
        if nr:
            counts[self.rank + 1] = nr
            self.send[nl:nl + nr].copy_(self.right[:nr])
        self.torch.cuda.synchronize()
        return counts

    def op_import(self, count):
        self.nat.check(self.lib.bdmi_slab_import(self._h, self.recv.data_ptr(), int(count)), "bdmi_slab_import")

    def op_step(self, dt):
        self.nat.check(self.lib.bdmi_step(self._h, float(dt), 1), "bdmi_step")

    def owned_rows(self):
        out = np.empty((self.cap, ROW))
        cnt = C.c_int64(0)
        self.nat.check(self.lib.bdmi_slab_get(self._h, self.nat.ptr(out), self.cap, C.addressof(cnt)), "bdmi_slab_get")
        return out[: int(cnt.value)]

    def close(self):
        if self._h:
            self.lib.bdmi_destroy(self._h)
            self._h = None


def _engines(nat, c, raw_ranks=()):
    """One engine per rank.  HipSlabEngine splits the planes itself; the ranks in `raw_ranks` go through the raw ABI
    with the faces of slab_ref (an empty one with NULL arrays)."""
    from boids.sharded import HipSlabEngine
    w, face = c["world"], S.faces(c["params"], c["world"])
    own = S.owner_of(c["pos"][:, 0], face)
    out = []
    for r in range(w):
        if r in raw_ranks:
            ids = np.flatnonzero(own == r)
            rows = S.rows_of(c["pos"][ids], c["vel"][ids], c["col"][ids], ids)
            out.append(RawSlabEngine(nat, rows, c["params"], face[r], face[r + 1], len(c["pos"]) + 1, r, w))
        else:
            out.append(HipSlabEngine(c["pos"], c["vel"], c["col"], c["params"], r, w))
            assert (out[-1].x_lo, out[-1].x_hi) == (face[r], face[r + 1])
    return out


def _sent(e, counts):
    """(rows for the left neighbour, rows for the right neighbour) of an engine after op_export, on the device."""
    nl = int(counts[e.rank - 1]) if e.rank > 0 else 0
    nr = int(counts[e.rank + 1]) if e.rank < e.world - 1 else 0
    return e.send[:nl], e.send[nl:nl + nr]


def _exchange(engs):
    """Export on every rank, route, import.  Returns per rank the exported (left, right) rows as NumPy arrays."""
    import torch
    w = len(engs)
    sent = [_sent(e, e.op_export()) for e in engs]
    host = [(a.cpu().numpy().copy(), b.cpu().numpy().copy()) for a, b in sent]
    for r, e in enumerate(engs):
        parts = ([sent[r - 1][1]] if r > 0 else []) + ([sent[r + 1][0]] if r < w - 1 else [])
        k = 0
        for p in parts:
            e.recv[k:k + len(p)].copy_(p)
            k += len(p)
        torch.cuda.synchronize()
        e.op_import(k)
    return host


def _close(engs):
    for e in engs:
        e.close()


def _ids(rows):
    ids = rows[:, 9].astype(np.int64)
    assert np.array_equal(ids.astype(np.float64), rows[:, 9])
    return ids


def _same_rows(rows, state, what):
    """The rows' nine values are the state of their ids, bit for bit; no id twice."""
    ids = _ids(rows)
    assert len(np.unique(ids)) == len(ids), what
    assert R.same_bits(rows[:, :9], state[ids]), what


def _gather(engs, n):
    """(state (n, 9) in id order, owners per rank); every id exactly once."""
    rows = [e.owned_rows() for e in engs]
    owners = [_ids(x) for x in rows]
    S.assert_partition(owners, n)
    full = np.concatenate(rows)
    out = np.empty((n, 9))
    out[_ids(full)] = full[:, :9]
    return out, owners


def _state(c):
    return np.concatenate([c["pos"], c["vel"], c["col"]], axis=1)


def _all_pairs_step(c):
    F = R.flocking(c["pos"], c["vel"], c["col"], c["params"])
    p, v, cl = R.physics(c["pos"], c["vel"], c["col"], (F.sep, F.ali, F.coh, F.avg), c["params"], c["dt"])
    return F, p, v, cl


# ---- 1: what export selects --------------------------------------------------------------------------------------
def _check_export(e, counts, rows_before, cell, has_left, has_right, state, what):
    left, right = (t.cpu().numpy() for t in _sent(e, counts))
    x = rows_before[:, 0]
    ml, mr, dem = S.export_sets(x, np.ones(len(x), dtype=bool), e.x_lo, e.x_hi, cell, has_left, has_right)
    ids = _ids(rows_before)
    for got, mask, side in ((left, ml, "left"), (right, mr, "right")):
        assert len(got) == mask.sum(), (what, side, len(got), mask.sum())  # the counts are the set sizes
        assert set(_ids(got)) == set(ids[mask]), (what, side)
        _same_rows(got, state, (what, side))
    kept = e.owned_rows()  # what bdmi_slab_get returns after the export: the owned rows still inside the slab
    assert len(kept) == (~dem).sum() and set(_ids(kept)) == set(ids[~dem]), (what, "kept")
    _same_rows(kept, state, (what, "kept"))
    return int(ml.sum()), int(mr.sum()), int(dem.sum())


_EXPORT_CASES = {**{f"faces_{w}": (lambda w=w: SC.faces(w)) for w in (2, 3, 7)},
                 **{f"faces_sep_{w}": (lambda w=w: SC.faces_sep(w)) for w in (2, 3, 7)}, "outside": SC.outside}


@pytest.mark.parametrize("name", sorted(_EXPORT_CASES))
def test_export_selects_the_reference_sets(gpu, name):
    c = _EXPORT_CASES[name]()
    w, face, state = c["world"], S.faces(c["params"], c["world"]), _state(c)
    own = S.owner_of(c["pos"][:, 0], face)
    engs = _engines(gpu, c)
    try:
        for r, e in enumerate(engs):
            ids = np.flatnonzero(own == r)
            before = S.rows_of(c["pos"][ids], c["vel"][ids], c["col"][ids], ids)
            got = e.owned_rows()
            assert set(_ids(got)) == set(ids)
            _same_rows(got, state, (name, r, "created"))
            nl, nr, _ = _check_export(e, e.op_export(), before, SC.CELL, r > 0, r < w - 1, state, (name, r))
            assert (nl > 0) == (r > 0) and (nr > 0) == (r < w - 1)
    finally:
        _close(engs)


@pytest.mark.parametrize("n,where", SC.TILE_NAMES)
def test_export_at_scan_tile_edges(gpu, n, where):
    c = SC.tile_edges(n, where)
    lo, hi = c["slab"]
    rows = S.rows_of(c["pos"], c["vel"], c["col"], np.arange(n))
    e = RawSlabEngine(gpu, rows, c["params"], lo, hi, n + 7, 1, 3)
    try:
        nl, nr, nd = _check_export(e, e.op_export(), rows, SC.CELL, True, True, _state(c), c["name"])
        assert nl + nr == c["selected"].sum() and nl >= 1
        assert gpu.load().bdmi_slab_count(e._h) == n - nd
    finally:
        e.close()


# ---- 2: one exchange and step against the all-pairs reference --------------------------------------------------------
def _check_step(c, engs, tol_where_sep):
    n, face = len(c["pos"]), S.faces(c["params"], c["world"])
    F, ep, ev, ec = _all_pairs_step(c)
    _exchange(engs)
    for e in engs:
        e.op_step(c["dt"])
    got, owners = _gather(engs, n)
    p, v, cl = got[:, 0:3], got[:, 3:6], got[:, 6:9]
    bad = np.flatnonzero(np.any(cl != ec, axis=1))
    assert R.same_bits(cl, ec), (c["name"], "colours", len(bad), bad[:5], F.nb[bad[:5]])
    k = F.nsep == 0
    assert R.same_bits(p[k], ep[k]) and R.same_bits(v[k], ev[k]), (c["name"], "state where nsep == 0")
    dp, dv = np.abs(p - ep).max(), np.abs(v - ev).max()
    print(f"{c['name']}: n={n}, boids with a separation term {(~k).sum()}, there max |dp| {dp:.2e} |dv| {dv:.2e}")
    assert dp <= tol_where_sep and dv <= tol_where_sep
    for r, ids in enumerate(owners):  # owned by the slab of the step-start x
        assert (S.owner_of(c["pos"][ids, 0], face) == r).all(), (c["name"], r)
    return got, owners


_STEP_CASES = {**_EXPORT_CASES, "empty_slab": SC.empty_slab}


@pytest.mark.parametrize("name", sorted(_STEP_CASES))
def test_exchange_and_step_equal_all_pairs(gpu, name):
    c = _STEP_CASES[name]()
    engs = _engines(gpu, c, raw_ranks=(1,) if name == "empty_slab" else ())
    try:
        # without separation terms nothing but bit equality is accepted; with them the project's 1e-9
        got, owners = _check_step(c, engs, 0.0 if name.startswith("faces_") and "sep" not in name else 1e-9)
        if name == "empty_slab":
            # the middle slab was created without boids and has just stepped ghosts only; the next exchange populates it
            assert len(owners[1]) == 0
            c2 = dict(c, pos=got[:, 0:3], vel=got[:, 3:6], col=got[:, 6:9])
            _, ep, ev, ec = _all_pairs_step(c2)
            _exchange(engs)
            for e in engs:
                e.op_step(c["dt"])
            got2, owners2 = _gather(engs, len(c["pos"]))
            model = S.SlabModel(c["pos"], c["vel"], c["col"], c["params"], 3)
            for _ in range(2):
                model.exchange()
                model.step(c["dt"])
            assert len(owners2[1]) >= 80
            assert [set(o) for o in owners2] == [set(o) for o in model.owners()]
            assert np.abs(got2[:, 0:3] - ep).max() <= 1e-9 and np.abs(got2[:, 3:6] - ev).max() <= 1e-9
            assert np.abs(got2[:, 6:9] - ec).max() <= 1e-9 * np.abs(ec).max()
    finally:
        _close(engs)


# ---- 3: migration -------------------------------------------------------------------------------------------------
_MIGRATION = {"migration_3": lambda: SC.migration(3), "migration_7": lambda: SC.migration(7),
              "draining_slab": SC.draining_slab}


@pytest.mark.parametrize("name", sorted(_MIGRATION))
def test_migration_against_the_oracle(gpu, oracle, name):
    """25 steps of 1/60 against oracle.FlockStepper under the bounds of test_flock_vs_reference (positions 1e-8,
    velocities 1e-7, colours 1e-10).  The reference's own spread at 25 steps, measured on the CPU between the
    oracle with and without use_numpy_argsort (two summation orders): positions 3.9e-14 / 5.0e-14 / 3.6e-14,
    velocities 3.3e-13 / 2.3e-13 / 2.6e-13, colours 2.2e-16 (migration_3 / migration_7 / draining_slab), all far
    below a tenth of the bounds, so the run keeps its 25 steps.  (With unscaled id colours, up to 2^20, the
    colour spread is 2 ulp = 2.3e-10, above the absolute bound itself from the second step on: these cases
    carry the id colours times 2^-20, see slab_cases._case.)"""
    c = _MIGRATION[name]()
    n, w, dt, steps = len(c["pos"]), c["world"], c["dt"], 25
    st = oracle.FlockStepper(c["pos"], c["vel"], c["col"], c["params"])
    engs = _engines(gpu, c)
    try:
        prev = S.owner_of(c["pos"][:, 0], S.faces(c["params"], w))
        up, down, drained = 0, 0, False
        for _ in range(steps):
            _exchange(engs)
            for e in engs:
                e.op_step(dt)
            got, owners = _gather(engs, n)  # the owned counts sum to n and no id is there twice
            now = np.empty(n, dtype=np.int64)
            for r, ids in enumerate(owners):
                now[ids] = r
            assert np.abs(now - prev).max() <= 1
            up, down = up + int((now > prev).sum()), down + int((now < prev).sum())
            drained |= len(owners[1]) == 0
            prev = now
            st.step(dt)
        assert up > 0 and down > 0
        if name == "draining_slab":
            assert drained
        dp, dv, dc = (np.abs(got[:, k:k + 3] - a).max() for k, a in ((0, st.pos), (3, st.vel), (6, st.col)))
        print(f"{name}: {up} moves right, {down} moves left; after {steps} steps max abs diff pos {dp:.2e} vel {dv:.2e} "
              f"col {dc:.2e}")
        assert dp <= 1e-8 and dv <= 1e-7 and dc <= 1e-10
    finally:
        _close(engs)


# ---- 4: the longest step -------------------------------------------------------------------------------------------
def test_longest_allowed_step(gpu):
    c = SC.long_step()
    n, lib = len(c["pos"]), gpu.load()
    engs = _engines(gpu, c)
    try:
        _check_step(c, engs, 1e-9)
        for _ in range(2):  # the boids that flew one slab further are handed over, nobody is lost
            _exchange(engs)
            for e in engs:
                e.op_step(c["dt"])
            _gather(engs, n)
        counts = [int(lib.bdmi_slab_count(e._h)) for e in engs]
        assert sum(counts) == n
        for e, cnt in zip(engs, counts):
            rc = lib.bdmi_step(e._h, SC.TOO_LONG_DT, 1)
            msg = gpu.last_error()
            assert rc == -1 and "2 * perception_radius = 10" in msg and "= 10.15" in msg, (rc, msg)
            assert lib.bdmi_step(e._h, -SC.TOO_LONG_DT, 1) == -1  # |dt| counts
            assert lib.bdmi_slab_count(e._h) == cnt
        for e in engs:  # and the handles still step
            e.op_step(c["dt"])
        _gather(engs, n)
    finally:
        _close(engs)


# ---- 5: capacity ---------------------------------------------------------------------------------------------------
def _small_slab(nat, n=100, cap=120, seed=5):
    """One slab [-10, 5) with a neighbour on both sides and n owned lattice boids inside it."""
    rng = np.random.default_rng(seed)
    pos = R.lattice(np.stack([rng.uniform(-10, 5, n), rng.uniform(-20, 20, n), rng.uniform(-20, 20, n)], axis=1), SC.PB)
    vel = R.lattice(rng.uniform(-12.5, 12.5, (n, 3)), SC.VB)
    rows = S.rows_of(pos, vel, R.id_colours(n), np.arange(n))
    return RawSlabEngine(nat, rows, SC.params(), -10.0, 5.0, cap, 1, 3), rows


def _incoming(k, first_id, inside):
    """k rows for import: `inside` of them within [-10, 5), the others beyond its right face (ghosts)."""
    x = np.where(np.arange(k) < inside, -2.5, 7.5)
    pos = np.stack([x, 25.0 + np.arange(k) * 0.0, -25.0 + 0.5 * np.arange(k)], axis=1)
    return S.rows_of(pos, np.ones((k, 3)), R.id_colours(k, first_id), first_id + np.arange(k))


def test_capacity(gpu):
    import torch
    lib = gpu.load()
    e, rows = _small_slab(gpu)
    try:
        assert lib.bdmi_slab_count(e._h) == 100
        inc = _incoming(21, 1000, 12)
        e.recv[:21].copy_(torch.from_numpy(inc))
        torch.cuda.synchronize()
        rc = lib.bdmi_slab_import(e._h, e.recv.data_ptr(), 21)
        msg = gpu.last_error()
        assert rc == -4 and all(s in msg for s in ("100", "21", "120")), (rc, msg)
        assert lib.bdmi_slab_count(e._h) == 100
        assert lib.bdmi_slab_import(e._h, e.recv.data_ptr(), 20) == 0, gpu.last_error()  # fills the handle to the brim
        got = e.owned_rows()
        assert len(got) == 112 and set(_ids(got)) == set(range(100)) | set(range(1000, 1012))
        _same_rows(got[_ids(got) < 1000], rows[:, :9], "kept")
        k = _ids(got) >= 1000
        assert R.same_bits(got[k][np.argsort(_ids(got[k]))], inc[:12])
        assert lib.bdmi_slab_import(e._h, e.recv.data_ptr(), 1) == -4  # 120 rows are in use, eight of them ghosts
        # bdmi_slab_get below the count
        out = np.full((112, ROW), SENTINEL)
        cnt = C.c_int64(-1)
        gpu.check(lib.bdmi_slab_get(e._h, gpu.ptr(out), 50, C.addressof(cnt)), "bdmi_slab_get")
        assert cnt.value == 112 and (out[50:] == SENTINEL).all() and not (out[:50] == SENTINEL).any()
        assert set(_ids(out[:50])) <= set(_ids(got))
        cnt = C.c_int64(-1)
        gpu.check(lib.bdmi_slab_get(e._h, None, 0, C.addressof(cnt)), "bdmi_slab_get")
        assert cnt.value == 112
        assert lib.bdmi_slab_count(e._h) == 112
    finally:
        e.close()


# ---- 6: refusals -----------------------------------------------------------------------------------------------------
_CAM = np.array([0, 0, 100.0, 0, 0, -1.0, 1.0, 0, 0, 0, 1.0, 0])


def _five_calls(nat, h, n):
    """Every id-indexed call on `h` with sentinel-filled outputs for n boids: [(name, rc, error text, outputs)]."""
    lib = nat.load()
    full = lambda *shape, dt=np.float64: np.full(shape, SENTINEL, dtype=dt)  # noqa: E731
    res = []

    def call(name, outs, fn):
        rc = fn()
        res.append((name, rc, nat.last_error(), outs))

    o = [full(n, 3) for _ in range(3)]
    call("bdmi_get_state", o, lambda: lib.bdmi_get_state(h, *[nat.ptr(a) for a in o]))
    cells = full(n, dt=np.int32)
    call("bdmi_get_cell_indices", [cells], lambda: lib.bdmi_get_cell_indices(h, nat.ptr(cells)))
    f = [full(n, 3) for _ in range(4)]
    call("bdmi_get_forces", f, lambda: lib.bdmi_get_forces(h, *[nat.ptr(a) for a in f]))
    vv, vc, cnt = full(n * 6, 3, dt=np.float32), full(n * 6, 3, dt=np.float32), full(1, dt=np.int64)
    call("bdmi_visible_vertices", [vv, vc, cnt],
         lambda: lib.bdmi_visible_vertices(h, nat.ptr(_CAM), 1.0, 1.0, 800.0, 1.2, 0.4, nat.ptr(vv), nat.ptr(vc), n,
                                           nat.ptr(cnt)))
    s = [np.zeros((n, 3)) for _ in range(3)]
    call("bdmi_set_state", [], lambda: lib.bdmi_set_state(h, *[nat.ptr(a) for a in s]))
    return res


def test_id_indexed_calls_refuse_slab_handles(gpu):
    import torch
    lib = gpu.load()
    e, rows = _small_slab(gpu)
    try:
        inc = _incoming(10, 1000, 4)
        e.recv[:10].copy_(torch.from_numpy(inc))
        torch.cuda.synchronize()
        e.op_import(10)  # six ghosts: rows with ids -1001 .. in A.id
        before = e.owned_rows()
        assert len(before) == 104
        for name, rc, msg, outs in _five_calls(gpu, e._h, 110):
            assert rc == -1, (name, rc)
            assert "slab" in msg and "bdmi_slab_get" in msg and name in msg, (name, msg)
            for a in outs:
                assert (a == np.array(SENTINEL).astype(a.dtype)).all(), name  # untouched (integers hold -7)
        after = e.owned_rows()
        assert R.same_bits(before, after)  # bdmi_set_state wrote nothing
        dim, cells = C.c_int32(0), C.c_int64(0)
        gpu.check(lib.bdmi_grid_info(e._h, C.addressof(dim), C.addressof(cells), None), "bdmi_grid_info")
        assert (dim.value, cells.value) == (14, 14 ** 3)
        e.op_step(SC.DT)  # and the handle still steps and synchronises
        gpu.check(lib.bdmi_sync(e._h), "bdmi_sync")
    finally:
        e.close()
    # an ordinary handle still answers all five
    pos, vel, col = rows[:, 0:3].copy(), rows[:, 3:6].copy(), rows[:, 6:9].copy()
    prm = SC.params()
    h = lib.bdmi_create(100, gpu.ptr(pos), gpu.ptr(vel), gpu.ptr(col), gpu.ptr(prm), 0)
    assert h, gpu.last_error()
    try:
        res = {name: (rc, outs) for name, rc, _, outs in _five_calls(gpu, h, 100)}
        assert all(rc == 0 for rc, _ in res.values()), res
        p, v, cl = res["bdmi_get_state"][1]
        assert R.same_bits(p, pos) and R.same_bits(v, vel) and R.same_bits(cl, col)
        assert np.array_equal(res["bdmi_get_cell_indices"][1][0], R.cell_index(pos, prm))
        assert 0 <= res["bdmi_visible_vertices"][1][2][0] <= 100
        z = [np.empty((100, 3)) for _ in range(3)]
        gpu.check(lib.bdmi_get_state(h, *[gpu.ptr(a) for a in z]), "bdmi_get_state")
        assert not z[0].any() and not z[1].any() and not z[2].any()  # bdmi_set_state took the zeros
    finally:
        lib.bdmi_destroy(h)
