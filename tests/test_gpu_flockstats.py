"""The flock-analysis calls (include/bdmi.h: bdmi_flocks, bdmi_flock_catalogue, bdmi_diagnostics, bdmi_neighbour_stats;
csrc/bdmi.hip) against the NumPy restatement tests/flockstats_ref.py.

All inputs are on the dyadic lattice of boids_cases.py, so the sums of positions and velocities are exact in any order.
Per case labels, n_flocks, links, count, nn_d2, the catalogue's label, members, order and count and the row fields m, c,
vbar, lo, hi must equal the restatement bit for bit; polarisation and milling must be within 2 m 2^-53 and mean_speed
within m 2^-53 max s_j of it (flockstats_ref.row_bounds: the terms are the restatement's bit for bit, only the order of
the sums differs).
"""
import ctypes as C

import numpy as np
import pytest

import boids_cases as BC
import boids_ref as R
import flockstats_cases as FC
import flockstats_ref as FR
from test_gpu_boids import RawFlock

pytestmark = pytest.mark.gpu


class Stats(RawFlock):
    """RawFlock plus the four calls; every output array is the caller's, so a refusal can be seen to leave it alone."""

    def flocks(self, link, labels=True):
        lab = np.full(self.n, -7, dtype=np.int32) if labels else None
        out = [C.c_int64(-7) for _ in range(3)]
        rc = self.lib.bdmi_flocks(self.h, link, self.nat.ptr(lab), *[C.addressof(x) for x in out])
        return rc, dict(labels=lab, n_flocks=out[0].value, links=out[1].value, evals=out[2].value)

    def catalogue(self, link, min_members=1, capacity=0, null_outputs=False):
        label = np.full(max(capacity, 0), -7, dtype=np.int32)
        members = np.full(max(capacity, 0), -7, dtype=np.int64)
        rows = np.full((max(capacity, 0), 16), -7.0)
        cnt = C.c_int64(-7)
        ptrs = [None] * 3 if null_outputs else [self.nat.ptr(a) for a in (label, members, rows)]
        rc = self.lib.bdmi_flock_catalogue(self.h, link, min_members, capacity, *ptrs, C.addressof(cnt))
        return rc, dict(count=cnt.value, label=label, members=members, rows=rows)

    def diagnostics(self):
        row = np.full(16, -7.0)
        return self.lib.bdmi_diagnostics(self.h, self.nat.ptr(row)), row

    def neighbours(self, radius):
        count, nn, ev = np.full(self.n, -7, dtype=np.int32), np.full(self.n, -7.0), C.c_int64(-7)
        rc = self.lib.bdmi_neighbour_stats(self.h, radius, self.nat.ptr(count), self.nat.ptr(nn), C.addressof(ev))
        return rc, dict(count=count, nn_d2=nn, evals=ev.value)


def _check_rows(got_rows, want_rows, smax, what):
    got, want = np.asarray(got_rows, np.float64), np.asarray(want_rows, np.float64)
    assert got.shape == want.shape, what
    ex = list(FR.EXACT)
    # + 0.0: a minimum over +0.0 and -0.0 may keep either
    bad = np.flatnonzero(((got[:, ex] + 0.0).view(np.int64) != (want[:, ex] + 0.0).view(np.int64)).any(axis=1))
    assert len(bad) == 0, (what, bad[:5], got[bad[:2]], want[bad[:2]])
    m = want[:, 0]
    bound = np.zeros_like(want)
    bound[:, 7] = bound[:, 9] = 2.0 * m * FR.U
    bound[:, 8] = m * FR.U * np.asarray(smax, np.float64)
    for k in np.flatnonzero(m > 0)[:3]:
        assert np.array_equal(bound[k], FR.row_bounds(want[k], smax[k]))
    diff = np.abs(got - want)
    bad = np.flatnonzero((diff > bound).any(axis=1))
    assert len(bad) == 0, (what, bad[:5], diff[bad[:3]][:, [7, 8, 9]], bound[bad[:3]][:, [7, 8, 9]])
    assert (got[:, [7, 9]] >= 0.0).all() and (got[:, [7, 9]] <= 1.0 + bound[:, [7, 9]]).all(), what


def _check_state(f, pos, vel, link, what, min_members=1):
    """all four calls on the handle's current state (pos, vel: what bdmi_get_state returns) against the restatement"""
    want = FR.analyse(pos, link)
    rc, got = f.flocks(link)
    assert rc == 0, f.nat.last_error()
    assert np.array_equal(got["labels"], want["labels"]), what
    assert (got["n_flocks"], got["links"]) == (want["n_flocks"], want["links"]), what
    assert got["evals"] >= got["links"]
    rc, nb = f.neighbours(link)
    assert rc == 0, f.nat.last_error()
    assert np.array_equal(nb["count"], want["count"]), what
    assert R.same_bits(nb["nn_d2"], want["nn_d2"]), what
    assert int(nb["count"].astype(np.int64).sum()) == 2 * got["links"], what
    cat = FR.catalogue(pos, vel, want["labels"], min_members)
    rc, head = f.catalogue(link, min_members, 0, null_outputs=True)  # capacity 0, NULL outputs: the count alone
    assert rc == 0 and head["count"] == cat["count"], (what, f.nat.last_error())
    rc, full = f.catalogue(link, min_members, cat["count"])
    assert rc == 0 and full["count"] == cat["count"], (what, f.nat.last_error())
    assert np.array_equal(full["label"], cat["label"]) and np.array_equal(full["members"], cat["members"]), what
    _check_rows(full["rows"], cat["rows"], cat["smax"], what)
    if cat["count"] > 1:  # fewer rows than flocks: the first ones of the order, the rest of the arrays untouched
        k = cat["count"] // 2
        rc, part = f.catalogue(link, min_members, k)
        assert rc == 0 and part["count"] == cat["count"]
        assert np.array_equal(part["label"], full["label"][:k]) and R.same_bits(part["rows"], full["rows"][:k]), what
    rc, row = f.diagnostics()
    assert rc == 0, f.nat.last_error()
    wrow, smax = FR.row(pos, vel)
    _check_rows(row[None], wrow[None], [smax], what + " diagnostics")
    if want["n_flocks"] == 1 and min_members <= len(pos):
        assert R.same_bits(row, full["rows"][0]), what  # one flock of all: the same reduction
    return want, got, full


def _check_case(nat, c, link=None, **kw):
    f = Stats(nat, c["pos"], c["vel"], c["col"], c["params"])
    try:
        return _check_state(f, c["pos"], c["vel"], FC.perception(c) if link is None else link, c["name"], **kw)
    finally:
        f.close()


# ---- the constructed cases -------------------------------------------------------------------------------------------
def test_thresholds_at_and_below_the_link(gpu):
    c = BC.thresholds()
    want, got, _ = _check_case(gpu, c, 5.0)
    assert (want["nn_d2"] == 25.0).any() and (want["nn_d2"] == 0.0).any()  # pairs exactly at the link, coincident pairs
    below, _, _ = _check_case(gpu, c, 5.0 - 2.0 ** -16)  # the pairs at exactly 5 are now just outside
    assert below["links"] < want["links"] and below["n_flocks"] > want["n_flocks"]


@pytest.mark.parametrize("dim", [3, 4, 31, 32, 33, 34, 63, 64, 65])
def test_grid_dims_and_clamped_boids(gpu, dim):
    c = BC.grid_dims(dim)
    _, d, off = R.grid(c["params"])
    assert d == dim and (np.abs(c["pos"]) > off + 1).any()  # some boids lie outside the grid and are clamped
    _check_case(gpu, c)


def test_hit_list_sizes_1_to_81_with_ties(gpu):
    _, _, cat = _check_case(gpu, BC.hit_list())
    # two clusters of each size 1 .. 81 (one of 10 and one of 41 lie within the link of each other and make one of 51)
    assert sorted(set(cat["members"].tolist())) == list(range(1, 82))
    assert (np.bincount(cat["members"])[1:] >= 2).sum() == 79  # ties in members, broken by label


@pytest.mark.parametrize("count", [4095, 4096, 4097])
def test_run_lengths(gpu, count):
    c = BC.run_length(count)
    assert BC.grid_facts(c["pos"], c["params"])["runs"].max() >= count  # a run above 4 095 from 4 096 on
    want, _, _ = _check_case(gpu, c)
    assert np.bincount(np.unique(want["labels"], return_inverse=True)[1]).max() >= count  # one heavily contended root


def test_mixed_lanes(gpu):
    _check_case(gpu, BC.mixed_lanes())


@pytest.mark.parametrize("name", ["perception_2.5", "perception_7.25"])
def test_parameter_cases(gpu, name):
    c = next(x for x in BC.parameter_cases() if x["name"] == name)
    _check_case(gpu, c)
    _check_case(gpu, c, 0.5 * FC.perception(c), min_members=3)  # a link below the cell size


def test_chain_and_chain_with_a_gap(gpu):
    c, _ = FC.chain(6000)
    want, got, cat = _check_case(gpu, c)
    assert got["n_flocks"] == 1 and got["links"] == 5999 and cat["members"].tolist() == [6000]
    g, _ = FC.chain(6000, gap_at=3020)
    want, got, cat = _check_case(gpu, g)
    assert got["n_flocks"] == 2 and got["links"] == 5998 and cat["members"].tolist() == [3021, 2979]


def test_flock_sizes_at_the_chunk_edges(gpu):
    c = FC.blobs()
    _, got, cat = _check_case(gpu, c, c["link"])
    assert cat["members"].tolist() == [8193, 4097, 4096, 4095]
    assert got["links"] == sum(m * (m - 1) // 2 for m in (4095, 4096, 4097, 8193))


@pytest.mark.parametrize("pairs", [2047, 2048, 2049])
def test_qualifying_flocks_at_the_scan_tile_edges(gpu, pairs):
    c = FC.isolated_pairs(pairs)
    _, got, cat = _check_case(gpu, c, c["link"], min_members=2)
    assert cat["count"] == pairs and got["n_flocks"] == pairs + 500


def test_min_members_selecting_none(gpu):
    c = BC.hit_list()
    f = Stats(gpu, c["pos"], c["vel"], c["col"], c["params"])
    try:
        rc, cat = f.catalogue(5.0, 82, 8)
        assert rc == 0 and cat["count"] == 0 and (cat["label"] == -7).all() and (cat["rows"] == -7.0).all()
    finally:
        f.close()


@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_flocks(gpu, n):
    pos = R.lattice(np.array([[1.0, 2.0, 3.0], [1.5, 2.0, 3.0]])[:n], 16).reshape(n, 3)
    vel = R.lattice(np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]])[:n], 20).reshape(n, 3)
    f = Stats(gpu, pos, vel, np.zeros((n, 3)), BC.params(bounds=20.0))
    try:
        want, got, cat = _check_state(f, pos, vel, 5.0, f"n={n}")
        assert got["n_flocks"] == min(n, 1) and got["links"] == (1 if n == 2 else 0) and cat["count"] == min(n, 1)
        rc, row = f.diagnostics()
        assert rc == 0 and row[0] == n and (n > 0 or not row.any())
        if n == 1:
            assert row.tolist() == [1, 1, 2, 3, 0, 0, 0, 0, 0, 0, 1, 2, 3, 1, 2, 3]  # a boid at rest: u = 0
    finally:
        f.close()


def _untouched(res):
    for k, v in res.items():
        a = np.asarray(v)
        assert (a == -7).all(), k


def test_refusals_leave_the_outputs_alone(gpu):
    c = BC.hit_list()
    f = Stats(gpu, c["pos"], c["vel"], c["col"], c["params"])
    try:
        for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), 5.0 + 2.0 ** -16, 1e300):
            for name, call in (("bdmi_flocks", lambda: f.flocks(bad)), ("bdmi_flock_catalogue", lambda: f.catalogue(bad, 1, 4)),
                               ("bdmi_neighbour_stats", lambda: f.neighbours(bad))):
                rc, res = call()
                msg = gpu.last_error()
                assert rc == -1 and msg.startswith(name + ": "), (bad, name, rc, msg)
                assert "perception radius 5" in msg and ("radius" if "neighbour" in name else "link") in msg
                if bad == 1e300:
                    assert "1e+300" in msg
                _untouched(res)
        for mm, cap in ((0, 4), (-3, 4), (1, -1)):
            rc, res = f.catalogue(5.0, mm, cap)
            assert rc == -1 and gpu.last_error().startswith("bdmi_flock_catalogue: ")
            _untouched(res)
        rc, res = f.catalogue(5.0, 1, 4, null_outputs=True)  # capacity > 0 needs its arrays
        assert rc == -1 and res["count"] == -7
        assert f.lib.bdmi_diagnostics(f.h, None) == -1
        rc, ok = f.flocks(5.0)
        assert rc == 0 and ok["n_flocks"] == 161  # and the handle works on
    finally:
        f.close()


def test_slab_handle_refused(gpu):
    lib = gpu.load()
    n = 64
    rng = np.random.default_rng(0)
    pos, vel, col = rng.uniform(-20, 20, (n, 3)), rng.uniform(-5, 5, (n, 3)), rng.random((n, 3))
    ids = np.arange(n, dtype=np.int32)
    prm = BC.params(bounds=30.0)
    h = lib.bdmi_create_slab(n, gpu.ptr(pos), gpu.ptr(vel), gpu.ptr(col), gpu.ptr(ids), 2 * n, gpu.ptr(prm), -35.0, 35.0, 0, 0, 0)
    assert h, gpu.last_error()
    try:
        f = Stats.__new__(Stats)
        f.lib, f.nat, f.n, f.h = lib, gpu, n, h
        for name, call in (("bdmi_flocks", lambda: f.flocks(5.0)), ("bdmi_flock_catalogue", lambda: f.catalogue(5.0, 1, 4)),
                           ("bdmi_neighbour_stats", lambda: f.neighbours(5.0))):
            rc, res = call()
            assert rc == -1 and gpu.last_error().startswith(name + ": refused on a slab handle"), gpu.last_error()
            _untouched(res)
        rc, row = f.diagnostics()
        assert rc == -1 and gpu.last_error().startswith("bdmi_diagnostics: refused on a slab handle") and (row == -7).all()
    finally:
        lib.bdmi_destroy(h)


# ---- stepped states --------------------------------------------------------------------------------------------------
def _stepping_case():
    c = next(x for x in BC.parameter_cases() if x["name"] == "perception_2.5")
    return c, FC.perception(c)


def test_rows_no_longer_in_caller_order(gpu):
    """Three steps leave the handle's rows in cell order.  The stepped state is put back on the lattice through
    bdmi_set_state, which keeps that row order, so that the comparison stays bit for bit."""
    c, link = _stepping_case()
    f = Stats(gpu, c["pos"], c["vel"], c["col"], c["params"])
    try:
        f.step(c["dt"], 3)
        p, v, col = f.state()
        p, v = R.lattice(p, 16), R.lattice(v, 20)
        gpu.check(f.lib.bdmi_set_state(f.h, gpu.ptr(p), gpu.ptr(v), None), "bdmi_set_state")
        p2, v2, _ = f.state()
        assert R.same_bits(p, p2) and R.same_bits(v, v2) and not np.array_equal(p, c["pos"])
        _check_state(f, p2, v2, link, "stepped", min_members=2)
    finally:
        f.close()


def test_calls_between_steps_change_nothing_and_repeat_bit_for_bit(gpu):
    c, link = _stepping_case()
    a = Stats(gpu, c["pos"], c["vel"], c["col"], c["params"])
    b = Stats(gpu, c["pos"], c["vel"], c["col"], c["params"])
    try:
        for k in range(3):
            a.step(c["dt"])
            b.step(c["dt"])
            first = (b.flocks(link), b.catalogue(link, 2, 50), b.diagnostics(), b.neighbours(link))
            again = (b.flocks(link), b.catalogue(link, 2, 50), b.diagnostics(), b.neighbours(link))
            for (rc1, r1), (rc2, r2) in zip(first, again):
                assert rc1 == 0 and rc2 == 0, gpu.last_error()
                for x, y in zip((r1.values() if isinstance(r1, dict) else [r1]), (r2.values() if isinstance(r2, dict) else [r2])):
                    assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), k
            assert first[1][1]["count"] > 0 and first[0][1]["links"] > 0
        for x, y in zip(a.state(), b.state()):
            assert R.same_bits(x, y)
    finally:
        a.close()
        b.close()


def test_grid_info_describes_the_query_grid(gpu):
    c = BC.hit_list()
    f = Stats(gpu, c["pos"], c["vel"], c["col"], c["params"])
    try:
        assert f.diagnostics()[0] == 0
        occ = C.c_int64(0)
        gpu.check(f.lib.bdmi_grid_info(f.h, None, None, C.addressof(occ)), "bdmi_grid_info")
        assert occ.value == len(np.unique(R.cell_index(c["pos"], c["params"])))
    finally:
        f.close()


def test_flock_class_methods(gpu):
    from boids import Flock
    from boids.analysis import row_dict, size_histogram
    fl = Flock(3000, seed=5)
    try:
        rng = np.random.default_rng(5)  # the configured box is far too large for 3000 boids to meet: clumps instead
        centres = rng.uniform(-30, 30, (12, 3))
        fl.set_state(positions=centres[rng.integers(0, 12, 3000)] + rng.normal(0, 4.0, (3000, 3)))
        fl.update(1.0 / 60.0, 2)
        pos, vel = fl.positions, fl.velocities
        link = float(fl.perception_radius)
        want = FR.analyse(pos, link)
        got = fl.flocks()
        assert np.array_equal(got["labels"], want["labels"]) and got["links"] == want["links"]
        nb = fl.neighbour_stats()
        assert np.array_equal(nb["count"], want["count"]) and R.same_bits(nb["nn_d2"], want["nn_d2"])
        cat = fl.flock_catalogue(min_members=2, capacity=5)
        ref = FR.catalogue(pos, vel, want["labels"], 2)
        assert cat["count"] == ref["count"] and np.array_equal(cat["label"], ref["label"][:5])
        assert np.array_equal(cat["members"], ref["members"][:5]) and cat["rows"].shape == (min(5, ref["count"]), 16)
        d = row_dict(fl.diagnostics())
        assert d["members"] == 3000 and 0.0 <= d["polarisation"] <= 1.0 and 0.0 <= d["milling"] <= 1.0
        assert sum(size_histogram(fl.flock_catalogue(capacity=3000)["members"]).values()) == got["n_flocks"]
        assert fl.flocks(link=2.0)["links"] < got["links"]
        with pytest.raises(ValueError, match="bdmi_flocks"):
            fl.flocks(link=link * 2)
    finally:
        fl.close()
