"""Flock analysis on periodic handles (include/bdmi.h: bdmi_periodic_flocks, bdmi_periodic_flock_catalogue,
bdmi_periodic_neighbour_stats; csrc/bdmi.hip) against the NumPy restatement tests/torus_ref.py on the constructed cases of
tests/torus_cases.py.  Everything is compared bit for bit: labels, counts, links, evaluations, nn_d2, the catalogue's
order, members, cuts and all 16 doubles of every row (the restatement adds in the header's order).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import boids_cases as BC
import boids_ref as R
import periodic_ref as PR
import torus_cases as TC
import torus_ref as TR
from test_gpu_boids import RawFlock
from test_gpu_boids_periodic import PeriodicFlock
from test_gpu_boids_topological import TOPOLOGICAL, same_state, set_mode
from test_gpu_flockstats import Stats

pytestmark = pytest.mark.gpu

NAMES = tuple(c["name"] + (f"_link_{c['link']!r}" if c["name"] == "face_pair" else "") for c in TC.gpu_cases())


class TorusStats(PeriodicFlock):
    """PeriodicFlock plus the three calls; every output array is the caller's, so a refusal can be seen to leave it alone."""

    def flocks(self, link, labels=True):
        lab = np.full(self.n, -7, dtype=np.int32) if labels else None
        out = [C.c_int64(-7) for _ in range(3)]
        rc = self.lib.bdmi_periodic_flocks(self.h, link, self.nat.ptr(lab), *[C.addressof(x) for x in out])
        return rc, dict(labels=lab, n_flocks=out[0].value, links=out[1].value, evals=out[2].value)

    def catalogue(self, link, min_members=1, capacity=0, null_outputs=False, null_wrap=False):
        label = np.full(max(capacity, 0), -7, dtype=np.int32)
        members = np.full(max(capacity, 0), -7, dtype=np.int64)
        rows = np.full((max(capacity, 0), 16), -7.0)
        wrap = np.full((max(capacity, 0), 3), -7, dtype=np.int32)
        cnt = C.c_int64(-7)
        ptrs = [None] * 3 if null_outputs else [self.nat.ptr(a) for a in (label, members, rows)]
        rc = self.lib.bdmi_periodic_flock_catalogue(self.h, link, min_members, capacity, *ptrs,
                                                    None if null_outputs or null_wrap else self.nat.ptr(wrap), C.addressof(cnt))
        return rc, dict(count=cnt.value, label=label, members=members, rows=rows, wrap=wrap)

    def neighbours(self, radius):
        count, nn, ev = np.full(self.n, -7, dtype=np.int32), np.full(self.n, -7.0), C.c_int64(-7)
        rc = self.lib.bdmi_periodic_neighbour_stats(self.h, radius, self.nat.ptr(count), self.nat.ptr(nn), C.addressof(ev))
        return rc, dict(count=count, nn_d2=nn, evals=ev.value)


@functools.lru_cache(maxsize=None)
def _want(name):
    """The case and its restatement, computed once and shared (read only)."""
    c = TC.gpu_cases()[NAMES.index(name)]
    a = TR.analyse(c["pos"], c["params"], c["link"])
    return c, a, TR.catalogue(c["pos"], c["vel"], a["labels"], c["params"])


def _check(f, c, a, cat, what, min_members=1):
    """All three calls on a handle whose state is the case, against the restatement (a, cat)."""
    link = c["link"]
    rc, got = f.flocks(link)
    assert rc == 0, f.nat.last_error()
    assert np.array_equal(got["labels"], a["labels"]), what
    assert (got["n_flocks"], got["links"], got["evals"]) == (a["n_flocks"] if f.n else 0, a["links"], a["evals"]), what
    rc, nb = f.neighbours(link)
    assert rc == 0, f.nat.last_error()
    assert np.array_equal(nb["count"], a["count"]) and R.same_bits(nb["nn_d2"], a["nn_d2"]), what
    assert nb["evals"] == a["nb_evals"] and int(nb["count"].astype(np.int64).sum()) == 2 * got["links"], what
    rc, head = f.catalogue(link, min_members, 0, null_outputs=True)  # capacity 0, NULL outputs: the count alone
    assert rc == 0 and head["count"] == cat["count"], (what, f.nat.last_error())
    rc, full = f.catalogue(link, min_members, cat["count"])
    assert rc == 0 and full["count"] == cat["count"], (what, f.nat.last_error())
    assert np.array_equal(full["label"], cat["label"]) and np.array_equal(full["members"], cat["members"]), what
    assert np.array_equal(full["wrap"], cat["wrap"]), (what, full["wrap"][:4], cat["wrap"][:4])
    bad = [k for k in range(cat["count"]) if not TR.same_rows(full["rows"][k], cat["rows"][k])]
    assert not bad, (what, bad[:5], full["rows"][bad[0]], cat["rows"][bad[0]])
    rc, again = f.catalogue(link, min_members, cat["count"], null_wrap=True)  # wrap3 == NULL; the same bits twice
    assert rc == 0 and R.same_bits(again["rows"], full["rows"]) and (again["wrap"] == -7).all(), what
    if cat["count"] > 1:  # fewer rows than flocks: the first ones of the order, the rest of the arrays untouched
        k = cat["count"] // 2
        label = np.full(cat["count"], -7, dtype=np.int32)
        members = np.full(cat["count"], -7, dtype=np.int64)
        rows, wrap, cnt = np.full((cat["count"], 16), -7.0), np.full((cat["count"], 3), -7, dtype=np.int32), C.c_int64(-7)
        rc = f.lib.bdmi_periodic_flock_catalogue(f.h, link, min_members, k, *[f.nat.ptr(x) for x in (label, members, rows, wrap)],
                                                 C.addressof(cnt))
        assert rc == 0 and cnt.value == cat["count"], what
        assert np.array_equal(label[:k], cat["label"][:k]) and np.array_equal(members[:k], cat["members"][:k]), what
        assert R.same_bits(rows[:k], full["rows"][:k]) and np.array_equal(wrap[:k], cat["wrap"][:k]), what
        assert (label[k:] == -7).all() and (members[k:] == -7).all() and (rows[k:] == -7).all() and (wrap[k:] == -7).all()
    return got, nb, full


def _run(nat, c, a, cat, **kw):
    f = TorusStats(nat, c["pos"], c["vel"], c["col"], c["params"])
    try:
        return _check(f, c, a, cat, c["name"], **kw)
    finally:
        f.close()


@pytest.mark.parametrize("name", NAMES)
def test_cases_match_restatement(gpu, name):
    c, a, cat = _want(name)
    got, _, full = _run(gpu, c, a, cat)
    spans = int((cat["wrap"] == -1).any(axis=1).sum()) if cat["count"] else 0
    print(f"{name}: n={len(c['pos'])} flocks {got['n_flocks']} links {got['links']} evals {got['evals']}, largest "
          f"{cat['members'][:1].tolist()}, spanning {spans}")
    # what the constructed cases are for
    if name.startswith("face_pair"):
        assert got["links"] == (1 if c["link"] == 1.0 else 0)
    if name == "chain" or name == "chain_2_3":
        assert full["wrap"][0, 0] == -1 and (full["wrap"][0, 1:] >= 0).all() and got["n_flocks"] == 1
    if name.startswith("big_blob"):
        assert cat["members"].tolist() == [4200] and cat["wrap"][0, 0] == 3 and full["rows"][0, 13] > 10.0
    if name.startswith("face_blob"):
        assert full["rows"][0, 13] > 10.0 and abs(full["rows"][0, 1]) <= 10.0
    if name == "n_0":
        assert (got["n_flocks"], got["links"], got["evals"], full["count"]) == (0, 0, 0, 0)
    if name == "n_1":
        assert (got["n_flocks"], got["labels"].tolist(), full["members"].tolist()) == (1, [0], [1])


def test_min_members_and_a_second_link(gpu):
    c, a, _ = _want("mixed_2048")
    _run(gpu, c, a, TR.catalogue(c["pos"], c["vel"], a["labels"], c["params"], min_members=3), min_members=3)
    half = dict(c, link=1.25)
    a = TR.analyse(c["pos"], c["params"], 1.25)
    _run(gpu, half, a, TR.catalogue(c["pos"], c["vel"], a["labels"], c["params"]))


def test_caller_permutation_and_block_order(gpu, monkeypatch):
    """The permuted input against the restatement OF the permuted input (the member order follows the rows), the same
    flocks as before the permutation, and the hardware block order (BDMI_XCD=0) the same bits as the default one."""
    c, a, cat = _want("box_4")
    t, perm = TC.permuted(c)
    at = TR.analyse(t["pos"], t["params"], t["link"])
    catt = TR.catalogue(t["pos"], t["vel"], at["labels"], t["params"])
    _, _, full = _run(gpu, t, at, catt)
    assert np.array_equal(np.sort(catt["members"]), np.sort(cat["members"])) and at["links"] == a["links"]
    inv = np.argsort(perm)  # boid i of the case is row inv[i] of the permuted one
    assert np.array_equal(a["labels"][perm] == a["labels"][perm][:, None], at["labels"] == at["labels"][:, None])
    assert np.array_equal(at["count"], a["count"][perm]) and inv[perm[5]] == 5
    monkeypatch.setenv("BDMI_XCD", "0")
    _, _, full_x = _run(gpu, t, at, catt)
    assert R.same_bits(full_x["rows"], full["rows"])


def test_translation_across_a_face(gpu):
    """The whole state moved by a lattice vector and wrapped: every d2 is the same number, so the same partition, the same
    labels (the smallest index of a flock does not move) and the same members; the rows follow the restatement."""
    c, a, cat = _want("box_4")
    t = TC.translated(c, [3.0 + 2.0 ** -3, -7.0 - 2.0 ** -10, 10.0 + 2.0 ** -16])
    assert PR.crossings(c["pos"] + [3.0 + 2.0 ** -3, -7.0 - 2.0 ** -10, 10.0 + 2.0 ** -16], t["pos"], c["params"]).mean() > 0.3
    at = TR.analyse(t["pos"], t["params"], t["link"])
    catt = TR.catalogue(t["pos"], t["vel"], at["labels"], t["params"])
    got, nb, full = _run(gpu, t, at, catt)
    assert np.array_equal(got["labels"], a["labels"]) and (got["n_flocks"], got["links"]) == (a["n_flocks"], a["links"])
    assert np.array_equal(nb["count"], a["count"]) and R.same_bits(nb["nn_d2"], a["nn_d2"])
    assert np.array_equal(full["label"], cat["label"]) and np.array_equal(full["members"], cat["members"])


def test_interior_flock_equals_a_walled_handle(gpu):
    """Further than `link` from every face nothing is shifted: labels, n_flocks, links and members are those of
    bdmi_flocks / bdmi_flock_catalogue on a walled handle with the same constants (the rows differ in their order of
    summation, because the cell order of the two grids differs: they are checked against the restatement only)."""
    c = TC.interior()
    a = TR.analyse(c["pos"], c["params"], c["link"])
    cat = TR.catalogue(c["pos"], c["vel"], a["labels"], c["params"])
    got, _, full = _run(gpu, c, a, cat)
    w = Stats(gpu, c["pos"], c["vel"], c["col"], c["params"])
    try:
        rc, wf = w.flocks(c["link"])
        assert rc == 0, gpu.last_error()
        rc, wc = w.catalogue(c["link"], 1, cat["count"])
        assert rc == 0, gpu.last_error()
    finally:
        w.close()
    assert np.array_equal(wf["labels"], got["labels"]) and (wf["n_flocks"], wf["links"]) == (got["n_flocks"], got["links"])
    assert wc["count"] == full["count"] and np.array_equal(wc["label"], full["label"])
    assert np.array_equal(wc["members"], full["members"]) and (full["wrap"] >= 0).all()


@pytest.mark.parametrize("mode", ["metric", "topological"])
def test_calls_between_steps_change_nothing(gpu, mode):
    """Ten noisy steps with all three calls between every step give the state bits of ten steps without."""
    c = TC.mixed()
    out = []
    for calls in (False, True):
        f = TorusStats(gpu, c["pos"], c["vel"], c["col"], c["params"])
        try:
            if mode == "topological":
                assert set_mode(f, TOPOLOGICAL, 7) == 0, gpu.last_error()
            gpu.check(f.lib.bdmi_set_noise(f.h, 0.5, 9, -1), "bdmi_set_noise")
            for s in range(10):
                f.step(c["dt"])
                if calls:
                    assert f.flocks(c["link"])[0] == 0 and f.neighbours(c["link"])[0] == 0, gpu.last_error()
                    assert f.catalogue(c["link"], 2, 16)[0] == 0, gpu.last_error()
            out.append(f.state())
            if calls:  # ... and bdmi_grid_info afterwards describes the grid of the current positions
                dim, cells, occ = C.c_int32(0), C.c_int64(0), C.c_int64(0)
                gpu.check(f.lib.bdmi_grid_info(f.h, C.addressof(dim), C.addressof(cells), C.addressof(occ)), "bdmi_grid_info")
                assert (dim.value, cells.value) == (7, 343)
                assert occ.value == len(np.unique(PR.cell_index(out[-1][0], c["params"])))
                # the stepped state (rows now in cell order, which the restatement is told) against the restatement
                pos, vel, _ = out[-1]
                a = TR.analyse(pos, c["params"], c["link"])
                rc, got = f.flocks(c["link"])
                assert rc == 0 and np.array_equal(got["labels"], a["labels"]) and got["links"] == a["links"]
        finally:
            f.close()
    assert same_state(out[0], out[1])


def _refused(nat, rc, call):
    assert rc == -1 and nat.last_error().startswith(call + ": "), (rc, nat.last_error())
    return nat.last_error()


def test_refusals(gpu):
    lib = gpu.load()
    c = TC.sizes(255)
    n = 255
    names = ("bdmi_periodic_flocks", "bdmi_periodic_flock_catalogue", "bdmi_periodic_neighbour_stats")
    labels = np.full(n, -7, dtype=np.int32)
    cnt, nn = np.full(n, -7, dtype=np.int32), np.full(n, -7.0)
    lab16, mem16, rows16 = np.full(16, -7, dtype=np.int32), np.full(16, -7, dtype=np.int64), np.full((16, 16), -7.0)
    wrap16 = np.full((16, 3), -7, dtype=np.int32)
    nf = C.c_int64(-7)
    p, a = gpu.ptr, C.addressof

    def all_three(h, link=2.0):
        """(return code, message) of each call, the message read before the next call replaces it"""
        calls = (lambda: lib.bdmi_periodic_flocks(h, link, p(labels), a(nf), a(nf), a(nf)),
                 lambda: lib.bdmi_periodic_flock_catalogue(h, link, 1, 16, p(lab16), p(mem16), p(rows16), p(wrap16), a(nf)),
                 lambda: lib.bdmi_periodic_neighbour_stats(h, link, p(cnt), p(nn), a(nf)))
        out = []
        for call, name in zip(calls, names):
            rc = call()
            out.append(_refused(gpu, rc, name) if rc else "")
        return out

    def untouched():
        return nf.value == -7 and all((x == -7).all() for x in (labels, cnt, nn, lab16, mem16, rows16, wrap16))

    # a null handle
    assert all("null" in m for m in all_three(None)) and untouched()
    # a walled handle: the message points to the walled call
    w = RawFlock(gpu, c["pos"], c["vel"], c["col"], c["params"])
    try:
        for m, walled in zip(all_three(w.h), ("bdmi_flocks", "bdmi_flock_catalogue", "bdmi_neighbour_stats")):
            assert "walled" in m and m.endswith("use " + walled), m
        assert untouched()
    finally:
        w.close()
    # a slab handle
    ids = np.arange(n, dtype=np.int32)
    prm = BC.params(bounds=30.0)
    slab = lib.bdmi_create_slab(n, p(c["pos"]), p(c["vel"]), p(c["col"]), p(ids), 2 * n, p(prm), -35.0, 35.0, 0, 0, 0)
    assert slab, gpu.last_error()
    try:
        assert all("slab" in m for m in all_three(slab)) and untouched()
    finally:
        lib.bdmi_destroy(slab)
    f = TorusStats(gpu, c["pos"], c["vel"], c["col"], c["params"])
    try:
        before = f.state()
        # a bad link or radius: the message names both numbers
        for bad in (0.0, -1.0, np.nan, np.inf, np.nextafter(5.0, 6.0)):
            for m in all_three(f.h, link=bad):
                assert "perception radius 5" in m and ("nan" in m or "inf" in m or f"{bad:g}" in m), m
        assert untouched()
        # min_members < 1, capacity < 0, a null count, a null output with capacity > 0
        rc = lib.bdmi_periodic_flock_catalogue(f.h, 2.0, 0, 16, p(lab16), p(mem16), p(rows16), p(wrap16), a(nf))
        assert "min_members = 0" in _refused(gpu, rc, names[1])
        rc = lib.bdmi_periodic_flock_catalogue(f.h, 2.0, 1, -1, p(lab16), p(mem16), p(rows16), p(wrap16), a(nf))
        assert "capacity = -1" in _refused(gpu, rc, names[1])
        rc = lib.bdmi_periodic_flock_catalogue(f.h, 2.0, 1, 16, p(lab16), p(mem16), p(rows16), p(wrap16), None)
        assert "null count" in _refused(gpu, rc, names[1])
        for k in range(3):
            outs = [p(lab16), p(mem16), p(rows16)]
            outs[k] = None
            rc = lib.bdmi_periodic_flock_catalogue(f.h, 2.0, 1, 16, *outs, p(wrap16), a(nf))
            assert "null output" in _refused(gpu, rc, names[1])
        assert untouched()
        # the largest link is the perception radius itself
        assert all_three(f.h, link=5.0) == ["", "", ""], gpu.last_error()
        # the old calls still refuse the periodic handle
        nf.value = -7
        for x in (labels, cnt, nn, lab16, mem16, rows16, wrap16):
            x[...] = -7
        rc = lib.bdmi_flocks(f.h, 2.0, p(labels), a(nf), None, None)
        assert "periodic" in _refused(gpu, rc, "bdmi_flocks")
        rc = lib.bdmi_flock_catalogue(f.h, 2.0, 1, 16, p(lab16), p(mem16), p(rows16), a(nf))
        assert "periodic" in _refused(gpu, rc, "bdmi_flock_catalogue")
        rc = lib.bdmi_neighbour_stats(f.h, 2.0, p(cnt), p(nn), a(nf))
        assert "periodic" in _refused(gpu, rc, "bdmi_neighbour_stats")
        assert untouched() and same_state(f.state(), before)
    finally:
        f.close()


def test_python_layer(gpu):
    """Flock.periodic_* and boids.analysis.percolation_summary on a 2 048-boid periodic flock."""
    from boids import Flock
    from boids.analysis import percolation_summary
    import config.boids as config
    saved = dict(config.BOIDS)
    config.BOIDS["bounds"] = 18.75  # 2 048 boids in a box of 7 cells per side: near percolation at link 2.5
    try:
        f, g, w = Flock(2048, seed=5, periodic=True), Flock(2048, seed=6, periodic=True), Flock(64, seed=5)
        prm = np.array([float(config.BOIDS[k]) for k in config.PARAM_ORDER])
    finally:
        config.BOIDS.clear()
        config.BOIDS.update(saved)
    try:
        f.update(1.0 / 60.0, 5)
        pos, vel = f.positions.copy(), f.velocities.copy()
        a = TR.analyse(pos, prm, 2.5)
        fl = f.periodic_flocks(2.5)
        assert np.array_equal(fl["labels"], a["labels"]) and (fl["n_flocks"], fl["links"]) == (a["n_flocks"], a["links"])
        nb = f.periodic_neighbour_stats(2.5)
        assert np.array_equal(nb["count"], a["count"]) and R.same_bits(nb["nn_d2"], a["nn_d2"])
        # after steps the handle's rows are in the last step's cell order, which Python cannot see: the member order is the
        # restatement's only for a freshly uploaded state
        g.set_state(pos, vel, None)  # g has not stepped: its row order is the caller's order
        cat = g.periodic_flock_catalogue(2.5, min_members=2, capacity=32)
        want = TR.catalogue(pos, vel, a["labels"], prm, min_members=2)
        k = min(32, want["count"])
        assert cat["count"] == want["count"] and np.array_equal(cat["label"], want["label"][:k])
        assert np.array_equal(cat["members"], want["members"][:k]) and np.array_equal(cat["wrap"], want["wrap"][:k])
        assert cat["spans"].dtype == bool and np.array_equal(cat["spans"], want["wrap"][:k] == -1)
        assert all(TR.same_rows(cat["rows"][r], want["rows"][r]) for r in range(k))
        s = percolation_summary(cat, 2048)
        assert s["largest_fraction"] == want["members"][0] / 2048 and s["largest_spans"] == (want["wrap"][0] == -1).tolist()
        assert s["spanning_flocks"] == int((want["wrap"][:k] == -1).any(axis=1).sum()) and 0 < s["largest_fraction"] <= 1
        whole = f.periodic_flocks()  # the default link is the perception radius: about 20 friends each, one flock
        assert whole["n_flocks"] == 1 and np.all(whole["labels"] == 0)
        assert f.periodic_flock_catalogue()["spans"].tolist() == [[True, True, True]]
        with pytest.raises(ValueError, match="bdmi_periodic_flocks: .*perception"):
            f.periodic_flocks(link=6.0)
        with pytest.raises(ValueError, match="bdmi_periodic_flock_catalogue: "):
            f.periodic_flock_catalogue(min_members=0)
        with pytest.raises(ValueError, match="bdmi_periodic_neighbour_stats: "):
            f.periodic_neighbour_stats(radius=-1.0)
        with pytest.raises(ValueError, match="bdmi_periodic_flocks: .*walled"):
            w.periodic_flocks()
    finally:
        f.close()
        g.close()
        w.close()
