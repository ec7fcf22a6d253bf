"""The constructed slab cases (tests/slab_cases.py) and the slab protocol's NumPy restatement
(tests/slab_ref.py), checked on the host: every case has what it claims, one exchange and step of the
model equals the all-pairs reference of the whole flock (tests/boids_ref.py), the step guard's condition
is the one at which the model starts to lose boids, and the plane split equals boids.sharded.slab_planes.
"""
import numpy as np
import pytest

import boids_ref as R
import slab_cases as SC
import slab_ref as S

_MULTI = {
    **{f"faces_{w}": (lambda w=w: SC.faces(w)) for w in (2, 3, 7)},
    **{f"faces_sep_{w}": (lambda w=w: SC.faces_sep(w)) for w in (2, 3, 7)},
    "outside": SC.outside,
    "empty_slab": SC.empty_slab,
    "draining_slab": SC.draining_slab,
    "migration_3": lambda: SC.migration(3),
    "migration_7": lambda: SC.migration(7),
    "long_step": SC.long_step,
}


def _pairs(c):
    """Neighbour pairs (i, j), i < j, of a case by distance alone (the test of boids_ref.flocking)."""
    pos, p = c["pos"], R.unpack(c["params"])["perception_radius"]
    d = pos[:, None, :] - pos[None, :, :]
    dsq = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    i, j = np.nonzero(np.triu((dsq < p * p) & (dsq > 0.0001), 1))
    return i, j, dsq


@pytest.mark.parametrize("name", sorted(_MULTI))
def test_names_and_sizes(name):
    c = _MULTI[name]()
    assert c["name"] == name and 100 <= len(c["pos"]) <= 5000
    assert R.grid(c["params"]) == (5.0, 14, 35.0)
    # positions on the 2^-16 lattice (the face cases: a few boids on 2^-20, between two of its values)
    fine = ~np.all(c["pos"] == R.lattice(c["pos"], SC.PB), axis=1)
    assert fine.sum() == (2 * (c["world"] - 1) if name.startswith("faces") else 0)
    assert np.array_equal(c["pos"], R.lattice(c["pos"], 20)) and np.array_equal(c["vel"], R.lattice(c["vel"], SC.VB))


@pytest.mark.parametrize("world", [2, 3, 7])
@pytest.mark.parametrize("sep", [False, True])
def test_faces_have_what_they_claim(world, sep):
    c = SC.faces_sep(world) if sep else SC.faces(world)
    pos, face, h = c["pos"], S.faces(c["params"], world), SC.H
    own = S.owner_of(pos[:, 0], face)
    i, j, dsq = _pairs(c)
    F = R.flocking(pos, c["vel"], c["col"], c["params"])
    if sep:
        assert F.nsep.max() > 0
    else:
        assert F.nsep.max() == 0
        off = dsq + np.eye(len(pos)) * 1e9
        assert off.min() >= 9.0  # nothing coincident either (a pair below 0.01 would hide from the neighbour test)
    cc = R.cell_coords(pos, c["params"])
    for k, f in enumerate(face[1:-1]):
        # every x the layout names is there
        for dx in (0, -h, h, 5, -5, 5 - h, 5 + h, -5 - h, -5 + h):
            assert (pos[:, 0] == f + dx).any(), (f, dx)
        cross = (own[i] == k) & (own[j] == k + 1) | (own[i] == k + 1) & (own[j] == k)
        assert cross.sum() >= 20, (f, cross.sum())  # neighbour pairs that only a ghost can supply
        dx = np.abs(pos[i, 0] - pos[j, 0])
        assert (cross & (dx == 5 - h)).any()  # just under the perception radius, along x
        # the last lattice x of either halo zone is somebody's neighbour across the face
        xa, xb = np.minimum(pos[i, 0], pos[j, 0]), np.maximum(pos[i, 0], pos[j, 0])
        assert (cross & (xb == f + 5 - h) & (xa < f)).any()
        assert (cross & (xa > f - 5) & (xa < f - 5 + h) & (xb == f)).any()
        a, b = np.nonzero(np.triu(dsq == 25.0, 1))
        assert ((own[a] != own[b]) & (np.minimum(pos[a, 0], pos[b, 0]) < f) & (np.maximum(pos[a, 0], pos[b, 0]) >= f)).any()
        assert (cross & (cc[i, 1] != cc[j, 1]) & (cc[i, 2] != cc[j, 2])).any()  # diagonal, across a y and a z border too
        if sep:
            assert (cross & (dsq[i, j] < 9.0)).sum() >= 5
    if world == 7:
        assert np.array_equal(np.diff(face), np.full(7, 10.0))  # seven slabs of two cells
        # the chain across a two-cell slab: a boid whose two neighbours leave as halo rows in opposite directions,
        # and in the same slab boids with a neighbour in the slab on the left and on the right
        for r in range(1, 6):
            mine = own == r
            left = np.zeros(len(pos), dtype=bool)
            right = np.zeros(len(pos), dtype=bool)
            for a, b in ((i, j), (j, i)):
                np.logical_or.at(left, a[(own[b] == r - 1)], True)
                np.logical_or.at(right, a[(own[b] == r + 1)], True)
            assert (mine & left).any() and (mine & right).any()
            assert not (mine & left & right).any()  # impossible: the slab is 2 p wide


def test_outside_has_clamped_boids_on_every_side():
    c = SC.outside()
    pos, face = c["pos"], S.faces(c["params"], 3)
    assert (pos[:, 0] < -35).sum() > 50 and (pos[:, 0] >= 35).sum() > 50
    for f in face[1:-1]:
        near = np.abs(pos[:, 0] - f) < 5
        for ax in (1, 2):
            assert (near & (pos[:, ax] < -35) & (pos[:, 0] < f)).any() and (near & (pos[:, ax] < -35) & (pos[:, 0] >= f)).any()
            assert (near & (pos[:, ax] > 35) & (pos[:, 0] < f)).any() and (near & (pos[:, ax] > 35) & (pos[:, 0] >= f)).any()
    own = S.owner_of(pos[:, 0], face)
    i, j, _ = _pairs(c)
    out = (np.abs(pos) > 35).any(axis=1)
    assert ((own[i] != own[j]) & (out[i] | out[j])).sum() >= 10  # neighbours across a face, beyond the grid


def test_empty_slab_fills_by_import_only():
    c = SC.empty_slab()
    m = S.SlabModel(c["pos"], c["vel"], c["col"], c["params"], 3)
    assert len(m.owned(1)) == 0 and len(m.owned(0)) > 0 and len(m.owned(2)) > 0
    assert (c["pos"][:, 0] == -10 - SC.H).sum() == 40 and (c["pos"][:, 0] == 10).sum() == 40
    m.exchange()
    assert len(m.owned(1)) == 0 and m.ghost[1].sum() >= 80  # a ghost-only slab in its first step
    m.step(c["dt"])
    m.exchange()
    assert len(m.owned(1)) >= 80  # both groups have arrived


def test_draining_slab_drains():
    c = SC.draining_slab()
    m = S.SlabModel(c["pos"], c["vel"], c["col"], c["params"], 3)
    counts = []
    for _ in range(8):
        m.exchange()
        counts.append(len(m.owned(1)))
        m.step(c["dt"])
    print("owned by the middle slab:", counts)
    assert counts[0] == 300 and counts[-1] == 0
    S.assert_partition(m.owners(), len(c["pos"]))


@pytest.mark.parametrize("n,where", SC.TILE_NAMES)
def test_tile_edges_placement(n, where):
    c = SC.tile_edges(n, where)
    x = c["pos"][:, 0]
    lo, hi = c["slab"]
    assert len(x) == n and hi - lo == 15.0
    left, right, dem = S.export_sets(x, np.ones(n, dtype=bool), lo, hi, SC.CELL, True, True)
    sel = left | right
    assert np.array_equal(sel, c["selected"]) and not (left & right).any()
    tile = np.arange(n) // SC.TILE
    ntiles = (n + SC.TILE - 1) // SC.TILE
    if where == "last":
        assert set(tile[sel]) == {ntiles - 1}
    elif where == "first":
        assert set(tile[sel]) == {0} and sel[:min(n, SC.TILE)].all()
    else:
        assert sel.all() and set(tile[sel]) == set(range(ntiles))
    assert left.sum() >= 1 and (where == "last" and (n - 1) % SC.TILE == 0 or right.sum() >= 1)
    if sel.sum() >= 8:
        assert (dem & left).any() and (dem & right).any() and (left & ~dem).any() and (right & ~dem).any()
    if sel.sum() >= 6:
        for v, l, r, d in ((-5 - SC.H, 1, 0, 0), (0.0, 0, 1, 0), (-10.0, 1, 0, 0), (5 - SC.H, 0, 1, 0), (-10 - SC.H, 1, 0, 1),
                           (5.0, 0, 1, 1)):
            k = np.flatnonzero(x == v)
            assert len(k) >= 1 and (left[k] == l).all() and (right[k] == r).all() and (dem[k] == d).all(), v
    for v in (-5.0, -SC.H)[:int((~sel).sum())]:  # the first x that neither side selects
        assert (~sel[x == v]).all() and (x == v).any()


@pytest.mark.parametrize("name", sorted(_MULTI))
def test_model_step_equals_all_pairs(name):
    """One exchange and step of the slab model = one step of the whole flock: colours bit for bit, positions and
    velocities bit for bit where no separation term enters (otherwise to the summation-order bound, 1e-9)."""
    c = _MULTI[name]()
    pos, vel, col, prm, dt, n = c["pos"], c["vel"], c["col"], c["params"], c["dt"], len(c["pos"])
    F = R.flocking(pos, vel, col, prm)
    ep, ev, ec = R.physics(pos, vel, col, (F.sep, F.ali, F.coh, F.avg), prm, dt)
    m = S.SlabModel(pos, vel, col, prm, c["world"])
    m.exchange()
    m.step(dt)
    S.assert_partition(m.owners(), n)
    p, v, cl = m.gather(n)
    assert R.same_bits(cl, ec)
    k = F.nsep == 0
    assert R.same_bits(p[k], ep[k]) and R.same_bits(v[k], ev[k])
    assert np.abs(p - ep).max() <= 1e-9 and np.abs(v - ev).max() <= 1e-9
    # every boid is owned by the slab of its step-start x
    face = S.faces(prm, c["world"])
    for r, ids in enumerate(m.owners()):
        assert (S.owner_of(pos[ids, 0], face) == r).all()


@pytest.mark.parametrize("world", [3, 7])
def test_migration_crosses_every_face_both_ways(world):
    c = SC.migration(world)
    face = S.faces(c["params"], world)
    m = S.SlabModel(c["pos"], c["vel"], c["col"], c["params"], world)
    start = S.owner_of(c["pos"][:, 0], face)
    up = np.zeros(world, dtype=np.int64)
    down = np.zeros(world, dtype=np.int64)
    prev = start
    for _ in range(25):
        m.exchange()
        m.step(c["dt"])
        now = np.empty(len(start), dtype=np.int64)
        for r, ids in enumerate(m.owners()):
            now[ids] = r
        S.assert_partition(m.owners(), len(start))
        assert np.abs(now - prev).max() <= 1
        np.add.at(up, prev[now == prev + 1], 1)
        np.add.at(down, prev[now == prev - 1], 1)
        prev = now
    print("moved right from rank", up, "moved left from rank", down)
    assert (up[:-1] > 0).all() and (down[1:] > 0).all()


def _survivors(c, exchanges=3):
    m = S.SlabModel(c["pos"], c["vel"], c["col"], c["params"], c["world"])
    for _ in range(exchanges):
        m.exchange()
        m.step(c["dt"])
    m.exchange()
    return np.concatenate(m.owners())


def test_step_guard_condition_on_the_model():
    """max_speed * dt < two cells keeps every boid; the next lattice dt loses the boids that fly straight."""
    c = SC.long_step()
    P = R.unpack(c["params"])
    assert c["world"] == 7 and c["dt"] == SC.LONG_DT == 25 / 64
    assert P["max_speed"] * SC.LONG_DT < 2 * SC.CELL <= P["max_speed"] * SC.TOO_LONG_DT
    assert SC.TOO_LONG_DT - SC.LONG_DT == 1 / 64
    n = len(c["pos"])
    ids = _survivors(c)
    assert len(ids) == n and np.array_equal(np.sort(ids), np.arange(n))
    # the straight flyers have no neighbours and end a step in the adjacent slab, h short of its far face
    F = R.flocking(c["pos"], c["vel"], c["col"], c["params"])
    fly = np.abs(c["vel"][:, 0]) == 25.0
    assert fly.sum() == 6 * 24 and F.nb[fly].max() == 0
    face = S.faces(c["params"], 7)
    ep, _, _ = R.physics(c["pos"], c["vel"], c["col"], (F.sep, F.ali, F.coh, F.avg), c["params"], c["dt"])
    assert (np.abs(S.owner_of(ep[fly, 0], face) - S.owner_of(c["pos"][fly, 0], face)) == 1).all()
    bad = SC.long_step(dt=SC.TOO_LONG_DT)
    assert R.same_bits(bad["pos"], c["pos"]) and R.same_bits(bad["vel"], c["vel"])
    lost = n - len(np.unique(_survivors(bad)))
    print("boids lost at dt = 26/64:", lost)
    assert lost >= 1


def test_plane_split_equals_slab_planes():
    from boids.sharded import slab_planes
    for dim in range(4, 65):
        refused = None
        for world in range(1, dim + 2):
            try:
                want = slab_planes(dim, world)
            except ValueError:
                with pytest.raises(ValueError):
                    S.planes(dim, world)
                refused = world
                break
            b = S.planes(dim, world)
            assert b == want and b[0] == 0 and b[-1] == dim and min(np.diff(b)) >= 2
        assert refused is not None and refused <= dim // 2 + 1
    prm = SC.params()
    assert np.array_equal(S.faces(prm, 3), [-35.0, -10.0, 10.0, 35.0])
    assert np.array_equal(S.faces(prm, 7), -35.0 + 10.0 * np.arange(8))
    with pytest.raises(ValueError):
        S.faces(prm, 8)
