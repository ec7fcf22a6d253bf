"""Constructed slab-mode boids states (bdmi_create_slab / bdmi_slab_* in csrc/bdmi.hip, the ghost branch of
`k_flock`, boids/sharded.py), shared by the host tests (tests/test_slab_cases_host.py) and the GPU tests
(tests/test_gpu_boids_slab.py).  Conventions of tests/boids_cases.py: positions on the 2^-16 lattice, velocities on
2^-20, integer id colours, params(bounds=30): cell 5, grid dimension 14, offset 35, so every cell plane, and with
it every slab face, is an integer and a lattice value.

A case is a dict {name, pos, vel, col, params, dt, world} (tile_edges: one slab, see there).  The colours are
boids_ref.id_colours, scaled into [0, 1) for the cases that run 25 steps against the CPU oracle (see _case).

Layout of the face cases.  Boids sit in `slots`: columns along x at (y0, z0) on a 6-spaced square lattice, with
offsets of at most 1.5 in y and z.  Two boids of different slots are at least 3 = the separation radius apart in y
or z, so they never give a separation term.  Faces 10 apart (world 7) take the two colours of the slots'
checkerboard, so the boids at f + 5 of one face and at f' - 5 of the next never meet.  Inside a slot every pair is
more than 3 apart unless the case says otherwise (faces_sep).
"""
import numpy as np

import boids_cases as BC
import boids_ref as R
import slab_ref as S

PB, VB = BC.PB, BC.VB
H = 2.0 ** -PB
CELL = 5.0
DT = BC.DT


def params(**over):
    return BC.params(bounds=30.0, **over)


def _case(name, pos, vel, world, prm=None, dt=DT, unit_colours=False, pos_bits=PB):
    """unit_colours: the id colours times 2^-20 (an exact scaling: the sums stay exact in any order), which lie in
    [0, 1) like the colours of a real flock.  For the cases that run many steps against the CPU oracle under the
    ABSOLUTE colour bound 1e-10 of test_flock_vs_reference: that bound was made for colours in [0, 1], and is below
    one unit in the last place of an id colour near 2^20 (1.2e-10)."""
    pos = R.lattice(np.asarray(pos, dtype=np.float64), pos_bits)
    vel = R.lattice(np.asarray(vel, dtype=np.float64), VB)
    assert len(pos) == len(vel)
    col = R.id_colours(len(pos)) * (2.0 ** -20 if unit_colours else 1.0)
    return dict(name=name, pos=pos, vel=vel, col=col, params=params() if prm is None else prm, dt=dt, world=world)


# ---- the face layout -------------------------------------------------------------------------------------------
# groups of (dx from the face, dy, dz); each goes to a slot of its own
_EDGE_GROUPS = [
    [(0, 0, 0), (-3.5, 0, 0)],                     # on the face: owned by the right slab, its neighbour by the left
    [(-H, 0, 0), (3.5, 0, 0)],
    [(H, 0, 0), (-3.5, 0, 0)],
    [(5, 0, 0), (1.5, 0, 0), (-2, 0, 0)],          # f + cell: the first x outside the left-going halo
    [(-5, 0, 0), (-1.5, 0, 0), (2, 0, 0)],         # f - cell: the first x inside the right-going halo
    [(5 - H, 0, 0), (1.25, 0, 0), (-2.5, 0, 0)],
    [(5 + H, 0, 0), (1.5, 0, 0), (-2, 0, 0)],
    [(-5 - H, 0, 0), (-1.5, 0, 0), (2, 0, 0)],
    [(-5 + H, 0, 0), (-1.25, 0, 0), (2.5, 0, 0)],
    [(-2.5, 0, 0), (2.5 - H, 0, 0)],               # |dx| = p - h across the face: neighbours only a ghost supplies
    [(-H, 0, 0), (5 - 2 * H, 0, 0)],               # the same with one boid hard at the face, the other at the halo's end
    [(-5 + H, 0, 0), (0, 0, 0)],
    [(-2.5, 0, 0), (2.5, 0, 0)],                   # exactly p: excluded
    [(-2, -1.5, 0), (2, 1.5, 0)],                  # exactly p from two components (16 + 9)
    [(-5, 0, 0), (0, 0, 0)],                       # exactly p, halo's first x to the face
]
# Between two lattice values (x on the 2^-20 lattice, still exact in every sum): the only neighbours that need the
# halo's LAST lattice step.  On the lattice alone a row at f + 5 - h has no neighbour left of the face (|dx| >= 5),
# so a halo one step too narrow would give the same step; a boid at f - h / 16 does see it, and likewise on the
# other side.  (A halo one step too WIDE, or `>` for `>=` at x = f - 5, sends or drops rows that are exactly p or
# more from every boid beyond the face: no step can tell, only the exported sets can.)
_SUB_GROUPS = [
    [(5 - H, 0, 0), (-H / 16, 0, 0)],
    [(-5 + H / 16, 0, 0), (0, 0, 0)],
]
# diagonal across the face: placed in a slot whose y and z offsets cross a cell border (see _slots)
_DIAGONAL = [(-1.5, -1.25, -1.25), (1.5, 1.25, 1.25)]
# pairs across the face inside the separation radius (faces_sep)
_SEP_GROUPS = [
    [(-1, 0, 0), (1, 0, 0)],
    [(-H, 0, 0), (H, 1, 0)],
    [(-0.5, -1, 0.5), (0, 1, 0)],
    [(-2.75, 0, 0), (-H, 0, 0), (2.5, 0, 0)],
    [(0, 0, 0), (-0.125, 0, 0)],                   # dist^2 = 2^-6 > 1e-4: a large separation term across the face
]


def _slots(colour):
    """(diagonal slot, the other slots) of one checkerboard colour: (y0, z0) = -27 + 6 (iy, iz).  The diagonal slot
    is (9, 9) or (9, 15): offsets of +-1.25 there cross the cell borders y = 10 and z = 10 or 15."""
    diag = (6, 6) if colour == 0 else (6, 7)
    rest = [(iy, iz) for iy in range(10) for iz in range(10) if (iy + iz) % 2 == colour and (iy, iz) != diag]
    at = lambda s: np.array([0.0, -27.0 + 6 * s[0], -27.0 + 6 * s[1]])  # noqa: E731
    return at(diag), [at(s) for s in rest]


def _chain():
    """Across the two-cell slab [f, f + 10): a boid of the left slab, three of this one, one of the right slab, each
    the neighbour of the next.  (A single boid of a two-cell slab with neighbours in BOTH adjacent slabs cannot
    exist: they would be x_r - x_l > 10 = 2 p apart in x, and each less than p from it.  What exists is a slab
    whose boids need ghosts from both sides in the same step, and a boid, the middle one, both of whose
    neighbours are halo rows going out in opposite directions.)"""
    return [(-2.25, 0, 0), (1.5, 0, 0), (5, 0, 0), (8.5, 0, 0), (12.25, 0, 0)]


def _face_layout(world, sep, seed):
    rng = np.random.default_rng(seed)
    prm = params()
    face = S.faces(prm, world)
    pos = []
    for k, f in enumerate(face[1:-1]):
        diag, rest = _slots(k % 2)
        groups = list(_EDGE_GROUPS) + _SUB_GROUPS + (list(_SEP_GROUPS) if sep else [])
        if k + 2 < len(face) and face[k + 2] - f == 2 * CELL:
            groups.append(_chain())
        pos.append(diag + np.array(_DIAGONAL) + [f, 0, 0])
        for g, at in zip(groups, rest):
            pos.append(at + np.array(g, dtype=np.float64) + [f, 0, 0])
        for at in rest[len(groups):]:  # filler: three boids along x, at least 3 apart, on both sides of the face
            u = rng.integers(0, 1 << PB, 3) / float(1 << PB)
            x = np.array([-4.5 + 0.75 * u[0], -0.75 + 1.5 * u[1], 3.75 + 0.75 * u[2]])
            yz = rng.integers(-(1 << PB), (1 << PB) + 1, (3, 2)) / float(1 << PB)  # within 1 of the slot's axis
            pos.append(at + np.concatenate([R.lattice(x[:, None], PB) + f, yz], axis=1))
    pos = np.concatenate(pos)
    vel = rng.uniform(-12.5, 12.5, pos.shape)
    return _case(f"faces{'_sep' if sep else ''}_{world}", pos, vel, world, prm, pos_bits=20)


def faces(world):
    return _face_layout(world, False, 10 + world)


def faces_sep(world):
    return _face_layout(world, True, 20 + world)


# ---- outside the grid --------------------------------------------------------------------------------------------
def outside(seed=30):
    """World 3 (faces -10 and 10).  Boids beyond the grid's x range on both ends (cells clamped; owned by the open
    end slabs) with boids of the border cells next to them, and boids beyond the grid in y and in z around both
    interior faces (clamped cells on both sides of a face)."""
    rng = np.random.default_rng(seed)
    u = lambda lo, hi, n: rng.uniform(lo, hi, n)  # noqa: E731
    parts = []
    for s in (-1.0, 1.0):
        parts.append(np.stack([s * u(35, 60, 120), u(-34, 34, 120), u(-34, 34, 120)], axis=1))  # beyond the x end
        parts.append(np.stack([s * u(29, 36, 120), u(-34, 34, 120), u(-34, 34, 120)], axis=1))  # around the grid's edge
        for f in (-10.0, 10.0):
            parts.append(np.stack([f + u(-6, 6, 80), s * u(33, 50, 80), u(-12, 12, 80)], axis=1))  # beyond in y
            parts.append(np.stack([f + u(-6, 6, 80), u(-12, 12, 80), s * u(33, 50, 80)], axis=1))  # beyond in z
    pos = np.concatenate(parts)
    return _case("outside", pos, rng.uniform(-12.5, 12.5, pos.shape), 3)


# ---- slabs without boids ------------------------------------------------------------------------------------------
def empty_slab(seed=31):
    """World 3 with the middle slab [-10, 10) empty at creation (n = 0, ids = NULL).  Boids one lattice step left of
    its left face move right at vx = 12 (0.2 per step): after the first step they lie inside it, and the second
    exchange hands them over, so the slab is populated by import only.  Boids at its right face (x = 10, owned by
    the right slab) move left likewise.  The rest: random boids of the two end slabs, none inside [-10, 10)."""
    rng = np.random.default_rng(seed)
    m = 40
    yz = np.stack([-27.0 + 6 * (np.arange(m) % 10), -27.0 + 6 * (np.arange(m) // 10)], axis=1)
    a = np.concatenate([np.full((m, 1), -10.0 - H), yz], axis=1)
    b = np.concatenate([np.full((m, 1), 10.0), yz + 3.0], axis=1)
    va = np.tile([12.0, 0.0, 0.0], (m, 1))
    n = 150
    left = np.stack([rng.uniform(-30, -10.5, n), rng.uniform(-28, 28, n), rng.uniform(-28, 28, n)], axis=1)
    right = np.stack([rng.uniform(10.5, 30, n), rng.uniform(-28, 28, n), rng.uniform(-28, 28, n)], axis=1)
    pos = np.concatenate([a, b, left, right])
    vel = np.concatenate([va, -va, rng.uniform(-12.5, 12.5, (2 * n, 3))])
    return _case("empty_slab", pos, vel, 3)


def draining_slab(seed=32):
    """World 3.  Every boid of the middle slab lies within 0.75 of one of its faces and heads out through it at
    20 to 24 (a third of a unit and more per step), with the boids of the end slabs near that face heading the
    same way, so alignment and cohesion do not turn it round: the slab is empty within a few steps (owned == 0
    in export, a ghost-only handle in bdmi_step).  Boids of the end slabs far from the faces are random."""
    rng = np.random.default_rng(seed)
    parts, vels = [], []
    for s in (-1.0, 1.0):
        for lo, hi, n in ((9.25, 10.0, 150), (10.0, 16.0, 400)):
            x = s * rng.uniform(lo, hi, n) - (H if s > 0 else 0.0)  # the right group stays below the face x = 10
            parts.append(np.stack([x, rng.uniform(-26, 26, n), rng.uniform(-26, 26, n)], axis=1))
            vels.append(np.stack([s * rng.uniform(20, 24, n), rng.uniform(-2, 2, n), rng.uniform(-2, 2, n)], axis=1))
        n = 300
        parts.append(np.stack([s * rng.uniform(17, 30, n), rng.uniform(-28, 28, n), rng.uniform(-28, 28, n)], axis=1))
        vels.append(rng.uniform(-12.5, 12.5, (n, 3)))
    return _case("draining_slab", np.concatenate(parts), np.concatenate(vels), 3, unit_colours=True)


# ---- scan tiles of the export's compactions -----------------------------------------------------------------------
TILE = 2048  # scan::kTile (csrc/scan.h)
TILE_SLAB = (-10.0, 5.0)  # one slab of three cells with a neighbour on both sides


def tile_edges(n, where, seed=33):
    """One slab handle [-10, 5) of `n` owned rows in creation order = row order.  Rows not selected lie in
    [-5, 0); the selected rows lie, alternating, in the left halo zone [-10, -5) and the right one [0, 5), a
    quarter of them beyond the face they go through (exported and demoted); `where`: "last" = only rows of
    the last scan tile are selected, "first" = only rows of the first, "all" = every row."""
    rng = np.random.default_rng(seed + n)
    lat = lambda lo, hi, k: lo + rng.integers(0, int((hi - lo) * (1 << PB)), k) / float(1 << PB)  # noqa: E731
    rows = np.arange(n)
    last0 = (n - 1) // TILE * TILE
    sel = {"last": rows >= last0, "first": rows < TILE, "all": np.ones(n, dtype=bool)}[where]
    x = lat(-5.0, 0.0, n)
    k = np.flatnonzero(sel)
    side = np.arange(len(k)) % 2
    out = np.arange(len(k)) % 8 >= 6
    xl = np.where(out, lat(-14.0, -10.0, len(k)), lat(-10.0, -5.0, len(k)))
    xr = np.where(out, lat(5.0, 9.0, len(k)), lat(0.0, 5.0, len(k)))
    x[k] = np.where(side == 0, xl, xr)
    # the exact edges, on selected rows: -5 - h and 0 are selected, -10 and 5 - h stay owned, -10 - h and 5 do not
    edge = [-5.0 - H, 0.0, -10.0, 5.0 - H, -10.0 - H, 5.0]
    x[k[:len(edge)]] = edge[:len(k)]
    x[np.flatnonzero(~sel)[:2]] = [-5.0, -H][:min(2, int((~sel).sum()))]  # and the first x not selected on either side
    pos = np.stack([x, lat(-30.0, 30.0, n), lat(-30.0, 30.0, n)], axis=1)
    c = _case(f"tile_edges_{n}_{where}", pos, rng.uniform(-12.5, 12.5, pos.shape), 1)
    c["slab"] = TILE_SLAB
    c["selected"] = sel
    return c


# ---- migration ----------------------------------------------------------------------------------------------------
def migration(world, seed=34, n=4000):
    """Random lattice boids over the whole box, |vx| between 8 and 20 with a random sign: in 25 steps of 1/60 a boid
    travels 3 to 8 units in x, and boids cross every face in both directions."""
    rng = np.random.default_rng(seed + world)
    pos = rng.uniform(-30, 30, (n, 3))
    vel = rng.uniform(-12.5, 12.5, (n, 3))
    vel[:, 0] = rng.choice([-1.0, 1.0], n) * rng.uniform(8, 20, n)
    return _case(f"migration_{world}", pos, vel, world, unit_colours=True)


# ---- the longest step a slab handle takes -----------------------------------------------------------------------------
LONG_DT = 25.0 / 64.0        # 25 * 25 / 64 = 9.765625 < 10 = two cells; the next multiple of 1 / 64 gives 10.15625
TOO_LONG_DT = 26.0 / 64.0


def long_step(dt=LONG_DT, seed=35):
    """World 7 (seven two-cell slabs), max_speed 25.  At every interior face f: boids at f - h heading right and
    boids at f (owned by the right slab) heading left, at exactly max_speed along x, in slots of their own (no
    neighbours, and |y|, |z| <= 27 - the wall margin's inner edge -, so nothing turns them: each lands
    max_speed * dt = 9.765625 further, h short of the adjacent slab's far face or just inside it); plus random
    boids that do have neighbours."""
    rng = np.random.default_rng(seed)
    prm = params()
    face = S.faces(prm, 7)
    pos, vel = [], []
    for k, f in enumerate(face[1:-1]):
        _, rest = _slots(k % 2)
        for j, at in enumerate(rest[:24]):
            right = j % 2 == 0
            pos.append(at + [f - H if right else f, 0, 0])
            vel.append([25.0 if right else -25.0, 0.0, 0.0])
    pos, vel = np.array(pos), np.array(vel)
    m = 600
    # the random boids stay at y >= 6, more than the perception radius from the slots used above (y0 <= -3)
    rp = np.stack([rng.uniform(-34, 34, m), rng.uniform(6, 27, m), rng.uniform(-27, 27, m)], axis=1)
    rv = rng.uniform(-12.5, 12.5, (m, 3))
    return _case("long_step", np.concatenate([pos, rp]), np.concatenate([vel, rv]), 7, prm, dt=dt)


def face_cases():
    return [faces(w) for w in (2, 3, 7)] + [faces_sep(w) for w in (2, 3, 7)]


TILE_NAMES = [(n, w) for n in (2047, 2048, 2049, 4097) for w in ("last", "first", "all")]
