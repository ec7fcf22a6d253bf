"""Plain NumPy restatement of the slab protocol of include/bdmi.h (bdmi_slab_export / bdmi_slab_import /
bdmi_step on a slab handle), with nothing from the library: no cell grid, no boids.sharded.
TEST INFRASTRUCTURE ONLY.

    faces()        the slab faces: Flock.__init__'s grid split into `world` runs of whole cell planes
    export_sets()  which owned rows go to the left neighbour, to the right neighbour, and are demoted
    SlabModel      `world` row sets of owned and ghost rows; exchange() = export, routing, import;
                   step() = boids_ref.flocking of the owned rows over owned + ghost rows, then physics

The model may lose a boid exactly as the library would (a boid that no rank owns after an exchange):
`owners()` reports what is there, it does not repair it.
"""
import numpy as np

import boids_ref as R

ROW = 10  # position, velocity, colour, global id


def planes(dim, world):
    """Rank r owns the cell planes [b[r], b[r + 1]); every slab at least two planes wide."""
    b = [round(r * dim / world) for r in range(world + 1)]
    if any(b[r + 1] - b[r] < 2 for r in range(world)):
        raise ValueError(f"{world} slabs of {dim} planes: a slab narrower than two cells")
    return b


def faces(params, world):
    """The world + 1 face coordinates, faces[r] <= x < faces[r + 1] being rank r's slab (the outer side
    of the two end slabs is open)."""
    cell, dim, offset = R.grid(params)
    return np.array([b * cell - offset for b in planes(dim, world)], dtype=np.float64)


def export_sets(x, owned, x_lo, x_hi, cell, has_left, has_right):
    """Masks over the rows: (to the left neighbour, to the right neighbour, demoted to a ghost)."""
    x = np.asarray(x, dtype=np.float64)
    owned = np.asarray(owned, dtype=bool)
    left = owned & (x < x_lo + cell) if has_left else np.zeros(len(x), dtype=bool)
    right = owned & (x >= x_hi - cell) if has_right else np.zeros(len(x), dtype=bool)
    lo = x_lo if has_left else -np.inf
    hi = x_hi if has_right else np.inf
    return left, right, owned & ~((x >= lo) & (x < hi))


def rows_of(pos, vel, col, ids):
    return np.concatenate([pos, vel, col, np.asarray(ids, dtype=np.float64)[:, None]], axis=1)


class SlabModel:
    def __init__(self, pos, vel, col, params, world, face=None):
        self.params = np.asarray(params, dtype=np.float64)
        self.world = world
        self.cell = R.grid(self.params)[0]
        self.face = faces(self.params, world) if face is None else np.asarray(face, dtype=np.float64)
        pos = np.asarray(pos, dtype=np.float64)
        self.rows, self.ghost = [], []
        for r in range(world):
            lo = -np.inf if r == 0 else self.face[r]
            hi = np.inf if r == world - 1 else self.face[r + 1]
            own = np.flatnonzero((pos[:, 0] >= lo) & (pos[:, 0] < hi))
            self.rows.append(rows_of(pos[own], np.asarray(vel)[own], np.asarray(col)[own], own))
            self.ghost.append(np.zeros(len(own), dtype=bool))

    def exchange(self):
        """Export on every rank, the rows to the neighbours, import.  Returns per rank the ids sent
        (left, right)."""
        w = self.world
        out, sent = [[] for _ in range(w)], []
        for r in range(w):
            rows = self.rows[r][~self.ghost[r]]  # last step's ghosts are gone
            left, right, dem = export_sets(rows[:, 0], np.ones(len(rows), dtype=bool), self.face[r], self.face[r + 1],
                                           self.cell, r > 0, r < w - 1)
            if r > 0:
                out[r - 1].append(rows[left])
            if r < w - 1:
                out[r + 1].append(rows[right])
            sent.append((rows[left, 9].astype(np.int64), rows[right, 9].astype(np.int64)))
            self.rows[r], self.ghost[r] = rows, dem
        for r in range(w):
            got = np.concatenate(out[r]) if out[r] else np.zeros((0, ROW))
            lo = -np.inf if r == 0 else self.face[r]
            hi = np.inf if r == w - 1 else self.face[r + 1]
            self.rows[r] = np.concatenate([self.rows[r], got])
            self.ghost[r] = np.concatenate([self.ghost[r], ~((got[:, 0] >= lo) & (got[:, 0] < hi))])
        return sent

    def step(self, dt):
        """Flock.update for the owned rows of every rank; the ghosts only take part as neighbours."""
        for r in range(self.world):
            rows, own = self.rows[r], np.flatnonzero(~self.ghost[r])
            if len(own) == 0:
                continue
            p, v, c = rows[:, 0:3], rows[:, 3:6], rows[:, 6:9]
            F = R.flocking(p, v, c, self.params, query=own)
            np_, nv, nc = R.physics(p[own], v[own], c[own], (F.sep, F.ali, F.coh, F.avg), self.params, dt)
            rows = rows.copy()
            rows[own, 0:3], rows[own, 3:6], rows[own, 6:9] = np_, nv, nc
            self.rows[r] = rows

    def owned(self, r):
        return self.rows[r][~self.ghost[r]]

    def owners(self):
        """Per rank the ids it owns."""
        return [self.owned(r)[:, 9].astype(np.int64) for r in range(self.world)]

    def gather(self, n):
        """(pos, vel, col) in id order; asserts that the owners partition range(n)."""
        full = np.concatenate([self.owned(r) for r in range(self.world)])
        assert_partition([self.owners()[r] for r in range(self.world)], n)
        out = np.empty((n, 9))
        out[full[:, 9].astype(np.int64)] = full[:, :9]
        return out[:, 0:3], out[:, 3:6], out[:, 6:9]


def assert_partition(owners, n):
    ids = np.concatenate(owners) if len(owners) else np.zeros(0, dtype=np.int64)
    assert len(ids) == n and np.array_equal(np.sort(ids), np.arange(n)), \
        ("the owners do not partition the ids", len(ids), n, len(np.unique(ids)))


def owner_of(x, face):
    """The rank whose slab contains x (the end slabs are open outwards)."""
    return np.clip(np.searchsorted(np.asarray(face)[1:-1], x, side="right"), 0, len(face) - 2)
