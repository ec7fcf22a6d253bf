"""Constructed boids inputs at the edges of the sweep kernel (csrc/bdmi.hip `k_flock`), shared by
the host tests (tests/test_boids_ref_host.py) and the GPU tests (tests/test_gpu_boids_sweep.py).

Every input is on a dyadic lattice (positions multiples of 2^-16, velocities of 2^-20) with integer
colours that encode the boid's id (boids_ref.id_colours), so the alignment, cohesion and colour
sums are exact in any order: those outputs must match bit for bit wherever the neighbour sets agree.

Each case is a dict {name, pos, vel, col, params, dt}.  `grid_facts` restates the kernel's cell rule
in NumPy so that the host tests can assert that a case reaches the branch it is named for.
"""
import numpy as np

import boids_ref as R

PB, VB = 16, 20  # lattice bits of positions and velocities
DT = 1.0 / 60.0
_DEFAULT = dict(bounds=500.0, wall_margin=3.0, wall_weight=10.0, max_speed=25.0, max_force=60.0,
                perception_radius=5.0, separation_radius=3.0, separation_weight=2.5, alignment_weight=1.0,
                cohesion_weight=1.0, color_blend_rate=1.0)


def params(**over):
    d = dict(_DEFAULT)
    d.update(over)
    return np.array([d[k] for k in R._KEYS], dtype=np.float64)


def _case(name, pos, prm, rng, dt=DT, vel=None):
    pos = R.lattice(pos, PB)
    if vel is None:
        vel = rng.uniform(-12.5, 12.5, pos.shape)
    return dict(name=name, pos=pos, vel=R.lattice(vel, VB), col=R.id_colours(len(pos)), params=prm, dt=dt)


def cell_low(c, prm):
    """Lowest coordinate of cell coordinate c (a lattice value for the grids used here)."""
    cell, _, offset = R.grid(prm)
    return c * cell - offset


def _micro_clusters(rng, n, corner, k=3):
    """n boids in k tight clumps inside the cell whose lowest corner is `corner`: every clump has a
    radius below 0.004, so pairs inside one clump are closer than 0.01 (not neighbours, dist^2 <=
    1e-4), while the clumps are 1.5 - 2.5 apart (neighbours and separation terms in few directions:
    a well-conditioned separation sum however many terms it has)."""
    centres = np.array([[0.5, 0.5, 0.5], [2.0, 0.7, 0.6], [0.8, 2.2, 1.9]])[:k]
    which = np.arange(n) % k
    jit = rng.integers(-(1 << 7), (1 << 7) + 1, (n, 3)) / float(1 << PB)
    return corner + centres[which] + jit


# ---- 1 / 2: run lengths and the `big` fallback --------------------------------------------------------
def run_length(count, seed=0):
    """`count` boids in one cell (its row's other two cells empty), plus boids in the cells of the
    neighbouring rows, whose own row runs then include the crowded cell."""
    rng = np.random.default_rng(seed)
    prm = params(bounds=20.0)
    corner = np.array([cell_low(4, prm)] * 3)
    blob = _micro_clusters(rng, count, corner)
    around = []
    for dy in (-1, 1):
        for dz in (-1, 0, 1):
            for dx in (-1, 0, 1):
                around.append(corner + np.array([dx, dy, dz]) * 5.0 + rng.uniform(0.2, 4.8, (6, 3)))
    return _case(f"run_length_{count}", np.concatenate([blob] + around), prm, rng)


def mixed_lanes(seed=1):
    """8 200 boids in one cell amid 24 sparse boids per cell around it: in cell order, wavefronts
    hold lanes whose rows contain the crowded cell (`big`) next to lanes whose rows do not."""
    rng = np.random.default_rng(seed)
    prm = params(bounds=30.0)
    corner = np.array([cell_low(6, prm)] * 3)
    blob = _micro_clusters(rng, 8200, corner)
    near = corner - 10.0 + rng.uniform(0, 25.0, (3000, 3))
    near = near[~np.all((near >= corner) & (near < corner + 5.0), axis=1)]
    far = rng.uniform(-30, 30, (3000, 3))
    return _case("mixed_lanes", np.concatenate([blob, near, far]), prm, rng)


# ---- 3: the per-lane hit list ------------------------------------------------------------------------
def hit_list(seed=2, kmax=80, reps=2):
    """Isolated clusters of k + 1 boids, k = 0 .. kmax: all pairs of a cluster closer than 4.4 and
    further than 0.05 apart, clusters 12 apart, so every boid of a cluster has exactly k neighbours
    (flush threshold 28, list capacity 32, repeated flushes, every run length mod 4)."""
    rng = np.random.default_rng(seed)
    prm = params(bounds=80.0)
    pts = []
    slots = [(x, y, z) for z in range(13) for y in range(13) for x in range(13)]
    rng.shuffle(slots)
    s = 0
    for _ in range(reps):
        for k in range(kmax + 1):
            centre = -72.0 + 12.0 * np.array(slots[s], dtype=np.float64) + rng.uniform(0, 5.0, 3)
            s += 1
            while True:
                d = rng.normal(size=(k + 1, 3))
                d *= (2.15 * rng.uniform(0, 1, (k + 1, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
                c = R.lattice(centre + d, PB)
                dd = np.linalg.norm(c[:, None] - c[None], axis=2) + np.eye(k + 1)
                if dd.min() > 0.05:
                    break
            pts.append(c)
    return _case("hit_list", np.concatenate(pts), prm, rng)


# ---- 4: distance thresholds --------------------------------------------------------------------------
def thresholds(seed=3):
    """Pairs at exactly the perception distance (excluded), exactly the separation distance
    (a neighbour, no separation term), just inside each, coincident boids, and dist^2 = 2^-13 / 2^-14
    on either side of the 1e-4 floor; each group isolated, some across cell borders."""
    rng = np.random.default_rng(seed)
    prm = params(bounds=100.0)
    h = 2.0 ** -PB
    groups = [
        [[0, 0, 0], [5, 0, 0]],            # dist^2 = 25 = perception^2: excluded
        [[0, 0, 0], [0, 3, 4]],            # 25 again, from two components
        [[0, 0, 0], [5 - h, 0, 0]],        # just inside
        [[0, 0, 0], [0, 0, 3]],            # dist^2 = 9 = separation^2: neighbour, no separation
        [[0, 0, 0], [3 - h, 0, 0]],        # just inside the separation radius
        [[0, 0, 0], [0, 0, 0]],            # coincident
        [[0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 1, 1]],
        [[0, 0, 0], [2 ** -7, 2 ** -7, 0]],  # dist^2 = 2^-13 > 1e-4: neighbour (|t| = 90.5)
        [[0, 0, 0], [0, 2 ** -7, 0]],      # dist^2 = 2^-14 < 1e-4: excluded
        [[0, 0, 0], [2 ** -7, 2 ** -7, 0], [0, 2 ** -7, 0], [4, 0, 0]],
    ]
    pts = []
    base_cells = [(x, y, z) for z in range(2, 40, 4) for y in range(2, 40, 4) for x in range(2, 40, 4)]
    rng.shuffle(base_cells)
    b = 0
    for g in groups:
        for off in ([0, 0, 0], [4.5, 2.25, 1], [5 - h, 0, 0], [0, 5, 0], [0, 0, 5], [2.5, 2.5, 2.5]):
            corner = np.array([cell_low(c, prm) for c in base_cells[b]])
            b += 1
            pts.append(corner + np.array(off, dtype=np.float64) + np.array(g, dtype=np.float64))
            # and mirrored, so that the pair also crosses borders in the other direction
            corner = np.array([cell_low(c, prm) for c in base_cells[b]])
            b += 1
            pts.append(corner + 5.0 - np.array(off, dtype=np.float64) - np.array(g, dtype=np.float64))
    return _case("thresholds", np.concatenate(pts), prm, rng)


# ---- 5: grid dimensions ------------------------------------------------------------------------------
def grid_dims(dim, seed=4, interior=4000, outside=300):
    """Perception 1, bounds (dim - 2) / 2: a grid of `dim` cells per side.  One boid in every border
    cell, random boids inside, and boids far outside the grid on every side (clamped)."""
    rng = np.random.default_rng(seed + dim)
    b = (dim - 2) / 2.0
    prm = params(bounds=b, perception_radius=1.0, separation_radius=0.6, wall_margin=min(3.0, b / 2 + 0.25))
    c = np.stack(np.meshgrid(*[np.arange(dim)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    border = c[np.any((c == 0) | (c == dim - 1), axis=1)]
    pos = [cell_low(border, prm) + rng.uniform(0, 0.999, border.shape)]
    pos.append(rng.uniform(-b - 1, b + 1, (interior, 3)))
    far = rng.uniform(-b - 1, b + 1, (outside, 3))
    ax = rng.integers(0, 3, outside)
    far[np.arange(outside), ax] = rng.choice([-1.0, 1.0], outside) * rng.uniform(b + 1, 3 * b + 40, outside)
    pos.append(far)
    return _case(f"grid_{dim}", np.concatenate(pos), prm, rng)


def largest_grid(seed=5):
    """Perception 1, bounds 644: dimension 1290, the largest allowed (dim^3 < 2^31).  Boids near the
    far corner (cell ids near 2^31), beyond it (clamped), and a few near the near corner."""
    rng = np.random.default_rng(seed)
    prm = params(bounds=644.0, perception_radius=1.0, separation_radius=0.6)
    corner = rng.uniform(638.0, 652.0, (6000, 3))
    low = rng.uniform(-652.0, -638.0, (500, 3))
    mid = rng.uniform(-644.0, 644.0, (500, 3))
    return _case("grid_1290", np.concatenate([corner, low, mid]), prm, rng)


# ---- 6: parameters -----------------------------------------------------------------------------------
def _clumpy(rng, n, bounds, sigma):
    centres = rng.uniform(-0.8 * bounds, 0.8 * bounds, (max(n // 400, 1), 3))
    return centres[rng.integers(0, len(centres), n)] + rng.normal(0, sigma, (n, 3))


def parameter_cases(seed=6):
    rng = np.random.default_rng(seed)
    out = []
    for name, over, sigma, dt in (
            ("perception_2.5", dict(perception_radius=2.5, separation_radius=1.5), 2.0, DT),
            ("perception_7.25", dict(perception_radius=7.25, separation_radius=4.0), 4.0, DT),
            ("separation_above_perception", dict(separation_radius=6.0), 3.0, DT),
            ("max_force_clamps", dict(max_force=1e-3), 3.0, DT),
            ("zero_weights", dict(separation_weight=0.0, alignment_weight=0.0, cohesion_weight=0.0), 3.0, DT),
            ("blend_saturates", dict(color_blend_rate=120.0), 3.0, DT)):
        prm = params(bounds=40.0, **over)
        out.append(_case(name, _clumpy(rng, 8000, 40.0, sigma), prm, rng, dt=dt))
    return out


def host_cases():
    """Every case that fits the oracle's dense cell tables (all but the 1290 grid)."""
    cs = [run_length(c) for c in (4094, 4095, 4096, 4097)]
    cs += [mixed_lanes(), hit_list(), thresholds()]
    cs += [grid_dims(d) for d in (3, 4, 31, 32, 33, 34, 63, 64, 65)]
    cs += parameter_cases()
    return cs


# ---- the kernel's cell rule, restated ----------------------------------------------------------------
def grid_facts(pos, prm):
    """Per boid, as k_flock sees its nine rows of three cells: the run length of each row (n, 9),
    whether a row's run exceeds 4095 (`big`), the candidate count, and whether some row spans two
    32-cell occupancy words with boids in both; plus the cell-sorted order (a stable sort by cell of
    the id order, the kernel's order on a fresh handle)."""
    _, dim, _ = R.grid(prm)
    cc = R.cell_coords(pos, prm)
    ids = cc[:, 0] + cc[:, 1] * dim + cc[:, 2] * dim * dim
    keys = np.sort(ids)
    x_lo = np.maximum(cc[:, 0] - 1, 0)
    x_hi = np.minimum(cc[:, 0] + 1, dim - 1)
    runs = np.zeros((len(pos), 9), dtype=np.int64)
    straddle = np.zeros(len(pos), dtype=bool)
    k = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            ny, nz = cc[:, 1] + dy, cc[:, 2] + dz
            ok = (ny >= 0) & (ny < dim) & (nz >= 0) & (nz < dim)
            row = ny * dim + nz * dim * dim
            lo, hi = row + x_lo, row + x_hi
            cnt = np.searchsorted(keys, hi, "right") - np.searchsorted(keys, lo, "left")
            runs[:, k] = np.where(ok, cnt, 0)
            two = (lo >> 5) != (hi >> 5)
            a = np.searchsorted(keys, lo | 31, "right") - np.searchsorted(keys, lo, "left")
            b = np.searchsorted(keys, hi, "right") - np.searchsorted(keys, hi & ~31, "left")
            straddle |= ok & two & (a > 0) & (b > 0)
            k += 1
    order = np.argsort(ids, kind="stable")
    return dict(cells=ids, runs=runs, big=(runs > 4095).any(axis=1), candidates=runs.sum(axis=1),
                straddle=straddle, order=order)
