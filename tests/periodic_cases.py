"""Constructed inputs for the periodic box of include/bdmi.h, shared by tests/test_periodic_host.py (which asserts that
each reaches the branch it is named for) and tests/test_gpu_boids_periodic.py.

As in tests/boids_cases.py every input is on a dyadic lattice (positions multiples of 2^-16, velocities of 2^-20) with
integer colours that name the boid, and the half box B is a multiple of the lattice step: L = 2 B, every image q +- L and
every difference p - q' is exact, so the alignment, cohesion and colour sums are exact in any order.
Each case is a dict {name, pos, vel, col, params, dt}.
"""
import numpy as np

import boids_cases as BC
import boids_ref as R
import periodic_ref as PR

NOTE_LIMIT = 2047  # the longest run k_flock's 16-bit notes address on a periodic grid (11 bits of offset)


def wrapped(pos, B):
    """Into [-B, B) by whole box lengths (exact on the lattice)."""
    return (np.asarray(pos, dtype=np.float64) + B) % (2 * B) - B


def _case(name, pos, prm, rng, vel=None):
    c = BC._case(name, pos, prm, rng, vel=vel)
    B = PR.box(prm)[0]
    assert np.all(np.abs(c["pos"]) <= B), name
    return c


def box_params(dim):
    """dim 3: the smallest box (bounds 7.5, perception 5); 4: bounds 10; 33: perception 1, bounds 16.5.  3^3 = 27 and
    33^3 = 35 937 are no multiples of 32, so rows of cells straddle the occupancy words; 4^3 = 64 fills exactly two."""
    if dim == 33:
        return BC.params(bounds=16.5, perception_radius=1.0, separation_radius=0.6)
    return BC.params(bounds=2.5 * dim, perception_radius=5.0)


def box(dim, seed=40):
    """Uniform boids, blobs on faces, edges and corners (wrapped into the box), and boids at exactly +-B."""
    rng = np.random.default_rng(seed + dim)
    prm = box_params(dim)
    B, L, d, cell = PR.box(prm)
    assert d == dim
    p = R.unpack(prm)["perception_radius"]
    n_uniform, n_blob = (1500, 160) if dim == 33 else (60 * dim, 20)
    pts = [rng.uniform(-B, B, (n_uniform, 3))]
    for centre in ([B, 0, 0], [0, -B, 0], [0.3, 0.2, B], [B, B, 0], [-B, 0.4, B], [0, B, -B], [B, B, B], [-B, B, -B],
                   [B - cell, -B, 0.1], [-B + cell, 0, B]):
        pts.append(wrapped(np.array(centre) + rng.normal(0, 0.45 * p, (n_blob, 3)), B))
    exact = rng.uniform(-B, B, (24, 3))
    for r in range(24):  # one, two or three coordinates exactly on a face, either sign
        for ax in range(r % 3 + 1):
            exact[r, (r + ax) % 3] = B if (r >> ax) & 1 else -B
    return _case(f"box_{dim}", np.concatenate(pts + [exact]), prm, rng)  # (rounding to the lattice may reach +B: legal)


def face_waves(seed=50):
    """In cell order, whole waves of 64 boids in x-face cells (two runs per row) and whole waves in interior cells (one).
    Cells (dim-1, cy, cz) and (0, cy+1, cz) are neighbours in the cell order: 200 boids in each make 400 consecutive
    face boids; the interior boids sit in rows without a face boid."""
    rng = np.random.default_rng(seed)
    prm = BC.params(bounds=20.0)  # dim 8, cell 5
    B = 20.0
    def cell(cx, cy, cz, n):
        return np.array([cx, cy, cz]) * 5.0 - B + rng.uniform(0.1, 4.9, (n, 3))
    pts = [cell(7, 2, 3, 200), cell(0, 3, 3, 200), cell(0, 2, 3, 30), cell(7, 3, 3, 30)]
    for cy in (5, 6):
        for cx in range(1, 7):
            pts.append(cell(cx, cy, 3, 40))
    return _case("face_waves", np.concatenate(pts), prm, rng)


def long_run(count, seed=60):
    """`count` boids in cell 0 of one row, 60 in the row's cell 1 and 60 in its cell dim-1: the boids of cell dim-1 have
    the run {0} of `count` boids THROUGH THE FACE, those of cells 0 and 1 have it in their run {0, 1} or {0, 1, 2}, and
    those of cell 0 the run {dim-1} through the face.  Tight clumps as in boids_cases.run_length, so the separation sums
    stay well conditioned."""
    rng = np.random.default_rng(seed + count)
    prm = BC.params(bounds=20.0)
    B = 20.0
    row = np.array([0.0, 15.0, 20.0]) - B  # cells (., 3, 4)
    pts = [BC._micro_clusters(rng, count, row + [0.0, 0, 0]), row + [5.0, 0, 0] + rng.uniform(0.2, 4.8, (60, 3)),
           row + [35.0, 0, 0] + rng.uniform(0.2, 4.8, (60, 3))]
    for dy in (-1, 1):  # sparse boids in the rows around, on both sides of the face
        for cx in (7, 0, 1, 2):
            pts.append(row + [5.0 * cx, 5.0 * dy, 0] + rng.uniform(0.2, 4.8, (8, 3)))
    return _case(f"long_run_{count}", np.concatenate(pts), prm, rng)


def sizes(n, seed=70):
    rng = np.random.default_rng(seed + n)
    prm = box_params(3)
    return _case(f"n_{n}", rng.uniform(-7.5, 7.5, (n, 3)), prm, rng)


def interior_cluster(seed=80, n=1500):
    """Everything further than one cell from every face of a large box: no image is shifted."""
    rng = np.random.default_rng(seed)
    prm = BC.params(bounds=30.0)  # dim 12, cell 5
    return _case("interior", rng.uniform(-12.0, 12.0, (n, 3)), prm, rng)


def trajectory(seed=11, n=2000):
    """About 20 metric neighbours per boid; fast enough for dozens of face crossings in ten steps."""
    rng = np.random.default_rng(seed)
    prm = BC.params(bounds=18.75)
    return _case("trajectory", rng.uniform(-18.75, 18.75, (n, 3)), prm, rng)


def gpu_cases():
    return [box(3), box(4), box(33), face_waves(), long_run(2100), long_run(4200)]


def wave_facts(pos, prm):
    """Per wave of 64 boids in cell order (a stable sort by cell of the id order): how many sit in an x-face cell."""
    f = PR.run_facts(pos, prm)
    order = np.argsort(PR.cell_index(pos, prm), kind="stable")
    face = f["face"][order]
    pad = (-len(face)) % 64
    lanes = np.concatenate([np.ones(len(face), dtype=bool), np.zeros(pad, dtype=bool)]).reshape(-1, 64).sum(axis=1)
    faces = np.concatenate([face, np.zeros(pad, dtype=bool)]).reshape(-1, 64).sum(axis=1)
    return dict(lanes=lanes, face=faces, longest=f["longest"])
