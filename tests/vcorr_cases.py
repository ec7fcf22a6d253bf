"""Inputs for bdmi_velocity_correlation (include/bdmi.h), shared by tests/test_vcorr_host.py (which checks the
restatement on them and that the candidate mask cuts nothing where it should not) and tests/test_gpu_boids_vcorr.py.

Like tests/boids_cases.py every input is on the dyadic lattice (positions multiples of 2^-16, velocities of 2^-20) unless
a case says otherwise.  Each case is a dict {name, pos, vel, col, params, periodic}; edges are chosen by the tests.
"""
import numpy as np

import boids_cases as BC
import boids_ref as R
import periodic_cases as PC
import torus_cases as TC

WALLED = BC.params(bounds=12.5, perception_radius=5.0)  # dim 7, cell 5, the grid covers [-17.5, 17.5]


def _case(name, pos, prm, seed, periodic=False, vel=None):
    make = PC._case if periodic else BC._case
    c = make(name, np.asarray(pos, dtype=np.float64).reshape(-1, 3), prm, np.random.default_rng(seed), vel=vel)
    c["periodic"] = periodic
    return c


def uniform(n, seed=100):
    """n boids uniform in the box of bounds 12.5, every 16th up to two cells outside it (beyond the grid: clamped)."""
    rng = np.random.default_rng(seed + n)
    pos = rng.uniform(-12.5, 12.5, (n, 3))
    out = np.arange(n) % 16 == 5
    pos[out] = rng.uniform(-22.5, 22.5, (int(out.sum()), 3))
    return _case(f"uniform_{n}", pos, WALLED, seed + n)


WHOLE_GRID = 80.0  # 45 sqrt(3) < 80 = 16 cells: reaches every pair of uniform()


def edge_sets(seed, count=20, max_last=15.0):
    """`count` edge sets with 1 - 64 bins (both ends included), linear and logarithmic, with and without a zero first
    edge, the last edge in (1, max_last]."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        nb = (1, 64, 2, 63)[k] if k < 4 else int(rng.integers(1, 65))
        last = float(rng.uniform(1.0, max_last)) if k % 5 else max_last
        zero = bool(k & 1)
        if k % 3 == 2:  # logarithmic: a positive first edge, or zero in front of one
            e = np.geomspace(last / 64.0, last, nb + (0 if zero else 1))
            e = np.concatenate([[0.0], e]) if zero else e
        else:
            e = np.linspace(0.0 if zero else last / (4.0 * nb), last, nb + 1)
        assert len(e) == nb + 1 and np.all(np.diff(e * e) > 0)
        out.append(e)
    return out


def periodic_box(dim):
    c = dict(PC.box(dim))
    c["periodic"] = True
    c["name"] = f"periodic_box_{dim}"
    return c


def torus_pair(kind):
    """torus_cases.face_pair and through(face | edge | corner) as they are: boxes of dim 3 and 4, reach 1 only."""
    c = dict(TC.face_pair() if kind == "face_pair" else TC.through(kind))
    c["periodic"] = True
    return c


def wide_pair(kind):
    """The same pairs in the dim 5 box (B = 12.5), where reach 2 is admissible: through a face, an edge and a corner,
    and the face pair at exactly distance 1 with its partner pair at dx == +-B (not shifted)."""
    if kind == "face_pair":
        pos = [[12.0, 1.0, 1.0], [-12.0, 1.0, 1.0], [6.25, -5.0, 2.0], [-6.25, -5.0, 2.0]]
    else:
        a = {"face": [12.25, 1.0, 2.0], "edge": [12.25, -12.0, 2.0], "corner": [12.25, -12.0, 12.375]}[kind]
        b = {"face": [-12.0, 1.25, 2.5], "edge": [-12.0, 12.25, 2.5], "corner": [-12.0, 12.25, -12.25]}[kind]
        pos = [a, b]
    return _case("wide_" + kind, pos, PC.box_params(5), 21, periodic=True)


def corner_blob():
    """300 boids in a cube of side 2.5 around a corner of the dim 5 box: all eight octants through the faces."""
    rng = np.random.default_rng(22)
    pts = (TC.GRID - 1.25)[rng.choice(len(TC.GRID), 300, replace=False)] + np.array([12.5, 12.5, -12.5])
    return _case("corner_blob_5", PC.wrapped(pts, 12.5), PC.box_params(5), 22, periodic=True)


def lattice16(periodic):
    """The 16^3 unit lattice at the cell centres of a grid of cell 1: walled (bounds 8, the grid's two border layers
    empty) or periodic with L = 16."""
    g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) - 7.5
    prm = BC.params(bounds=8.0, perception_radius=1.0, separation_radius=0.6)
    return _case("lattice16_" + ("periodic" if periodic else "walled"), g, prm, 23, periodic=periodic)


LATTICE_EDGES = np.sort(np.concatenate([np.sqrt([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 9.0]),
                                        np.nextafter(np.sqrt([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 9.0]), 0.0)]))


def boundary(m=2):
    """Walled, cell 5: boids 0 and 1 exactly m cells apart at d = m * 5 (a candidate, counted in the last bin whose edge is
    m * 5), boid 2 one ulp before boid 0's cell (in the cell below): m + 1 cells from boid 1 and not a candidate for it."""
    x0 = -12.5
    pos = np.array([[x0, 1.0, 2.0], [x0 + 5.0 * m, 1.0, 2.0], [np.nextafter(x0, -np.inf), 1.0, 2.0]])
    c = _case(f"boundary_{m}", pos, WALLED, 24)
    c["pos"] = pos  # off the lattice on purpose
    return c


def boundary_face(m=2):
    """The periodic variant in the dim 7 box (B = 17.5, cell 5): boid 0 at x == +B lies in the LAST cell, boid 1 at
    -B + m * 5 in cell m: their distance through the face is exactly m * 5 <= the last edge, their cyclic cell distance
    m + 1.  The one input on which the candidate mask removes a pair in range; boid 2 at -B + m * 5 - 2^-16 is a candidate."""
    B = 17.5
    pos = np.array([[B, 1.0, 2.0], [-B + 5.0 * m, 1.0, 2.0], [-B + 5.0 * m - 2.0 ** -16, 1.0, 2.0]])
    return _case(f"boundary_face_{m}", pos, PC.box_params(7), 25, periodic=True)


def sizes(n, seed=26):
    rng = np.random.default_rng(seed + n)
    return _case(f"n_{n}", rng.uniform(-12.5, 12.5, (n, 3)), WALLED, seed + n)


def twins():
    """40 coincident pairs: with edges[0] == 0 every twin pair is in the slot "below"."""
    rng = np.random.default_rng(27)
    p = rng.uniform(-12.0, 12.0, (40, 3))
    return _case("twins", np.concatenate([p, p]), WALLED, 27)


def crowded(count=3000):
    """`count` boids in one cell (a run far longer than a block) and 200 around it."""
    rng = np.random.default_rng(28)
    pos = np.concatenate([rng.uniform(-2.4, 2.4, (count, 3)), rng.uniform(-12.5, 12.5, (200, 3))])
    return _case(f"crowded_{count}", pos, WALLED, 28)


def with_velocities(c, vel, tag):
    t = dict(c)
    t["vel"] = np.ascontiguousarray(vel, dtype=np.float64)
    t["name"] = c["name"] + "_" + tag
    return t


def permuted(c, seed=29):
    perm = np.random.default_rng(seed).permutation(len(c["pos"]))
    t = dict(c)
    for k in ("pos", "vel", "col"):
        t[k] = c[k][perm]
    t["name"] = c["name"] + "_permuted"
    return t


def mean_heading(vel):
    """A mean on the lattice of 2^-24 near the mean heading (any admissible mean will do for a test)."""
    import vcorr_ref as VR
    _, u = VR.headings(vel)
    m = u.mean(axis=0) if len(u) else np.zeros(3)
    return np.clip(R.lattice(m, 24), -1.0, 1.0)
