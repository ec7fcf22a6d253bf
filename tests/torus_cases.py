"""Constructed inputs for the flock analysis on periodic handles (include/bdmi.h), shared by tests/test_torus_host.py
(which asserts that each is what its name says) and tests/test_gpu_boids_periodic_flocks.py.

On the dyadic lattice of boids_cases.py, inside the box [-B, B] with B a multiple of the lattice step, like the cases of
periodic_cases.py that some of them reuse.  Each builder returns that kind of dict plus `link`.
"""
import numpy as np

import boids_cases as BC
import periodic_cases as PC
import periodic_ref as PR

H = 2.0 ** -16
GRID = np.stack(np.meshgrid(*[np.arange(21)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) * 0.125  # a cube of side 2.5


def _case(name, pos, prm, link, seed, vel=None):
    c = PC._case(name, pos, prm, np.random.default_rng(seed), vel=vel)
    c["link"] = float(link)
    return c


def box(dim):
    """periodic_cases.box: uniform boids, blobs on faces, edges and corners, boids at exactly +-B.  At half the perception
    radius in the small boxes (the blobs are flocks of their own, cut on one, two or three axes), at the perception
    radius (one cell) in the box of 33."""
    c = dict(PC.box(dim))
    c["link"] = 1.0 if dim == 33 else 2.5
    return c


def sizes(n):
    c = dict(PC.sizes(n))
    c["link"] = 2.0  # about two and a half friends per boid at n = 255: flocks of many sizes
    return c


def face_pair(link=1.0):
    """Two boids at x = +-7 in the box of B = 7.5: dx = -14 -> 1 through the face, d2 == 1 exactly; and two at
    x = +-3.75 (other y), whose dx == +-B exactly is not shifted."""
    pos = np.array([[7.0, 1.0, 1.0], [-7.0, 1.0, 1.0], [3.75, -5.0, 2.0], [-3.75, -5.0, 2.0]])
    return _case("face_pair", pos, PC.box_params(3), link, 1)


def through(kind):
    """A pair through a face, an edge and a corner of the dim 4 box (B = 10), off the lattice's symmetric points."""
    a = {"face": [9.75, 1.0, 2.0], "edge": [9.75, -9.5, 2.0], "corner": [9.75, -9.5, 9.875]}[kind]
    b = {"face": [-9.5, 1.25, 2.5], "edge": [-9.5, 9.75, 2.5], "corner": [-9.5, 9.75, -9.75]}[kind]
    return _case("through_" + kind, np.array([a, b]), PC.box_params(4), 5.0, 2)


def blob(centre, m, name, seed=3, heavy_side=None):
    """m distinct points of a cube of side 2.5 around `centre`, wrapped into the dim 4 box: every two are linked at
    link = 5.  heavy_side = +1 / -1 keeps only every fourth point on the other side of the plane x = centre_x, so that
    the unwrapped centre lies clearly beyond / before the face."""
    rng = np.random.default_rng(seed)
    g = GRID - 1.25
    if heavy_side is not None:
        light = np.flatnonzero(g[:, 0] * heavy_side < 0)
        g = np.delete(g, light[np.arange(len(light)) % 4 != 0], axis=0)
    pts = g[rng.choice(len(g), m, replace=False)] + np.asarray(centre, dtype=np.float64)
    return _case(name, PC.wrapped(pts, 10.0), PC.box_params(4), 5.0, seed)


def face_blob(heavy_side=+1):
    return blob([10.0, 0.5, -2.0], 300, f"face_blob_{heavy_side:+d}", heavy_side=heavy_side)


def corner_blob():
    return blob([10.0, 10.0, -10.0], 300, "corner_blob", seed=4)


def single():
    return _case("single", np.array([[9.5, -3.0, 0.25]]), PC.box_params(4), 5.0, 5)


def chain(gap=()):
    """Boids 1 apart along the whole of x in the dim 4 box (x = -10 .. 9; 9 and -10 are 1 apart through the face), link 1:
    a ring.  gap = the x values left out: (2, 3) opens the ring into a C that still has a member in every slab."""
    x = np.array([v for v in range(-10, 10) if v not in gap], dtype=np.float64)
    pos = np.stack([x, np.full_like(x, 6.25), np.full_like(x, -7.5)], axis=1)
    return _case("chain" + "".join(f"_{g}" for g in gap), pos, PC.box_params(4), 1.0, 6)


def big_blob(m=4200):
    """4 200 members across the +x face (two chunks of the row reduction), all in the two cells next to the face on one
    (y, z): cell runs far longer than a block."""
    return blob([10.0, 2.5, 2.5], m, f"big_blob_{m}", seed=7)


def crowded_cell(m=300):
    """m boids in ONE cell (a run longer than a block of 256), next to a face, and a few friends through it."""
    rng = np.random.default_rng(8)
    g = GRID[(GRID[:, 0] < 1.3)]
    pts = g[rng.choice(len(g), m, replace=False)] + np.array([8.5, 0.25, 0.25])
    friends = np.array([[-9.75, 1.0, 1.0], [-9.5, 2.0, 1.5], [-6.0, 1.0, 1.0]])
    return _case(f"crowded_{m}", np.concatenate([pts, friends]), PC.box_params(4), 5.0, 8)


def interior(seed=9, n=1500):
    """periodic_cases.interior_cluster with link 2: further than one cell from every face, flocks of many sizes."""
    c = dict(PC.interior_cluster(seed, n))
    c["link"] = 2.0
    return c


def mixed(n=2048, seed=10):
    """Uniform boids in the dim 7 box of bounds 18.75 at link 2.5: hundreds of flocks, several through faces."""
    prm = BC.params(bounds=18.75)
    rng = np.random.default_rng(seed)
    return _case(f"mixed_{n}", rng.uniform(-18.75, 18.75, (n, 3)), prm, 2.5, seed)


def translated(c, shift):
    """The case moved by a lattice vector and wrapped back into the box (exact)."""
    B = PR.box(c["params"])[0]
    t = dict(c)
    t["pos"] = PC.wrapped(c["pos"] + np.asarray(shift, dtype=np.float64), B)
    t["name"] = c["name"] + "_moved"
    return t


def permuted(c, seed=11):
    perm = np.random.default_rng(seed).permutation(len(c["pos"]))
    t = dict(c)
    for k in ("pos", "vel", "col"):
        t[k] = c[k][perm]
    t["name"] = c["name"] + "_permuted"
    return t, perm


def gpu_cases():
    return [box(3), box(4), box(33), face_pair(), face_pair(np.nextafter(1.0, 0.0)), through("face"), through("edge"),
            through("corner"), face_blob(+1), face_blob(-1), corner_blob(), single(), chain(), chain((2, 3)), big_blob(),
            crowded_cell(), mixed()] + [sizes(n) for n in (0, 1, 2, 255, 256, 257)]
