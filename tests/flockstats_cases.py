"""Constructed inputs for the flock-analysis calls (include/bdmi.h), next to those of boids_cases.py that they reuse.

Like those, every input is on the dyadic lattice (positions multiples of 2^-16, velocities of 2^-20), so the sums of
positions and velocities are exact in any order.  Each builder returns a boids_cases-style dict plus `link`.
"""
import numpy as np

import boids_cases as BC
import boids_ref as R

H = 2.0 ** -16


def _case(name, pos, prm, link, seed):
    rng = np.random.default_rng(seed)
    c = BC._case(name, pos, prm, rng)
    c["link"] = float(link)
    return c


def chain_path(n, row=60):
    """n integer points of a path whose consecutive points are exactly 1 apart and no other two closer than sqrt(2):
    rows of `row` points along x, alternately forth and back, two apart in y, joined by one connector point."""
    pts = []
    x, y, step = 0, 0, 1
    while len(pts) < n:
        for _ in range(row):
            pts.append((x, y))
            x += step
        x -= step
        pts.append((x, y + 1))  # the connector; the next row starts above it
        y += 2
        step = -step
    return np.array(pts[:n], dtype=np.float64)


def chain(n=6000, gap_at=None, seed=20):
    """A chain of n boids spaced exactly link = perception = 1 apart on axis-parallel segments through many cells
    (every boid sits on a cell border): one flock, n - 1 links, parent chains as deep as the path is long.  With
    gap_at = k everything behind boid k is moved 2^-16 along the row that k is in, so that one pair is 1 + 2^-16 apart:
    two flocks, n - 2 links."""
    xy = chain_path(n)
    assert gap_at is None or (0 < gap_at % 61 < 58), "the gap must lie inside a row"
    ext = xy.max(axis=0)
    prm = BC.params(bounds=float(np.ceil(ext.max() / 2)) + 1.0, perception_radius=1.0, separation_radius=0.6)
    pos = np.zeros((n, 3))
    pos[:, :2] = xy - np.floor(ext / 2)
    if gap_at is not None:  # along the direction of travel of k's row (even rows run towards +x)
        pos[gap_at + 1:, 0] += H if (gap_at // 61) % 2 == 0 else -H
    # shuffle the caller's order: labels must not depend on it, and rank order is then not id order
    perm = np.random.default_rng(seed).permutation(n)
    return _case(f"chain_{n}" + ("" if gap_at is None else f"_gap_{gap_at}"), pos[perm], prm, 1.0, seed), perm


def blobs(sizes=(4095, 4096, 4097, 8193), seed=21):
    """One blob per size: distinct lattice points of a cube of side 2.5 (diagonal 4.33 < link = 5), so every two boids
    of a blob are linked; the blobs 20 apart.  Flock sizes at the chunk edges of the row reduction."""
    rng = np.random.default_rng(seed)
    prm = BC.params(bounds=60.0)
    g = np.stack(np.meshgrid(*[np.arange(21)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) * 0.125
    pts = []
    for k, m in enumerate(sizes):
        pick = rng.choice(len(g), m, replace=False)
        pts.append(g[pick] + np.array([-40.0 + 20.0 * (k % 4), -40.0 + 20.0 * (k // 4), 0.25]))
    pos = np.concatenate(pts)
    return _case("blobs_" + "_".join(map(str, sizes)), pos[rng.permutation(len(pos))], prm, 5.0, seed)


def isolated_pairs(pairs, singles=500, seed=22):
    """`pairs` pairs 0.5 apart (link = perception = 1) on a grid of spacing 3, and `singles` lone boids on other grid
    points: with min_members = 2 exactly `pairs` flocks qualify."""
    rng = np.random.default_rng(seed + pairs)
    side = int(np.ceil((pairs + singles) ** (1 / 3)))
    slots = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    slots = slots[rng.permutation(len(slots))[:pairs + singles]] * 3.0 - 1.5 * (side - 1)
    prm = BC.params(bounds=float(np.ceil(1.5 * side)) + 2.0, perception_radius=1.0, separation_radius=0.6)
    a = slots[:pairs]
    b = a + rng.choice(np.array([[0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5], [-0.5, 0, 0]]), pairs)
    pos = np.concatenate([a, b, slots[pairs:]])
    return _case(f"pairs_{pairs}", pos[rng.permutation(len(pos))], prm, 1.0, seed)


def with_link(case, link):
    c = dict(case)
    c["link"] = float(link)
    return c


def perception(case):
    return float(R.unpack(case["params"])["perception_radius"])
