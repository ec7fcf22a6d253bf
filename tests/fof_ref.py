"""NumPy restatement of the friends-of-friends definitions of include/nbmi.h (nbmi_fof).

Bodies i != j are linked iff d2(i, j) <= b2 with d2 = (dx dx + dy dy) + dz dz, dx = x_j - x_i, float64 in this
association, and b2 = b * b; a group is a connected component; label[i] = the smallest body index of i's group.
Candidate pairs come from a grid hash (cells a little wider than b, the 27 neighbours), the decision from d2 as above,
the components from min-label hooking with pointer jumping.  NumPy only.
"""
import numpy as np

import knn_ref as kr

PAIR_CHUNK = 1 << 21  # candidate pairs looked at in one go
_MUL = (np.uint64(0x9E3779B97F4A7C15), np.uint64(0xC2B2AE3D27D4EB4F), np.uint64(0x165667B19E3779F9))


def d2_pairs(p, i, j):
    """d2(i, j) of the index arrays i, j: the header's three products and two sums"""
    dx, dy, dz = p[j, 0] - p[i, 0], p[j, 1] - p[i, 1], p[j, 2] - p[i, 2]
    return (dx * dx + dy * dy) + dz * dz


def _cell_keys(cells):
    """a uint64 hash of integer cell coordinates (wrapping arithmetic): equal cells give equal keys; unequal cells that
    collide only add candidates, which the distance test rejects"""
    c = cells.astype(np.int64).view(np.uint64)
    with np.errstate(over="ignore"):
        return c[..., 0] * _MUL[0] + c[..., 1] * _MUL[1] + c[..., 2] * _MUL[2]


def _sweep_chunks(p, edge):
    """the pairs no further apart than `edge` in x, by a sweep over the bodies sorted by x (for linking lengths so small
    against the extent that a grid cannot be indexed; the slabs are then nearly empty)"""
    order = np.argsort(p[:, 0], kind="stable")
    x = p[order, 0]
    cnt = np.searchsorted(x, x + edge * 1.001, "right") - np.arange(len(x)) - 1
    start = 0
    while start < len(x):
        stop = start + max(1, int(np.searchsorted(np.cumsum(cnt[start:]), PAIR_CHUNK, "right")))
        c = cnt[start:stop]
        a = np.repeat(np.arange(start, stop), c)
        b = a + 1 + np.arange(c.sum()) - np.repeat(np.cumsum(c) - c, c)
        i, j = order[a], order[b]
        yield np.minimum(i, j), np.maximum(i, j)
        start = stop


def candidate_chunks(p, b):
    """yields (i, j) index arrays with i < j that together hold every pair whose bodies lie in the same or in
    neighbouring cells of a grid of edge 1.001 b - a superset of the pairs within b per axis (a quotient of two
    coordinates at most b apart differs by at most 0.999 and a rounding, so their floors by at most one)"""
    p = np.asarray(p, np.float64)
    n = len(p)
    if n == 0:
        return
    edge = 1.001 * float(b)
    quot = (p - p.min(axis=0)) / edge
    if not quot.max() < 2.0 ** 50:  # cells finer than the doubles that index them: a sweep along x instead
        yield from _sweep_chunks(p, edge)
        return
    cells = np.floor(quot).astype(np.int64)
    key = _cell_keys(cells)
    order = np.argsort(key, kind="stable")
    skey = key[order]
    offsets = np.array([(a, b_, c) for a in (-1, 0, 1) for b_ in (-1, 0, 1) for c in (-1, 0, 1)], np.int64)
    # the 27 offsets may hash to equal keys where the grid is tiny: each distinct key once per body
    nkeys = _cell_keys(cells[:, None, :] + offsets[None, :, :])  # (n, 27)
    nkeys.sort(axis=1)
    fresh = np.ones(nkeys.shape, bool)
    fresh[:, 1:] = nkeys[:, 1:] != nkeys[:, :-1]
    lo = np.searchsorted(skey, nkeys, "left")
    cnt = np.where(fresh, np.searchsorted(skey, nkeys, "right") - lo, 0)
    per_body = cnt.sum(axis=1)
    start = 0
    while start < n:
        stop, total = start, 0
        while stop < n and (stop == start or total + per_body[stop] <= PAIR_CHUNK):
            total += per_body[stop]
            stop += 1
        c = cnt[start:stop].ravel()
        first = lo[start:stop].ravel()
        i = np.repeat(np.repeat(np.arange(start, stop), 27), c)
        within = np.arange(c.sum()) - np.repeat(np.cumsum(c) - c, c)
        j = order[np.repeat(first, c) + within]
        keep = i < j
        yield i[keep], j[keep]
        start = stop


def _compress(lab):
    while True:
        nxt = lab[lab]
        if np.array_equal(nxt, lab):
            return lab
        lab = nxt


def labels_from_pairs(n, chunks):
    """min-label hooking: lab[] is a forest with lab[i] <= i; a linked pair whose roots differ hooks the larger root under
    the smaller; pointer jumping flattens.  The root of a tree is the smallest index in it."""
    lab = np.arange(n, dtype=np.int64)
    for i, j in chunks:
        while len(i):
            lab = _compress(lab)
            a, b = lab[i], lab[j]
            open_ = a != b
            if not open_.any():
                break
            i, j, a, b = i[open_], j[open_], a[open_], b[open_]
            np.minimum.at(lab, np.maximum(a, b), np.minimum(a, b))
    return _compress(lab).astype(np.int32)


def linked_chunks(p, b):
    p = np.asarray(p, np.float64)
    b2 = float(b) * float(b)
    for i, j in candidate_chunks(p, b):
        ok = d2_pairs(p, i, j) <= b2
        yield i[ok], j[ok]


def fof(p, b):
    """(labels int32 (N,), n_groups)"""
    p = np.asarray(p, np.float64)
    lab = labels_from_pairs(len(p), linked_chunks(p, b))
    return lab, len(np.unique(lab))


def fof_naive(p, b):
    """the definition as a double loop with a union-find (small n only)"""
    p = np.asarray(p, np.float64)
    n = len(p)
    b2 = float(b) * float(b)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a
    for i in range(n):
        for j in range(i + 1, n):
            dx, dy, dz = p[j, 0] - p[i, 0], p[j, 1] - p[i, 1], p[j, 2] - p[i, 2]
            if (dx * dx + dy * dy) + dz * dz <= b2:
                a, c = find(i), find(j)
                if a != c:
                    parent[max(a, c)] = min(a, c)
    lab = np.array([find(i) for i in range(n)], np.int32)
    return lab, len(set(lab.tolist()))


def group_sizes(labels):
    """member counts of the groups, largest first"""
    return np.sort(np.bincount(np.unique(labels, return_inverse=True)[1]))[::-1]


def catalogue(p, v, m, labels, min_members=1):
    """The header's catalogue of the groups with members >= min_members, ordered by members descending, ties by label:
    a dict of count, label, members, mass, center, velocity, lo, hi - and, for the tests' error bounds, the raw sums
    ``sum_mx`` / ``sum_mv`` and the sums of the terms' magnitudes ``abs_m`` / ``abs_mx`` / ``abs_mv``."""
    p, v, m = (np.asarray(a, np.float64) for a in (p, v, m))
    uniq, inv = np.unique(labels, return_inverse=True)
    g = len(uniq)
    members = np.bincount(inv, minlength=g).astype(np.int64)
    M = np.bincount(inv, weights=m, minlength=g)
    smx = np.stack([np.bincount(inv, weights=m * p[:, a], minlength=g) for a in range(3)], 1)
    smv = np.stack([np.bincount(inv, weights=m * v[:, a], minlength=g) for a in range(3)], 1)
    sx = np.stack([np.bincount(inv, weights=p[:, a], minlength=g) for a in range(3)], 1)
    sv = np.stack([np.bincount(inv, weights=v[:, a], minlength=g) for a in range(3)], 1)
    lo = np.full((g, 3), np.inf)
    hi = np.full((g, 3), -np.inf)
    np.minimum.at(lo, inv, p)
    np.maximum.at(hi, inv, p)
    massless = M == 0.0
    div = np.where(massless, members.astype(np.float64), M)[:, None]
    center = np.where(massless[:, None], sx, smx) / div
    velocity = np.where(massless[:, None], sv, smv) / div
    keep = np.nonzero(members >= min_members)[0]
    keep = keep[np.lexsort((uniq[keep], -members[keep]))]
    return {"count": len(keep), "label": uniq[keep].astype(np.int32), "members": members[keep], "mass": M[keep],
            "center": center[keep], "velocity": velocity[keep], "lo": lo[keep], "hi": hi[keep],
            "sum_mx": smx[keep], "sum_mv": smv[keep], "abs_m": np.bincount(inv, weights=np.abs(m), minlength=g)[keep],
            "abs_mx": np.stack([np.bincount(inv, weights=np.abs(m * p[:, a]), minlength=g) for a in range(3)], 1)[keep],
            "abs_mv": np.stack([np.bincount(inv, weights=np.abs(m * v[:, a]), minlength=g) for a in range(3)], 1)[keep]}


GREY = 0.25


def group_t(label):
    """where on the ramp a group's colour lies: ((uint32)(label * 2654435761) >> 8) / 2^24"""
    h = (np.asarray(label, np.int64).astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return (h >> np.uint64(8)).astype(np.float64) / 16777216.0


def group_colors(labels, min_members):
    """float64 (N, 3): what nbmi_compute_group_colors stores as float32"""
    labels = np.asarray(labels)
    uniq, inv, counts = np.unique(labels, return_inverse=True, return_counts=True)
    out = kr.ramp(group_t(labels))
    out[counts[inv] < min_members] = GREY
    return out
