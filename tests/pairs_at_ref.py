"""NumPy restatement of the counts about arbitrary points of include/nbmi.h (nbmi_pair_counts_at; DESIGN.md section
4.28): a chunked brute force over all (point, body) pairs.

d2 is formed in the header's association, (dx dx + dy dy) + dz dz in float64 with dx = x_j - p_i, body minus point - NumPy
does not fuse, so the association holds - and E[k] = edges[k] * edges[k] is one float64 product.  A pair's column is
np.searchsorted(E, d2, side="left"): 0 = d2 <= E[0], k + 1 = E[k] < d2 <= E[k + 1] (the upper edge belongs to the bin),
nb + 1 = beyond the last edge, which no column holds.  Nothing is excluded: a point is not a body.
"""
import numpy as np

from pairs_ref import squares

CHUNK = 256  # points per block: 256 x N float64 temporaries


def d2_rows(points, bodies):
    """d2 of every point (rows) to every body (columns)"""
    q, x = np.asarray(points, dtype=np.float64), np.asarray(bodies, dtype=np.float64)
    dx = x[None, :, 0] - q[:, None, 0]
    dy = x[None, :, 1] - q[:, None, 1]
    dz = x[None, :, 2] - q[:, None, 2]
    return (dx * dx + dy * dy) + dz * dz


def per_point(points, bodies, edges):
    """(m, nb + 1) int32: nbmi_pair_counts_at's per_point rows"""
    q = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    x = np.asarray(bodies, dtype=np.float64).reshape(-1, 3)
    E = squares(edges)
    cols = len(E)
    out = np.zeros((len(q), cols), dtype=np.int32)
    if len(x) == 0:
        return out
    for a in range(0, len(q), CHUNK):
        b = min(a + CHUNK, len(q))
        col = np.searchsorted(E, d2_rows(q[a:b], x), side="left")  # (b - a, N), values 0 .. nb + 1
        flat = col + (cols + 1) * np.arange(b - a)[:, None]
        out[a:b] = np.bincount(flat.reshape(-1), minlength=(cols + 1) * (b - a)).reshape(b - a, cols + 1)[:, :cols]
    return out


def totals(rows):
    """(counts int64 (nb,), below int): the column sums of per-point rows"""
    s = np.asarray(rows, dtype=np.int64).sum(axis=0)
    return s[1:].copy(), int(s[0])


def pair_counts_at(points, bodies, edges):
    """(counts int64 (nb,), below int, rows int32 (m, nb + 1)) as nbmi_pair_counts_at defines them"""
    rows = per_point(points, bodies, edges)
    counts, below = totals(rows)
    return counts, below, rows


def per_point_naive(points, bodies, edges):
    """the definition as a plain double loop (small sizes only)"""
    q = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    x = np.asarray(bodies, dtype=np.float64).reshape(-1, 3)
    E = squares(edges)
    nb = len(E) - 1
    out = np.zeros((len(q), nb + 1), dtype=np.int32)
    for i in range(len(q)):
        for j in range(len(x)):
            dx, dy, dz = x[j, 0] - q[i, 0], x[j, 1] - q[i, 1], x[j, 2] - q[i, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            if d2 <= E[0]:
                out[i, 0] += 1
                continue
            for k in range(nb):
                if E[k] < d2 <= E[k + 1]:
                    out[i, k + 1] += 1
                    break
    return out
