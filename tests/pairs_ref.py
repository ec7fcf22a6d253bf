"""NumPy restatement of the binned pair counts of include/nbmi.h (nbmi_pair_counts): a chunked
brute force over the unordered pairs i < j.

d2 is formed in the header's association, (dx dx + dy dy) + dz dz in float64 - NumPy does not fuse, so the association
holds - and E[k] = edges[k] * edges[k] is one float64 product.  A pair's counter is
np.searchsorted(E, d2, side="left"): 0 = ``below`` (d2 <= E[0]), k + 1 = bin k (E[k] < d2 <= E[k + 1], the upper edge
belongs to the bin), nb + 1 = beyond the last edge.
"""
import numpy as np

CHUNK = 256  # rows per block: 256 x N float64 temporaries


def squares(edges):
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    return e * e


def exact_root(v):
    """a float64 e with e * e == v exactly, or None: most integers have none (2, 3, 5, 6 and 8 do not), which is why the
    lattice tests scale the lattice until every edge they want has one"""
    e = np.sqrt(np.float64(v))
    for c in (e, np.nextafter(e, 0.0), np.nextafter(e, np.inf)):
        if c * c == v:
            return float(c)
    return None


def d2_rows(p, a, b):
    """d2 of the bodies a .. b - 1 against the bodies a + 1 .. n - 1, and the mask of the pairs i < j"""
    p = np.asarray(p, dtype=np.float64)
    q = p[a + 1:]
    dx = q[None, :, 0] - p[a:b, None, 0]
    dy = q[None, :, 1] - p[a:b, None, 1]
    dz = q[None, :, 2] - p[a:b, None, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    upper = np.arange(a + 1, len(p))[None, :] > np.arange(a, b)[:, None]
    return d2, upper


def pair_counts_multi(p, edge_sets):
    """[(counts int64 (nb,), below int, beyond int)] for every set of edges, from one pass over the distances"""
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    Es = [squares(e) for e in edge_sets]
    acc = [np.zeros(len(E) + 1, dtype=np.int64) for E in Es]
    total = 0
    for a in range(0, max(n - 1, 0), CHUNK):
        b = min(a + CHUNK, n)
        d2, upper = d2_rows(p, a, b)
        d = d2[upper]
        total += len(d)
        for E, c in zip(Es, acc):
            near = d[d <= E[-1]]
            c[:len(E)] += np.bincount(np.searchsorted(E, near, side="left"), minlength=len(E))[:len(E)]
            c[len(E)] += len(d) - len(near)
    assert total == n * (n - 1) // 2
    return [(c[1:-1].copy(), int(c[0]), int(c[-1])) for c in acc]


def pair_counts(p, edges):
    """(counts int64 (nb,), below int) as nbmi_pair_counts defines them"""
    c, below, _ = pair_counts_multi(p, [edges])[0]
    return c, below


def pair_counts_naive(p, edges):
    """the definition as a plain double loop (small n only)"""
    p = np.asarray(p, dtype=np.float64)
    E = squares(edges)
    nb = len(E) - 1
    counts, below = [0] * nb, 0
    for i in range(len(p)):
        for j in range(i + 1, len(p)):
            dx, dy, dz = p[j, 0] - p[i, 0], p[j, 1] - p[i, 1], p[j, 2] - p[i, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            if d2 <= E[0]:
                below += 1
                continue
            for k in range(nb):
                if E[k] < d2 <= E[k + 1]:
                    counts[k] += 1
                    break
    return np.array(counts, dtype=np.int64), below


def nearest_d2(p):
    """the squared distance of every body to its nearest other body (knn(1)'s r2_k), chunked"""
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    out = np.empty(n)
    for a in range(0, n, CHUNK):
        b = min(a + CHUNK, n)
        dx = p[None, :, 0] - p[a:b, None, 0]
        dy = p[None, :, 1] - p[a:b, None, 1]
        dz = p[None, :, 2] - p[a:b, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d2[np.arange(b - a), np.arange(a, b)] = np.inf
        out[a:b] = d2.min(axis=1)
    return out
