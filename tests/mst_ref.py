"""NumPy restatement of the minimum spanning tree of include/nbmi.h (nbmi_mst), in two
independent forms.

d2(i, j) = (dx dx + dy dy) + dz dz with dx = x_j - x_i, float64 in this association; the unordered pair {i, j}, i < j, has
the key (d2, i, j), compared lexicographically - a strict total order, so the tree is unique.  ``prim`` grows it from
body 0 and keeps the full key of every outside body's best link (d2 row by row: no N x N matrix); ``kruskal`` takes all
pairs in np.lexsort((j, i, d2)) order (N up to about 2 000).  Both return (edges int32 (N - 1, 2), d2 float64 (N - 1,))
sorted ascending by the key, edges[:, 0] < edges[:, 1].  A plain helper module: NumPy only, no fixtures.
"""
import numpy as np

from fof_ref import d2_pairs


def _sorted(i, j, d2):
    i, j, d2 = np.asarray(i, np.int64), np.asarray(j, np.int64), np.asarray(d2, np.float64)
    order = np.lexsort((j, i, d2))
    return np.stack([i[order], j[order]], 1).astype(np.int32).reshape(-1, 2), d2[order]


def prim(p):
    p = np.asarray(p, np.float64)
    n = len(p)
    if n < 2:
        return np.empty((0, 2), np.int32), np.empty(0, np.float64)
    everyone = np.arange(n)
    outside = np.ones(n, bool)
    bd2 = np.full(n, np.inf)
    bi = np.full(n, n, np.int64)
    bj = np.full(n, n, np.int64)
    ei, ej, ed = [], [], []
    v = 0
    for _ in range(n - 1):
        outside[v] = False
        row = d2_pairs(p, np.full(n, v), everyone)  # symmetric bit for bit: a negated difference squares to the same
        lo, hi = np.minimum(v, everyone), np.maximum(v, everyone)
        less = outside & ((row < bd2) | ((row == bd2) & ((lo < bi) | ((lo == bi) & (hi < bj)))))
        bd2[less], bi[less], bj[less] = row[less], lo[less], hi[less]
        cand = np.nonzero(outside)[0]
        cand = cand[bd2[cand] == bd2[cand].min()]
        cand = cand[bi[cand] == bi[cand].min()]
        v = int(cand[np.argmin(bj[cand])])
        ei.append(bi[v]); ej.append(bj[v]); ed.append(bd2[v])
    return _sorted(ei, ej, ed)


def kruskal(p):
    p = np.asarray(p, np.float64)
    n = len(p)
    if n < 2:
        return np.empty((0, 2), np.int32), np.empty(0, np.float64)
    i, j = np.triu_indices(n, 1)
    d2 = d2_pairs(p, i, j)
    order = np.lexsort((j, i, d2))
    parent = list(range(n))

    def find(a):
        root = a
        while parent[root] != root:
            root = parent[root]
        while parent[a] != root:
            parent[a], a = root, parent[a]
        return root

    taken = []
    for k in order.tolist():
        a, b = find(int(i[k])), find(int(j[k]))
        if a != b:
            parent[max(a, b)] = min(a, b)
            taken.append(k)
            if len(taken) == n - 1:
                break
    taken = np.array(taken, np.int64)
    return _sorted(i[taken], j[taken], d2[taken])


_REF = {}


def reference(name, p):
    """prim(p), made once per name and shared by the tests; callers do not write to it"""
    if name not in _REF:
        _REF[name] = prim(p)
    return _REF[name]
