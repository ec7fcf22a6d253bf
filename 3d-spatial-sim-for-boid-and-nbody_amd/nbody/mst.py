"""Host side of the minimum spanning tree (include/nbmi.h nbmi_mst): what is derived from the
``edges`` (N - 1, 2) and ``d2`` (N - 1,) that ``HIPBarnesHutSimulation.minimum_spanning_tree`` returns, sorted ascending
by (d2, i, j).  Pure NumPy, no device."""
import numpy as np


def _arrays(n, edges, d2):
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    d = np.asarray(d2, dtype=np.float64).reshape(-1)
    if len(e) != len(d) or len(d) != max(int(n) - 1, 0):
        raise ValueError(f"mst: expected {max(int(n) - 1, 0)} edges for {n} bodies, got {len(e)} edges and {len(d)} d2")
    return e, d


def _kept(d, link):
    """how many of the sorted d2 are <= link * link (the product nbmi_fof forms)"""
    link = float(link)
    if not (np.isfinite(link) and link > 0.0):
        raise ValueError(f"mst: the linking length {link} is not finite and > 0")
    return int(np.searchsorted(d, link * link, side="right"))


def group_count(n, d2, link):
    """The number of friends-of-friends groups at ``link``, singletons included: N minus the edges with d2 <= link^2."""
    d = np.asarray(d2, dtype=np.float64).reshape(-1)
    return int(n) - _kept(d, link)


def cut(n, edges, d2, link):
    """labels (N,) int32 with nbmi_fof's convention - the smallest body index of the group - of the components left when
    the edges longer than ``link`` are cut: exactly ``find_groups(link)``."""
    e, d = _arrays(n, edges, d2)
    k = _kept(d, link)
    i, j = e[:k, 0], e[:k, 1]
    lab = np.arange(int(n), dtype=np.int64)
    while True:  # min-label hooking with pointer jumping: lab[] is a forest with lab[x] <= x
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
        a, b = lab[i], lab[j]
        open_ = a != b
        if not open_.any():
            return lab.astype(np.int32)
        i, j, a, b = i[open_], j[open_], a[open_], b[open_]
        np.minimum.at(lab, np.maximum(a, b), np.minimum(a, b))


def linkage(n, edges, d2):
    """The (N - 1, 4) float64 single-linkage matrix in SciPy's convention: row k merges the clusters Z[k, 0] < Z[k, 1]
    (0 .. N - 1: the bodies; N + r: the cluster row r made) at the height Z[k, 2] = sqrt(d2[k]) into one of Z[k, 3] bodies.
    Rows are in the tree's order, so ties in height are merged in the order of the edges' indices."""
    e, d = _arrays(n, edges, d2)
    n = int(n)
    parent = list(range(n))
    cluster = list(range(n))  # of a root: the id of its cluster
    size = [1] * n
    Z = np.empty((len(d), 4), dtype=np.float64)
    h = np.sqrt(d)

    def find(a):
        root = a
        while parent[root] != root:
            root = parent[root]
        while parent[a] != root:
            parent[a], a = root, parent[a]
        return root

    for k, (i, j) in enumerate(e.tolist()):
        a, b = find(i), find(j)
        if a == b:
            raise ValueError(f"mst.linkage: edge {k} = ({i}, {j}) closes a cycle: not a tree")
        ca, cb = cluster[a], cluster[b]
        if size[a] < size[b]:
            a, b = b, a
        parent[b] = a
        size[a] += size[b]
        cluster[a] = n + k
        Z[k] = (min(ca, cb), max(ca, cb), h[k], size[a])
    return Z


def link_for_groups(n, d2, n_groups):
    """The smallest linking length at which there are at most ``n_groups`` groups: the smallest float64 whose square, as
    nbmi_fof forms it, reaches the (N - n_groups)-th edge's d2; 0.0 if N bodies are at most that many groups already."""
    d = np.asarray(d2, dtype=np.float64).reshape(-1)
    n, n_groups = int(n), int(n_groups)
    if n_groups < 1:
        raise ValueError(f"mst: n_groups = {n_groups} is < 1")
    need = n - n_groups
    if need <= 0:
        return 0.0
    if need > len(d):
        raise ValueError(f"mst: {len(d)} edges cannot leave {n_groups} groups of {n} bodies")
    x = float(d[need - 1])
    if x == 0.0:  # coincident bodies: every valid link joins them
        return float(np.nextafter(0.0, 1.0))
    link = float(np.sqrt(x))
    while link * link < x:
        link = float(np.nextafter(link, np.inf))
    while True:
        below = float(np.nextafter(link, 0.0))
        if not (below > 0.0 and below * below >= x):
            break
        link = below
    return link
