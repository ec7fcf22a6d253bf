"""Plain NumPy float64 restatement of the topological interaction of include/bdmi.h ("the k nearest neighbours within
sight"), built on tests/boids_ref.py.  TEST INFRASTRUCTURE ONLY.

    neighbours()  T_i per boid: the first min(k, |N_i|) members of the metric set N_i in ascending (d2, id) order
    flocking()    compute_flocking_spatial with T_i in the place of the neighbour set, every sum from +0.0, term by
                  term in the order of T_i
    step()        flocking() + boids_ref.physics()

Candidate search as boids_ref.flocking: boids sorted by x, a chunk of queries takes the candidates whose x lies within
the (slightly widened) perception radius of the chunk's x range.  The selection is np.lexsort (a stable sort) on
(d2, id) per query: the lexicographic order of the header.  The id of a boid is its row number.
"""
import numpy as np

import boids_ref as R

K_MAX = 16


def neighbours(pos, params, k, chunk=128):
    """dict of ids (n, k) int32 padded with -1, d2 (n, k) float64 padded with +inf, count (n,) int32 = |T_i| and
    metric (n,) int64 = |N_i|."""
    if not 1 <= k <= K_MAX:
        raise ValueError(f"k = {k} must be in 1..{K_MAX}")
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    P = R.unpack(params)
    n = len(pos)
    ps = P["perception_radius"] ** 2
    reach = P["perception_radius"] * (1 + 1e-9) + 1e-12
    ids = np.full((n, k), -1, dtype=np.int32)
    d2 = np.full((n, k), np.inf)
    count = np.zeros(n, dtype=np.int32)
    metric = np.zeros(n, dtype=np.int64)
    order = np.argsort(pos[:, 0], kind="stable")
    xs = pos[order, 0]
    for s in range(0, n, chunk):
        qi = order[s:s + chunk]
        qx = pos[qi, 0]
        lo = np.searchsorted(xs, qx.min() - reach, "left")
        hi = np.searchsorted(xs, qx.max() + reach, "right")
        cand = order[lo:hi]
        # dx = p_i - p_j and d2 = (dx^2 + dy^2) + dz^2, as the header writes them
        d = [pos[qi, c][:, None] - pos[cand, c][None, :] for c in range(3)]
        dist_sq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        hit = (dist_sq < ps) & (dist_sq > 0.0001) & (qi[:, None] != cand[None, :])
        metric[qi] = hit.sum(axis=1)
        count[qi] = np.minimum(metric[qi], k)
        key = np.where(hit, dist_sq, np.inf)
        if len(cand) > k:
            # only the entries up to a row's (k + 1)-th smallest d2 can be among its first k, ties included
            bound = np.partition(key, k, axis=1)[:, k]
            hit &= key <= bound[:, None]
        rr, cc = np.nonzero(hit)
        o = np.lexsort((cand[cc], key[rr, cc], rr))  # by row, then (d2, id)
        rr, cc = rr[o], cc[o]
        rank = np.arange(len(rr)) - np.searchsorted(rr, rr, "left")
        keep = rank < k
        rr, cc, rank = rr[keep], cc[keep], rank[keep]
        ids[qi[rr], rank] = cand[cc]
        d2[qi[rr], rank] = key[rr, cc]
    return dict(ids=ids, d2=d2, count=count, metric=metric)


def first_k(rows, k):
    """neighbours(pos, params, k) from the rows of a larger k: T_i for k is a prefix of T_i for any larger k."""
    assert 1 <= k <= rows["ids"].shape[1]
    return dict(ids=rows["ids"][:, :k].copy(), d2=rows["d2"][:, :k].copy(),
                count=np.minimum(rows["metric"], k).astype(np.int32), metric=rows["metric"])


def flocking(pos, vel, col, params, k, nb=None):
    """A boids_ref.Forces (sep, ali, coh, avg, nb = |T_i|, nsep) for every boid, plus .rows = neighbours()."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    vel = np.ascontiguousarray(vel, dtype=np.float64)
    col = np.ascontiguousarray(col, dtype=np.float64)
    P = R.unpack(params)
    n = len(pos)
    rows = neighbours(pos, params, k) if nb is None else nb
    ss = P["separation_radius"] ** 2
    S, A, Cq, Cl = (np.zeros((n, 3)) for _ in range(4))  # every sum starts at +0.0
    nsep = np.zeros(n, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for s in range(k):  # rank by rank: term s of every boid's sums
            m = s < rows["count"]
            j = np.where(m, rows["ids"][:, s], 0)
            d = pos - pos[j]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            sm = m & (d2 < ss)
            dist = np.sqrt(d2)
            inv = 1.0 / dist
            t = d * inv[:, None] / dist[:, None]  # (dx * inv_dist) / dist
            S = np.where(sm[:, None], S + t, S)
            nsep += sm
            A = np.where(m[:, None], A + vel[j], A)
            Cq = np.where(m[:, None], Cq + pos[j], Cq)
            Cl = np.where(m[:, None], Cl + col[j], Cl)
        F = R.Forces(n)
        F.nb, F.nsep = rows["count"].astype(np.int64), nsep
        F.rows = rows
        ms, mf = P["max_speed"], P["max_force"]
        h = nsep > 0
        F.sep[h] = R._steer(S[h] / nsep[h, None], vel[h], ms, mf, P["separation_weight"])
        h = F.nb > 0
        cnt = F.nb[h, None].astype(np.float64)
        F.ali[h] = R._steer(A[h] / cnt, vel[h], ms, mf, P["alignment_weight"])
        F.coh[h] = R._steer(Cq[h] / cnt - pos[h], vel[h], ms, mf, P["cohesion_weight"])
        F.avg[:] = col
        F.avg[h] = (Cl[h] + col[h]) / (cnt + 1)
    return F


def step(pos, vel, col, params, k, dt):
    """One Flock.update(dt) in topological mode: the new (pos, vel, col)."""
    F = flocking(pos, vel, col, params, k)
    return R.physics(pos, vel, col, (F.sep, F.ali, F.coh, F.avg), params, dt)


def distinct_d2(rows_k_plus_1):
    """True where a boid's first k + 1 neighbours (neighbours(pos, params, k + 1)) have pairwise different d2: no tie
    decides its T_i, so its result cannot depend on the ids."""
    d2 = rows_k_plus_1["d2"]
    same = (d2[:, 1:] == d2[:, :-1]) & np.isfinite(d2[:, 1:])
    return ~same.any(axis=1)
