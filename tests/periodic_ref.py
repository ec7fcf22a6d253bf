"""Plain NumPy float64 restatement of the periodic box of include/bdmi.h ("Periodic handles"), built on
tests/boids_ref.py and tests/topo_ref.py.  TEST INFRASTRUCTURE ONLY.

    box()            B, L, dim, cell_size of a parameter vector
    cell_index()     the periodic grid's cell id per boid
    image()          q' per axis: q + L if p - q > B, q - L if p - q < -B, else q (equality does not shift)
    neighbours()     topo_ref.neighbours with the image's d2: T_i in ascending (d2, id) order
    flocking()       the topological forces, every sum from +0.0 in the order of T_i, q' in the place of q
    metric()         the metric forces (boids_ref.Forces with sep_sum / sep_abs for boids_ref.check_sep)
    physics()        update_physics without the wall terms, an optional kick A * xi, and the wrap
    step()           flocking() or metric() + physics()
    run_facts()      the kernel's candidate runs, restated: per boid the lengths of its up to 18 runs

Neighbours are found by distance alone, all pairs: with dim >= 3 and cell_size >= the perception radius the 27 wrapped
cells hold every boid once, and the image above is the only one of its images that can be closer than the perception
radius (any other differs by L >= 3 perception radii on some axis).  The id of a boid is its row number.
"""
import numpy as np

import boids_ref as R
import topo_ref as T


def box(params):
    P = R.unpack(params)
    B = P["bounds"]
    L = 2 * B
    dim = int(np.floor(L / P["perception_radius"]))
    return B, L, dim, L / dim


def cell_coords(pos, params):
    B, _, dim, cell = box(params)
    c = np.trunc((np.asarray(pos, dtype=np.float64) + B) / cell)
    return np.clip(c.astype(np.int64), 0, dim - 1)


def cell_index(pos, params):
    _, _, dim, _ = box(params)
    c = cell_coords(pos, params)
    return c[:, 0] + c[:, 1] * dim + c[:, 2] * dim * dim


def image(p, q, B, L):
    """q' for p (broadcast): the operations of the header, per axis."""
    d0 = p - q
    return np.where(d0 > B, q + L, np.where(d0 < -B, q - L, q))


def wrap(x, B, L):
    return np.where(x > B, x - L, np.where(x < -B, x + L, x))


def _pairs(pos, params, chunk):
    """Per chunk of queries: (rows qi, images (3 x (len(qi), n)), d (3 x ...), dist_sq, hit)."""
    P = R.unpack(params)
    B, L, _, _ = box(params)
    n = len(pos)
    ps = P["perception_radius"] ** 2
    allj = np.arange(n)
    for s in range(0, n, chunk):
        qi = np.arange(s, min(s + chunk, n))
        img = [image(pos[qi, c][:, None], pos[:, c][None, :], B, L) for c in range(3)]
        d = [pos[qi, c][:, None] - img[c] for c in range(3)]
        dist_sq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        hit = (dist_sq < ps) & (dist_sq > 0.0001) & (qi[:, None] != allj[None, :])
        yield qi, img, d, dist_sq, hit


def neighbours(pos, params, k, chunk=256):
    """As topo_ref.neighbours: ids (n, k) padded with -1, d2 (n, k) padded with +inf, count = |T_i|, metric = |N_i|."""
    if not 1 <= k <= T.K_MAX:
        raise ValueError(f"k = {k} must be in 1..{T.K_MAX}")
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    n = len(pos)
    ids = np.full((n, k), -1, dtype=np.int32)
    d2 = np.full((n, k), np.inf)
    count = np.zeros(n, dtype=np.int32)
    metric = np.zeros(n, dtype=np.int64)
    for qi, _, _, dist_sq, hit in _pairs(pos, params, chunk):
        metric[qi] = hit.sum(axis=1)
        count[qi] = np.minimum(metric[qi], k)
        key = np.where(hit, dist_sq, np.inf)
        if n > k:
            # only the entries up to a row's (k + 1)-th smallest d2 can be among its first k, ties included
            bound = np.partition(key, k, axis=1)[:, k]
            hit &= key <= bound[:, None]
        rr, cc = np.nonzero(hit)
        o = np.lexsort((cc, key[rr, cc], rr))  # by row, then (d2, id)
        rr, cc = rr[o], cc[o]
        rank = np.arange(len(rr)) - np.searchsorted(rr, rr, "left")
        keep = rank < k
        rr, cc, rank = rr[keep], cc[keep], rank[keep]
        ids[qi[rr], rank] = cc
        d2[qi[rr], rank] = key[rr, cc]
    return dict(ids=ids, d2=d2, count=count, metric=metric)


def _finish(F, S, A, Cq, Cl, pos, vel, col, P):
    ms, mf = P["max_speed"], P["max_force"]
    with np.errstate(divide="ignore", invalid="ignore"):
        h = F.nsep > 0
        F.sep[h] = R._steer(S[h] / F.nsep[h, None], vel[h], ms, mf, P["separation_weight"])
        h = F.nb > 0
        cnt = F.nb[h, None].astype(np.float64)
        F.ali[h] = R._steer(A[h] / cnt, vel[h], ms, mf, P["alignment_weight"])
        F.coh[h] = R._steer(Cq[h] / cnt - pos[h], vel[h], ms, mf, P["cohesion_weight"])
        F.avg[:] = col
        F.avg[h] = (Cl[h] + col[h]) / (cnt + 1)
    return F


def flocking(pos, vel, col, params, k, nb=None):
    """topo_ref.flocking on the periodic box: q' in the place of the neighbour's position."""
    pos, vel, col = (np.ascontiguousarray(a, dtype=np.float64) for a in (pos, vel, col))
    P = R.unpack(params)
    B, L, _, _ = box(params)
    n = len(pos)
    rows = neighbours(pos, params, k) if nb is None else nb
    ss = P["separation_radius"] ** 2
    S, A, Cq, Cl = (np.zeros((n, 3)) for _ in range(4))  # every sum starts at +0.0
    nsep = np.zeros(n, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for s in range(rows["ids"].shape[1]):  # rank by rank: term s of every boid's sums
            m = s < rows["count"]
            j = np.where(m, rows["ids"][:, s], 0)
            q = image(pos, pos[j], B, L)
            d = pos - q
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            sm = m & (d2 < ss)
            dist = np.sqrt(d2)
            inv = 1.0 / dist
            t = d * inv[:, None] / dist[:, None]  # (dx * inv_dist) / dist
            S = np.where(sm[:, None], S + t, S)
            nsep += sm
            A = np.where(m[:, None], A + vel[j], A)
            Cq = np.where(m[:, None], Cq + q, Cq)
            Cl = np.where(m[:, None], Cl + col[j], Cl)
    F = R.Forces(n)
    F.nb, F.nsep = rows["count"].astype(np.int64), nsep
    F.rows = rows
    return _finish(F, S, A, Cq, Cl, pos, vel, col, P)


def metric(pos, vel, col, params, chunk=256):
    """boids_ref.flocking on the periodic box, all pairs.  On lattice inputs whose box is a multiple of the lattice step
    the alignment, cohesion and colour sums are exact in any order; the separation sum comes with sep_sum / sep_abs."""
    pos, vel, col = (np.ascontiguousarray(a, dtype=np.float64) for a in (pos, vel, col))
    P = R.unpack(params)
    n = len(pos)
    ss = P["separation_radius"] ** 2
    F = R.Forces(n)
    S, A, Cq, Cl = (np.zeros((n, 3)) for _ in range(4))
    for qi, img, d, dist_sq, hit in _pairs(pos, params, chunk):
        w = hit.astype(np.float64)
        F.nb[qi] = hit.sum(axis=1)
        A[qi] = w @ vel
        Cl[qi] = w @ col
        for c in range(3):
            Cq[qi, c] = (w * img[c]).sum(axis=1)
        a, b = np.nonzero(hit & (dist_sq < ss))
        dist = np.sqrt(dist_sq[a, b])
        inv = 1.0 / dist
        F.nsep[qi] = np.bincount(a, minlength=len(qi))
        for c in range(3):
            t = d[c][a, b] * inv / dist
            S[qi, c] = np.bincount(a, weights=t, minlength=len(qi))
            F.sep_abs[qi, c] = np.bincount(a, weights=np.abs(t), minlength=len(qi))
    F.sep_sum = S.copy()
    return _finish(F, S, A, Cq, Cl, pos, vel, col, P)


def physics(pos, vel, col, forces, params, dt, kick=None):
    """update_physics without the wall terms: acc = ((sep + ali) + coh) [+ kick], the velocity clamp, p' = p + v' dt and
    one wrap.  kick = A * xi (n, 3) of a noisy step, or None."""
    P = R.unpack(params)
    B, L, _, _ = box(params)
    sep, ali, coh, avg = (np.asarray(f, dtype=np.float64) for f in forces)
    pos, vel, col = (np.asarray(a, dtype=np.float64) for a in (pos, vel, col))
    acc = (sep + ali) + coh
    if kick is not None:
        acc = acc + kick
    nv = vel + acc * dt
    speed = np.sqrt(nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1] + nv[:, 2] * nv[:, 2])
    k = speed > P["max_speed"]
    nv[k] *= (P["max_speed"] / speed[k])[:, None]
    blend = P["color_blend_rate"] * dt
    blend = blend if blend < 1.0 else 1.0
    return wrap(pos + nv * dt, B, L), nv, col + (avg - col) * blend


def step(pos, vel, col, params, k, dt, kick=None):
    """One update of a periodic flock: topological with k, metric with k = None."""
    F = metric(pos, vel, col, params) if k is None else flocking(pos, vel, col, params, k)
    return physics(pos, vel, col, (F.sep, F.ali, F.coh, F.avg), params, dt, kick)


def crossings(before, after, params):
    """The boids that the wrap moved: |after - before| of more than B on some axis."""
    B = box(params)[0]
    return np.any(np.abs(np.asarray(after) - np.asarray(before)) > B, axis=1)


def run_facts(pos, params):
    """Per boid, as the periodic sweep sees its rows: runs (n, 18) = the lengths of the two x segments of each of its nine
    wrapped rows (the second one 0 away from the x faces), face = the boid sits in an x-face cell."""
    _, _, dim, _ = box(params)
    cc = cell_coords(pos, params)
    keys = np.sort(cell_index(pos, params))
    cx = cc[:, 0]
    face = (cx == 0) | (cx == dim - 1)
    lo0 = np.where(cx == 0, 0, np.where(cx == dim - 1, dim - 2, cx - 1))
    hi0 = np.where(cx == 0, 1, np.where(cx == dim - 1, dim - 1, cx + 1))
    lo1 = np.where(cx == 0, dim - 1, 0)
    runs = np.zeros((len(cc), 18), dtype=np.int64)
    k = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            row = ((cc[:, 1] + dy) % dim) * dim + ((cc[:, 2] + dz) % dim) * dim * dim
            runs[:, k] = np.searchsorted(keys, row + hi0, "right") - np.searchsorted(keys, row + lo0, "left")
            seg = np.searchsorted(keys, row + lo1, "right") - np.searchsorted(keys, row + lo1, "left")
            runs[:, k + 1] = np.where(face, seg, 0)
            k += 2
    return dict(runs=runs, face=face, longest=runs.max(axis=1))
