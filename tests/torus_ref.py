"""NumPy restatement of "Flock analysis on periodic handles" of include/bdmi.h (bdmi_periodic_flocks,
bdmi_periodic_flock_catalogue, bdmi_periodic_neighbour_stats).  TEST INFRASTRUCTURE ONLY.

    d2_pairs()      the header's distance: the DIFFERENCE is brought into [-B, B], equality does not shift
    analyse()       labels, n_flocks, links, evals, count, nn_d2, nb_evals from all pairs (no grid is used to FIND the
                    linked pairs; the cell coordinates only count the evaluations the header promises)
    wrap_of()       wrap_a of a set of cell coordinates: -1 if all dim are occupied, else the smallest occupied one
                    whose cyclic predecessor is free
    row()           the 16 doubles of one flock and its wrap, the sums in the header's order: members t, t + 256, .. of a
                    chunk of 4096 per thread from +0.0, the butterfly over 32, 16, .. 1 inside a wave of 64, the four
                    waves left to right, the chunks in chunk order.  Float64 without FMA, as NumPy evaluates it.
    catalogue()     the flocks with members >= min_members, members descending, ties by label; member order = a stable
                    sort by label of the cell-sorted boids

Everything is meant to be compared bit for bit.  The id of a boid is its row number; `order` (default: the row order)
is the order of the handle's rows before its sort by cell, which is the caller's order on a handle that has not stepped.
"""
import numpy as np

import fof_ref
import periodic_ref as PR

CHUNK, BLOCK, WAVE = 4096, 256, 64


def diff_pairs(pos, i, j, B, L):
    """The three differences x_j - x_i of the index arrays i, j (broadcast), brought into [-B, B]: (..., 3)."""
    pos = np.asarray(pos, dtype=np.float64)
    d = pos[j] - pos[i]
    return np.where(d > B, d - L, np.where(d < -B, d + L, d))


def d2_pairs(pos, i, j, B, L):
    """d2(i, j) for index arrays i, j (broadcast)."""
    d = diff_pairs(pos, i, j, B, L)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def analyse(pos, params, link, chunk=256):
    """All pairs, `chunk` rows at a time.  evals = the unordered pairs whose cells are the same or cyclic neighbours on
    every axis (what the link kernel evaluates, each once); nb_evals = twice that (every boid meets each such other)."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    n = len(pos)
    B, L, dim, _ = PR.box(params)
    b2 = float(link) * float(link)
    cc = PR.cell_coords(pos, params) if n else np.zeros((0, 3), np.int64)
    count = np.zeros(n, np.int64)
    nn = np.full(n, np.inf)
    links = [0]
    evals = [0]
    allj = np.arange(n)

    def chunks():
        for s in range(0, n, chunk):
            qi = np.arange(s, min(s + chunk, n))
            d2 = d2_pairs(pos, qi[:, None], allj[None, :], B, L)
            other = qi[:, None] != allj[None, :]
            hit = (d2 <= b2) & other
            count[qi] = hit.sum(axis=1)
            nn[qi] = np.where(hit, d2, np.inf).min(axis=1, initial=np.inf)
            near = other.copy()
            for a in range(3):
                k = (cc[qi, a][:, None] - cc[:, a][None, :]) % dim
                near &= (k == 0) | (k == 1) | (k == dim - 1)
            evals[0] += int(near.sum())
            assert not (hit & ~near).any(), "a linked pair outside the 27 cells"
            i, j = np.nonzero(hit & (qi[:, None] < allj[None, :]))
            links[0] += len(i)
            yield qi[i], j
    lab = fof_ref.labels_from_pairs(n, chunks()).astype(np.int32)
    return dict(labels=lab, n_flocks=len(np.unique(lab)), links=links[0], evals=evals[0] // 2, count=count.astype(np.int32),
                nn_d2=nn, nb_evals=evals[0])


def wrap_of(coords, dim):
    occ = np.zeros(dim, dtype=bool)
    occ[np.asarray(coords, dtype=np.int64)] = True
    if occ.all():
        return -1
    starts = np.flatnonzero(occ & ~np.roll(occ, 1))  # roll: element c gets the flag of (c - 1) mod dim
    return int(starts[0])


def _lane0(acc):
    """acc (256, k): the per-thread partial sums of one block -> (k,), folded as the kernel folds them."""
    a = acc.reshape(BLOCK // WAVE, WAVE, -1)
    lanes = np.arange(WAVE)
    o = WAVE // 2
    while o > 0:
        a = a + a[:, lanes ^ o]
        o >>= 1
    x = a[0, 0]
    for w in range(1, BLOCK // WAVE):
        x = x + a[w, 0]
    return x


def ordered_sum(terms):
    """sum of the rows of terms (m, k) in the header's order, m >= 1."""
    terms = np.asarray(terms, dtype=np.float64)
    total = None
    for c0 in range(0, len(terms), CHUNK):
        t = terms[c0:c0 + CHUNK]
        acc = np.zeros((BLOCK, terms.shape[1]))
        for s in range(0, len(t), BLOCK):
            seg = t[s:s + BLOCK]
            acc[:len(seg)] = acc[:len(seg)] + seg
        part = _lane0(acc)
        total = part if total is None else total + part
    return total


def _norm(a):
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def row(pos, vel, params):
    """(row (16,), wrap (3,) int32) of the flock whose members are the rows of pos / vel, in member order."""
    p, v = np.asarray(pos, np.float64).reshape(-1, 3), np.asarray(vel, np.float64).reshape(-1, 3)
    B, L, dim, _ = PR.box(params)
    m = len(p)
    cc = PR.cell_coords(p, params)
    wrap = np.array([wrap_of(cc[:, a], dim) for a in range(3)], dtype=np.int32)
    y = np.where(cc < wrap[None, :], p + L, p)
    s = _norm(v)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where((s == 0.0)[:, None], 0.0, v / s[:, None])
    fm = float(m)
    S = ordered_sum(np.concatenate([y, v, u, s[:, None]], axis=1))
    ct = S[0:3] / fm
    out = np.zeros(16)
    out[0] = fm
    out[1:4] = np.where(ct > B, ct - L, ct)
    out[4:7] = S[3:6] / fm
    out[7] = np.sqrt((S[6] * S[6] + S[7] * S[7]) + S[8] * S[8]) / fm
    out[8] = S[9] / fm
    r = y - ct
    rho = _norm(r)
    with np.errstate(invalid="ignore", divide="ignore"):
        rh = np.where((rho == 0.0)[:, None], 0.0, r / rho[:, None])
    w = np.stack([rh[:, 1] * u[:, 2] - rh[:, 2] * u[:, 1], rh[:, 2] * u[:, 0] - rh[:, 0] * u[:, 2],
                  rh[:, 0] * u[:, 1] - rh[:, 1] * u[:, 0]], axis=1)
    W = ordered_sum(w)
    out[9] = np.sqrt((W[0] * W[0] + W[1] * W[1]) + W[2] * W[2]) / fm
    out[10:13] = y.min(axis=0)
    out[13:16] = y.max(axis=0)
    return out, wrap


def member_order(pos, labels, params, order=None):
    """The boids as the catalogue takes them: the handle's rows sorted by cell (stable), then by label (stable)."""
    n = len(pos)
    order = np.arange(n) if order is None else np.asarray(order)
    by_cell = order[np.argsort(PR.cell_index(pos, params)[order], kind="stable")]
    return by_cell[np.argsort(np.asarray(labels)[by_cell], kind="stable")]


def catalogue(pos, vel, labels, params, min_members=1, order=None):
    """dict(count, label int32, members int64, rows (count, 16), wrap int32 (count, 3), idx: the members of each row in
    member order)."""
    pos, vel = np.asarray(pos, np.float64).reshape(-1, 3), np.asarray(vel, np.float64).reshape(-1, 3)
    labels = np.asarray(labels)
    if len(pos) == 0:
        return dict(count=0, label=np.zeros(0, np.int32), members=np.zeros(0, np.int64), rows=np.zeros((0, 16)),
                    wrap=np.zeros((0, 3), np.int32), idx=[])
    mo = member_order(pos, labels, params, order)
    uniq, first, members = np.unique(labels[mo], return_index=True, return_counts=True)
    keep = np.nonzero(members >= min_members)[0]
    keep = keep[np.lexsort((uniq[keep], -members[keep]))]
    rows, wrap, idx = np.zeros((len(keep), 16)), np.zeros((len(keep), 3), np.int32), []
    for k, g in enumerate(keep):
        ids = mo[first[g]:first[g] + members[g]]
        rows[k], wrap[k] = row(pos[ids], vel[ids], params)
        idx.append(ids)
    return dict(count=len(keep), label=uniq[keep].astype(np.int32), members=members[keep].astype(np.int64), rows=rows,
                wrap=wrap, idx=idx)


def same_rows(got, want):
    """Bit for bit; lo and hi through + 0.0, since a minimum over +0.0 and -0.0 may keep either."""
    got, want = np.array(got, np.float64), np.array(want, np.float64)
    if got.shape != want.shape:
        return False
    got[..., 10:16] += 0.0
    want[..., 10:16] += 0.0
    return bool(np.array_equal(got.view(np.int64), want.view(np.int64)))
