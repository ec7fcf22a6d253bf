"""Plain NumPy restatement of bdmi_velocity_correlation (include/bdmi.h, "Velocity correlation C(r) beyond the sight
radius").  TEST INFRASTRUCTURE ONLY.

    headings()    s, u of the header: float64 in its association, 0 for a boid at rest
    quantise()    q = rint((u - mean) 2^24), ties to even, 0 where the difference is not finite: int64 (n, 3)
    reach()       m = (int)ceil(edges[nb] / cell_size)
    PairTable     every pair i < j of an input, gathered in chunks of rows: d2 and the cell distance (shared, read only)
    correlate()   the call: the brute force over that table with the candidate mask of the header and
                  searchsorted(E, d2, "left"); every sum in Python integers
    double_loop() the same by a plain double loop over the pairs (the check of correlate())
    hi_lo()       S -> the unique (hi, lo) with S = hi 2^32 + lo, 0 <= lo < 2^32

Cell coordinates come from boids_ref.cell_coords (walled) and periodic_ref.cell_coords (periodic).
"""
import math

import numpy as np

import boids_ref as R
import periodic_ref as PR

QUANTUM_BITS = 24
MAX_BINS, MAX_REACH = 64, 16


def headings(vel):
    v = np.asarray(vel, dtype=np.float64).reshape(-1, 3)
    s = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where((s != 0)[:, None], v / s[:, None], 0.0)
    return s, u


def quantise(vel, mean):
    _, u = headings(vel)
    d = u - np.asarray(mean, dtype=np.float64).reshape(1, 3)
    with np.errstate(invalid="ignore"):
        q = np.where(np.isfinite(d), np.rint(d * 2.0 ** QUANTUM_BITS), 0.0)
    return q.astype(np.int64)


def self5(q):
    qsum = [int(x) for x in q.sum(axis=0)] if len(q) else [0, 0, 0]
    qsq = sum(int(x) for x in (q * q).sum(axis=1))
    return qsum, qsq


def hi_lo(S):
    S = int(S)
    return S >> 32, S & 0xFFFFFFFF


def from_hi_lo(hi, lo):
    return (int(hi) << 32) + int(lo)


def grid_of(params, periodic):
    """cell_size and dim of the handle's grid."""
    if periodic:
        _, _, dim, cell = PR.box(params)
        return cell, dim
    cell, dim, _ = R.grid(params)
    return cell, dim


def reach(edges, params, periodic):
    cell, _ = grid_of(params, periodic)
    return int(math.ceil(float(edges[-1]) / cell))


def admissible(m, params, periodic):
    _, dim = grid_of(params, periodic)
    return 1 <= m <= MAX_REACH and (not periodic or 2 * m + 1 <= dim)


def _coords(pos, params, periodic):
    if len(pos) == 0:
        return np.zeros((0, 3), np.int64)
    return PR.cell_coords(pos, params) if periodic else R.cell_coords(pos, params)


def _d2(pos, i, j, params, periodic):
    d = pos[j] - pos[i]
    if periodic:
        B, L, _, _ = PR.box(params)
        d = np.where(d > B, d - L, np.where(d < -B, d + L, d))
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


class PairTable:
    """Every pair i < j of a set of positions, gathered `chunk` rows at a time: d2 and the largest per-axis (cyclic) cell
    distance.  Computed once per input and shared (read only) by every correlate() on it."""

    def __init__(self, pos, params, periodic=False, chunk=256):
        self.pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        self.params, self.periodic, self.n = params, bool(periodic), len(self.pos)
        _, dim = grid_of(params, periodic)
        cc = _coords(self.pos, params, periodic)
        allj = np.arange(self.n)
        I, J, D, K = [], [], [], []
        for s in range(0, self.n, chunk):
            qi = np.arange(s, min(s + chunk, self.n))
            ii, jj = np.nonzero(qi[:, None] < allj[None, :])
            ii = qi[ii]
            k = np.abs(cc[ii] - cc[jj])
            if periodic:
                k = np.minimum(k, dim - k)
            I.append(ii.astype(np.int32)); J.append(jj.astype(np.int32))
            D.append(_d2(self.pos, ii, jj, params, periodic)); K.append(k.max(axis=1).astype(np.int16))
        cat = lambda x, t: np.concatenate(x) if x else np.zeros(0, t)
        d2 = cat(D, np.float64)
        order = np.argsort(d2, kind="stable")  # by distance (NaN last): a slot is then one range of the table
        self.i, self.j, self.d2, self.cheb = cat(I, np.int32)[order], cat(J, np.int32)[order], d2[order], cat(K, np.int16)[order]


def correlate(pos, vel, params, edges, mean, periodic=False, table=None):
    """dict of pairs (int64 (nb+1,)), dot (Python ints), evals, qsum, qsq, reach, and `cut`: the number of pairs with
    d2 <= E[nb] that the candidate mask removed (0 except for inputs built to sit on the boundary)."""
    t = table if table is not None else PairTable(pos, params, periodic)
    edges = np.asarray(edges, dtype=np.float64)
    nb = len(edges) - 1
    E = edges * edges
    q = quantise(vel, mean)
    qsum, qsq = self5(q)
    m = reach(edges, params, periodic)
    evals = int((t.cheb <= m).sum())
    end = np.searchsorted(t.d2, E, "right")  # end[k] = the pairs with d2 <= E[k]: slot k is the range end[k-1] .. end[k]
    top = int(end[nb])
    cand = t.cheb[:top] <= m
    g = (q[t.i[:top]] * q[t.j[:top]]).sum(axis=1) * cand  # |g| <= 3 * 2^50: exact in int64
    # running sums of the count and of the two halves of g (26 + 26 bits: exact in int64 for any table a test can hold)
    zero = np.zeros(1, dtype=np.int64)
    cnt = np.concatenate([zero, np.cumsum(cand, dtype=np.int64)])
    hi = np.concatenate([zero, np.cumsum(g >> 26, dtype=np.int64)])
    lo = np.concatenate([zero, np.cumsum(g & ((1 << 26) - 1), dtype=np.int64)])
    b = np.concatenate([[0], end]).astype(np.int64)
    pairs = cnt[b[1:]] - cnt[b[:-1]]
    dot = [(int(hi[b[k + 1]] - hi[b[k]]) << 26) + int(lo[b[k + 1]] - lo[b[k]]) for k in range(nb + 1)]
    return dict(pairs=pairs, dot=dot, evals=evals, qsum=qsum, qsq=qsq, reach=m, cut=top - int(cnt[top]), q=q)


def double_loop(pos, vel, params, edges, mean, periodic=False):
    """correlate() restated pair by pair in Python scalars."""
    pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    n = len(pos)
    E = [float(e) * float(e) for e in edges]
    nb = len(E) - 1
    q = quantise(vel, mean).tolist()
    m = reach(edges, params, periodic)
    _, dim = grid_of(params, periodic)
    cc = _coords(pos, params, periodic).tolist()
    if periodic:
        B, L, _, _ = PR.box(params)
    pairs, dot, evals = [0] * (nb + 1), [0] * (nb + 1), 0
    P = pos.tolist()
    for i in range(n):
        for j in range(i + 1, n):
            ok = True
            for a in range(3):
                k = abs(cc[i][a] - cc[j][a])
                if periodic:
                    k = min(k, dim - k)
                ok = ok and k <= m
            if not ok:
                continue
            evals += 1
            d = []
            for a in range(3):
                x = P[j][a] - P[i][a]
                if periodic:
                    x = x - L if x > B else (x + L if x < -B else x)
                d.append(x)
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            if not d2 <= E[nb]:
                continue
            k = 0
            while E[k] < d2:
                k += 1
            pairs[k] += 1
            dot[k] += q[i][0] * q[j][0] + q[i][1] * q[j][1] + q[i][2] * q[j][2]
    return dict(pairs=pairs, dot=dot, evals=evals)


def result_dict(want, edges, n):
    """The restatement's result in the shape of Flock.velocity_correlation's dict (for boids.analysis)."""
    return dict(edges=np.asarray(edges, dtype=np.float64), pairs=np.asarray(want["pairs"], dtype=np.int64), dot=list(want["dot"]),
                quantum=2.0 ** -QUANTUM_BITS, reach=want["reach"], evals=want["evals"], qsum=list(want["qsum"]), qsq=want["qsq"],
                n=n)
