"""NumPy restatement of the flock-analysis text of include/bdmi.h (bdmi_flocks, bdmi_flock_catalogue, bdmi_diagnostics,
bdmi_neighbour_stats).

Boids i != j are linked iff d2(i, j) <= b2 with d2 = (dx dx + dy dy) + dz dz, dx = x_j - x_i, float64 in this association,
b2 = link * link; a flock is a connected component, its label the smallest boid index in it.  The linked pairs come from
fof_ref (a grid hash that knows nothing of the boids grid or of clamping), the components from its min-label hooking.
The rows of 16 doubles follow the header formula by formula; their sums are taken with math.fsum (the exactly rounded
sum, which no summation order can beat), so a kernel that adds the same terms in any order differs from them by at most
its own summation error.  NumPy and the standard library only.
"""
import math

import numpy as np

import fof_ref

U = 2.0 ** -53


def analyse(pos, link):
    """One pass over the linked pairs (i < j) of fof_ref: dict(labels int32 (N,), n_flocks, links, count int32 (N,),
    nn_d2 float64 (N,)) - the flock labels, the number of linked pairs, and per boid the others within `link` and the
    least d2 among them (+inf without one)."""
    pos = np.asarray(pos, np.float64)
    n = len(pos)
    count = np.zeros(n, np.int64)
    nn = np.full(n, np.inf)
    links = [0]

    def chunks():
        for i, j in fof_ref.linked_chunks(pos, link):
            links[0] += len(i)
            count[:] += np.bincount(i, minlength=n) + np.bincount(j, minlength=n)
            d2 = fof_ref.d2_pairs(pos, i, j)
            np.minimum.at(nn, i, d2)
            np.minimum.at(nn, j, d2)
            yield i, j
    lab = fof_ref.labels_from_pairs(n, chunks())
    return dict(labels=lab, n_flocks=len(np.unique(lab)), links=links[0], count=count.astype(np.int32), nn_d2=nn)


def _fsum3(a):
    return np.array([math.fsum(a[:, 0]), math.fsum(a[:, 1]), math.fsum(a[:, 2])])


def _norm(a):
    return np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])


def row(pos, vel):
    """The row of the group whose members are the rows of pos / vel, and the largest speed among them (for the bound
    on mean_speed).  Zeros for an empty group."""
    p, v = np.asarray(pos, np.float64).reshape(-1, 3), np.asarray(vel, np.float64).reshape(-1, 3)
    out = np.zeros(16)
    m = len(p)
    if m == 0:
        return out, 0.0
    s = _norm(v)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where((s == 0.0)[:, None], 0.0, v / s[:, None])
    fm = float(m)
    c = _fsum3(p) / fm
    su = _fsum3(u)
    r = p - c
    rho = _norm(r)
    with np.errstate(invalid="ignore", divide="ignore"):
        rh = np.where((rho == 0.0)[:, None], 0.0, r / rho[:, None])
    w = np.stack([rh[:, 1] * u[:, 2] - rh[:, 2] * u[:, 1], rh[:, 2] * u[:, 0] - rh[:, 0] * u[:, 2],
                  rh[:, 0] * u[:, 1] - rh[:, 1] * u[:, 0]], axis=1)
    sw = _fsum3(w)
    out[0] = fm
    out[1:4] = c
    out[4:7] = _fsum3(v) / fm
    out[7] = math.sqrt((su[0] * su[0] + su[1] * su[1]) + su[2] * su[2]) / fm
    out[8] = math.fsum(s) / fm
    out[9] = math.sqrt((sw[0] * sw[0] + sw[1] * sw[1]) + sw[2] * sw[2]) / fm
    out[10:13] = p.min(axis=0)
    out[13:16] = p.max(axis=0)
    return out, float(s.max())


def catalogue(pos, vel, labels, min_members=1):
    """The flocks with members >= min_members, members descending, ties by label ascending:
    dict(count, label int32, members int64, rows (count, 16), smax (count,))"""
    pos, vel = np.asarray(pos, np.float64), np.asarray(vel, np.float64)
    labels = np.asarray(labels)
    uniq, inv, members = np.unique(labels, return_inverse=True, return_counts=True)
    keep = np.nonzero(members >= min_members)[0]
    keep = keep[np.lexsort((uniq[keep], -members[keep]))]
    order = np.argsort(inv, kind="stable")
    start = np.concatenate([[0], np.cumsum(members)])
    rows, smax = np.zeros((len(keep), 16)), np.zeros(len(keep))
    for k, g in enumerate(keep):
        idx = order[start[g]:start[g + 1]]
        rows[k], smax[k] = row(pos[idx], vel[idx])
    return dict(count=len(keep), label=uniq[keep].astype(np.int32), members=members[keep].astype(np.int64), rows=rows,
                smax=smax)


EXACT = (0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 13, 14, 15)  # m, c, vbar, lo, hi: exact on the tests' dyadic lattice


def row_bounds(want_row, smax):
    """What a kernel row may differ by from `want_row`: 0 in the EXACT fields, 2 m 2^-53 for polarisation and milling,
    m 2^-53 max s_j for mean_speed (the header's terms are the restatement's bit for bit; only the order of the sums
    differs, and (m - 1) u sum|t| bounds any order)."""
    m = float(want_row[0])
    b = np.zeros(16)
    b[7] = b[9] = 2.0 * m * U
    b[8] = m * U * smax
    return b


def all_pairs_links(pos, link):
    """the dense count of linked pairs (small n only)"""
    p = np.asarray(pos, np.float64)
    i, j = np.triu_indices(len(p), 1)
    return int((fof_ref.d2_pairs(p, i, j) <= float(link) * float(link)).sum())
