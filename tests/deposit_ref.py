"""NumPy restatement of nbmi_deposit (include/nbmi.h): the header's text, step by step, with
np.ldexp, np.rint and int64 np.add.at.  Every product and sum below is one float64 NumPy operation in the association the
header writes, so there is no FMA to avoid.  Not a test module."""
import numpy as np

NGP, CIC = 0, 1
NUMBER, MASS, MOMENTUM, KINETIC = 1, 2, 4, 8
ALL = NUMBER | MASS | MOMENTUM | KINETIC


def plane_quantities(masses, velocities, quantities):
    """The (P, N) float64 rows q of the selected planes, in the order of the bits."""
    m = np.asarray(masses, dtype=np.float64)
    v = np.asarray(velocities, dtype=np.float64).reshape(-1, 3)
    rows = []
    with np.errstate(all="ignore"):
        if quantities & NUMBER:
            rows.append(np.ones(len(m)))
        if quantities & MASS:
            rows.append(m.copy())
        if quantities & MOMENTUM:
            rows += [m * v[:, 0], m * v[:, 1], m * v[:, 2]]
        if quantities & KINETIC:
            rows.append(m * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]))
    return np.array(rows, dtype=np.float64).reshape(len(rows), len(m))


def exponents_of(q):
    """(e (P,) int32, live (P,) bool) of the rows q: e = E + L - 62 with frexp(max |q|) = (f, E), L = bit length of N;
    0 for a plane of zeros.  ValueError for a maximum that is not finite, as the library refuses it."""
    P, n = q.shape
    e, live = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=bool)
    if n == 0:
        return e, live
    L = int(n).bit_length()
    for p in range(P):
        mx = np.max(np.abs(q[p]))
        if not np.isfinite(mx):
            raise ValueError(f"plane {p}: the largest |q| is not finite")
        if mx != 0.0:
            live[p] = True
            e[p] = int(np.frexp(mx)[1]) + L - 62
    return e, live


def axis_cells(x, lo, hi, dim, cic):
    """Per body the cells and weights on one axis: a list of (floored index as float64, weight, takes part)."""
    with np.errstate(all="ignore"):
        inv = np.float64(dim) / (np.float64(hi) - np.float64(lo))
        u = (x - np.float64(lo)) * inv
        if not (cic and dim >= 2):
            i = np.floor(u)
            return [(i, np.ones_like(u), (i >= 0.0) & (i < dim))]
        s = u - 0.5
        i = np.floor(s)
        f = s - i
        i1 = i + 1.0
        return [(i, 1.0 - f, (i >= 0.0) & (i < dim)), (i1, f, (i1 >= 0.0) & (i1 < dim))]


def contributions(positions, lo, hi, dims, scheme):
    """Every (body, cell) contribution: (body index, flat cell index, weight (wx wy) wz) as three arrays, plus the mask of
    the bodies with finite coordinates.  Cell (ix, iy, iz) has the flat index (iz ny + iy) nx + ix."""
    x = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    finite = np.isfinite(x).all(axis=1)
    idx = np.nonzero(finite)[0]
    xs = x[idx]
    axes = [axis_cells(xs[:, a], lo[a], hi[a], int(dims[a]), scheme == CIC) for a in range(3)]
    bodies, cells, weights = [], [], []
    for iz, wz, okz in axes[2]:
        for iy, wy, oky in axes[1]:
            for ix, wx, okx in axes[0]:
                ok = okx & oky & okz
                if not ok.any():
                    continue
                cell = (iz[ok].astype(np.int64) * int(dims[1]) + iy[ok].astype(np.int64)) * int(dims[0]) + ix[ok].astype(np.int64)
                bodies.append(idx[ok])
                cells.append(cell)
                weights.append((wx[ok] * wy[ok]) * wz[ok])
    if not bodies:
        z = np.zeros(0, dtype=np.int64)
        return z, z, np.zeros(0), finite
    return np.concatenate(bodies), np.concatenate(cells), np.concatenate(weights), finite


def deposit(positions, velocities, masses, lo, hi, dims, scheme, quantities):
    """(out (P, nz, ny, nx) float64, stats3 int64, exponents (P,) int32): nbmi_deposit, bit for bit."""
    dims = [int(d) for d in dims]
    ncell = dims[0] * dims[1] * dims[2]
    q = plane_quantities(masses, velocities, quantities)
    P, n = q.shape
    e, live = exponents_of(q)
    body, cell, w, finite = contributions(positions, lo, hi, dims, scheme)
    K = np.zeros((P, ncell), dtype=np.int64)
    for p in range(P):
        if live[p]:
            c = q[p][body] * w
            k = np.rint(np.ldexp(c, -int(e[p]))).astype(np.int64)
            np.add.at(K[p], cell, k)
    out = np.stack([np.ldexp(K[p].astype(np.float64), int(e[p])) for p in range(P)]) if P else np.zeros((0, ncell))
    stats = np.array([len(np.unique(body)), len(body), int((~finite).sum())], dtype=np.int64)
    return out.reshape(P, dims[2], dims[1], dims[0]), stats, e


def deposit_float(positions, velocities, masses, lo, hi, dims, scheme, quantities):
    """The plain float64 np.add.at deposit of the same contributions c, and what the error bounds need:
    (sum c (P, cells), contributions per cell (cells,), sum |c| (P, cells))."""
    dims = [int(d) for d in dims]
    ncell = dims[0] * dims[1] * dims[2]
    q = plane_quantities(masses, velocities, quantities)
    body, cell, w, _ = contributions(positions, lo, hi, dims, scheme)
    S, A = np.zeros((len(q), ncell)), np.zeros((len(q), ncell))
    for p in range(len(q)):
        c = q[p][body] * w
        np.add.at(S[p], cell, c)
        np.add.at(A[p], cell, np.abs(c))
    return S, np.bincount(cell, minlength=ncell).astype(np.int64), A
