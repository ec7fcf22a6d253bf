"""NumPy restatement of nbmi_radial_profile and nbmi_mass_radii (include/nbmi.h): the header's
text, step by step, with elementwise float64 operations in the association the header writes (so there is no FMA to
avoid), np.rint(np.ldexp(...)), int64 / Python-integer sums and a stable sort for the selection.  Not a test module."""
import math

import numpy as np

NUMBER, MASS, RADIAL_MOMENTUM, RADIAL_KINETIC, KINETIC, ANGULAR_MOMENTUM = 1, 2, 4, 8, 16, 32
ALL = 63
SINGLE = (NUMBER, MASS, RADIAL_MOMENTUM, RADIAL_KINETIC, KINETIC, ANGULAR_MOMENTUM)
PLANES_OF = {NUMBER: [0], MASS: [1], RADIAL_MOMENTUM: [2], RADIAL_KINETIC: [3], KINETIC: [4], ANGULAR_MOMENTUM: [5, 6, 7]}
PLANE_NAMES = ("NUMBER", "MASS", "RADIAL_MOMENTUM", "RADIAL_KINETIC", "KINETIC", "ANGULAR_MOMENTUM x",
               "ANGULAR_MOMENTUM y", "ANGULAR_MOMENTUM z")


def planes_of(quantities):
    """indices into the eight quantities of the planes that ``quantities`` selects, in the order of the bits"""
    return [p for q in SINGLE if quantities & q for p in PLANES_OF[q]]


def squared_edges(edges):
    """E[k] = edges[k] * edges[k]; ValueError where the library refuses"""
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    nb = len(e) - 1
    if not 1 <= nb <= 256:
        raise ValueError(f"nb = {nb} is outside 1 .. 256")
    for k in range(nb + 1):
        if not np.isfinite(e[k]) or e[k] < 0.0 or (k > 0 and not e[k] > e[k - 1]):
            raise ValueError(f"edges[{k}] = {e[k]}: the edges must be finite, >= 0 and strictly increasing")
    with np.errstate(all="ignore"):
        E = e * e
    for k in range(nb + 1):
        if not np.isfinite(E[k]) or (k > 0 and not E[k] > E[k - 1]):
            raise ValueError(f"the square of edges[{k}] = {e[k]} is not finite or not above the one before it")
    return E


def radii2(positions, center):
    """(rx, ry, rz, r2) per body: r = x - c, r2 = (rx rx + ry ry) + rz rz"""
    x = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    c = np.asarray(center, dtype=np.float64).reshape(3)
    with np.errstate(all="ignore"):
        rx, ry, rz = x[:, 0] - c[0], x[:, 1] - c[1], x[:, 2] - c[2]
        r2 = (rx * rx + ry * ry) + rz * rz
    return rx, ry, rz, r2


def body_quantities(positions, velocities, masses, center, bulk_velocity):
    """(q (8, N), r2 (N,)): the eight quantities of every body (the rows of skipped bodies mean nothing)"""
    rx, ry, rz, r2 = radii2(positions, center)
    v = np.asarray(velocities, dtype=np.float64).reshape(-1, 3)
    m = np.asarray(masses, dtype=np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        if bulk_velocity is None:
            wx, wy, wz = v[:, 0].copy(), v[:, 1].copy(), v[:, 2].copy()
        else:
            b = np.asarray(bulk_velocity, dtype=np.float64).reshape(3)
            wx, wy, wz = v[:, 0] - b[0], v[:, 1] - b[1], v[:, 2] - b[2]
        rho = np.sqrt(r2)
        dot = (rx * wx + ry * wy) + rz * wz
        vr = np.where(rho == 0.0, 0.0, dot / np.where(rho == 0.0, 1.0, rho))
        w2 = (wx * wx + wy * wy) + wz * wz
        mvr = m * vr
        q = np.array([np.ones(len(m)), m, mvr, mvr * vr, m * w2,
                      m * (ry * wz - rz * wy), m * (rz * wx - rx * wz), m * (rx * wy - ry * wx)], dtype=np.float64)
    return q.reshape(8, len(m)), r2


def radial_profile(positions, velocities, masses, center, bulk_velocity, edges, quantities):
    """(out (P, nb + 1) float64, stats3 int64, exponents (P,) int32): nbmi_radial_profile, bit for bit.  ValueError where
    the library refuses."""
    if quantities == 0 or quantities & ~ALL:
        raise ValueError(f"quantities = {quantities} selects nothing or has unknown bits")
    if not np.isfinite(np.asarray(center, dtype=np.float64)).all():
        raise ValueError("center is not finite")
    if bulk_velocity is not None and not np.isfinite(np.asarray(bulk_velocity, dtype=np.float64)).all():
        raise ValueError("bulk_velocity is not finite")
    E = squared_edges(edges)
    nb = len(E) - 1
    q, r2 = body_quantities(positions, velocities, masses, center, bulk_velocity)
    n = q.shape[1]
    sel = planes_of(quantities)
    take = np.isfinite(r2)
    slot = (E[None, :] < r2[:, None]).sum(axis=1)  # the number of k with E[k] < r2
    inside = take & (slot <= nb)
    out = np.zeros((len(sel), nb + 1), dtype=np.float64)
    ex = np.zeros(len(sel), dtype=np.int32)
    L = int(n).bit_length()
    for row, p in enumerate(sel):
        mx = np.max(np.abs(q[p][take])) if take.any() else 0.0
        if not np.isfinite(mx):
            raise ValueError(f"the largest |q| of plane {row} ({PLANE_NAMES[p]}) is not finite")
        if mx == 0.0:
            continue
        e = int(np.frexp(mx)[1]) + L - 62
        k = np.rint(np.ldexp(q[p][inside], -e)).astype(np.int64)
        K = np.zeros(nb + 1, dtype=np.int64)
        np.add.at(K, slot[inside], k)
        out[row] = np.ldexp(K.astype(np.float64), e)
        ex[row] = e
    stats = np.array([int(inside.sum()), int((take & (slot > nb)).sum()), int((~take).sum())], dtype=np.int64)
    return out, stats, ex


def profile_float(positions, velocities, masses, center, bulk_velocity, edges, quantities):
    """What the error bound needs, per selected plane and slot: (sum |q| (P, nb + 1), bodies per slot (nb + 1,))."""
    E = squared_edges(edges)
    nb = len(E) - 1
    q, r2 = body_quantities(positions, velocities, masses, center, bulk_velocity)
    take = np.isfinite(r2)
    slot = (E[None, :] < r2[:, None]).sum(axis=1)
    inside = take & (slot <= nb)
    sel = planes_of(quantities)
    A = np.zeros((len(sel), nb + 1))
    for row, p in enumerate(sel):
        np.add.at(A[row], slot[inside], np.abs(q[p][inside]))
    return A, np.bincount(slot[inside], minlength=nb + 1).astype(np.int64)


def mass_quantum(masses):
    """(e, k (N,) int64): e = Ex + L - 53 from the largest mass (0 when it is 0 or N == 0), k = rint(ldexp(m, -e)).
    ValueError for a mass that is negative or not finite."""
    m = np.asarray(masses, dtype=np.float64).reshape(-1)
    if len(m) == 0:
        return 0, np.zeros(0, dtype=np.int64)
    if not np.isfinite(m).all():
        raise ValueError("a mass is not finite")
    if (m < 0.0).any():
        raise ValueError("a mass is negative")
    mx = np.max(m)
    if mx == 0.0:
        return 0, np.zeros(len(m), dtype=np.int64)
    e = int(np.frexp(mx)[1]) + int(len(m)).bit_length() - 53
    return e, np.rint(np.ldexp(m, -e)).astype(np.int64)


def thresholds(fractions, k_total):
    f = np.asarray(fractions, dtype=np.float64).reshape(-1)
    if not 1 <= len(f) <= 64:
        raise ValueError(f"nf = {len(f)} is outside 1 .. 64")
    for i, x in enumerate(f):
        if not np.isfinite(x) or not x > 0.0 or x > 1.0:
            raise ValueError(f"fractions[{i}] = {x} is not in (0, 1]")
    return [max(1, int(math.ceil(float(x * np.float64(k_total))))) for x in f]


def mass_radii(positions, masses, center, fractions):
    """(radius2 (nf,), inside (nf,) int64, mass_inside (nf,), total_mass, stats2 int64, exponent): nbmi_mass_radii, bit
    for bit: a stable sort by r2, the cumulative integer masses, and per fraction the first tie run whose cumulative
    value reaches T."""
    if not np.isfinite(np.asarray(center, dtype=np.float64)).all():
        raise ValueError("center is not finite")
    thresholds(fractions, 0)  # (the argument checks come before the masses')
    _, _, _, r2 = radii2(positions, center)
    e, k = mass_quantum(masses)
    take = np.isfinite(r2)
    stats = np.array([int(take.sum()), int((~take).sum())], dtype=np.int64)
    r2t, kt = r2[take], k[take]
    order = np.argsort(r2t, kind="stable")
    rs, ks = r2t[order], kt[order]
    C = np.cumsum(ks, dtype=np.int64)
    k_total = int(C[-1]) if len(C) else 0
    nf = len(np.asarray(fractions).reshape(-1))
    radius2, inside, mass = np.full(nf, np.nan), np.zeros(nf, dtype=np.int64), np.zeros(nf)
    if k_total > 0:
        last = np.nonzero(np.append(rs[1:] != rs[:-1], True))[0]  # the last entry of every tie run
        c_run = C[last]
        for i, T in enumerate(thresholds(fractions, k_total)):
            j = int(np.searchsorted(c_run, T, side="left"))  # the first run with C_run >= T
            radius2[i], inside[i], mass[i] = rs[last[j]], last[j] + 1, np.ldexp(np.float64(c_run[j]), e)
    return radius2, inside, mass, float(np.ldexp(np.float64(k_total), e)), stats, e
