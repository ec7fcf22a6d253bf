"""NumPy restatement of the k-nearest-neighbour query and the density colours (include/nbmi.h, nbmi_knn /
nbmi_set_color_mode).  Brute force over all pairs, float64, the header's association:

    d2(i, j) = (dx dx + dy dy) + dz dz,  dx = x_j - x_i

NumPy evaluates `a * a + b * b` as two rounded products and a rounded sum (no FMA), so the values are the header's bit
for bit.  r2_k is the k-th smallest of {d2(i, j) : j != i} with multiplicity (self removed by index, not by value),
mass_k = m_i + the masses at d2 <= r2_k, rho = mass_k / (4/3 pi r_k^3) and +inf at r2_k == 0.
"""
import numpy as np

SPHERE = 4.1887902047863905  # 4/3 pi as the header spells it


def d2_rows(p, rows):
    """(len(rows), N) float64 matrix of d2(i, j) for i in rows"""
    p = np.asarray(p, np.float64)
    d2 = p[None, :, 0] - p[rows, None, 0]
    np.multiply(d2, d2, out=d2)
    for a in (1, 2):  # (dx dx + dy dy) + dz dz, each product and sum rounded once
        t = p[None, :, a] - p[rows, None, a]
        np.multiply(t, t, out=t)
        d2 += t
    return d2


def knn_many(p, m, ks, chunk=None):
    """{k: (r2_k, mass_k)} of every body for all k of `ks` from one pass over the pairs, chunked over rows so that a
    (chunk, N) matrix stays near 2 MiB.  Only the max(ks) smallest entries of a row are kept and sorted; mass_k is summed
    over them, and over the whole row where entries equal to r2_k may lie beyond the kept ones (ties at the last)."""
    p = np.ascontiguousarray(p, np.float64)
    m = np.ascontiguousarray(m, np.float64)
    n = len(p)
    ks = sorted(set(int(k) for k in ks))
    assert ks and 1 <= ks[0] and ks[-1] <= n - 1
    if chunk is None:
        chunk = max(1, min(n, (1 << 18) // max(n, 1)))
    keep = ks[-1]
    out = {k: (np.empty(n), np.empty(n)) for k in ks}
    for r0 in range(0, n, chunk):
        rows = np.arange(r0, min(n, r0 + chunk))
        d2 = d2_rows(p, rows)
        d2[np.arange(len(rows)), rows] = np.inf  # self, by identity (d2 <= r2_k is then false for it: r2_k is finite)
        idx = np.argpartition(d2, keep - 1, axis=1)[:, :keep]
        val = np.take_along_axis(d2, idx, axis=1)
        order = np.argsort(val, axis=1, kind="stable")
        idx, val = np.take_along_axis(idx, order, axis=1), np.take_along_axis(val, order, axis=1)
        for k in ks:
            r2 = val[:, k - 1]
            mk = m[rows] + np.where(val <= r2[:, None], m[idx], 0.0).sum(axis=1)
            for i in np.nonzero(r2 == val[:, -1])[0]:
                mk[i] = m[rows[i]] + m[d2[i] <= r2[i]].sum()
            out[k][0][rows] = r2
            out[k][1][rows] = mk
    return out


def knn(p, m, k, chunk=None):
    """(r2_k, mass_k) of every body"""
    return knn_many(p, m, [k], chunk)[k]


def knn_naive(p, m, k):
    """the definition as a double loop (small n only)"""
    n = len(p)
    r2 = np.empty(n)
    mk = np.empty(n)
    for i in range(n):
        d = []
        for j in range(n):
            if j == i:
                continue
            dx, dy, dz = p[j][0] - p[i][0], p[j][1] - p[i][1], p[j][2] - p[i][2]
            d.append(((dx * dx + dy * dy) + dz * dz, j))
        d.sort()
        r2[i] = d[k - 1][0]
        mk[i] = m[i] + sum(m[j] for dd, j in d if dd <= r2[i])
    return r2, mk


def density(r2, mk):
    r2 = np.asarray(r2, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.asarray(mk, np.float64) / (SPHERE * (r2 * np.sqrt(r2)))
    return np.where(r2 == 0.0, np.inf, rho)


# the colour ramp as a function of t in [0, 1] (csrc/nbmi.hip color_ramp_t; the reference's compute_colors_by_velocity
# with t = speed / max_speed): breakpoints and the pieces between them
BREAKPOINTS = (0.15, 0.30, 0.30 + 0.25 * 0.6, 0.55, 0.90, 0.95, 0.99)


def ramp(t):
    """(..., 3) float64 colours of t (clamped to [0, 1] by the callers)"""
    t = np.asarray(t, np.float64)
    out = np.empty(t.shape + (3,))
    flat = out.reshape(-1, 3)
    for i, x in enumerate(t.reshape(-1)):
        if x < 0.55:
            if x < 0.15:
                s = x / 0.15
                c = (0.4 - 0.2 * s, 0.2 + 0.2 * s, 0.8 + 0.1 * s)
            elif x < 0.30:
                s = (x - 0.15) / 0.15
                c = (0.2 + 0.1 * s, 0.4 + 0.1 * s, 0.9 + 0.05 * s)
            else:
                s = (x - 0.30) / 0.25
                if s < 0.6:
                    s2 = s / 0.6
                    c = (0.3 - 0.1 * s2, 0.5 + 0.3 * s2, 0.95 + 0.05 * s2)
                else:
                    s2 = (s - 0.6) / 0.4
                    c = (0.2 + 0.8 * s2, 0.8 + 0.2 * s2, 1.0)
        elif x < 0.90:
            c = (1.0, 1.0, 1.0)
        elif x < 0.95:
            s = (x - 0.90) / 0.05
            c = (1.0, 1.0 - 0.05 * s, 1.0 - 1.0 * s)
        elif x < 0.99:
            s = (x - 0.95) / 0.04
            c = (1.0, 0.95 - 0.45 * s, 0.0)
        else:
            s = (x - 0.99) / 0.01
            c = (1.0, 0.5 - 0.5 * s, 0.0)
        flat[i] = c
    return out


def density_t(rho, lo, hi):
    with np.errstate(divide="ignore"):
        t = (np.log10(np.asarray(rho, np.float64)) - lo) / (hi - lo)
    return np.clip(t, 0.0, 1.0)


def density_colors(rho, lo, hi):
    """float64 (N, 3): what nbmi_compute_colors stores as float32 in density mode"""
    return ramp(density_t(rho, lo, hi))


def default_log10_range(rho):
    """the recorder's default range: 1st percentile of the finite log10 rho, 99.9th percentile plus one decade"""
    rho = np.asarray(rho, np.float64)
    lg = np.log10(rho[np.isfinite(rho) & (rho > 0.0)])
    return float(np.percentile(lg, 1.0)), float(np.percentile(lg, 99.9)) + 1.0
