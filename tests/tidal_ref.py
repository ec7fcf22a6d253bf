"""NumPy float64 restatement of nbmi_tidal_at / nbmi_get_tidal_f64 (include/nbmi.h): the tidal tensor
T_ab = da_a/dx_b = -d^2 phi / dx_a dx_b at arbitrary points, rows {Txx, Tyy, Tzz, Txy, Txz, Tyz}.

mono_term / quad_term: what one applied node adds, in the header's association operation by operation (NumPy's
elementwise *, +, -, / and sqrt are single correctly rounded float64 operations, never fused).
direct_tidal: the exact sum over all bodies of mono_term with the one guard dist_sq > eps^2.
tree_tidal: field_ref.tree_field's frontier walk over the ORACLE's octree with these terms: a leaf is always accepted, a
cell when (2 half) / dist < theta, otherwise its children join the next frontier; an accepted node is applied when
node_mass > 0 and dist_sq > eps^2; in quadrupole mode an applied cell also adds quad_term with
quadrupole_ref.cell_moments.  The accepted set, and so `terms`, is tree_field's.

mag: the sum over the applied terms of the magnitudes of their parts in Frobenius norm (|I| = sqrt 3, |d d^T| = |d|^2,
|P| <= tr P for the positive semi-definite P, |g d^T + d g^T| <= 2 |g| |d|):
    sqrt(3) |w| + |w5| |d|^2          and for a cell also      sqrt(3) |A| + |B| |d|^2 + C tr P + 2 D |g| |d|.

bound: what the device's cell centres allow, as potential_ref and field_ref make it.  The device's centre of mass of a
cell is good to delta = DELTA_REL maxabs (maxabs over the bodies), so d moves by e with |e| <= delta; a leaf's centre is
its body's position and moves by nothing.  Write r = dist; then |d| <= r, u^-k/2 <= r^-k, and to first order in e, part by
part, in Frobenius norm:

Monopole term G M [3 d d^T u^-5/2 - I u^-3/2]:
    3 (e d^T + d e^T) u^-5/2            <= 3 * 2 |d| delta / r^5                          <=  6       delta / r^4
    3 d d^T * d(u^-5/2) = -15 d d^T (d.e) u^-7/2   <= 15 |d|^3 delta / r^7               <= 15       delta / r^4
    I * d(u^-3/2) = -3 I (d.e) u^-5/2   <= 3 sqrt(3) |d| delta / r^5                      <=  3 sqrt3 delta / r^4
  sum: (6 + 3 sqrt 3 + 15) = 26.2 <= 27:          bound += 27 G M delta / r^4.

Second-order term A I + B d d^T + C P - D (g d^T + d g^T) with t = tr P, |P| <= t, |g| <= t |d|, q <= t |d|^2 and
    |d i5| = 5 |d.e| u^-7/2 <= 5 delta / r^6,  |d i7| <= 7 delta / r^8,  |d i9| <= 9 delta / r^10,
    |d q| = 2 |g.e| <= 2 t r delta,            |d g| = |P e| <= t delta:
    A = 1.5 t i5 - 7.5 q i7:    |dA| <= 1.5 t 5/r^6 + 7.5 (2 t r / r^7 + t r^2 7 / r^8) = (7.5 + 15 + 52.5) t / r^6 = 75 t / r^6
                                times |I| = sqrt 3:  129.9                                 <= 130 t delta / r^6
    B = 52.5 q i9 - 7.5 t i7:   |dB| <= 52.5 (2 t r / r^9 + t r^2 9 / r^10) + 7.5 t 7 / r^8 = (105 + 472.5 + 52.5) t / r^8
                                times |d|^2 <= r^2:  630;   |B| <= (52.5 + 7.5) t / r^7 = 60 t / r^7 times
                                |d(d d^T)| <= 2 r delta:  120                              <= 750 t delta / r^6
    C = 3 i5:                   |dC| |P| <= 15 t / r^6                                     <=  15 t delta / r^6
    D = 15 i7:                  |dD| |g d^T + d g^T| <= 105 / r^8 * 2 t r^2 = 210;  D |d(g d^T + d g^T)| <=
                                15 / r^7 * 2 (t delta r + t r delta) = 60                  <= 270 t delta / r^6
  sum: 130 + 750 + 15 + 270:                      bound += 1165 tr P delta / r^6.
Everything else is rounding: 1e-12 of mag, which the caller adds (direct handles: 1e-11 of mag and no bound).
"""
import numpy as np

from potential_ref import DELTA_REL, build_tree  # noqa: F401  (build_tree re-exported)
import quadrupole_ref as qr

SQRT3 = float(np.sqrt(3.0))
MONO_BOUND = 27.0
QUAD_BOUND = 1165.0


def mono_term(d, u, gm):
    """(t6 (k,6), mag (k,)) of applied nodes: d (k,3) = c - p, u (k,) = dist_sq, gm (k,) = G M."""
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    dist = np.sqrt(u)
    w = gm / (dist * u)
    w5 = (3.0 * w) / u
    t6 = np.stack([(dx * dx) * w5 - w, (dy * dy) * w5 - w, (dz * dz) * w5 - w,
                   (dx * dy) * w5, (dx * dz) * w5, (dy * dz) * w5], axis=1)
    mag = SQRT3 * np.abs(w) + np.abs(w5) * ((dx * dx + dy * dy) + dz * dz)
    return t6, mag


def quad_term(d, u, P6):
    """(t6 (k,6), mag (k,)) of the second-order term of applied internal cells: P6 (k,6) = {Pxx, Pyy, Pzz, Pxy, Pxz, Pyz}."""
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    pxx, pyy, pzz, pxy, pxz, pyz = (P6[:, k] for k in range(6))
    gx = (pxx * dx + pxy * dy) + pxz * dz
    gy = (pxy * dx + pyy * dy) + pyz * dz
    gz = (pxz * dx + pyz * dy) + pzz * dz
    q = (dx * (pxx * dx + 2.0 * (pxy * dy + pxz * dz)) + dy * (pyy * dy + 2.0 * (pyz * dz))) + dz * (pzz * dz)
    tr = (pxx + pyy) + pzz
    dist = np.sqrt(u)
    i5 = ((1.0 / dist) / u) / u
    i7 = i5 / u
    i9 = i7 / u
    A = (1.5 * tr) * i5 - (7.5 * q) * i7
    B = (52.5 * q) * i9 - (7.5 * tr) * i7
    C = 3.0 * i5
    D = 15.0 * i7
    t6 = np.stack([((A + B * (dx * dx)) + C * pxx) - D * (gx * dx + dx * gx),
                   ((A + B * (dy * dy)) + C * pyy) - D * (gy * dy + dy * gy),
                   ((A + B * (dz * dz)) + C * pzz) - D * (gz * dz + dz * gz),
                   (B * (dx * dy) + C * pxy) - D * (gx * dy + dx * gy),
                   (B * (dx * dz) + C * pxz) - D * (gx * dz + dx * gz),
                   (B * (dy * dz) + C * pyz) - D * (gy * dz + dy * gz)], axis=1)
    d2 = (dx * dx + dy * dy) + dz * dz
    gn = np.sqrt((gx * gx + gy * gy) + gz * gz)
    mag = SQRT3 * np.abs(A) + np.abs(B) * d2 + C * tr + 2.0 * D * gn * np.sqrt(d2)
    return t6, mag


def trace(t6):
    return (t6[:, 0] + t6[:, 1]) + t6[:, 2]


def direct_tidal(points, pos, mass, G, eps, chunk=256):
    """(t6 (m,6), terms (m,) int, mag (m,)): the exact sum over all bodies in body order."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    gm = G * np.asarray(mass, np.float64)
    m, n = len(p), len(pos)
    eps2 = eps * eps
    t6, terms, mag = np.zeros((m, 6)), np.zeros(m, dtype=np.int64), np.zeros(m)
    for a in range(0, m, chunk):
        b = min(m, a + chunk)
        d = (pos[None, :, :] - p[a:b, None, :]).reshape(-1, 3)
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] + eps2
        ok = d2 > eps2
        t, g = mono_term(d, np.where(ok, d2, 1.0), np.tile(gm, b - a))
        t6[a:b] = np.where(ok[:, None], t, 0.0).reshape(b - a, n, 6).sum(axis=1)
        mag[a:b] = np.where(ok, g, 0.0).reshape(b - a, n).sum(axis=1)
        terms[a:b] = ok.reshape(b - a, n).sum(axis=1)
    return t6, terms, mag


def tree_tidal(oracle, points, pos, mass, G, eps, theta, tree=None, multipole="monopole", P=None):
    """dict: t6 (m,6), terms (m,) int, mag (m,) the summed term magnitudes, bound (m,) what the device's cell centres
    allow (see the module text), margin = the smallest |(2 half) / dist - theta| / theta over every tested (point, cell)
    pair (inf if none was tested)."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    pos = np.ascontiguousarray(pos, np.float64)
    mass = np.ascontiguousarray(mass, np.float64)
    m, n = len(p), len(pos)
    out = {"t6": np.zeros((m, 6)), "terms": np.zeros(m, dtype=np.int64), "mag": np.zeros(m), "bound": np.zeros(m),
           "margin": np.inf}
    if n == 0 or m == 0:
        return out
    nd, nn = tree if tree is not None else build_tree(oracle, pos, mass)
    quad = multipole == "quadrupole"
    if quad and P is None:
        P = qr.cell_moments(nd, nn, pos, mass, G)
    eps2 = eps * eps
    delta = DELTA_REL * float(np.abs(pos).max())
    com, half, nmass = nd.com[:nn], nd.half[:nn], nd.mass[:nn]
    children, leaf = nd.children[:nn], nd.leaf[:nn].astype(bool)
    bi = np.arange(m, dtype=np.int64)
    no = np.zeros(m, dtype=np.int64)
    while len(bi):
        lf = leaf[no]
        d = com[no] - p[bi]
        dist_sq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] + eps2
        dist = np.sqrt(dist_sq)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = (half[no] * 2.0) / dist
            acc = lf | (ratio < theta)
        if theta > 0 and np.any(~lf):
            out["margin"] = min(out["margin"], float((np.abs(ratio[~lf] - theta) / theta).min()))
        app = acc & (nmass[no] > 0) & (dist_sq > eps2)
        ba, na, da, dd = bi[app], no[app], dist_sq[app], d[app]
        gm = G * nmass[na]
        cell = ~leaf[na]
        t, mag = mono_term(dd, da, gm)
        bound = np.where(cell, MONO_BOUND * gm * delta / (da * da), 0.0)
        if quad and np.any(cell):
            Pc = P[na[cell]]
            tq, mq = quad_term(dd[cell], da[cell], Pc)
            t[cell] += tq
            mag[cell] += mq
            bound[cell] += QUAD_BOUND * ((Pc[:, 0] + Pc[:, 1]) + Pc[:, 2]) * delta / da[cell] ** 3
        for c in range(6):
            out["t6"][:, c] += np.bincount(ba, weights=t[:, c], minlength=m)
        out["mag"] += np.bincount(ba, weights=mag, minlength=m)
        out["bound"] += np.bincount(ba, weights=bound, minlength=m)
        out["terms"] += np.bincount(ba, minlength=m)
        op = ~acc
        ch = children[no[op]]  # (k, 8)
        bo = np.repeat(bi[op], 8)
        cf = ch.reshape(-1)
        ok = cf >= 0
        bi, no = bo[ok], cf[ok].astype(np.int64)
    return out


def error(t6, ref):
    """(m,) Frobenius norm of the symmetric matrix of the difference of two sets of rows"""
    e = np.asarray(t6) - np.asarray(ref)
    return np.sqrt(((e[:, 0] ** 2 + e[:, 1] ** 2) + e[:, 2] ** 2) + 2.0 * ((e[:, 3] ** 2 + e[:, 4] ** 2) + e[:, 5] ** 2))
