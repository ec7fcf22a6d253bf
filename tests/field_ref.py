"""NumPy float64 restatement of nbmi_field_at (include/nbmi.h): the field at arbitrary points.

direct_field: the exact sum over all bodies,  acc += d G m / (dist dist_sq),  phi -= G m / dist  with d = x_j - p,
dist_sq = |d|^2 + eps^2, applied when dist_sq > eps^2.

tree_field: the frontier form of potential_ref.tree_potential with points in place of bodies and no own-leaf filter,
over the ORACLE's octree (oracle.pyref.build_octree): a leaf is always accepted, a cell when (2 half) / dist < theta,
otherwise its children join the next frontier; an accepted node is applied when node_mass > 0 and dist_sq > eps^2.  In
quadrupole mode an applied cell carries quadrupole_ref.term's second-order terms with quadrupole_ref.cell_moments.

Error bounds, as potential_ref makes them: the device's centre of mass of a cell is good to delta = DELTA_REL maxabs
(maxabs over the bodies; the prefix sums know nothing of the probes), which moves a cell's phi term by at most
G M delta / dist_sq and its acc term by at most 2 G M delta / dist^3 (the derivative of d u^-3/2 is at most 2 u^-3/2 in
norm).  The second-order terms, part by part with |d| <= dist and the largest eigenvalue of the positive semi-definite
P at most tr P: the gradient of 1/2 [tr P u^-3/2 - 3 (d^T P d) u^-5/2] is at most 1/2 (3 + 6 + 15) tr P / dist^4, so the
phi term moves by at most 12 tr P delta / dist^4; the derivative of the acc correction is at most
(75 + 9 + 18) tr P / dist^5, so it moves by at most 102 tr P delta / dist^5.  Everything else is rounding: 1e-12 of the
summed term magnitudes, which the caller adds.
"""
import numpy as np

from potential_ref import DELTA_REL, build_tree  # noqa: F401  (build_tree re-exported)
import quadrupole_ref as qr


def direct_field(points, pos, mass, G, eps, chunk=256):
    """(acc (m,3), phi (m,), terms (m,) int, mag_acc (m,), mag_phi (m,)): the last two are the summed term magnitudes."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    gm = G * np.asarray(mass, np.float64)
    m = len(p)
    eps2 = eps * eps
    acc, phi, terms = np.zeros((m, 3)), np.zeros(m), np.zeros(m, dtype=np.int64)
    mag_a, mag_p = np.zeros(m), np.zeros(m)
    for a in range(0, m, chunk):
        b = min(m, a + chunk)
        d = pos[None, :, :] - p[a:b, None, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2] + eps2
        ok = d2 > eps2
        safe = np.where(ok, d2, 1.0)
        dist = np.sqrt(safe)
        t = np.where(ok, gm[None, :] / dist, 0.0)
        w = np.where(ok, gm[None, :] / (dist * safe), 0.0)
        phi[a:b] = -t.sum(axis=1)
        acc[a:b] = (d * w[..., None]).sum(axis=1)
        terms[a:b] = ok.sum(axis=1)
        mag_p[a:b] = np.abs(t).sum(axis=1)
        mag_a[a:b] = (np.sqrt((d * d).sum(axis=2)) * np.abs(w)).sum(axis=1)
    return acc, phi, terms, mag_a, mag_p


def tree_field(oracle, points, pos, mass, G, eps, theta, tree=None, multipole="monopole", P=None):
    """dict: acc (m,3), phi (m,), terms (m,) int, mag_acc / mag_phi (m,) the summed term magnitudes, bound_acc /
    bound_phi (m,) what the device's cell centres allow (see the module text), margin = the smallest
    |(2 half) / dist - theta| / theta over every tested (point, cell) pair (inf if none was tested)."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    pos = np.ascontiguousarray(pos, np.float64)
    mass = np.ascontiguousarray(mass, np.float64)
    m, n = len(p), len(pos)
    out = {k: np.zeros(m) for k in ("phi", "mag_acc", "mag_phi", "bound_acc", "bound_phi")}
    out["acc"] = np.zeros((m, 3))
    out["terms"] = np.zeros(m, dtype=np.int64)
    out["margin"] = np.inf
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

    def add(name, idx, w):
        out[name] += np.bincount(idx, weights=w, minlength=m)

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
        P6 = np.where(cell[:, None], P[na], 0.0) if quad else np.zeros((len(na), 6))
        # the header's association for the monopole part; the second-order parts from quadrupole_ref.term
        sq = np.sqrt(da)
        w = gm / (sq * da)
        q, qphi = np.zeros_like(dd), np.zeros(len(na))
        if quad and np.any(cell):
            _, _, q[cell], qphi[cell] = qr.term(dd[cell], da[cell], gm[cell], P6[cell])
        a = dd * w[:, None] + q
        for c in range(3):
            out["acc"][:, c] += np.bincount(ba, weights=a[:, c], minlength=m)
        add("phi", ba, -gm / sq + qphi)
        dn = np.sqrt((dd * dd).sum(1))
        qn = np.sqrt((q * q).sum(1))
        add("mag_acc", ba, w * dn + qn)
        add("mag_phi", ba, gm / sq + np.abs(qphi))
        tr = P6[:, 0] + P6[:, 1] + P6[:, 2]
        add("bound_phi", ba[cell], gm[cell] * delta / da[cell] + 12.0 * tr[cell] * delta / da[cell] ** 2)
        add("bound_acc", ba[cell], 2.0 * gm[cell] * delta / (sq[cell] * da[cell]) + 102.0 * tr[cell] * delta / (sq[cell] * da[cell] ** 2))
        out["terms"] += np.bincount(ba, minlength=m)
        op = ~acc
        ch = children[no[op]]  # (k, 8)
        bo = np.repeat(bi[op], 8)
        cf = ch.reshape(-1)
        ok = cf >= 0
        bi, no = bo[ok], cf[ok].astype(np.int64)
    return out
