"""NumPy float64 restatement of quadrupole mode (include/nbmi.h, nbmi_set_multipole).

Over the ORACLE's octree (oracle.pyref.build_octree), in the style of potential_ref.tree_potential: a frontier of
(body, node) pairs, vectorised over the bodies; a leaf is always accepted, a cell when node_size / dist < theta on
the softened distance, otherwise its children join the next frontier; the body's own leaf is skipped; a term is
applied when node_mass > 0 and dist_sq > eps^2.  With all bodies in the frontier the applied-term count is asserted
to equal the oracle's `accepted`.

An internal cell n carries P_ab = sum_j G m_j (x_j - c_n)_a (x_j - c_n)_b, summed here body by body about the cell's
own centre of mass (no differences of large sums: good to ~n 2^-53 of its own size; moving c by the 1e-13 maxabs by
which device and oracle centres differ changes P by G M dc^2, nothing).  With d = c_n - x_i, u = |d|^2 + eps^2:

    a_i   += G M d u^-3/2 + [7.5 (d^T P d) u^-7/2 - 1.5 tr P u^-5/2] d - 3 u^-5/2 (P d)
    phi_i += -G M u^-1/2 + 1/2 [tr P u^-3/2 - 3 (d^T P d) u^-5/2]

`walk` returns per body what the tests' bounds are made of (see test_gpu_quadrupole.py).
"""
import numpy as np

from potential_ref import DELTA_REL, build_tree  # noqa: F401  (build_tree re-exported)

PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))  # order of the six entries: xx yy zz xy xz yz
TOL_P_REL = 2.0 ** -20


def term(d, u, gm, P6):
    """(acceleration (k,3), potential (k,), correction q (k,3), phi correction (k,)) of applied terms: d (k,3) = c - x,
    u (k,) = |d|^2 + eps^2, gm (k,) = G M, P6 (k,6)."""
    Pd = np.stack([P6[:, 0] * d[:, 0] + P6[:, 3] * d[:, 1] + P6[:, 4] * d[:, 2],
                   P6[:, 3] * d[:, 0] + P6[:, 1] * d[:, 1] + P6[:, 5] * d[:, 2],
                   P6[:, 4] * d[:, 0] + P6[:, 5] * d[:, 1] + P6[:, 2] * d[:, 2]], axis=1)
    dPd = (d * Pd).sum(1)
    tr = P6[:, 0] + P6[:, 1] + P6[:, 2]
    q = (7.5 * dPd * u ** -3.5 - 1.5 * tr * u ** -2.5)[:, None] * d - 3.0 * (u ** -2.5)[:, None] * Pd
    a = (gm * u ** -1.5)[:, None] * d + q
    qphi = 0.5 * (tr * u ** -1.5 - 3.0 * dPd * u ** -2.5)
    phi = -gm * u ** -0.5 + qphi
    return a, phi, q, qphi


def cell_moments(nd, nn, pos, mass, G):
    """P (nn, 6) of every node of the oracle's tree about nd.com (leaves: zeros), body by body up the parent chain."""
    pos = np.asarray(pos, np.float64)
    children, leaf, body = nd.children[:nn], nd.leaf[:nn].astype(bool), nd.body[:nn]
    parent = np.full(nn, -1, dtype=np.int64)
    r, c = np.nonzero(children >= 0)
    parent[children[r, c]] = r
    P = np.zeros((nn, 6))
    lf = np.nonzero(leaf & (body >= 0))[0]
    b = body[lf].astype(np.int64)
    assert len(np.unique(b)) == len(pos), "every body sits in exactly one leaf of the oracle's tree"
    cur = parent[lf]
    gm = G * np.asarray(mass, np.float64)[b]
    x = pos[b]
    while len(cur):
        ok = cur >= 0
        cur, gm, x = cur[ok], gm[ok], x[ok]
        if not len(cur):
            break
        d = x - nd.com[cur]
        for k, (i, j) in enumerate(PAIRS):
            P[:, k] += np.bincount(cur, weights=gm * d[:, i] * d[:, j], minlength=nn)
        cur = parent[cur]
    return P


def tol_p(nd, nn, G):
    """tol_P(n) = 2^-20 G M_n (2 hs_n)^2 per node."""
    return TOL_P_REL * G * nd.mass[:nn] * (2.0 * nd.half[:nn]) ** 2


def walk(oracle, pos, mass, G, eps, theta, tree=None, rows=None, multipole="quadrupole", P=None):
    """The restatement for the bodies `rows` (default: all).  Returns a dict of per-body arrays (len(rows)):
      a (k,3), phi, terms (int, total), and the sums over the body's applied terms
      q_abs       sum |q_in|                      (Euclidean norm of the correction of a term)
      q_abs_rel   sum |q_in| maxabs / |d|          (the f32-mode rounding bound's second part)
      mono_abs    sum |G M d u^-3/2|
      mono_delta  sum 4 G M delta u^-3/2          (cells only; delta = 2e-13 maxabs: a centre of mass off by delta)
      tolp_acc    sum 36 tol_P(n) |d| u^-5/2
      phi_delta   sum G M delta / u               (cells only, as potential_ref)
      tolp_phi    sum 6 tol_P(n) u^-3/2
    """
    pos = np.ascontiguousarray(pos, np.float64)
    mass = np.ascontiguousarray(mass, np.float64)
    n = len(pos)
    nd, nn = tree if tree is not None else build_tree(oracle, pos, mass)
    rows = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    k = len(rows)
    quad = multipole == "quadrupole"
    if quad and P is None:
        P = cell_moments(nd, nn, pos, mass, G)
    tp = tol_p(nd, nn, G)
    eps2 = eps * eps
    maxabs = float(np.abs(pos).max()) if n else 0.0
    delta = DELTA_REL * maxabs
    out = {key: np.zeros(k) for key in ("phi", "q_abs", "q_abs_rel", "mono_abs", "mono_delta", "tolp_acc", "phi_delta",
                                        "tolp_phi")}
    out["a"] = np.zeros((k, 3))
    terms = 0
    com, half, nmass = nd.com[:nn], nd.half[:nn], nd.mass[:nn]
    children, body, leaf = nd.children[:nn], nd.body[:nn], nd.leaf[:nn].astype(bool)
    bi = np.arange(k, dtype=np.int64)  # index into rows
    no = np.zeros(k, dtype=np.int64)

    def add(name, idx, w):
        out[name] += np.bincount(idx, weights=w, minlength=k)

    while len(bi):
        lf = leaf[no]
        keep = ~(lf & (body[no] == rows[bi]))  # the body's own leaf
        bi, no, lf = bi[keep], no[keep], lf[keep]
        d = com[no] - pos[rows[bi]]
        dist_sq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] + eps2
        dist = np.sqrt(dist_sq)
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = lf | ((half[no] * 2.0) / dist < theta)
        app = acc & (nmass[no] > 0) & (dist_sq > eps2)
        ba, na, da, dd = bi[app], no[app], dist_sq[app], d[app]
        gm = G * nmass[na]
        cell = ~leaf[na]
        P6 = np.where(cell[:, None], P[na], 0.0) if quad else np.zeros((len(na), 6))
        a, phi, q, _ = term(dd, da, gm, P6)
        for c in range(3):
            out["a"][:, c] += np.bincount(ba, weights=a[:, c], minlength=k)
        add("phi", ba, phi)
        qn = np.sqrt((q * q).sum(1))
        dn = np.sqrt((dd * dd).sum(1))
        add("q_abs", ba, qn)
        with np.errstate(divide="ignore", invalid="ignore"):
            add("q_abs_rel", ba, np.where(qn > 0, qn * maxabs / np.where(dn > 0, dn, 1.0), 0.0))
        add("mono_abs", ba, gm * dn * da ** -1.5)
        add("mono_delta", ba[cell], 4.0 * gm[cell] * delta * da[cell] ** -1.5)
        add("phi_delta", ba[cell], gm[cell] * delta / da[cell])
        if quad:
            add("tolp_acc", ba[cell], 36.0 * tp[na[cell]] * dn[cell] * da[cell] ** -2.5)
            add("tolp_phi", ba[cell], 6.0 * tp[na[cell]] * da[cell] ** -1.5)
        terms += int(app.sum())
        op = ~acc
        ch = children[no[op]]  # (m, 8)
        bo = np.repeat(bi[op], 8)
        cf = ch.reshape(-1)
        m = cf >= 0
        bi, no = bo[m], cf[m].astype(np.int64)
    if len(rows) == n and n and np.array_equal(rows, np.arange(n)):
        _, st = oracle.compute_forces_barnes_hut(pos, mass, nd, nn, theta, G, eps, stats=True)
        assert st["dropped"] == 0, "the oracle's stack walk dropped pushes: the frontier form would visit more pairs"
        assert terms == st["accepted"], (terms, st["accepted"])
    out["terms"] = terms
    out["maxabs"] = maxabs
    return out


def bound_f64(w):
    """B_i of float64 force precision: the monopole part to rounding and to the centres' 2e-13 maxabs, the correction's
    ~30 fp32 operations from the float64 difference (32 x 2^-24), and what tol_P lets a correction move."""
    return 1e-12 * w["mono_abs"] + w["mono_delta"] + 32.0 * 2.0 ** -24 * w["q_abs"] + w["tolp_acc"]


def bound_f32(w):
    """B_i of fp32 force precision: test_accelerations' 2e-4 |a_ref| for the monopole pass, the correction's roundings
    with the fp32 coordinates' (32 + 25 maxabs / |d|) 2^-24 per term, and tol_P's share."""
    a = np.sqrt((w["a"] * w["a"]).sum(1))
    return 2e-4 * a + 2.0 ** -24 * (32.0 * w["q_abs"] + 25.0 * w["q_abs_rel"]) + w["tolp_acc"]


def bound_phi(w):
    return 1e-12 * np.abs(w["phi"]) + w["phi_delta"] + w["tolp_phi"]
