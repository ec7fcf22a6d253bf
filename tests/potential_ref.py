"""NumPy float64 restatement of the potential of include/nbmi.h (nbmi_diagnostics).

direct_potential: phi_i = -sum_{j != i} G m_j / sqrt(|x_j - x_i|^2 + eps^2); eps == 0 skips pairs at zero distance.

tree_potential: the same sum over exactly the terms the reference's walk applies to body i (nbody/simulation.py:245-262),
over the ORACLE's octree (oracle.pyref.build_octree).  The walk is a frontier of (body, node) pairs, vectorised over the
bodies: a leaf is always accepted, a cell when node_size / dist < theta, otherwise its children join the next frontier;
the body's own leaf is skipped; a term is applied when node_mass > 0 and dist_sq > eps^2.  The reference's 64-entry
stack can drop pushes, which this breadth-first form does not; tree_potential asserts that the oracle's own walk
dropped none for the input, so both forms visit the same (body, node) pairs.

Per applied CELL term the restatement also returns the error the device's moments allow: the double-double prefix
sums give a cell's centre of mass to ~1e-13 of the largest coordinate, so a term may move by
G M_n delta / dist_sq with delta = 2e-13 maxabs.
"""
import numpy as np

DELTA_REL = 2e-13


def direct_potential(pos, mass, G, eps, chunk=512):
    pos = np.asarray(pos, np.float64)
    gm = G * np.asarray(mass, np.float64)
    n = len(pos)
    eps2 = eps * eps
    phi = np.zeros(n)
    terms = 0
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        d = pos[None, :, :] - pos[a:b, None, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2] + eps2
        ok = d2 > 0.0
        ok[np.arange(b - a), np.arange(a, b)] = False
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(ok, gm[None, :] / np.sqrt(np.where(ok, d2, 1.0)), 0.0)
        phi[a:b] = -t.sum(axis=1)
        terms += int(ok.sum())
    return phi, terms


def build_tree(oracle, pos, mass):
    pos = np.ascontiguousarray(pos, np.float64)
    mass = np.ascontiguousarray(mass, np.float64)
    b = oracle.compute_bounds(pos)
    nd = oracle.NodeArrays.for_bodies(len(pos), max(8192, 4 * len(pos)))
    nn = oracle.build_octree(pos, mass, b, nd)
    return nd, nn


def tree_potential(oracle, pos, mass, G, eps, theta, tree=None):
    """(phi, applied terms, per-body error bound) of the tree potential at `theta` over the oracle's octree."""
    pos = np.ascontiguousarray(pos, np.float64)
    mass = np.ascontiguousarray(mass, np.float64)
    n = len(pos)
    nd, nn = tree if tree is not None else build_tree(oracle, pos, mass)
    _, st = oracle.compute_forces_barnes_hut(pos, mass, nd, nn, theta, G, eps, stats=True)
    assert st["dropped"] == 0, "the oracle's stack walk dropped pushes: the frontier form would visit more pairs"
    eps2 = eps * eps
    delta = DELTA_REL * float(np.abs(pos).max()) if n else 0.0
    phi = np.zeros(n)
    bound = np.zeros(n)
    terms = 0
    com, half, nmass = nd.com[:nn], nd.half[:nn], nd.mass[:nn]
    children, body, leaf = nd.children[:nn], nd.body[:nn], nd.leaf[:nn].astype(bool)
    bi = np.arange(n, dtype=np.int64)
    no = np.zeros(n, dtype=np.int64)
    while len(bi):
        lf = leaf[no]
        keep = ~(lf & (body[no] == bi))  # the body's own leaf
        bi, no, lf = bi[keep], no[keep], lf[keep]
        dx = com[no, 0] - pos[bi, 0]
        dy = com[no, 1] - pos[bi, 1]
        dz = com[no, 2] - pos[bi, 2]
        dist_sq = dx * dx + dy * dy + dz * dz + eps2
        dist = np.sqrt(dist_sq)
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = lf | ((half[no] * 2.0) / dist < theta)
        app = acc & (nmass[no] > 0) & (dist_sq > eps2)
        ba, na, da = bi[app], no[app], dist_sq[app]
        gm = G * nmass[na]
        phi -= np.bincount(ba, weights=gm / np.sqrt(da), minlength=n)
        cell = ~leaf[na]
        bound += np.bincount(ba[cell], weights=gm[cell] * delta / da[cell], minlength=n)
        terms += int(app.sum())
        op = ~acc
        ch = children[no[op]]  # (k, 8)
        bo = np.repeat(bi[op], 8)
        cf = ch.reshape(-1)
        m = cf >= 0
        bi, no = bo[m], cf[m].astype(np.int64)
    assert terms == st["accepted"], (terms, st["accepted"])
    return phi, terms, bound


def sums(pos, vel, mass):
    """M, c, P, L, K, and sum m|v| (the momentum scale of the drift figures) in float64."""
    pos, vel, mass = (np.asarray(a, np.float64) for a in (pos, vel, mass))
    M = mass.sum()
    c = (mass[:, None] * pos).sum(0) / M if M else np.zeros(3)
    P = (mass[:, None] * vel).sum(0)
    L = (mass[:, None] * np.cross(pos, vel)).sum(0)
    K = 0.5 * (mass * (vel * vel).sum(1)).sum()
    mv = (mass * np.sqrt((vel * vel).sum(1))).sum()
    mxv = (mass * np.sqrt((pos * pos).sum(1)) * np.sqrt((vel * vel).sum(1))).sum()
    return dict(M=M, c=c, P=P, L=L, K=K, mv=mv, mxv=mxv)
