"""Float64 all-pairs accelerations for a sample of rows, by the reference's pair rule.

TEST INFRASTRUCTURE.  a_i = sum over j != i of G m_j d (|d|^2 + eps^2)^(-3/2), d = x_j - x_i, where a pair
contributes only when dist_sq = |d|^2 + eps^2 exceeds eps^2 (nbody/simulation.py:260): the reference's rule for
its own leaf and for coincident bodies, which also holds at eps = 0.  For eps > 0 and distinct bodies this is
oracle.direct_forces_subset's sum; at eps = 0 that sum has 0 * inf for every coincident pair.
"""
import numpy as np


def direct_accelerations(pos, masses, rows, G, softening, chunk=1 << 15):
    """(len(rows), 3) float64 accelerations of the bodies `rows` against all bodies."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    masses = np.ascontiguousarray(masses, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.int64)
    eps2 = float(softening) * float(softening)
    p = pos[rows]
    acc = np.zeros((len(rows), 3))
    for j0 in range(0, len(pos), chunk):
        q = pos[j0:j0 + chunk]
        d = q[None, :, :] - p[:, None, :]
        dist_sq = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) + eps2
        keep = dist_sq > eps2
        keep &= rows[:, None] != np.arange(j0, j0 + len(q))[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(keep, G * masses[None, j0:j0 + len(q)] / (dist_sq * np.sqrt(dist_sq)), 0.0)
        acc += np.einsum("ij,ijk->ik", w, d)
    return acc


def pair_weights(pos, masses, rows, G, softening, chunk=1 << 15):
    """Sum over the contributing pairs of G m_j / max(|d|, eps)^3 per sample row: how strongly a row's acceleration
    reacts to an error in its pair vectors (fp32-rounded coordinates move every d by up to an ulp of |x|)."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.int64)
    eps2 = float(softening) * float(softening)
    p = pos[rows]
    out = np.zeros(len(rows))
    for j0 in range(0, len(pos), chunk):
        q = pos[j0:j0 + chunk]
        d = q[None, :, :] - p[:, None, :]
        r2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        keep = (r2 + eps2 > eps2) & (rows[:, None] != np.arange(j0, j0 + len(q))[None, :])
        with np.errstate(divide="ignore", invalid="ignore"):
            out += np.where(keep, G * np.abs(masses[None, j0:j0 + len(q)]) / np.maximum(r2, eps2) ** 1.5, 0.0).sum(1)
    return out
