"""Plain NumPy float64 restatement of the noise of include/bdmi.h ("Noise"), on tests/icgen_ref.py's Philox4x32-10.
TEST INFRASTRUCTURE ONLY.

    vectors()         xi_i(step) for the ids i, with the attempt and the pair each was accepted at
    kick()            A * xi with A = eta * max_force (one product)
    physics_walled()  boids_ref.physics with the kick added to ((sep + ali) + coh) ahead of the wall terms
"""
import numpy as np

import boids_ref as R
from icgen_ref import philox4x32_10

SCALE = 2.0 ** -31


def counters(ids, step, attempt):
    """(n, 4) uint32: {i, (uint32)step, (uint32)(step >> 32), a}."""
    ids = np.asarray(ids, dtype=np.int64)
    c = np.empty((len(ids), 4), dtype=np.uint32)
    c[:, 0] = ids.astype(np.uint32)
    c[:, 1] = np.uint32(step & 0xFFFFFFFF)
    c[:, 2] = np.uint32((step >> 32) & 0xFFFFFFFF)
    c[:, 3] = np.asarray(attempt).astype(np.uint32)
    return c


def key(seed):
    return np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)


def vectors(seed, step, ids):
    """xi (n, 3) float64, attempt (n,) and pair (n,) int64 of the accepted draw."""
    ids = np.asarray(ids, dtype=np.int64)
    n = len(ids)
    xi = np.zeros((n, 3))
    attempt = np.full(n, -1, dtype=np.int64)
    pair = np.full(n, -1, dtype=np.int64)
    todo = np.arange(n)
    a = 0
    while len(todo):
        w = philox4x32_10(counters(ids[todo], step, np.full(len(todo), a)), key(seed)[None, :])
        open_ = np.ones(len(todo), dtype=bool)
        for pr in (0, 1):
            x1 = (w[:, 2 * pr].astype(np.float64) + 0.5) * SCALE - 1.0
            x2 = (w[:, 2 * pr + 1].astype(np.float64) + 0.5) * SCALE - 1.0
            s = x1 * x1 + x2 * x2
            acc = open_ & (s < 1.0)
            t = np.sqrt(1.0 - s[acc])
            rows = todo[acc]
            xi[rows, 0] = (2.0 * x1[acc]) * t
            xi[rows, 1] = (2.0 * x2[acc]) * t
            xi[rows, 2] = 1.0 - 2.0 * s[acc]
            attempt[rows] = a
            pair[rows] = pr
            open_ &= ~acc
        todo = todo[open_]
        a += 1
    return xi, attempt, pair


def kick(params, eta, seed, step, n):
    """A * xi_i(step) for i = 0 .. n - 1, A = eta * max_force."""
    A = float(eta) * R.unpack(params)["max_force"]
    return A * vectors(seed, step, np.arange(n))[0]


def physics_walled(pos, vel, col, forces, params, dt, kick=None):
    """boids_ref.physics, the kick between the three forces and the wall terms."""
    P = R.unpack(params)
    sep, ali, coh, avg = (np.asarray(f, dtype=np.float64) for f in forces)
    pos, vel, col = (np.asarray(a, dtype=np.float64) for a in (pos, vel, col))
    margin, bounds = P["wall_margin"], P["bounds"]
    wall = P["max_force"] * P["wall_weight"]
    acc = (sep + ali) + coh
    if kick is not None:
        acc = acc + kick
    dist_pos = pos - (bounds - margin)
    k = dist_pos > 0
    acc[k] -= np.minimum(dist_pos[k] / margin * 2.0, 1.0) * wall
    dist_neg = (-bounds + margin) - pos
    k = dist_neg > 0
    acc[k] += np.minimum(dist_neg[k] / margin * 2.0, 1.0) * wall
    nv = vel + acc * dt
    speed = np.sqrt(nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1] + nv[:, 2] * nv[:, 2])
    k = speed > P["max_speed"]
    nv[k] *= (P["max_speed"] / speed[k])[:, None]
    blend = P["color_blend_rate"] * dt
    blend = blend if blend < 1.0 else 1.0
    return pos + nv * dt, nv, col + (avg - col) * blend
