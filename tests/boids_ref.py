"""Plain NumPy float64 restatement of one boids step, with no cell grid: the all-pairs reference
of the sweep kernel (csrc/bdmi.hip `k_flock`).  TEST INFRASTRUCTURE ONLY.

    flocking()  compute_flocking_spatial (reference boids/flock.py:68-238, oracle/bdref.c:66-187)
    physics()   update_physics (flock.py:241-308, bdref.c:189-218), blend = min(1, rate * dt)

Neighbours are found by distance alone.  That gives exactly the grid's neighbour set for every
input: the grid's cell size equals the perception radius p, and the cell of a coordinate is
int((x + offset) / p) clamped to [0, dim - 1].  Two boids closer than p differ by less than p in
each coordinate, so their unclamped cell coordinates differ by at most one; clamping maps both
to the border cell or leaves them one apart, never further.  So every pair within p sits in
adjacent cells, the grid's 27-cell candidate set contains every neighbour, and the distance
test (the same expression on both sides) decides the rest: the cell-based neighbour set is the
all-pairs set.

Candidate search: boids sorted by x; a chunk of queries (sorted by x too) takes the candidates
whose x lies within p of the chunk's x range (slightly widened: dropping a boid here is only
safe when |dx| >= p, where the squared distance, a sum of non-negative rounded terms, cannot be
below the rounded p^2).

Per boid the sums run in an order of NumPy's choosing.  The separation sum's absolute sum
(`sep_abs`) is returned for the conditioning bound `sep_bound`.
"""
import numpy as np

U = 2.0 ** -53  # unit roundoff of float64

_KEYS = ["bounds", "wall_margin", "wall_weight", "max_speed", "max_force", "perception_radius",
         "separation_radius", "separation_weight", "alignment_weight", "cohesion_weight", "color_blend_rate"]


def unpack(params):
    return dict(zip(_KEYS, (float(x) for x in params)))


def grid(params):
    """Flock.__init__'s grid (flock.py:478-481): cell size, dimension, offset."""
    P = unpack(params)
    cell = P["perception_radius"]
    return cell, int(np.ceil(P["bounds"] * 2 / cell)) + 2, P["bounds"] + cell


def cell_coords(pos, params):
    """get_cell_index (flock.py:16-27) per axis: int() truncates toward zero, then clamp."""
    cell, dim, offset = grid(params)
    c = np.trunc((np.asarray(pos, dtype=np.float64) + offset) / cell)
    c = np.clip(c, -1, dim)  # keeps far-away values inside int64 before the real clamp
    return np.clip(c.astype(np.int64), 0, dim - 1)


def cell_index(pos, params):
    """The cell id cx + cy dim + cz dim^2, in int64 (the kernel's int32 must equal it)."""
    _, dim, _ = grid(params)
    c = cell_coords(pos, params)
    return c[:, 0] + c[:, 1] * dim + c[:, 2] * dim * dim


def _steer(x, v, max_speed, max_force, w):
    """steer() of bdmi.hip / the repeated block of flock.py:174-234, row-wise; rows whose
    magnitude is 0 give 0.  Same operation order as the kernel (no fused operations)."""
    out = np.zeros_like(x)
    mag = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
    ok = mag > 0
    y = (x[ok] / mag[ok, None]) * max_speed - v[ok]
    m2 = np.sqrt(y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1] + y[:, 2] * y[:, 2])
    cl = m2 > max_force
    y[cl] = (y[cl] / m2[cl, None]) * max_force
    out[ok] = y * w
    return out


class Forces:
    """Per query boid: sep, ali, coh, avg (n, 3); nb and nsep (neighbour and separation counts);
    sep_sum / sep_abs (the raw sum of the separation terms and the sum of their absolute values)."""

    def __init__(self, nq):
        self.sep = np.zeros((nq, 3))
        self.ali = np.zeros((nq, 3))
        self.coh = np.zeros((nq, 3))
        self.avg = np.zeros((nq, 3))
        self.nb = np.zeros(nq, dtype=np.int64)
        self.nsep = np.zeros(nq, dtype=np.int64)
        self.sep_sum = np.zeros((nq, 3))
        self.sep_abs = np.zeros((nq, 3))


def flocking(pos, vel, col, params, query=None, chunk=128):
    """compute_flocking_spatial for the boids `query` (default: all), all-pairs by distance.
    Returns a Forces whose rows follow `query`."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    vel = np.ascontiguousarray(vel, dtype=np.float64)
    col = np.ascontiguousarray(col, dtype=np.float64)
    P = unpack(params)
    n = len(pos)
    query = np.arange(n) if query is None else np.asarray(query, dtype=np.int64)
    nq = len(query)
    ps, ss = P["perception_radius"] ** 2, P["separation_radius"] ** 2
    reach = P["perception_radius"] * (1 + 1e-9) + 1e-12
    order = np.argsort(pos[:, 0], kind="stable")
    xs = pos[order, 0]
    qorder = np.argsort(pos[query, 0], kind="stable")  # rows of `query`, by x
    sums = np.zeros((nq, 15))  # ali 3, coh 3, colour 3, sep 3, |sep| 3
    nb = np.zeros(nq, dtype=np.int64)
    nsep = np.zeros(nq, dtype=np.int64)
    for s in range(0, nq, chunk):
        rows = qorder[s:s + chunk]
        qi = query[rows]
        qx = pos[qi, 0]
        lo = np.searchsorted(xs, qx.min() - reach, "left")
        hi = np.searchsorted(xs, qx.max() + reach, "right")
        cand = order[lo:hi]
        # dx = p_i - p_j and dist_sq = (dx^2 + dy^2) + dz^2, as the kernel writes them
        d = [pos[qi, k][:, None] - pos[cand, k][None, :] for k in range(3)]
        dist_sq = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        hit = (dist_sq < ps) & (dist_sq > 0.0001) & (qi[:, None] != cand[None, :])
        nb[rows] = hit.sum(axis=1)
        # 0/1 weights times lattice values: exact products, so any summation order of the product gives
        # the sum of the neighbours' values
        sums[rows, 0:9] = hit.astype(np.float64) @ np.concatenate([vel[cand], pos[cand], col[cand]], axis=1)
        a, b = np.nonzero(hit & (dist_sq < ss))
        dist = np.sqrt(dist_sq[a, b])
        inv = 1.0 / dist
        nsep[rows] = np.bincount(a, minlength=len(rows))
        for k in range(3):
            t = d[k][a, b] * inv / dist  # (dx * inv_dist) / dist
            sums[rows, 9 + k] = np.bincount(a, weights=t, minlength=len(rows))
            sums[rows, 12 + k] = np.bincount(a, weights=np.abs(t), minlength=len(rows))
    F = Forces(nq)
    F.nb, F.nsep = nb, nsep
    F.sep_sum, F.sep_abs = sums[:, 9:12].copy(), sums[:, 12:15].copy()
    pq, vq, cq = pos[query], vel[query], col[query]
    ms, mf = P["max_speed"], P["max_force"]
    with np.errstate(divide="ignore", invalid="ignore"):
        k = nsep > 0
        F.sep[k] = _steer(sums[k, 9:12] / nsep[k, None], vq[k], ms, mf, P["separation_weight"])
        k = nb > 0
        cnt = nb[k, None].astype(np.float64)
        F.ali[k] = _steer(sums[k, 0:3] / cnt, vq[k], ms, mf, P["alignment_weight"])
        F.coh[k] = _steer(sums[k, 3:6] / cnt - pq[k], vq[k], ms, mf, P["cohesion_weight"])
        F.avg[:] = cq
        F.avg[k] = (sums[k, 6:9] + cq[k]) / (cnt + 1)
    return F


def physics(pos, vel, col, forces, params, dt):
    """update_physics (flock.py:241-308) on the forces (sep, ali, coh, avg): new (pos, vel, col).
    Wall force max_force * wall_weight, colour blend min(1, rate * dt) (flock.py:662, :673)."""
    P = unpack(params)
    sep, ali, coh, avg = (np.asarray(f, dtype=np.float64) for f in forces)
    pos = np.asarray(pos, dtype=np.float64)
    vel = np.asarray(vel, dtype=np.float64)
    col = np.asarray(col, dtype=np.float64)
    margin, bounds = P["wall_margin"], P["bounds"]
    wall = P["max_force"] * P["wall_weight"]
    acc = sep + ali + coh
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


def sep_bound(F, vel, params):
    """Per boid: a bound on the max-norm difference between two evaluations of the separation force
    that sum the same terms t in different orders (everything else is the same operations on the
    same values).

    Any order of a recursive sum errs by at most g = (m - 1) u / (1 - (m - 1) u) times the sum of
    |t| (per component), so two orders differ by dS with ||dS|| <= 2 g ||sum |t|||.  The force is
    w * clamp(S / |S| * max_speed - v): normalising moves by at most 2 ||dS|| / |S| (|S| is the
    exact sum, at least the computed one minus g ||sum |t|||), the clamp is 1-Lipschitz.  A factor 2
    of safety, plus 32 u of the operands' size for the rounding of the two evaluations; the force is
    never larger than w * max_force, which caps the bound for an ill-conditioned (near zero) sum."""
    P = unpack(params)
    w, ms, mf = abs(P["separation_weight"]), P["max_speed"], P["max_force"]
    m = np.maximum(F.nsep - 1, 0).astype(np.float64)
    g = m * U / (1 - m * U)
    A = np.linalg.norm(F.sep_abs, axis=1)
    S = np.linalg.norm(F.sep_sum, axis=1) - g * A
    cap = 2 * w * mf * (1 + 64 * U)
    with np.errstate(divide="ignore", invalid="ignore"):
        b = w * ms * 2 * (2 * 2 * g * A / S) + 32 * U * w * (ms + np.linalg.norm(vel, axis=1) + mf)
    b = np.where(S > 0, np.minimum(b, cap), cap)
    return np.where(F.nsep > 0, b, 0.0)


def check_sep(got, F, vel, params, what=""):
    """Assert |got - F.sep| <= sep_bound per boid, and that the bound is tight (< 1e-9) for at least
    99 % of the boids that have a separation term.  Returns (max difference, worst bound)."""
    b = sep_bound(F, vel, params)
    diff = np.abs(np.asarray(got) - F.sep).max(axis=1)
    bad = np.flatnonzero(diff > b)
    assert len(bad) == 0, (what, "sep beyond its bound", bad[:5], diff[bad[:5]], b[bad[:5]])
    has = F.nsep > 0
    if has.any():
        tight = (b[has] < 1e-9).mean()
        assert tight >= 0.99, (what, "sep bound too loose to mean anything", tight)
    return float(diff.max(initial=0.0)), float(b.max(initial=0.0))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def lattice(x, bits):
    """Round to multiples of 2^-bits (exact in float64 for |x| < 2^(53 - bits))."""
    s = float(2 ** bits)
    return np.round(np.asarray(x, dtype=np.float64) * s) / s


def id_colours(n, first=0):
    """Integer colours that name the boid: id % 4096, id // 4096 and a hash of the id (< 2^20).
    Sums of them are exact in any order, and a neighbour lost or counted twice changes them."""
    i = np.arange(first, first + n, dtype=np.int64)
    h = (i * 2654435761) % (1 << 20)
    return np.stack([i % 4096, i // 4096, h], axis=1).astype(np.float64)
