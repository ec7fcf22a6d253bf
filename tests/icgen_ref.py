"""Host replay of the device-side initial conditions (csrc/icgen.hip), body by body.

The device generator is a pure function of (seed, n, R, G): every random number is one half of a Philox4x32-10
block addressed by (seed, body index, draw number, stream tag).  This module restates it in plain NumPy from the
formulas of tools/presets.py and the draw roles documented in icgen.hip - which uniform feeds which quantity - so
the GPU suite can compare every generated body with an independent value (tests/test_gpu_icgen_replay.py), not
only distributions.

Every generator takes ``dtype``: np.float64 evaluates the formulas as the device does, np.longdouble evaluates the
same formulas (same float64 constants and the same float64 uniforms, which are the generator's inputs) in extended
precision.  The difference of the two replays is E_ref, the rounding error of the float64 formulas themselves,
from which the device tolerance is built.
"""
import numpy as np

TWO_PI = 6.283185307179586          # the kernel's double constant: 2 pi rounded to float64
TAG_BODIES = 0x49436E62             # "ICnb": per-body draws, counter = body index
TAG_NODES = 0x49436E6E              # "ICnn": filament node table, counter = node index
WEB_GRID = 8

# one preset per distribution: (spawn radius, G, softening) of quick_galaxy, extreme_10m_collision,
# spiral_milkyway, accurate_cluster and cosmic_web
PRESET = {"galaxy": (500.0, 0.15, 3.0), "collision": (2000.0, 0.08, 6.0), "spiral": (600.0, 0.08, 2.0),
          "cluster": (300.0, 0.05, 1.0), "filament": (1200.0, 0.02, 5.0)}
SEEDS = (42, 2 ** 32 + 42)
# 1, 2; around one 256-thread block; past one 2048-item sort tile (with floor ties); 20 011
SIZES = (1, 2, 255, 256, 257, 4099, 20011)
COLLISION_SIZES = SIZES + (1001,)   # odd: halves of 500/501 (4099: 2049/2050)
COM_REMOVED = ("galaxy", "spiral", "cluster")


def cases():
    """(distribution, n, seed) of every case the device is compared at."""
    out = []
    for dist in PRESET:
        for n in sorted(COLLISION_SIZES if dist == "collision" else SIZES):
            out += [(dist, n, seed) for seed in SEEDS]
    return out


_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays: counter (..., 4), key (..., 2) -> (..., 4) uint32.
    uint64 arithmetic; a 32 x 32-bit product fits."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & _M32, (p0 >> _S32) ^ c[3] ^ k[1], p0 & _M32]
        k = [(k[0] + w0) & _M32, (k[1] + w1) & _M32]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


class Draws:
    """The numbered draws of the items `index` (body or node indices) under `seed` in stream `tag`."""

    def __init__(self, seed, index, tag=TAG_BODIES, dtype=np.float64):
        seed = int(seed) & (2 ** 64 - 1)
        index = np.asarray(index, dtype=np.uint64)
        self.key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
        self.lo, self.hi = index & _M32, index >> _S32
        self.tag, self.dtype = tag, dtype
        self._blocks = {}

    def uniform(self, k):
        """Uniform number k in (0, 1]: ((53 bits) + 0.5) 2^-53 from words 0,1 (even k) or 2,3 (odd k) of block
        k >> 1.  The float64 value is the generator's input, so both precisions start from the same number."""
        b = k >> 1
        if b not in self._blocks:
            ctr = np.stack([self.lo, self.hi, np.full_like(self.lo, b), np.full_like(self.lo, self.tag)], axis=-1)
            self._blocks[b] = philox4x32_10(ctr, self.key).astype(np.uint64)
        w = self._blocks[b]
        hi, lo = (w[..., 2], w[..., 3]) if k & 1 else (w[..., 0], w[..., 1])
        bits = ((hi << _S32) | lo) >> np.uint64(11)
        return ((bits.astype(np.float64) + 0.5) * 2.0 ** -53).astype(self.dtype)

    def normal2(self, k):
        """Standard normal pair k: Box-Muller on uniforms 2k, 2k+1, cosine branch first."""
        u1, u2 = self.uniform(2 * k), self.uniform(2 * k + 1)
        rad = np.sqrt(-2.0 * np.log(u1))
        ang = TWO_PI * u2
        return rad * np.cos(ang), rad * np.sin(ang)


def stable_ranks(r):
    """Rank of each entry under a stable sort: ties rank in index order."""
    order = np.argsort(r, kind="stable")
    rank = np.empty(len(r), dtype=np.int64)
    rank[order] = np.arange(len(r))
    return rank


def disk(seed, first, count, R, G, scale_length, softening, max_r, height, disp, spin, x0=0.0, y0=0.0, vx_add=0.0,
         arms=0, min_speed_frac=0.0, dtype=np.float64):
    """One rotating exponential disk of bodies [first, first + count) (presets._disk_galaxy / _spiral_galaxy;
    unit masses, so the enclosed mass of a body is its radius rank + 1 among the disk's own bodies).
    Draws: u0 radius; u1 angle (galaxy) or arm (spiral); normal pair 1 = (height, arm scatter); pair 2 =
    (v_x, v_z) dispersion; pair 3 first = v_y dispersion."""
    d = Draws(seed, first + np.arange(count), dtype=dtype)
    r = -scale_length * np.log(d.uniform(0))
    r = r * (1 - np.exp(-max_r / (r + 0.01)))
    r = np.maximum(r, R * 0.001)
    n_height, n_arm = d.normal2(1)
    if arms:
        arm = np.minimum(np.floor(d.uniform(1) * arms), arms - 1)
        theta = -np.log(r / (R * 0.02) + 1) / 0.35 + arm * (TWO_PI / arms) + n_arm * (0.12 + 0.15 * np.sqrt(r / R))
    else:
        theta = TWO_PI * d.uniform(1)
    pos = np.empty((count, 3), dtype=dtype)
    pos[:, 0] = r * np.cos(theta) + x0
    pos[:, 1] = n_height * (R * height * (1 + np.sqrt(r / R) * 0.3)) + y0
    pos[:, 2] = r * np.sin(theta)
    # rotation curve from the enclosed mass (presets.compute_rotation_curve)
    rank = stable_ranks(r)
    eps_sq = (softening * 2) ** 2
    r_sq = r ** 2
    speed = np.sqrt(G * (rank + 1) * r_sq / (r_sq + eps_sq) ** 1.5)
    speed = speed * np.maximum(r_sq / (r_sq + eps_sq), 0.3)
    if min_speed_frac:
        speed = np.maximum(speed, np.sqrt(G * (count * 0.001) / (r + softening)) * min_speed_frac)
    sigma = speed * disp * (r / (r + softening * 2)) + np.sqrt(G * count * 0.00005)
    n_x, n_z = d.normal2(2)
    n_y, _ = d.normal2(3)
    vel = np.empty((count, 3), dtype=dtype)
    vel[:, 0] = -speed * np.sin(theta) * spin + n_x * sigma + vx_add
    vel[:, 1] = n_y * sigma * 0.25
    vel[:, 2] = speed * np.cos(theta) * spin + n_z * sigma
    return {"pos": pos, "vel": vel, "radius": r, "angle": theta, "rank": rank, "speed": speed, "sigma": sigma}


def _finish(out, n, mass, dtype, remove_com):
    if remove_com and n:
        out["vel"] = out["vel"] - out["vel"].sum(axis=0) / n  # unit masses
    out["mass"] = np.full(n, mass, dtype=dtype)
    return out


def galaxy(seed, n, R, G, dtype=np.float64):
    R, G = dtype(R), dtype(G)
    out = disk(seed, 0, n, R, G, R * 0.3, R * 0.03, R * 1.0, 0.012, 0.12, +1.0, dtype=dtype)
    return _finish(out, n, 1.0, dtype, True)


def spiral(seed, n, R, G, dtype=np.float64):
    """The galaxy disk on 4 trailing arms, rotation speed floored at 0.7 of a point mass's, dispersion 0.10."""
    R, G = dtype(R), dtype(G)
    out = disk(seed, 0, n, R, G, R * 0.3, R * 0.03, R * 1.0, 0.012, 0.10, +1.0, arms=4, min_speed_frac=0.7,
               dtype=dtype)
    return _finish(out, n, 1.0, dtype, True)


def collision(seed, n, R, G, dtype=np.float64):
    """Two counter-rotating disks approaching each other; the second disk's bodies draw under their global index.
    `rank` is each body's rank within its own disk.  No centre-of-mass correction."""
    R, G = dtype(R), dtype(G)
    half = n // 2
    separation = (R * 0.5) * 3.5
    speed = np.sqrt(2 * G * (n * 0.001) / separation) * 0.6
    a = disk(seed, 0, half, R, G, R * 0.25, R * 0.025, R * 0.5, 0.01, 0.10, +1.0, x0=-separation / 2, vx_add=speed,
             dtype=dtype)
    b = disk(seed, half, n - half, R, G, R * 0.25, R * 0.025, R * 0.5, 0.01, 0.10, -1.0, x0=separation / 2,
             y0=R * 0.15, vx_add=-speed, dtype=dtype)
    out = {k: np.concatenate([a[k], b[k]]) for k in a}
    out["half"] = half
    return _finish(out, n, 1.0, dtype, False)


def cluster(seed, n, R, G, dtype=np.float64):
    """Plummer sphere.  Draws: u0 radius, u1 azimuth, u2 cos(polar angle); normal pair 2 first = speed, u6 / u7 the
    velocity's azimuth / cos(polar angle)."""
    R, G = dtype(R), dtype(G)
    d = Draws(seed, np.arange(n), dtype=dtype)
    a = R * 0.3
    with np.errstate(divide="ignore"):
        r = a / np.sqrt(d.uniform(0) ** (-2.0 / 3.0) - 1)
    r = np.clip(r, 0, R * 1.5)
    phi = TWO_PI * d.uniform(1)
    cos_t = 2 * d.uniform(2) - 1
    sin_t = np.sqrt(1 - cos_t ** 2)
    pos = np.stack([r * sin_t * np.cos(phi), r * cos_t, r * sin_t * np.sin(phi)], axis=1)
    base = G * (n * 0.001) / (6 * a)
    sigma = np.sqrt(np.maximum(base * (1 + (r / a) ** 2) ** (-0.5), base * 0.01))
    v_mag = np.abs(d.normal2(2)[0] * (sigma * np.sqrt(dtype(3))))
    v_phi = TWO_PI * d.uniform(6)
    v_cos = 2 * d.uniform(7) - 1
    v_sin = np.sqrt(1 - v_cos ** 2)
    vel = np.stack([v_mag * v_sin * np.cos(v_phi), v_mag * v_cos, v_mag * v_sin * np.sin(v_phi)], axis=1)
    out = {"pos": pos.astype(dtype), "vel": vel.astype(dtype), "radius": r, "angle": phi, "cos_t": cos_t,
           "sigma": sigma}
    return _finish(out, n, 1.0, dtype, True)


def _unit(v):
    return v / (np.sqrt((v * v).sum(axis=-1, keepdims=True)) + 1e-10)


def web_nodes(seed, R, dtype=np.float64):
    """The filament's node table: the 8^3 grid over [-1.25R, 1.25R]^3 in (ix, iy, iz) order, node j drawing under
    counter j of stream TAG_NODES.  u0 < 0.35: active; weight sqrt(u1) (numpy's power(2)); normal pairs 1, 2 =
    elongation axis (3 of 4 numbers), pairs 3, 4 = the vector made perpendicular to it.  Returns the active nodes
    only, in grid order: grid index, centre, cdf (cumulative sum over the nodes in order, divided by the total,
    last entry 1), axis e, perpendicular unit vectors p1, p2."""
    R = dtype(R)
    g = WEB_GRID
    j = np.arange(g ** 3)
    d = Draws(seed, j, tag=TAG_NODES, dtype=dtype)
    active = d.uniform(0) < 0.35
    weight = np.sqrt(d.uniform(1))[active]
    cdf = np.cumsum(weight)
    cdf = cdf / cdf[-1]
    cdf[-1] = 1.0
    step = R * 2.5 / (g - 1)
    centre = -R * 1.25 + step * np.stack([j // (g * g), (j // g) % g, j % g], axis=1).astype(dtype)
    e01, e2 = d.normal2(1), d.normal2(2)
    p01, p2 = d.normal2(3), d.normal2(4)
    e = _unit(np.stack([e01[0], e01[1], e2[0]], axis=1))
    p = np.stack([p01[0], p01[1], p2[0]], axis=1)
    p = _unit(p - (p * e).sum(axis=1, keepdims=True) * e)
    q = _unit(np.cross(e, p))
    return {"grid_index": j[active], "centre": centre[active], "cdf": cdf, "weight": weight, "e": e[active],
            "p1": p[active], "p2": q[active]}


def filament(seed, n, R, G=None, dtype=np.float64):
    """Cosmic web: body i picks node searchsorted(cdf, u0, 'right') (clamped) and sits at centre + N(0, 0.8 s) e +
    N(0, 0.12 s) p1 + N(0, 0.12 s) p2, s = 2.5R/8 (normal pair 1 and the first of pair 2); velocity 0.05 x +
    0.3 N(0,1) per component (second of pair 2, pair 3).  Masses 0.1, no centre-of-mass correction.
    `cdf_margin` is the smallest distance of any body's u0 to a CDF edge."""
    T = web_nodes(seed, R, dtype)
    R = dtype(R)
    d = Draws(seed, np.arange(n), dtype=dtype)
    u = d.uniform(0)
    node = np.minimum(np.searchsorted(T["cdf"], u, "right"), len(T["cdf"]) - 1)
    s = R * 2.5 / WEB_GRID
    along, across1 = d.normal2(1)
    across2, g0 = d.normal2(2)
    g1, g2 = d.normal2(3)
    coef = np.stack([along * (0.8 * s), across1 * (0.12 * s), across2 * (0.12 * s)], axis=1)
    pos = (T["centre"][node] + coef[:, 0:1] * T["e"][node] + coef[:, 1:2] * T["p1"][node]
           + coef[:, 2:3] * T["p2"][node])
    noise = np.stack([g0, g1, g2], axis=1) * 0.3
    vel = pos * 0.05 + noise
    margin = np.abs(u[:, None] - T["cdf"][None, :]).min() if n else np.inf
    out = {"pos": pos.astype(dtype), "vel": vel.astype(dtype), "node": node, "coef": coef, "noise": noise,
           "nodes": T, "cdf_margin": float(margin)}
    return _finish(out, n, 0.1, dtype, False)


GENERATORS = {"galaxy": galaxy, "collision": collision, "spiral": spiral, "cluster": cluster, "filament": filament}


def generate(dist, seed, n, dtype=np.float64):
    """Replay of nbmi_create_generated(dist, n, R, seed, G) at the distribution's preset (R, G)."""
    R, G, _ = PRESET[dist]
    return GENERATORS[dist](seed, n, R, G, dtype=dtype)


def e_ref(lo, hi, R):
    """(position, velocity) E_ref of one case: the largest difference between the float64 replay `lo` and the
    extended-precision replay `hi`, positions relative to R, velocities to the replay's largest speed (0 where
    that speed is 0, which is one body with its centre-of-mass velocity removed)."""
    ep = float(np.abs(lo["pos"] - hi["pos"]).max() / R)
    vmax = speed_scale(lo)
    ev = float(np.abs(lo["vel"] - hi["vel"]).max() / vmax) if vmax > 0 else float(np.abs(lo["vel"] - hi["vel"]).max())
    return ep, ev


def speed_scale(rep):
    return float(np.sqrt((rep["vel"].astype(np.float64) ** 2).sum(axis=1)).max())
