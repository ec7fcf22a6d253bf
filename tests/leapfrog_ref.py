"""Float64 restatements of the two N-body integrators, and the systems the integrator tests run.

TEST INFRASTRUCTURE.  With a = F(x) the acceleration of the current positions:
  kick-drift (the reference, nbody/simulation.py:291-305):  a = F(x); v = (v + a dt) damping; x += v dt
  leapfrog (include/nbmi.h):                 v += a dt/2; x += v dt; a = F(x); v = (v + a dt/2) damping
The leapfrog state carries a = F(x) from one step to the next; the first step computes it ("priming").
"""
import numpy as np

from direct_ref import direct_accelerations


def direct_force(G, softening):
    """F(x, m): float64 all-pairs accelerations by the reference's pair rule (tests/direct_ref.py)."""
    def force(x, m):
        return direct_accelerations(x, m, np.arange(len(x)), G, softening, chunk=512)
    return force


def leapfrog(x, v, m, force, dt, steps, damping=1.0, a=None):
    """(x, v, a) after `steps` kick-drift-kick steps; `a` = F(x) of the initial state if known."""
    x = np.array(x, dtype=np.float64)
    v = np.array(v, dtype=np.float64)
    a = force(x, m) if a is None else a
    h = 0.5 * dt
    for _ in range(steps):
        v = v + a * h
        x = x + v * dt
        a = force(x, m)
        v = (v + a * h) * damping
    return x, v, a


def kick_drift(x, v, m, force, dt, steps, damping=1.0):
    """(x, v) after `steps` steps of the reference's scheme."""
    x = np.array(x, dtype=np.float64)
    v = np.array(v, dtype=np.float64)
    for _ in range(steps):
        a = force(x, m)
        v = (v + a * dt) * damping
        x = x + v * dt
    return x, v


def kepler_pair():
    """Circular two-body orbit: m1 = m2 = 1/2, G = 1, separation 1, softening 0, so omega = 1 and T = 2 pi."""
    x = np.array([[0.5, 0.0, 0.0], [-0.5, 0.0, 0.0]])
    v = np.array([[0.0, 0.5, 0.0], [0.0, -0.5, 0.0]])
    return x, v, np.array([0.5, 0.5])


def kepler_exact(t):
    """Positions and velocities of kepler_pair() at time t."""
    c, s = np.cos(t), np.sin(t)
    x = 0.5 * np.array([[c, s, 0.0], [-c, -s, 0.0]])
    v = 0.5 * np.array([[-s, c, 0.0], [s, -c, 0.0]])
    return x, v


def plummer(n, seed, scale=1.0, total_mass=1.0, G=1.0, vary=0.5, rmax=10.0):
    """Seeded Plummer sphere (Aarseth, Henon & Wielen 1974): radii from the cumulative mass, isotropic directions,
    speeds by rejection from q^2 (1 - q^2)^(7/2) of the escape speed; masses total_mass / n varied by +-vary; centre of
    mass and mean momentum removed.  Radii beyond rmax scale lengths are drawn again."""
    rng = np.random.RandomState(seed)

    def directions(k):
        z = rng.uniform(-1.0, 1.0, k)
        phi = rng.uniform(0.0, 2.0 * np.pi, k)
        s = np.sqrt(1.0 - z * z)
        return np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)

    r = np.empty(n)
    for i in range(n):
        while True:
            u = rng.uniform(1e-10, 1.0)
            ri = scale / np.sqrt(u ** (-2.0 / 3.0) - 1.0)
            if ri <= rmax * scale:
                r[i] = ri
                break
    x = r[:, None] * directions(n)
    q = np.empty(n)
    for i in range(n):
        while True:
            a, b = rng.uniform(0.0, 1.0), rng.uniform(0.0, 0.1)
            if b < a * a * (1.0 - a * a) ** 3.5:
                q[i] = a
                break
    vesc = np.sqrt(2.0 * G * total_mass / scale) * (1.0 + (r / scale) ** 2) ** -0.25
    v = (q * vesc)[:, None] * directions(n)
    m = total_mass / n * rng.uniform(1.0 - vary, 1.0 + vary, n)
    x -= (m[:, None] * x).sum(0) / m.sum()
    v -= (m[:, None] * v).sum(0) / m.sum()
    return x, v, m


def total_energy(x, v, m, G, softening):
    """K + W in float64, W = -1/2 sum_i sum_{j != i} G m_i m_j / sqrt(|x_j - x_i|^2 + eps^2)."""
    d = x[None, :, :] - x[:, None, :]
    r2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) + softening * softening
    np.fill_diagonal(r2, np.inf)
    w = -0.5 * G * np.sum(m[:, None] * m[None, :] / np.sqrt(r2))
    return 0.5 * np.sum(m * np.sum(v * v, axis=1)) + w
