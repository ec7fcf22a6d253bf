"""Inputs shared by the GPU tests of the tree queries (test_gpu_knn, test_gpu_fof, test_gpu_pairs,
test_gpu_query_shared) and by scripts/gen_query_evals_golden.py: a plain helper module like boids_cases.py, no fixtures.

Every generator returns positions and masses (presets: velocities too), always from the same RNG streams in the same
order, so a test that takes only the positions sees what a test that also takes the masses sees.
"""
import numpy as np


def bh(p, v=None, m=None, G=0.07, eps=1.5, theta=0.5, **kw):
    """a Barnes-Hut handle on positions p; at rest and unit masses unless given"""
    from nbody.gpu_backend import HIPBarnesHutSimulation
    p = np.ascontiguousarray(p, np.float64)
    v = np.zeros_like(p) if v is None else np.ascontiguousarray(v, np.float64)
    m = np.ones(len(p)) if m is None else np.ascontiguousarray(m, np.float64)
    return HIPBarnesHutSimulation(p, v, m, G, eps, 1.0, theta, **kw)


def preset(dist, n=20_000, seed=7, R=800.0, G=0.07, scale_masses=True):
    """(p, v, m) of a tools.presets distribution; scale_masses: unequal masses, so that a mass sum is not a count"""
    from tools.presets import generate_distribution
    np.random.seed(seed)
    p, v, m = generate_distribution(dist, n, R, G)
    m = np.ascontiguousarray(m, np.float64)
    if scale_masses:
        m = m * np.random.RandomState(seed).uniform(0.5, 2.0, n)
    return np.ascontiguousarray(p, np.float64), np.ascontiguousarray(v, np.float64), m


def ball(n, seed, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """n positions uniform in a ball (positions only: the building block of trap() and far())"""
    rng = np.random.RandomState(seed)
    u = rng.normal(size=(n, 3))
    u *= (rng.uniform(size=n) ** (1.0 / 3.0) / np.linalg.norm(u, axis=1))[:, None]
    return np.asarray(centre) + radius * u


def trap(seed=11):
    """DESIGN 4.14's trap (tests/test_gpu_quadrupole.py's shape): 2 048 bodies within 1e-3 of a point at coordinate 700
    plus 2 048 in +-800 - where a bound computed in fp32 breaks"""
    rng = np.random.RandomState(seed)
    p = np.concatenate([ball(2048, seed, 1e-3, (700.0, -650.0, 300.0)), rng.uniform(-800.0, 800.0, (2048, 3))])
    return p, rng.uniform(0.5, 1.5, len(p))


def far():
    """DESIGN 4.14's far body: one body 1e6 away from a ball of 4 096 - all of its neighbours are far, and it inflates
    the root cube"""
    p = np.concatenate([ball(4096, 3, 50.0), [[1.0e6, -2.0e5, 3.0e5]]])
    return p, np.random.RandomState(4).uniform(0.5, 1.5, len(p))


def uniform(n, seed):
    rng = np.random.RandomState(seed)
    return rng.uniform(-100.0, 100.0, (n, 3)), rng.uniform(0.5, 1.5, n)


def lattice(spacing=1.0, shuffle=True):
    """16^3 lattice, unit masses; shuffle: the caller's order is a fixed permutation"""
    g = spacing * np.arange(16, dtype=np.float64)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    if shuffle:
        p = p[np.random.RandomState(5).permutation(len(p))]
    return p, np.ones(len(p))


def _preset_pm(dist, **kw):
    p, _v, m = preset(dist, **kw)
    return p, m


def _given(rows):
    p = np.array(rows, dtype=np.float64)
    return p, np.ones(len(p))


SYSTEMS = {
    "galaxy": lambda: _preset_pm("galaxy"),        # a strong density contrast
    "collision": lambda: _preset_pm("collision"),
    "filament": lambda: _preset_pm("filament"),
    "cluster": lambda: _preset_pm("cluster"),
    "galaxy20k": lambda: system("galaxy"),         # test_gpu_knn's names: the same galaxy, and the cluster at its own scale
    "cluster20k": lambda: _preset_pm("cluster", R=300.0, G=0.05),
    "n2049": lambda: uniform(2049, 1),             # the last wave has one lane
    "n4097": lambda: uniform(4097, 2),
    "trap": trap,
    "far": far,
    "n1": lambda: _given([[1.0, 2.0, 3.0]]),
    "n2": lambda: _given([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]]),  # d2 = 25 exactly
    "n9": lambda: uniform(9, 5),
    "n65": lambda: uniform(65, 6),                 # one full wave and a one-lane wave
    "lattice33": lambda: lattice(33.0),
}
_SYS = {}


def system(name):
    """(positions, masses) of a named system, made once; callers do not write to them"""
    if name not in _SYS:
        _SYS[name] = SYSTEMS[name]()
    return _SYS[name]
