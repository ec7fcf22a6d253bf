"""The octree build gives the same tree and the same trajectories, bit for bit, whichever way its key sort runs:

  NBMI_SORT_DIGIT_BITS / NBMI_SORT_THREADS  the passes' digit width and threads per tile; by default chosen by size, and
                        these systems are far below the sizes from which more than 256 threads work on a tile, so the
                        large systems' forms (10 bits x 1024, 8 bits x 512) are forced here, and the others
  NBMI_SORT_FUSED_HIST  1: k_keys_hist counts the sort's digit histogram while it writes the packed words (what a handle
                        of up to 2 097 152 bodies does by default); 0: the sort reads them back for it (k_radix_hist)
  NBMI_SORT_PACKED      0: (key, index) pairs, 8-bit digits, 256 threads

The reference is the five-pass form the build had before any of this: 8 bits, 256 threads, histogram kernel.  The sorted
order is unique (the packed words are all distinct), so everything downstream must agree exactly.  Two systems: a
70 000-body galaxy (18 tiles; a 32-bit prefix, whose fourth 10-bit digit is partial) and the 4 099 bodies with a run of
301 equal upper key words of tests/test_gpu_build_paths.py, restated here.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G, EPS, THETA, DT, STEPS, RADIUS = 0.15, 2.0, 0.6, 0.05, 3, 500.0

LEGACY = dict(NBMI_SORT_DIGIT_BITS=8, NBMI_SORT_THREADS=256, NBMI_SORT_FUSED_HIST=0)
# what the size rule ships for large systems: WIDE up to 2 097 152 bodies, LARGE above
LARGE = dict(NBMI_SORT_DIGIT_BITS=8, NBMI_SORT_THREADS=512)
WIDE = dict(NBMI_SORT_DIGIT_BITS=10, NBMI_SORT_THREADS=1024)
PATHS = {
    "default": {},
    "large": LARGE,
    "large, histogram kernel": dict(LARGE, NBMI_SORT_FUSED_HIST=0),
    "10 bits x 1024": WIDE,
    "10 bits x 1024, histogram kernel": dict(WIDE, NBMI_SORT_FUSED_HIST=0),
    "10 bits x 256": dict(NBMI_SORT_DIGIT_BITS=10, NBMI_SORT_THREADS=256),
    "10 bits x 512": dict(NBMI_SORT_DIGIT_BITS=10, NBMI_SORT_THREADS=512),
    "8 bits x 1024": dict(NBMI_SORT_DIGIT_BITS=8, NBMI_SORT_THREADS=1024),
    "8 bits x 256, fused": dict(NBMI_SORT_DIGIT_BITS=8, NBMI_SORT_THREADS=256),
    "default, histogram kernel": dict(NBMI_SORT_FUSED_HIST=0),
    "default, fused": dict(NBMI_SORT_FUSED_HIST=1),
    "pairs": dict(NBMI_SORT_PACKED=0),
}


def _clumped():
    """The input of tests/test_gpu_build_paths.py: 4 099 bodies, 300 of them in a cube of edge 1e-7 around body 0 (one run
    of 301 equal upper key words, eight bodies exactly coincident), 100 more in a cube of edge 0.05."""
    from tools.presets import generate_distribution
    n, seed, clump, coincident, clump2 = 4099, 11, 300, 8, 100
    state = np.random.get_state()
    try:
        np.random.seed(seed)
        p, v, m = generate_distribution("cluster", n, RADIUS, G)
        m = m * np.random.uniform(0.5, 1.5, n)
    finally:
        np.random.set_state(state)
    p = np.array(p, dtype=np.float64)
    rng = np.random.default_rng(seed)
    p[1:1 + clump] = p[0] + rng.uniform(-0.5e-7, 0.5e-7, (clump, 3))
    p[1:coincident] = p[0]
    first2 = 1 + clump
    p[first2:first2 + clump2] = p[first2 + clump2] + rng.uniform(-0.025, 0.025, (clump2, 3))
    return p, np.array(v, dtype=np.float64), np.array(m, dtype=np.float64)


def _galaxy():
    from tools.presets import generate_distribution
    state = np.random.get_state()
    try:
        np.random.seed(5)
        p, v, m = generate_distribution("galaxy", 70_000, RADIUS, G)
    finally:
        np.random.set_state(state)
    return np.array(p, dtype=np.float64), np.array(v, dtype=np.float64), np.array(m, dtype=np.float64)


class _Env:
    def __init__(self, env):
        self.env = {k: str(v) for k, v in env.items()}

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, old in self.saved.items():
            if old is None:
                del os.environ[k]
            else:
                os.environ[k] = old


def _run(inputs, env):
    """The tree of a query build, then the float64 state after three steps, of one handle created under `env`."""
    from nbody.gpu_backend import HIPBarnesHutSimulation
    p, v, m = inputs
    with _Env(env):
        sim = HIPBarnesHutSimulation(p, v, m, G, EPS, 1.0, THETA)
    try:
        sim.build_tree()
        hi, lo = sim.sort_keys()
        level, key = sim.cells()
        out = dict(order=sim.key_order(), hi=hi, lo=lo, level=level, key=key)
        stats = sim.tree_stats()
        for _ in range(STEPS):
            sim.step(DT)
        out.update(pos=sim.get_positions_f64(), vel=sim.get_velocities())
        return out, stats
    finally:
        sim.close()


@pytest.fixture(scope="module", params=["galaxy", "clumped"])
def system(request):
    inputs = _galaxy() if request.param == "galaxy" else _clumped()
    return inputs, _run(inputs, LEGACY)


@pytest.mark.parametrize("path", list(PATHS))
def test_tree_and_steps_do_not_depend_on_the_sort(gpu, system, path):
    inputs, (ref, ref_stats) = system
    got, stats = _run(inputs, PATHS[path])
    assert stats == ref_stats
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k


def test_reference_order_is_the_keys_order(gpu, system):
    inputs, (ref, _) = system
    n = len(inputs[2])
    assert np.array_equal(ref["order"], np.lexsort((np.arange(n), ref["lo"], ref["hi"])))


def test_bad_switch_values_refuse_the_handle(gpu):
    from nbody.gpu_backend import HIPBarnesHutSimulation
    p, v, m = _clumped()
    for env in (dict(NBMI_SORT_DIGIT_BITS=9), dict(NBMI_SORT_THREADS=128)):
        with _Env(env):
            with pytest.raises(Exception):
                HIPBarnesHutSimulation(p, v, m, G, EPS, 1.0, THETA)
