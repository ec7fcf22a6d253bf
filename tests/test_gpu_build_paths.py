"""The octree build's alternative paths give the same tree and the same trajectories, bit for bit.

One library; the path is chosen by the environment at nbmi_create:
  NBMI_SORT_PACKED  1 (default): keys-only sort of (prefix << 24 | body index) words; 0: (key, index) pairs
  NBMI_KEYS_LEAN    1 (default) / 0: the stepping build's key form
  NBMI_SORT_BITS    48 widens the sorted prefix past the 40 bits a packed word can hold: the pair path, whatever
                    NBMI_SORT_PACKED says

The input is made to exercise the tie-fix, which is where the packed path differs most: 4 099 bodies (the Plummer
sphere of tests/test_gpu_walk_bits.py, restated), 300 of them moved into a cube of edge 1e-7 around body 0 - ONE run of
301 bodies that agree on the whole upper key word, longer than the 64 from which max_run is recorded and shorter than
the 4 096 that would widen the prefix - eight of those exactly coincident (equal 126-bit keys: the order falls back on
the body index), and 100 more in a cube of edge 0.05 (runs in the 40-bit prefix whose upper words differ).  The CPU
oracle confirms these properties before the GPU is used.  A different order puts different bodies into a wave and
changes fp32 sums, so the comparison of float64 states after 3 steps sees a single misplaced body.
"""
import os

import numpy as np
import pytest

N = 4099
G, EPS, THETA, DT, STEPS, RADIUS = 0.15, 2.0, 0.6, 0.05, 3, 500.0
SEED = 11
CLUMP, COINCIDENT, CLUMP2 = 300, 8, 100
PREFIX_SHIFT = 63 - 40  # the default sorted prefix at this size: 40 bits of the 63-bit upper word
# Force precision "auto" asks for float64 in the waves whose G rho dt^2 exceeds tau.  Over the waves of this input (64
# bodies in key order, the densest 16 of them, every box edge at least one softening length) that quantity runs from
# 2e-10 in the halo over 2e-8 at the median to 8e-4 in the first clump: the handle's default tau (5e-5) flags the clump's
# waves alone, 2e-8 about half of all waves.
AUTO_TAU = 2e-8


def make_input():
    from tools.presets import generate_distribution
    state = np.random.get_state()
    try:
        np.random.seed(SEED)
        p, v, m = generate_distribution("cluster", N, RADIUS, G)
        m = m * np.random.uniform(0.5, 1.5, N)
    finally:
        np.random.set_state(state)
    p = np.array(p, dtype=np.float64)
    rng = np.random.default_rng(SEED)
    p[1:1 + CLUMP] = p[0] + rng.uniform(-0.5e-7, 0.5e-7, (CLUMP, 3))
    p[1:COINCIDENT] = p[0]  # bodies 0 .. 7: one point
    first2 = 1 + CLUMP
    p[first2:first2 + CLUMP2] = p[first2 + CLUMP2] + rng.uniform(-0.025, 0.025, (CLUMP2, 3))
    return p, np.array(v, dtype=np.float64), np.array(m, dtype=np.float64)


@pytest.fixture(scope="module")
def inputs():
    return make_input()


def _runs(values):
    """Lengths of the runs of equal neighbours in a sorted array, and where they begin."""
    starts = np.flatnonzero(np.r_[True, values[1:] != values[:-1]])
    return np.diff(np.r_[starts, len(values)]), starts


def test_input_has_the_runs_it_is_meant_to_have(inputs):
    from oracle import pyref
    p = inputs[0]
    bounds = pyref.compute_bounds(p)
    assert abs(bounds - 834.9) < 0.05, bounds
    hi, lo = pyref.body_keys(p, bounds)
    order = np.lexsort((lo, hi))
    hi_s, lo_s = hi[order], lo[order]
    # the first clump: one run of 301 in the whole upper word, hence in the 40-bit prefix
    assert np.all(hi[:1 + CLUMP] == hi[0]) and np.count_nonzero(hi == hi[0]) == 1 + CLUMP
    plen, pstart = _runs(hi_s >> np.uint64(PREFIX_SHIFT))
    assert plen.max() == 1 + CLUMP and 64 < plen.max() < 4096
    # eight bodies with one 126-bit key, and no other group of equal keys
    full = np.stack([hi_s, lo_s], axis=1)
    same = np.all(full[1:] == full[:-1], axis=1)
    assert np.count_nonzero(same) == COINCIDENT - 1
    assert np.all(hi[:COINCIDENT] == hi[0]) and np.all(lo[:COINCIDENT] == lo[0])
    # the second clump: at least one prefix run of two or more bodies whose upper words differ
    mixed = [s for n, s in zip(plen, pstart) if n >= 2 and len(np.unique(hi_s[s:s + n])) > 1]
    assert mixed


class _Env:
    def __init__(self, **env):
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


def _tree(inputs, **env):
    from nbody.gpu_backend import HIPBarnesHutSimulation
    p, v, m = inputs
    with _Env(**env):
        sim = HIPBarnesHutSimulation(p, v, m, G, EPS, 1.0, THETA)
        try:
            sim.build_tree()
            hi, lo = sim.sort_keys()
            level, key = sim.cells()
            return dict(order=sim.key_order(), hi=hi, lo=lo, level=level, key=key, stats=sim.tree_stats())
        finally:
            sim.close()


@pytest.mark.gpu
def test_build_tree_is_the_same_on_both_sort_paths(gpu, inputs):
    a = _tree(inputs, NBMI_SORT_PACKED=0)
    b = _tree(inputs, NBMI_SORT_PACKED=1)
    assert a["stats"] == b["stats"]
    for k in ("order", "hi", "lo", "level", "key"):
        assert np.array_equal(a[k], b[k]), k
    # and the order is the one the keys ask for: (hi, lo, body index) ascending
    assert np.array_equal(b["order"], np.lexsort((np.arange(N), b["lo"], b["hi"])))


def _steps(inputs, prec, **env):
    from nbody.gpu_backend import HIPBarnesHutSimulation
    p, v, m = inputs
    with _Env(**env):
        sim = HIPBarnesHutSimulation(p, v, m, G, EPS, 1.0, THETA)
        try:
            if prec == "auto":
                sim.set_force_precision("auto", AUTO_TAU)
            elif prec == "f32":
                sim.set_force_precision("f32")
            for _ in range(STEPS):
                sim.step(DT)
            share = sim.force_precision_share()[0]
            return sim.get_positions_f64(), sim.get_velocities(), share
        finally:
            sim.close()


PATHS = [dict(NBMI_SORT_PACKED=sp, NBMI_KEYS_LEAN=kl) for sp in (0, 1) for kl in (0, 1)] + [dict(NBMI_SORT_BITS=48)]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "default", "auto"])
@pytest.mark.parametrize("walk", ["one_wave", "split"])
def test_steps_are_the_same_on_every_build_path(gpu, inputs, walk, prec):
    walk_env = {"NBMI_SPLIT_WAVES": 0} if walk == "one_wave" else {}
    ref = _steps(inputs, prec, **walk_env, **PATHS[0])
    print(walk, prec, "share of float64 waves", ref[2])
    if prec != "f32":
        assert 0.0 < ref[2] < 1.0, ref[2]  # some waves float64, some not: the flags of k_gather_scan matter
    for path in PATHS[1:]:
        got = _steps(inputs, prec, **walk_env, **path)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), path
        assert got[2] == ref[2], path
