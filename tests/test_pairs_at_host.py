"""Counts about arbitrary points, host side (nbmi_pair_counts_at): the NumPy restatement against
the definition as a double loop, its tie to the pair counts' restatement, the estimators and sphere counts of
nbody/pairs.py, the C ABI's declaration and the Python classes' refusals (no device)."""
import ctypes
import os
import re

import numpy as np
import pytest

import pairs_at_ref as par
import pairs_ref as pr
from conftest import ROOT


def _lattice6(spacing):
    g = spacing * np.arange(6, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def test_restatement_against_the_double_loop():
    rng = np.random.RandomState(0)
    for n, m, span, edges in ((300, 70, 5.0, (0.0, 0.5, 1.0, 2.0, 4.0)), (257, 65, 1e-3, (5e-5, 2e-4, 1e-3)),
                              (64, 3, 1e6, (1e5, 4e5)), (2, 5, 1.0, (0.1, 10.0)), (1, 5, 1.0, (0.1, 10.0)),
                              (0, 5, 1.0, (0.1, 10.0)), (40, 0, 1.0, (0.1, 10.0))):
        x = rng.uniform(-span, span, (n, 3))
        q = rng.uniform(-1.5 * span, 1.5 * span, (m, 3))
        if n and m:
            q[::7] = x[rng.randint(0, n, len(q[::7]))]  # points that coincide with a body
        counts, below, rows = par.pair_counts_at(q, x, edges)
        assert rows.dtype == np.int32 and rows.shape == (m, len(edges)) and counts.dtype == np.int64
        assert np.array_equal(rows, par.per_point_naive(q, x, edges)), (n, m, span)
        assert np.array_equal(counts, rows[:, 1:].sum(0)) and below == rows[:, 0].sum()  # totals = the column sums
        if n and m and edges[0] == 0.0:
            assert (rows[::7, 0] >= 1).all()  # a point on a body counts that body in column 0: nothing is excluded
    # exact edges: a 6^3 lattice at spacing 33, points at its sites and at the midpoints of its cells' x edges; every
    # edge of the set is an occurring distance (33^2 m and (33/2)^2 (1 + 4 m) have exact roots where used)
    x = _lattice6(33.0)[rng.permutation(216)]
    sites = _lattice6(33.0)[::5]
    mids = _lattice6(33.0)[::7] + np.array([16.5, 0.0, 0.0])
    edges = np.array([pr.exact_root(v) for v in (272.25, 1089.0, 1361.25, 2178.0, 3267.0)])  # 16.5^2, 33^2, 16.5^2 x 5, ...
    assert (edges * edges == np.array([272.25, 1089.0, 1361.25, 2178.0, 3267.0])).all()
    q = np.concatenate([sites, mids])
    counts, below, rows = par.pair_counts_at(q, x, edges)
    assert np.array_equal(rows, par.per_point_naive(q, x, edges))
    assert (rows[:len(sites), 0] == 1).all()  # a site within 16.5 of itself only
    assert below == len(sites) + rows[len(sites):, 0].sum() and rows[len(sites):, 0].max() == 2  # a midpoint AT 16.5 of two sites
    low = np.nextafter(edges, 0.0)
    shifted = par.pair_counts_at(q, x, low)
    assert np.array_equal(shifted[2], par.per_point_naive(q, x, low))
    # one ulp lower: the pairs at an edge move up a column - the midpoints lose their two sites, a site keeps itself (d2 = 0)
    assert (shifted[2][len(sites):, 0] == 0).all() and (shifted[2][:len(sites), 0] == 1).all()
    within = [np.concatenate([[r[1]], r[1] + np.cumsum(r[0])]) for r in ((counts, below), shifted)]
    assert (within[0] - within[1] > 0).all()  # every edge of the set has pairs exactly at it


def test_points_at_the_bodies_give_twice_the_pair_counts():
    rng = np.random.RandomState(3)
    base = rng.uniform(-2.0, 2.0, (150, 3))
    for x, edges in ((base, (0.0, 0.5, 1.0, 2.0, 8.0)), (base, (0.3, 0.9)), (np.concatenate([base, base[:40]]), (0.0, 0.5, 1.0)),
                     (_lattice6(1.0), (1.0, np.sqrt(2.0), 2.0))):
        n = len(x)
        counts, below, rows = par.pair_counts_at(x, x, edges)
        dd, below_dd = pr.pair_counts(x, edges)
        assert np.array_equal(counts, 2 * dd) and below == 2 * below_dd + n
        assert (rows[:, 0] >= 1).all()


def test_estimators_by_hand():
    from nbody.pairs import xi_davis_peebles, xi_landy_szalay, xi_natural
    # n = 5 bodies (10 pairs), m = 4 randoms (6 pairs, 20 cross pairs): every normalised count below is a dyadic
    # fraction, so the expected values are exact.
    #   bin 0: DD' = 5/10, DR' = 10/20, RR' = 3/6  ->  (0.5 - 1 + 0.5) / 0.5 = 0
    #   bin 1: DD' = 10/10, DR' = 10/20, RR' = 3/6 ->  (1 - 1 + 0.5) / 0.5 = 1
    #   bin 2: DD' = 10/10, DR' = 5/20, RR' = 6/6  ->  (1 - 0.5 + 1) / 1 = 1.5
    #   bin 3: RR = 0 -> nan
    xi = xi_landy_szalay([5, 10, 10, 4], [10, 10, 5, 3], [3, 3, 6, 0], 5, 4)
    assert xi.dtype == np.float64 and xi[:3].tolist() == [0.0, 1.0, 1.5] and np.isnan(xi[3])
    # Davis-Peebles: (2 m / (n - 1)) DD / DR - 1 = 2 DD / DR - 1 here
    xi = xi_davis_peebles([10, 5, 0, 4], [10, 20, 7, 0], 5, 4)
    assert xi.dtype == np.float64 and xi[:3].tolist() == [1.0, -0.5, -1.0] and np.isnan(xi[3])
    assert np.isnan(xi_landy_szalay([0], [0], [0], 5, 4)[0]) and np.isnan(xi_davis_peebles([0], [0], 5, 4)[0])
    # DR at its expectation.  For points without correlation to the bodies a random point sees, per bin, the fraction
    # of the bodies that a random point sees of the other random points: E[DR / (n m)] = RR / (m (m - 1) / 2), that is
    # DR' = RR'.  Then (DD' - 2 DR' + RR') / RR' = (DD' - RR') / RR' = DD' / RR' - 1, the natural estimator.  In counts:
    # DR = RR x n m / (m (m - 1) / 2) = 2 n RR / (m - 1).  n = 11, m = 21: DR = 1.1 RR, integers for RR = 210, 420, 630.
    n, m = 11, 21
    dd, rr = np.array([110, 55, 7]), np.array([210, 420, 630])
    dr = 2 * n * rr // (m - 1)
    assert (dr * (m - 1) == 2 * n * rr).all()
    ls, nat = xi_landy_szalay(dd, dr, rr, n, m), xi_natural(dd, rr, n, m)
    assert np.abs(ls - nat).max() <= 8.0 * np.finfo(np.float64).eps * np.abs(nat).max()  # (other roundings, the same value)
    assert abs(nat[0] - 1.0) < 1e-15  # DD' = 2, RR' = 1


def test_counts_within_and_sphere_density():
    from nbody.pairs import counts_within, sphere_density
    rows = np.array([[1, 0, 2, 5], [0, 0, 0, 0], [3, 1, 0, 2 ** 30]], dtype=np.int32)
    within = counts_within(rows)
    assert within.dtype == np.int64 and within.tolist() == [[1, 1, 3, 8], [0, 0, 0, 0], [3, 4, 4, 4 + 2 ** 30]]
    big = counts_within(np.full((1, 3), 2 ** 31 - 1, dtype=np.int32))
    assert big[0, 2] == 3 * (2 ** 31 - 1)  # summed in 64 bits
    edges = np.array([0.0, 1.0, 2.0, 4.0])
    rho = sphere_density(rows, edges, mass=2.0)
    vol = 4.1887902047863905 * edges ** 3
    assert rho.shape == (3, 4) and rho.dtype == np.float64
    assert rho[0, 0] == np.inf and np.isnan(rho[1, 0]) and rho[2, 0] == np.inf  # a zero radius: inf with a body, nan without
    assert np.array_equal(rho[:, 1:], 2.0 * within[:, 1:] / vol[1:])
    assert sphere_density(rows, edges)[0, 3] == 8.0 / vol[3]
    with pytest.raises(ValueError, match="columns"):
        sphere_density(rows, edges[:3])


def test_header_declares_and_library_exports_the_call():
    import nbmi_native
    text = open(os.path.join(ROOT, "include", "nbmi.h")).read()
    assert re.search(r"^int nbmi_pair_counts_at\(nbmi_sim \*sim, int64_t m, const double \*points_xyz", text, re.M)
    assert len(nbmi_native.PROTOTYPES["nbmi_pair_counts_at"][1]) == 10
    assert hasattr(ctypes.CDLL(nbmi_native.LIB_PATH), "nbmi_pair_counts_at")
    for word in ("per_point[i][0]", "body j minus point i", "a point is not a body", "at most 272 MB", "NBMI_FIELD_SORT=0 honoured",
                 '"nbmi_pair_counts_at: ..."'):
        assert word in text, word


def test_python_classes_refuse_without_a_device():
    from nbody.gpu_backend import HIPBarnesHutSimulation, HIPDirectSimulation, HIPOwnerSimulation
    pts, good = np.zeros((5, 3)), [1.0, 2.0]
    for cls, word in ((HIPDirectSimulation, "direct"), (HIPOwnerSimulation, "owner")):
        sim = cls.__new__(cls)  # no handle and no library: the refusal must come before any library call
        sim._h = None
        for call in (lambda: sim.pair_counts_at(pts, good), lambda: sim.pair_counts_at(pts, good, per_point=True, evals=True),
                     lambda: sim.neighbour_counts(good),
                     lambda: sim.correlation_function(good, pts, estimator="landy-szalay"),
                     lambda: sim.correlation_function(good, pts, estimator="davis-peebles")):
            with pytest.raises(ValueError, match=word):
                call()
    sim = HIPBarnesHutSimulation.__new__(HIPBarnesHutSimulation)
    sim._h = None
    for bad in (np.zeros(3), np.zeros((5, 2)), np.zeros((2, 3, 3)), np.zeros((3, 5))):
        with pytest.raises(ValueError, match=r"pair_counts_at: expected points of shape \(m, 3\)"):
            sim.pair_counts_at(bad, good)
    for bad in ([1.0], [], [1.0, 1.0], [2.0, 1.0], [-1.0, 1.0], [0.0, np.inf], [0.0, np.nan], list(range(67)), [1e-200, 2e-200],
                [1e200, 1e201]):
        with pytest.raises(ValueError, match="edges"):
            sim.pair_counts_at(pts, bad)
    for name in ("Landy-Szalay", "ls", "", None, "hamilton"):
        with pytest.raises(ValueError, match="estimator"):
            sim.correlation_function(good, pts, estimator=name)
