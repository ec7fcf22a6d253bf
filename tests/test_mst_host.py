"""The host side of nbmi_mst (include/nbmi.h) without a device: the two forms of the restatement
in tests/mst_ref.py against each other, nbody/mst.py's consumers against the friends-of-friends restatement and SciPy,
the header's declaration and the Python classes' refusals."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import fof_ref as fr
import mst_ref as mr
import query_cases as qc
from conftest import ROOT
from nbody import mst

SMALL = ("n1", "n2", "n9", "n65", "n2049")


def _lattice_subset():
    """1 500 points of the shuffled 16^3 lattice: every d2 is a small integer, nearly every tree edge ties another"""
    return qc.lattice()[0][:1500]


def _tree(name):
    p = _lattice_subset() if name == "lattice1500" else qc.system(name)[0]
    return p, mr.reference(name, p)


@pytest.mark.parametrize("name", SMALL + ("lattice1500",))
def test_prim_and_kruskal_agree_exactly(name):
    p, (edges, d2) = _tree(name)
    ke, kd = mr.kruskal(p)
    n = len(p)
    assert edges.dtype == np.int32 and d2.dtype == np.float64 and edges.shape == (max(n - 1, 0), 2)
    assert np.array_equal(edges, ke) and np.array_equal(d2, kd)
    assert (edges[:, 0] < edges[:, 1]).all()
    assert np.array_equal(d2, fr.d2_pairs(p, edges[:, 0], edges[:, 1]))
    key = np.lexsort((edges[:, 1], edges[:, 0], d2))
    assert np.array_equal(key, np.arange(len(d2)))  # ascending by (d2, i, j)
    if name == "lattice1500":
        _, counts = np.unique(d2, return_counts=True)
        ties = int(counts[counts > 1].sum())
        print(f"lattice subset: {ties} of {len(d2)} edges share their d2 with another, {int((d2 == 1.0).sum())} have d2 == 1.0")
        assert ties >= 1400  # what the case is for: the order is decided by the indices nearly everywhere
    if n >= 2:  # spanning: one component when nothing is cut
        assert (mst.cut(n, edges, d2, 2.0 * math.sqrt(d2[-1]) + 1.0) == 0).all()


CUTS = [("n2049", 8.0), ("n2049", 16.0), ("n65", 30.0), ("n2", 5.0), ("n2", 4.999), ("n9", 50.0), ("n1", 1.0),
        ("lattice1500", 1.0), ("lattice1500", float(np.nextafter(1.0, 0.0))), ("trap", 1e-4), ("trap", 2e-3), ("far", 5.0),
        ("far", 2.0e6)]


@pytest.mark.parametrize("name,link", CUTS, ids=[f"{n}-{b}" for n, b in CUTS])
def test_cut_is_friends_of_friends(name, link):
    p, (edges, d2) = _tree(name)
    lab, groups = fr.fof(p, link)
    got = mst.cut(len(p), edges, d2, link)
    assert got.dtype == np.int32 and np.array_equal(got, lab)
    assert mst.group_count(len(p), d2, link) == groups
    assert int((d2 <= link * link).sum()) == len(p) - groups


def test_n2_equality_links():
    p, (edges, d2) = _tree("n2")
    assert edges.tolist() == [[0, 1]] and d2.tolist() == [25.0]
    assert mst.group_count(2, d2, 5.0) == 1 and mst.group_count(2, d2, 4.999) == 2


@pytest.mark.parametrize("name", ("n65", "n2049"))
def test_linkage_against_scipy(name):
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    p, (edges, d2) = _tree(name)
    assert len(np.unique(d2)) == len(d2)  # tie-free: SciPy orders ties its own way
    Z = mst.linkage(len(p), edges, d2)
    ref = hier.linkage(p, method="single")
    assert Z.shape == ref.shape == (len(p) - 1, 4) and Z.dtype == np.float64
    # heights: the root of the same three squares, but SciPy's pdist sums them in its own order and may fuse: each sum is
    # within 3 roundings of the exact one, the root halves that and adds one: 2^-50 covers both sides
    err = np.abs(Z[:, 2] - ref[:, 2]) / ref[:, 2]
    print(f"{name}: largest relative height difference {err.max():.3e} (bound 2^-50 = {2.0 ** -50:.3e})")
    assert (err <= 2.0 ** -50).all()
    assert np.array_equal(Z[:, 3], ref[:, 3])
    assert np.array_equal(Z[:, :2], ref[:, :2])  # tie-free: the same merges under the same numbering
    assert (Z[:, 0] < Z[:, 1]).all() and Z[-1, 3] == len(p)


def test_linkage_by_hand():
    # bodies on a line at 0, 1, 3, 7: merges (0, 1) at 1, then with 2 at 2, then with 3 at 4
    edges = np.array([[0, 1], [1, 2], [2, 3]], np.int32)
    Z = mst.linkage(4, edges, np.array([1.0, 4.0, 16.0]))
    assert Z.tolist() == [[0.0, 1.0, 1.0, 2.0], [2.0, 4.0, 2.0, 3.0], [3.0, 5.0, 4.0, 4.0]]
    with pytest.raises(ValueError, match="cycle"):
        mst.linkage(3, np.array([[0, 1], [0, 1]], np.int32), np.array([1.0, 1.0]))
    with pytest.raises(ValueError, match="expected 3 edges"):
        mst.linkage(4, edges[:2], np.array([1.0, 4.0]))
    assert mst.linkage(1, np.empty((0, 2), np.int32), np.empty(0)).shape == (0, 4)


@pytest.mark.parametrize("name", ("n9", "n2049", "lattice1500"))
def test_link_for_groups_is_inverse_to_group_count(name):
    p, (edges, d2) = _tree(name)
    n = len(p)
    for g in sorted({1, 2, 3, n // 2, n - 1, n}):
        link = mst.link_for_groups(n, d2, g)
        if g >= n:
            assert link == 0.0
            continue
        got = mst.group_count(n, d2, link)
        assert got <= g
        # the smallest such link: one float64 below it there are more than g groups
        below = float(np.nextafter(link, 0.0))
        assert mst.group_count(n, d2, below) > g
        # and exactly g unless the (n - g)-th edge ties the next one
        k = n - g
        if k == len(d2) or d2[k] > d2[k - 1]:
            assert got == g
    for g in (0, -1):
        with pytest.raises(ValueError, match="n_groups"):
            mst.link_for_groups(n, d2, g)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="linking length"):
            mst.group_count(n, d2, bad)


def test_coincident_bodies_join_at_every_link():
    p = np.array([[1.0, 2.0, 3.0]] * 3 + [[4.0, 2.0, 3.0]])
    edges, d2 = mr.prim(p)
    ke, kd = mr.kruskal(p)
    assert np.array_equal(edges, ke) and np.array_equal(d2, kd)
    assert edges.tolist() == [[0, 1], [0, 2], [0, 3]] and d2.tolist() == [0.0, 0.0, 9.0]
    link = mst.link_for_groups(4, d2, 2)
    assert link > 0.0 and mst.group_count(4, d2, link) == 2
    assert mst.cut(4, edges, d2, link).tolist() == [0, 0, 0, 3]


def test_header_declares_and_library_exports_the_call():
    import nbmi_native
    text = open(os.path.join(ROOT, "include", "nbmi.h")).read()
    assert re.search(r"^int nbmi_mst\(nbmi_sim \*sim, int32_t \*edge_i", text, re.M)
    assert len(nbmi_native.PROTOTYPES["nbmi_mst"][1]) == 6
    assert hasattr(ctypes.CDLL(nbmi_native.LIB_PATH), "nbmi_mst")
    for word in ("(d2(i, j), i, j)", "symmetric in i and j bit for bit", "N - n_groups", "ceil(log2 N)", '"nbmi_mst: ..."',
                 "freed by nbmi_destroy"):
        assert word in text, word


def test_python_classes_refuse_without_a_device():
    from nbody.gpu_backend import HIPDirectSimulation, HIPOwnerSimulation
    for cls, word in ((HIPDirectSimulation, "direct"), (HIPOwnerSimulation, "owner")):
        sim = cls.__new__(cls)  # no handle and no library: the refusal must come before any library call
        sim._h = None
        for call in (lambda: sim.minimum_spanning_tree(), lambda: sim.minimum_spanning_tree(evals=True)):
            with pytest.raises(ValueError, match=word):
                call()
