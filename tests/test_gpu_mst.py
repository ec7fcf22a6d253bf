"""nbmi_mst on the GPU against the NumPy restatement of tests/mst_ref.py (include/nbmi.h).

Everything is compared EXACTLY: under the strict order (d2, i, j) on pairs the tree is unique, d2 is formed by the kernel
and by NumPy with the same three products and two sums, and the output is sorted by that key - so the device's arrays are
the restatement's, dtypes included, and cutting them gives nbmi_fof's labels on the same handle.
"""
import math

import numpy as np
import pytest

import mst_ref as mr
import query_cases as qc
from nbody import mst
from query_cases import bh as _bh
from test_gpu_fof import CASES as FOF_CASES

pytestmark = pytest.mark.gpu

NBMI_ERR_ARG = -1
NBMI_ERR_CAPACITY = -4
PRESETS = ("galaxy", "collision", "filament")
_SYS = {}


def _system(name):
    """positions of a system: query_cases' small ones, the presets at n = 8 000 (the dense Prim takes 5.6 s at 20 000)"""
    if name not in _SYS:
        _SYS[name] = qc.preset(name, n=8000)[0] if name in PRESETS else qc.system(name)[0]
    return _SYS[name]


def _reference(name):
    return mr.reference("gpu-" + name, _system(name))


def _check(tag, got, ref):
    edges, d2 = got[0], got[1]
    assert edges.dtype == np.int32 and d2.dtype == np.float64 and edges.shape == ref[0].shape and d2.shape == ref[1].shape, tag
    bad = np.nonzero((edges != ref[0]).any(axis=1) | (d2 != ref[1]))[0]
    print(f"{tag}: {len(bad)} of {len(d2)} edges differ from the reference")
    assert np.array_equal(edges, ref[0]) and np.array_equal(d2, ref[1]), (tag, bad[:8], edges[bad[:8]], ref[0][bad[:8]])


def _nearest_d2(n, edges, d2):
    """every body's nearest-neighbour d2: its nearest neighbour's edge is in the tree"""
    nn = np.full(n, np.inf)
    np.minimum.at(nn, edges[:, 0], d2)
    np.minimum.at(nn, edges[:, 1], d2)
    return nn


EXACT = ("n2", "n9", "n65", "n2049", "n4097", "trap", "far") + PRESETS


@pytest.mark.parametrize("name", EXACT)
def test_edges_exact_against_the_reference(gpu, name):
    p = _system(name)
    n = len(p)
    ref = _reference(name)
    e, d = ref
    # what the case is for, on the reference
    if name in PRESETS:
        below = int((d < np.median(_nearest_d2(n, e, d))).sum())
        print(f"{name}: {below} edges below the median nearest-neighbour d2")
        assert n == 8000 and below >= 2000, (name, "the case lost its point")
    elif name == "trap":
        assert (d < (2e-3) ** 2).sum() >= 2000 and (d > 1.0).sum() >= 2000
    elif name == "far":
        assert 4096 in e[-1].tolist() and d[-1] > 1e10 and (np.sort(e[:-1].ravel())[-1] < 4096)
    elif name == "n2049":
        assert n % 64 == 1  # the last wave has one lane
    sim = _bh(p)
    try:
        edges, d2, rounds, evals = sim.minimum_spanning_tree(evals=True)
        print(f"{name}: n {n}, rounds {rounds}, evals {evals} ({evals / n:.1f} per body)")
        _check(name, (edges, d2), ref)
        assert 1 <= rounds <= math.ceil(math.log2(n))
    finally:
        sim.close()


def test_ties_on_the_lattice(gpu):
    """16^3 integer lattice, spacing 1, shuffled: all 4 095 edges have d2 == 1.0 and the edge set is decided by the indices
    alone - lost by a comparison on d2 only, by < pruning at the bound, or by a mutual edge emitted twice"""
    p = qc.lattice()[0]
    ref = mr.reference("gpu-lattice", p)
    assert (ref[1] == 1.0).all() and len(ref[1]) == 4095
    sim = _bh(p)
    try:
        got = sim.minimum_spanning_tree()
        assert (got[1] == 1.0).all()
        _check("lattice", got, ref)
    finally:
        sim.close()


def test_coincident_twins(gpu):
    """test_gpu_fof's twins: every position held twice, eps = 0: the first 2 048 edges have d2 == 0 and are exactly the
    pairs (k, k + 2048)"""
    rng = np.random.RandomState(9)
    base = rng.uniform(-1e-9, 1e-9, (2048, 3))
    p = np.concatenate([base, base])
    ref = mr.reference("gpu-twins", p)
    sim = _bh(p, eps=0.0)
    try:
        edges, d2 = sim.minimum_spanning_tree()
        assert (d2[:2048] == 0.0).all() and (d2[2048:] > 0.0).all()
        assert np.array_equal(edges[:2048], np.stack([np.arange(2048), np.arange(2048) + 2048], 1))
        _check("twins", (edges, d2), ref)
    finally:
        sim.close()


CUT_SYSTEMS = [s for s in EXACT if any(n == s for n, _, _ in FOF_CASES)]


@pytest.mark.parametrize("name", CUT_SYSTEMS)
def test_cut_is_fof_on_the_same_handle(gpu, name):
    p = _system(name)
    n = len(p)
    links = [b for s, b, _ in FOF_CASES if s == name]
    assert links and (name != "n2" or links == [5.0, 4.999])  # n2: linked at equality, and not linked just below
    sim = _bh(p)
    try:
        edges, d2 = sim.minimum_spanning_tree()
        for b in links:
            lab = sim.find_groups(b)
            kept = int((d2 <= b * b).sum())
            print(f"{name} b={b}: groups {sim.n_groups}, edges kept {kept}")
            assert kept == n - sim.n_groups and mst.group_count(n, d2, b) == sim.n_groups
            got = mst.cut(n, edges, d2, b)
            assert got.dtype == np.int32 and np.array_equal(got, lab), (name, b)
    finally:
        sim.close()


def test_two_calls_and_another_history(gpu):
    p, v, m = qc.preset("galaxy", n=8000)
    sim = _bh(p, v, m)
    try:
        first = sim.minimum_spanning_tree(evals=True)
        again = sim.minimum_spanning_tree(evals=True)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
        assert first[2:] == again[2:]  # rounds, and evals: no wave sees another's progress
        sim.step_many(0.2, 3)
        sim.sync()
        sim.set_state(p, v)  # the same state, but the key order now has another history
        later = sim.minimum_spanning_tree()
        assert first[0].tobytes() == later[0].tobytes() and first[1].tobytes() == later[1].tobytes()
        _check("galaxy after steps and set_state", later, _reference("galaxy"))
    finally:
        sim.close()


def test_quadrupole_and_leapfrog_handles_give_the_same_arrays(gpu):
    p, v, m = qc.preset("galaxy", n=8000)
    ref = _reference("galaxy")
    for kw in ({"multipole": "quadrupole"}, {"integrator": "leapfrog"}):
        sim = _bh(p, v, m, **kw)
        try:
            _check(str(kw), sim.minimum_spanning_tree(), ref)
        finally:
            sim.close()


def test_permuted_caller_order(gpu):
    p = _system("n2049")
    ref = _reference("n2049")
    assert len(np.unique(ref[1])) == len(ref[1])  # tie-free: the edge set does not depend on the indices
    perm = np.random.RandomState(12).permutation(len(p))
    sim = _bh(p[perm])
    try:
        edges, d2 = sim.minimum_spanning_tree()
        assert np.array_equal(d2, ref[1])
        back = np.sort(perm[edges], axis=1)  # body k of the permuted call is body perm[k]
        assert np.array_equal(back, ref[0].astype(back.dtype))
    finally:
        sim.close()


def test_hooks_and_tiny_handles(gpu):
    p = _system("galaxy")
    n = len(p)
    sim = _bh(p)
    try:
        _e, _d, rounds, evals = sim.minimum_spanning_tree(evals=True)
        print(f"galaxy n = {n}: rounds {rounds}, evals {evals} = {evals / n:.1f} per body (all pairs: {n * (n - 1) // 2})")
        assert 1 <= rounds <= math.ceil(math.log2(n))
        assert 0 < evals < n * (n - 1) // 2
    finally:
        sim.close()
    for rows in (np.empty((0, 3)), np.array([[1.0, 2.0, 3.0]])):
        sim = _bh(rows)
        try:
            edges, d2, rounds, evals = sim.minimum_spanning_tree(evals=True)
            assert edges.shape == (0, 2) and edges.dtype == np.int32 and d2.shape == (0,) and d2.dtype == np.float64
            assert rounds == 0 and evals == 0
        finally:
            sim.close()


@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
def test_the_call_does_not_disturb_the_run(gpu, integrator):
    p, v, m = qc.preset("galaxy", n=8000)
    rng = np.random.RandomState(21)
    tp, tv = rng.uniform(-400.0, 400.0, (300, 3)), rng.uniform(-1.0, 1.0, (300, 3))

    def run(query):
        sim = _bh(p, v, m, integrator=integrator)
        try:
            sim.set_force_precision("auto")
            sim.set_tracers(tp, tv)
            shares = []
            for i in range(4):
                if query:
                    sim.minimum_spanning_tree()
                sim.step(0.2)
                shares.append(sim.force_precision_share())
            return (sim.get_positions_f64(), sim.get_velocities(), *sim.get_tracers(), sim.step_count(), shares,
                    sim.tree_stats())
        finally:
            sim.close()
    a, b = run(False), run(True)
    for k in range(4):
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k
    assert a[4] == b[4] == 4
    assert a[5] == b[5], (a[5], b[5])
    assert a[6] == b[6], (a[6], b[6])


def test_refusals(gpu):
    from nbody.gpu_backend import HIPBarnesHutSimulation, HIPDirectSimulation, HIPOwnerSimulation
    from nbody.sharded import let_capacities
    lib = gpu.load()
    rng = np.random.RandomState(1)
    n = 256
    p, v, m = rng.uniform(-10, 10, (n, 3)), np.zeros((n, 3)), np.ones(n)
    ei, ej, d2 = np.empty(n - 1, np.int32), np.empty(n - 1, np.int32), np.empty(n - 1)
    direct = HIPDirectSimulation(p, v, m, 0.07, 1.5, 1.0)
    cap, let_cap = let_capacities(n, 1)
    owner = HIPOwnerSimulation(p, v, m, np.arange(n, dtype=np.int32), cap, let_cap, 1, 0, 0.07, 1.5, 1.0)
    shard = HIPBarnesHutSimulation(p, v, m, 0.07, 1.5, 1.0, 0.5)
    try:
        shard.set_shard(0, n // 2)
        for sim, needle in ((direct, "direct N^2"), (owner, "owner-mode"), (shard, "sharded")):
            rc = lib.nbmi_mst(sim._h, gpu.ptr(ei), gpu.ptr(ej), gpu.ptr(d2), None, None)
            msg = gpu.last_error()
            assert rc == NBMI_ERR_ARG and "nbmi_mst: " in msg and needle in msg, (rc, msg)
        for sim in (direct, owner):  # the Python classes refuse on their own
            with pytest.raises(ValueError):
                sim.minimum_spanning_tree()
        with pytest.raises(ValueError, match="sharded"):
            shard.minimum_spanning_tree()
        shard.set_shard(0, n)
        _check("after the refusal", shard.minimum_spanning_tree(), mr.prim(p))
    finally:
        for sim in (direct, owner, shard):
            sim.close()


def test_capacity_error_is_a_steps_and_the_handle_goes_on(gpu):
    """test_gpu_fof's capacity input: one position held by 70 bodies at +-50 needs more node rows than 4 N"""
    lib = gpu.load()
    rng = np.random.RandomState(9)
    base = rng.uniform(-50.0, 50.0, (2048, 3))
    p = np.concatenate([base, base])
    p[2049:2049 + 68] = p[0]
    sim = _bh(p, eps=0.0)
    try:
        n = len(p)
        ei, ej, d2 = np.empty(n - 1, np.int32), np.empty(n - 1, np.int32), np.empty(n - 1)
        rc = lib.nbmi_mst(sim._h, gpu.ptr(ei), gpu.ptr(ej), gpu.ptr(d2), None, None)
        msg = gpu.last_error()
        assert rc == NBMI_ERR_CAPACITY and "octree needs" in msg and "rows allocated" in msg, (rc, msg)
        good = rng.uniform(-50.0, 50.0, (4096, 3))
        sim.set_state(good, np.zeros_like(good))
        _check("after the capacity error", sim.minimum_spanning_tree(), mr.prim(good))
    finally:
        sim.close()
