"""nbmi_pair_counts on the GPU against the NumPy brute force of tests/pairs_ref.py (include/nbmi.h; DESIGN.md section
4.16).

``counts`` and ``below`` are compared EXACTLY in every case: a pair's bin is a function of the float64 value d2(i, j),
which the kernel and NumPy form with the same three products and two sums, of the E[k] = edges[k] * edges[k], one
product each on both sides, and of comparisons; the sums are integers.  Every case first checks on the reference that
its input has the property the case is there for.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import pairs_ref as pr
import query_cases as qc
from query_cases import bh as _bh
from conftest import ROOT

pytestmark = pytest.mark.gpu

NBMI_ERR_ARG = -1
NBMI_ERR_CAPACITY = -4
R_SPAWN = 800.0
LINEAR = np.linspace(0.05 * R_SPAWN, 0.25 * R_SPAWN, 5)  # 5 linear edges out to a quarter of the spawn radius


def _preset(dist, n=20_000, seed=7):
    return qc.preset(dist, n, seed, R_SPAWN, 0.07, scale_masses=False)


def _system(name):
    return qc.system(name)[0]


def _lattice(spacing):
    return qc.lattice(spacing)[0]


def _check(tag, got, ref):
    counts, below = got[0], got[1]
    print(f"{tag}: below {below} (reference {ref[1]}), counts {counts.tolist()} (reference {ref[0].tolist()})")
    assert counts.dtype == np.int64 and below == ref[1] and np.array_equal(counts, ref[0]), tag


def _auto_edges(sim):
    from nbody.pairs import auto_pair_edges
    return np.array(auto_pair_edges(sim.knn(1)[0]))


_PRESET_REF = {}  # name -> (auto edges, reference of the auto edges, reference of the linear edges)


def _preset_reference(name, sim):
    if name not in _PRESET_REF:
        auto = _auto_edges(sim)
        refs = pr.pair_counts_multi(_system(name), [auto, LINEAR])
        _PRESET_REF[name] = (auto, refs[0], refs[1])
    return _PRESET_REF[name]


@pytest.mark.parametrize("name", ["galaxy", "collision", "filament", "cluster"])
def test_presets_exact_with_auto_and_linear_edges(gpu, name):
    p = _system(name)
    sim = _bh(p)
    try:
        auto, ref_auto, ref_lin = _preset_reference(name, sim)
        assert len(auto) == 13 and np.allclose(auto[12] / auto[0], 64.0)  # (from knn(1), which has its own suite)
        assert (ref_auto[0] > 0).all() and (ref_lin[0] > 0).all(), (name, "the case lost its point: an empty bin")
        got = sim.pair_counts(auto, evals=True)
        _check(f"{name} auto", got, ref_auto)
        print(f"    evals / body {got[2] / len(p):.1f}, cell pairs / body {got[3] / len(p):.1f}")
        got = sim.pair_counts(LINEAR, evals=True)
        _check(f"{name} linear", got, ref_lin)
        print(f"    evals / body {got[2] / len(p):.1f}, cell pairs / body {got[3] / len(p):.1f}")
        if name == "galaxy":
            assert got[3] > 0  # cells are counted whole
    finally:
        sim.close()


def _random_edge_sets(seed, count=20):
    """sorted edge sets of every size 1 .. 64 bins' worth of variety: linear and logarithmic, with and without a zero
    first edge, some reaching beyond the +-100 box's diameter of 346"""
    rng = np.random.RandomState(seed)
    sets = []
    for i in range(count):
        nb = int(rng.randint(1, 65))
        if i % 2:
            e = np.sort(rng.uniform(0.0, rng.choice([30.0, 150.0, 400.0]), nb + 1))
        else:
            e = np.sort(10.0 ** rng.uniform(-1.0, 2.6, nb + 1))
        if i % 5 == 0:
            e[0] = 0.0
        assert (np.diff(e * e) > 0.0).all()
        sets.append(e)
    return sets


@pytest.mark.parametrize("name,seed", [("n2049", 21), ("n4097", 22)])
def test_uniform_with_twenty_random_edge_sets(gpu, name, seed):
    p = _system(name)
    sets = _random_edge_sets(seed)
    refs = pr.pair_counts_multi(p, sets)
    assert sum(int(r[0].sum()) for r in refs) > 10 * len(p)
    sim = _bh(p)
    try:
        for i, (e, ref) in enumerate(zip(sets, refs)):
            _check(f"{name} set {i} (nb = {len(e) - 1})", sim.pair_counts(e), ref)
    finally:
        sim.close()


@pytest.mark.parametrize("name,edges", [("trap", [0.0, 1e-4, 5e-4, 2e-3, 50.0, 400.0]), ("trap", "auto"),
                                        ("far", [1.0, 5.0, 25.0, 100.0, 2.0e6]), ("far", "auto")],
                         ids=["trap-given", "trap-auto", "far-given", "far-auto"])
def test_trap_and_far_body(gpu, name, edges):
    p = _system(name)
    sim = _bh(p)
    try:
        e = _auto_edges(sim) if isinstance(edges, str) else np.array(edges)
        ref = pr.pair_counts(p, e)
        if isinstance(edges, str):  # (the median nearest-neighbour distance is the dense part's: the first bins may be empty)
            assert ref[0].sum() > 1000 and (ref[0][-3:] > 0).all()
        else:
            assert (ref[0] > 0).all(), "the case lost its point: an empty bin"
        if name == "far" and not isinstance(edges, str):
            assert ref[0][-1] == 4096 and ref[1] + ref[0].sum() == 4097 * 4096 // 2  # the far body's pairs, and every pair
        _check(f"{name} {edges}", sim.pair_counts(e), ref)
    finally:
        sim.close()


@pytest.mark.parametrize("spacing", [1.0, 33.0])
def test_lattice_decides_the_edge_rule_and_both_bounds(gpu, spacing):
    """16^3 lattice in shuffled caller order, edges at sqrt(1, 2, 3, 4, 5, 6, 8, 9) lattice spacings: thousands of pairs
    sit exactly AT an edge, so a `<` for a `<=`, a cell pruned at equality or a cell accepted whole across an edge changes
    a count.  No float64 squares to 2, 3, 5, 6 or 8, so on the unit lattice only the edges 1, 2 and 3 have E[k] equal to
    an occurring d2 (checked below); at spacing 33 all eight have (33^2 m has an exact root for each m).  Then the same
    with every edge one ulp lower: every pair at an edge moves up a bin."""
    ms = (1, 2, 3, 4, 5, 6, 8, 9)
    s2 = spacing * spacing
    roots = [pr.exact_root(s2 * m) for m in ms]
    if spacing == 1.0:
        assert [r is not None for r in roots] == [True, False, False, True, False, False, False, True]
        edges = np.array([r if r is not None else np.sqrt(float(m)) for r, m in zip(roots, ms)])
    else:
        assert all(r is not None for r in roots)
        edges = np.array(roots)
    exact = np.array([e * e == s2 * m for e, m in zip(edges, ms)])
    p = _lattice(spacing)
    sim = _bh(p)
    try:
        ref = pr.pair_counts(p, edges)
        low = np.nextafter(edges, 0.0)
        ref_low = pr.pair_counts(p, low)
        assert ref[1] == 3 * 15 * 256 and ref[0].sum() > 100_000  # the axis neighbours sit at edges[0]
        if exact.all():
            assert (ref[0] > 0).all()
        # lowering an exact edge moves the pairs AT it up a bin: those pairs exist (C = the pairs within each edge)
        within = [np.concatenate([[r[1]], r[1] + np.cumsum(r[0])]) for r in (ref, ref_low)]
        moved = within[0] - within[1]
        print(f"lattice x {spacing}: pairs that leave each edge when it is lowered by one ulp: {moved.tolist()}")
        assert (moved[exact] > 1000).all() and ref_low[1] == 0
        _check(f"lattice x {spacing}", sim.pair_counts(edges), ref)
        _check(f"lattice x {spacing}, edges one ulp lower", sim.pair_counts(low), ref_low)
    finally:
        sim.close()


def test_coincident_twins(gpu):
    """4 096 bodies, every position held twice (drawn within 1e-9 of the origin so that the tree fits, as DESIGN 4.14's
    test says): with edges[0] = 0, `below` counts the coincident pairs"""
    rng = np.random.RandomState(9)
    base = rng.uniform(-1e-9, 1e-9, (2048, 3))
    p = np.concatenate([base, base])
    edges = np.array([0.0, 1e-12, 1e-10, 1e-9, 4e-9])
    ref = pr.pair_counts(p, edges)
    assert ref[1] >= 2048 and (ref[0][1:] > 0).all()
    sim = _bh(p, eps=0.0)
    try:
        got = sim.pair_counts(edges)
        _check("twins", got, ref)
        assert got[1] >= 2048
    finally:
        sim.close()


def test_small_sizes(gpu):
    two = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]])  # d2 = 25 exactly
    for p, edges, want in ((np.empty((0, 3)), [1.0, 2.0], ([0], 0)), (np.array([[1.0, 2.0, 3.0]]), [1.0, 2.0], ([0], 0)),
                           (two, [1.0, 5.0, 9.0], ([1, 0], 0)),                       # at equality: the upper edge belongs to the bin
                           (two, [5.0, 9.0], ([0], 1)),                                # ... and to `below`
                           (two, [1.0, np.nextafter(5.0, 0.0), 9.0], ([0, 1], 0)),     # just outside the first bin
                           (two, [1.0, np.nextafter(5.0, 9.0), 9.0], ([1, 0], 0)),     # just inside
                           (two, [1.0, 4.0], ([0], 0))):
        sim = _bh(p)
        try:
            got = sim.pair_counts(edges, evals=True)
            assert got[0].tolist() == want[0] and got[1] == want[1], (len(p), edges, got)
            if len(p) < 2:
                assert got[2] == 0 and got[3] == 0
        finally:
            sim.close()
    for n in (64, 65, 129):  # a full wave; a last wave with one valid lane
        p = qc.uniform(n, n)[0]
        edges = [0.0, 20.0, 60.0, 120.0, 400.0]
        ref = pr.pair_counts(p, edges)
        assert ref[1] + ref[0].sum() == n * (n - 1) // 2 and (ref[0] > 0).all()
        sim = _bh(p)
        try:
            _check(f"n = {n}", sim.pair_counts(edges), ref)
        finally:
            sim.close()


def test_extremes_of_nb_and_edges(gpu):
    p = _system("n4097")
    n = len(p)
    pairs = n * (n - 1) // 2
    sets = {"nb1": np.array([10.0, 30.0]), "nb64": np.linspace(0.0, 352.0, 65),  # (the box's diameter is 346.4)
            "first edge beyond the diameter": np.array([400.0, 500.0, 600.0]),
            "edges that reach nothing": np.array([1e-9, 1e-8, 1e-7])}
    refs = dict(zip(sets, pr.pair_counts_multi(p, list(sets.values()))))
    assert refs["nb64"][1] + refs["nb64"][0].sum() == pairs and refs["nb64"][2] == 0 and (refs["nb64"][0] > 0).sum() >= 60
    assert refs["first edge beyond the diameter"][1] == pairs and refs["edges that reach nothing"][2] == pairs
    assert refs["nb1"][0][0] > 0
    sim = _bh(p)
    try:
        for tag, e in sets.items():
            got = sim.pair_counts(e)
            _check(tag, got, refs[tag])
        assert sim.pair_counts(sets["nb64"])[0].sum() == pairs
        got = sim.pair_counts(sets["first edge beyond the diameter"])
        assert got[1] == pairs and not got[0].any()
        got = sim.pair_counts(sets["edges that reach nothing"])
        assert got[1] == 0 and not got[0].any()
    finally:
        sim.close()


def test_without_whole_cells_the_same_numbers(gpu, tmp_path):
    """NBMI_PAIRS_CELLS=0 is read when the handle is created: a fresh child process counts three of the inputs above
    without ever accepting a cell whole - the same numbers by an independent path, cell_pairs == 0 and more distances"""
    cases = [("galaxy", LINEAR), ("n4097", _random_edge_sets(22)[1]), ("lattice33", np.array([pr.exact_root(1089.0 * m) for m in (1, 2, 3, 4)]))]
    files = []
    for i, (name, e) in enumerate(cases):
        f = str(tmp_path / f"case{i}.npz")
        np.savez(f, p=_system(name), edges=e)
        files.append(f)
    out = str(tmp_path / "out.npz")
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import __graft_entry__ as g; g._import_package();"
            "from nbody.gpu_backend import HIPBarnesHutSimulation as H;"
            "res = {};\n"
            "for i, f in enumerate(sys.argv[2:]):\n"
            "    d = np.load(f); p = d['p']\n"
            "    s = H(p, np.zeros_like(p), np.ones(len(p)), 0.07, 1.5, 1.0, 0.5)\n"
            "    c, b, ev, cp = s.pair_counts(d['edges'], evals=True); s.close()\n"
            "    res['c%%d' %% i] = c; res['x%%d' %% i] = np.array([b, ev, cp], dtype=np.int64)\n"
            "np.savez(sys.argv[1], **res)") % ROOT
    subprocess.run([sys.executable, "-c", code, out, *files], env=dict(os.environ, NBMI_PAIRS_CELLS="0"), check=True, timeout=300)
    child = np.load(out)
    for i, (name, e) in enumerate(cases):
        sim = _bh(_system(name))
        try:
            got = sim.pair_counts(e, evals=True)
        finally:
            sim.close()
        ref = _PRESET_REF[name][2] if name in _PRESET_REF else pr.pair_counts(_system(name), e)
        _check(f"{name} default", got, ref)
        b, ev, cp = (int(x) for x in child[f"x{i}"])
        print(f"    {name}: evals {got[2]} with whole cells ({got[3]} pairs through them), {ev} without")
        _check(f"{name} NBMI_PAIRS_CELLS=0", (child[f"c{i}"], b), ref)
        assert cp == 0 and ev >= got[2]
        if name == "galaxy":
            assert got[3] > 0 and ev > got[2]


def test_work_is_actually_saved(gpu):
    """conditions, not measurements: whole cells save distances, and pruning does"""
    from nbody.pairs import auto_pair_edges
    p = _system("n4097")
    n = len(p)
    sim = _bh(p)
    try:
        c, below, ev, cp = sim.pair_counts([0.0, 1.0e6], evals=True)
        print(f"uniform n = 4 097, one bin [0, 1e6]: {ev} distances ({ev / n:.1f} per body), {cp} pairs through whole cells; "
              f"a half walk without them evaluates {n * (n - 1) // 2}")
        assert below == 0 and c[0] == n * (n - 1) // 2 and ev + cp == n * (n - 1) // 2
        assert ev < n * (n - 1) / 8
        d1 = auto_pair_edges(sim.knn(1)[0])[2]  # the median nearest-neighbour distance
        e = [0.0, 2.0 * d1]
        c, below, ev, cp = sim.pair_counts(e, evals=True)
        print(f"last edge 2 d1 = {2.0 * d1:.3f}: {ev} distances ({ev / n:.1f} per body), {c[0]} pairs")
        _check("2 d1", (c, below), pr.pair_counts(p, e))
        assert c[0] > n / 4 and 0 < ev < n * n / 4
    finally:
        sim.close()


def test_other_handle_states_and_repeat_calls(gpu):
    p, v, m = _preset("galaxy", 4096, seed=3)
    edges = np.array([0.0, 3.0, 6.0, 12.0, 24.0, 48.0, 200.0])
    ref = pr.pair_counts(p, edges)
    assert (ref[0] > 0).all()
    for kw in ({}, {"multipole": "quadrupole"}, {"integrator": "leapfrog"}):
        sim = _bh(p, v, m, **kw)
        try:
            a = sim.pair_counts(edges, evals=True)
            b = sim.pair_counts(edges, evals=True)
            _check(str(kw), a, ref)
            assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], "two calls differ"
        finally:
            sim.close()
    sim = _bh(p, v, m)
    try:
        sim.step_many(0.2, 3)  # the state is now in key order: the counts are of the current positions
        x = sim.get_positions_f64()
        ref = pr.pair_counts(x, edges)
        _check("after 3 steps", sim.pair_counts(edges), ref)
    finally:
        sim.close()


@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
def test_pair_counts_do_not_disturb_the_run(gpu, integrator):
    p, v, m = _preset("galaxy")

    def run(query):
        sim = _bh(p, v, m, integrator=integrator)
        try:
            sim.set_force_precision("auto")
            shares = []
            for i in range(12):
                if query and i % 3 == 0:
                    sim.pair_counts(LINEAR)
                sim.step(0.2)
                shares.append(sim.force_precision_share())
            return sim.get_positions_f64(), sim.get_velocities(), sim.step_count(), shares
        finally:
            sim.close()
    a, b = run(False), run(True)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
    assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    assert a[2] == b[2] == 12
    assert a[3] == b[3], (a[3], b[3])


def test_capacity_error_is_a_steps_and_the_handle_goes_on(gpu):
    """DESIGN 4.14's capacity input: one position held by 70 bodies at +-50 needs more node rows than 4 N"""
    lib = gpu.load()
    rng = np.random.RandomState(9)
    base = rng.uniform(-50.0, 50.0, (2048, 3))
    p = np.concatenate([base, base])
    p[2049:2049 + 68] = p[0]
    sim = _bh(p, eps=0.0)
    try:
        edges = np.array([0.0, 1.0, 8.0])
        counts = np.zeros(2, np.int64)
        below = np.zeros(1, np.int64)
        rc = lib.nbmi_pair_counts(sim._h, 2, gpu.ptr(edges), gpu.ptr(counts), gpu.ptr(below), None, None)
        msg = gpu.last_error()
        assert rc == NBMI_ERR_CAPACITY and "octree needs" in msg and "rows allocated" in msg, (rc, msg)
        good = rng.uniform(-50.0, 50.0, (4096, 3))
        sim.set_state(good, np.zeros_like(good))
        _check("after the capacity error", sim.pair_counts(edges), pr.pair_counts(good, edges))
    finally:
        sim.close()


def test_refusals_leave_handle_and_state_untouched(gpu):
    from nbody.gpu_backend import HIPBarnesHutSimulation, HIPDirectSimulation, HIPOwnerSimulation
    from nbody.sharded import let_capacities
    lib = gpu.load()
    rng = np.random.RandomState(1)
    n = 256
    p, v, m = rng.uniform(-10, 10, (n, 3)), np.zeros((n, 3)), np.ones(n)
    counts = np.zeros(64, np.int64)
    below = np.zeros(1, np.int64)
    good = np.array([0.0, 2.0, 4.0])

    def refused(sim, nb, edges, *needles):
        rc = lib.nbmi_pair_counts(sim._h, nb, gpu.ptr(edges) if edges is not None else None, gpu.ptr(counts), gpu.ptr(below),
                                  None, None)
        msg = gpu.last_error()
        assert rc == NBMI_ERR_ARG and msg.startswith("nbmi_pair_counts: "), (rc, msg)
        for s in needles:
            assert s in msg, (s, msg)

    direct = HIPDirectSimulation(p, v, m, 0.07, 1.5, 1.0)
    cap, let_cap = let_capacities(n, 1)
    owner = HIPOwnerSimulation(p, v, m, np.arange(n, dtype=np.int32), cap, let_cap, 1, 0, 0.07, 1.5, 1.0)
    shard = HIPBarnesHutSimulation(p, v, m, 0.07, 1.5, 1.0, 0.5)
    bh = HIPBarnesHutSimulation(p, v, m, 0.07, 1.5, 1.0, 0.5)
    try:
        shard.set_shard(0, n // 2)
        for sim, needle in ((direct, "direct N^2"), (owner, "owner-mode"), (shard, "sharded")):
            refused(sim, 2, good, needle)
        for sim in (direct, owner):  # the Python classes refuse on their own
            with pytest.raises(ValueError):
                sim.pair_counts(good)
        with pytest.raises(ValueError, match="sharded"):
            shard.pair_counts(good)
        bh.compute_colors(15.0)
        before = (bh.get_positions_f64(), bh.get_velocities(), bh.get_colors(), bh.step_count())
        refused(bh, 0, good, "nb = 0")
        refused(bh, 65, np.arange(66.0), "nb = 65")
        refused(bh, -1, good, "nb = -1")
        refused(bh, 2, None, "null edges")
        for bad in ([0.0, np.inf, 4.0], [0.0, np.nan, 4.0], [-1.0, 2.0, 4.0], [0.0, 2.0, 2.0], [0.0, 3.0, 2.0],
                    [0.0, 1e200, 2e200], [1e-200, 2e-200, 1.0]):
            refused(bh, 2, np.array(bad), "edges[")
            with pytest.raises(ValueError, match="nbmi_pair_counts"):
                bh.pair_counts(bad)
        for bad in ([1.0], [], np.arange(67.0)):
            with pytest.raises(ValueError, match="nb ="):
                bh.pair_counts(bad)
        after = (bh.get_positions_f64(), bh.get_velocities(), bh.get_colors(), bh.step_count())
        for a, c in zip(before[:3], after[:3]):
            assert a.tobytes() == c.tobytes()
        assert before[3] == after[3] == 0
        # every handle goes on working
        direct.step(0.1)
        direct.sync()
        shard.set_shard(0, n)
        ref = pr.pair_counts(p, good)
        for sim in (shard, bh):
            _check("after refusals", sim.pair_counts(good), ref)
            sim.step(0.1)
            sim.sync()
    finally:
        for sim in (direct, owner, shard, bh):
            sim.close()


def test_correlation_function_against_two_reference_counts(gpu):
    from nbody.pairs import xi_natural
    p = _preset("galaxy", 4096, seed=3)[0]
    rnd = np.random.RandomState(12).uniform(-400.0, 400.0, (3000, 3))
    edges = np.array([5.0, 10.0, 20.0, 40.0, 80.0, 160.0])
    dd, rr = pr.pair_counts(p, edges)[0], pr.pair_counts(rnd, edges)[0]
    assert (dd > 0).all() and (rr > 0).all()
    want = xi_natural(dd, rr, len(p), len(rnd))
    assert want[0] > 10.0 * abs(want[-1]) or want[0] > 1.0  # the galaxy is clustered on small scales
    sim = _bh(p)
    try:
        got = sim.correlation_function(edges, rnd)
        print(f"xi = {got.tolist()}")
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
        none = sim.correlation_function([1e-9, 1e-8], rnd)
        assert np.isnan(none).all()
    finally:
        sim.close()


def test_recorder_pairs_sessions_plain_and_pipelined(gpu, tmp_path):
    """quick_galaxy cut to 4 096 bodies x 5 frames with --pairs 2: the plain and the pipelined loop write the same
    pairs.jsonl, the auto edges are in metadata.json, the lines are the restatement's of the states they describe, and the
    frame files are those of a session without --pairs"""
    import json
    from nbody.pairs import auto_pair_edges, correlation_dimension
    from tools import record as rec
    ap = rec.build_parser()
    base = ["--preset", "quick_galaxy", "--bodies", "4096", "--frames", "5"]
    dirs = {}
    for name, extra in (("plain", ["--pairs", "2"]), ("piped", ["--pairs", "2", "--pipeline"]), ("without", [])):
        cfg = rec.build_config(ap.parse_args(base + extra))
        dirs[name] = rec.record(dict(cfg, session_name=name), root=tmp_path, quiet=True, seed=1)
    text = (dirs["plain"] / rec.PAIRS_FILE).read_text()
    assert text == (dirs["piped"] / rec.PAIRS_FILE).read_text()
    assert not (dirs["without"] / rec.PAIRS_FILE).exists()
    for k in range(5):
        a = (dirs["without"] / f"frame_{k:04d}.npz").read_bytes()
        assert a == (dirs["plain"] / f"frame_{k:04d}.npz").read_bytes() == (dirs["piped"] / f"frame_{k:04d}.npz").read_bytes(), k
    metas = {k: rec.load_metadata(d) for k, d in dirs.items()}
    g = metas["plain"]["pairs"]
    assert g == metas["piped"]["pairs"] and g["every"] == 2 and "pairs" not in metas["without"]
    # the edges are the initial state's
    np.random.seed(1)
    cfg = rec.build_config(ap.parse_args(base))
    p, v, m = rec._generate_initial_conditions(cfg)
    assert g["edges"] == auto_pair_edges(pr.nearest_d2(p))
    rows = [json.loads(line) for line in text.splitlines()]
    assert [r["frame"] for r in rows] == [1, 3]
    from nbody.gpu_backend import HIPBarnesHutSimulation
    sim = HIPBarnesHutSimulation(p, v, m, cfg["G"], cfg["softening"], cfg["damping"], cfg.get("theta", 0.5))
    try:
        sim.step_many(cfg["dt_per_frame"] / cfg["substeps"], 2 * cfg["substeps"])
        x = sim.get_positions_f64()
    finally:
        sim.close()
    counts, below = pr.pair_counts(x, g["edges"])
    first = rows[0]
    assert first["edges"] == g["edges"] and first["below"] == below and first["counts"] == counts.tolist()
    d2, points = correlation_dimension(g["edges"], below, counts)
    assert first["d2"] == d2 and first["d2_points"] == points == 12
    assert rec.show_status("plain", root=tmp_path)
