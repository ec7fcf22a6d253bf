"""nbmi_fof / nbmi_fof_catalogue / nbmi_compute_group_colors on the GPU against the NumPy restatement of
tests/fof_ref.py (include/nbmi.h).

Labels and group counts are compared EXACTLY: the partition is a function of the float64 values d2(i, j), which the
kernel and NumPy form with the same three products and two sums, and a label is the smallest body index of its group.
The catalogue's member counts, labels, order and bounding boxes are exact too; its sums are compared within the
worst-case bound of ANY summation order, 4 members 2^-53 sum|terms| per group and component (each side is within
members 2^-53 sum|terms| of the exact sum of its rounded products, and those products are the same on both sides; the
other half of the factor covers the division by M on the device and the multiplication that undoes it here).
"""
import numpy as np
import pytest

import fof_ref as fr
import knn_ref as kr
import query_cases as qc
from query_cases import bh as _bh, preset as _preset

pytestmark = pytest.mark.gpu

NBMI_ERR_ARG = -1
NBMI_ERR_CAPACITY = -4
U = 2.0 ** -53


def _system(name):
    return qc.system(name)[0]


# what each case is for, checked on the reference before anything is asserted of the device:
# (largest group at least, groups at least, singletons at least)
CASES = [
    ("galaxy", 5.2, (4000, 10_000, 9000)),   # a core, thousands of small groups and singletons
    ("galaxy", 20.8, (19_000, 300, 200)),    # nearly everything in one group
    ("collision", 9.66, (6000, 3000, 2000)),  # two giant groups (checked below)
    ("filament", 46.6, (800, 2000, 1000)),   # hundreds of mid-size groups
    ("n2049", 8.0, (5, 1500, 1000)),
    ("n2049", 16.0, (1800, 50, 40)),
    ("n4097", 8.0, (10, 2000, 1000)),
    ("n4097", 16.0, (4000, 5, 5)),
    ("trap", 1e-4, (30, 2500, 2300)),        # links inside the 1e-3 ball only
    ("trap", 2e-3, (2048, 2049, 2048)),      # the ball is one group
    ("trap", 50.0, (2048, 1500, 1500)),
    ("far", 5.0, (3000, 100, 100)),
    ("far", 2.0e6, (4097, 1, 0)),            # everything is one group
    ("n1", 1.0, (1, 1, 1)),
    ("n2", 5.0, (2, 1, 0)),                  # linked at equality
    ("n2", 4.999, (1, 2, 2)),                # not linked
    ("n65", 30.0, (5, 30, 20)),           # one full wave and a one-lane wave
]
_REF = {}


def _reference(name, b):
    if (name, b) not in _REF:
        _REF[(name, b)] = fr.fof(_system(name), b)
    return _REF[(name, b)]


def _check_labels(tag, got, ng, ref):
    bad = np.nonzero(got != ref[0])[0]
    print(f"{tag}: label mismatches {len(bad)} / {len(got)}, n_groups {ng} (reference {ref[1]})")
    assert got.dtype == np.int32 and np.array_equal(got, ref[0]), (tag, bad[:8], got[bad[:8]], ref[0][bad[:8]])
    assert ng == ref[1], (tag, ng, ref[1])


@pytest.mark.parametrize("name,b,shape", CASES, ids=[f"{n}-{b}" for n, b, _ in CASES])
def test_labels_exact_against_the_reference(gpu, name, b, shape):
    p = _system(name)
    ref = _reference(name, b)
    sizes = fr.group_sizes(ref[0])
    print(f"{name} b={b}: reference groups {ref[1]}, largest {sizes[:3].tolist()}, of >= 20: {(sizes >= 20).sum()}, "
          f"singletons {(sizes == 1).sum()}")
    assert sizes[0] >= shape[0] and ref[1] >= shape[1] and (sizes == 1).sum() >= shape[2], (name, b, "the case lost its point")
    if name == "collision":
        assert sizes[1] >= 6000
    sim = _bh(p)
    try:
        _check_labels(f"{name} b={b}", sim.find_groups(b), sim.n_groups, ref)
    finally:
        sim.close()


def test_equality_links_and_nothing_at_the_bound_is_pruned(gpu):
    """16^3 integer lattice, spacing 1, shuffled: at b = 1 every link has d2 == b2 exactly (one group of 4 096 - lost
    if equality is pruned or tested with <), just below 1 there are no links at all"""
    p = qc.lattice()[0]
    sim = _bh(p)
    try:
        lab = sim.find_groups(1.0)
        assert sim.n_groups == 1 and (lab == 0).all()
        lab = sim.find_groups(np.nextafter(1.0, 0.0))
        assert sim.n_groups == 4096 and np.array_equal(lab, np.arange(4096, dtype=np.int32))
    finally:
        sim.close()


def _helix(n=3000):
    """points at arc spacing 1.0 along a helix of radius 40 and pitch 25 per turn"""
    r, c = 40.0, 25.0 / (2.0 * np.pi)
    t = np.arange(n) / np.hypot(r, c)
    return np.stack([r * np.cos(t), r * np.sin(t), c * t], 1)


def test_long_chains_across_waves(gpu):
    """a chain of 3 000 links through 47 waves, caller order shuffled: one group; with one body taken out mid-chain
    exactly two, with the reference's labels"""
    rng = np.random.RandomState(8)
    h = _helix()
    for tag, pts, groups in (("whole", h, 1), ("cut", np.delete(h, 1500, axis=0), 2)):
        p = pts[rng.permutation(len(pts))]
        ref = fr.fof(p, 1.05)
        assert ref[1] == groups, (tag, ref[1])
        sim = _bh(p)
        try:
            _check_labels(f"helix {tag}", sim.find_groups(1.05), sim.n_groups, ref)
        finally:
            sim.close()


def test_coincident_bodies_are_linked(gpu):
    """4 096 bodies, every position held twice (drawn within 1e-9 of the origin so that the tree fits, as section 4.14's
    test says): at b = 1e-12 the twins are linked, and little else"""
    rng = np.random.RandomState(9)
    base = rng.uniform(-1e-9, 1e-9, (2048, 3))
    p = np.concatenate([base, base])
    ref = fr.fof(p, 1e-12)
    assert (fr.group_sizes(ref[0]) >= 2).all() and ref[1] >= 2000
    sim = _bh(p, eps=0.0)
    try:
        lab = sim.find_groups(1e-12)
        _check_labels("coincident", lab, sim.n_groups, ref)
        assert np.array_equal(lab[2048:], lab[:2048])
    finally:
        sim.close()


def test_capacity_error_is_a_steps_and_the_handle_goes_on(gpu):
    """section 4.14's capacity input: one position held by 70 bodies at +-50 needs more node rows than 4 N"""
    lib = gpu.load()
    rng = np.random.RandomState(9)
    base = rng.uniform(-50.0, 50.0, (2048, 3))
    p = np.concatenate([base, base])
    p[2049:2049 + 68] = p[0]
    sim = _bh(p, eps=0.0)
    try:
        lab = np.empty(len(p), np.int32)
        rc = lib.nbmi_fof(sim._h, 1.0, gpu.ptr(lab), None, None)
        msg = gpu.last_error()
        assert rc == NBMI_ERR_CAPACITY and "octree needs" in msg and "rows allocated" in msg, (rc, msg)
        good = rng.uniform(-50.0, 50.0, (4096, 3))
        sim.set_state(good, np.zeros_like(good))
        _check_labels("after the capacity error", sim.find_groups(8.0), sim.n_groups, fr.fof(good, 8.0))
    finally:
        sim.close()


def test_callers_order_after_steps(gpu):
    p, v, m = _preset("galaxy", 4096, seed=3)
    sim = _bh(p, v, m)
    try:
        sim.step_many(0.2, 3)
        x = sim.get_positions_f64()
        ref = fr.fof(x, 12.0)
        assert 1 < ref[1] < len(x)
        _check_labels("after 3 steps", sim.find_groups(12.0), sim.n_groups, ref)
    finally:
        sim.close()


def test_quadrupole_and_leapfrog_handles_give_the_same_labels(gpu):
    p, v, m = _preset("galaxy", 4096, seed=3)
    ref = fr.fof(p, 12.0)
    for kw in ({"multipole": "quadrupole"}, {"integrator": "leapfrog"}):
        sim = _bh(p, v, m, **kw)
        try:
            _check_labels(str(kw), sim.find_groups(12.0), sim.n_groups, ref)
        finally:
            sim.close()


@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
def test_group_queries_do_not_disturb_the_run(gpu, integrator):
    p, v, m = _preset("galaxy")

    def run(query):
        sim = _bh(p, v, m, integrator=integrator)
        try:
            sim.set_force_precision("auto")
            shares = []
            for i in range(12):
                if query and i % 3 == 0:
                    sim.find_groups(5.2)
                    sim.group_catalogue(5.2, min_members=20)
                    sim.color_by_groups(5.2, min_members=20)
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


@pytest.mark.parametrize("dist,b", [("galaxy", 5.2), ("collision", 9.66)])
def test_catalogue_against_the_reference(gpu, dist, b):
    p, v, m = _preset(dist)
    lab = _reference(dist, b)[0]
    largest = int(fr.group_sizes(lab)[0])
    sim = _bh(p, v, m)
    try:
        for mm in (1, 2, 20, largest + 1):
            ref = fr.catalogue(p, v, m, lab, mm)
            got = sim.group_catalogue(b, min_members=mm)
            again = sim.group_catalogue(b, min_members=mm)
            print(f"{dist} min_members={mm}: count {got['count']} (reference {ref['count']})")
            assert got["count"] == ref["count"] and (mm <= largest) == (got["count"] > 0)
            assert got["label"].dtype == np.int32 and got["members"].dtype == np.int64
            assert np.array_equal(got["label"], ref["label"]) and np.array_equal(got["members"], ref["members"])
            for key in ("lo", "hi"):
                assert np.array_equal(got[key].view(np.uint64), ref[key].view(np.uint64)), key
            k = ref["members"].astype(np.float64)
            err = np.abs(got["mass"] - ref["mass"])
            bound = 4.0 * k * U * ref["abs_m"]
            worst = [float((err / bound).max())] if len(k) else []
            assert (err <= bound).all()
            for key, sums, mags in (("center", "sum_mx", "abs_mx"), ("velocity", "sum_mv", "abs_mv")):
                err = np.abs(got[key] * got["mass"][:, None] - ref[sums])
                bound = 4.0 * k[:, None] * U * ref[mags]
                if len(k):
                    worst.append(float((err / bound).max()))
                assert (err <= bound).all(), (key, mm)
            print(f"    largest error / bound for M, c, v: {worst}")
            for key in ("label", "members", "mass", "center", "velocity", "lo", "hi"):
                assert got[key].tobytes() == again[key].tobytes(), ("two calls differ", key)
        ref = fr.catalogue(p, v, m, lab, 2)
        few = sim.group_catalogue(b, min_members=2, capacity=5)
        assert few["count"] == ref["count"] > 5 and len(few["label"]) == 5
        assert np.array_equal(few["label"], ref["label"][:5]) and np.array_equal(few["members"], ref["members"][:5])
        none = sim.group_catalogue(b, min_members=2, capacity=0)
        assert none["count"] == ref["count"] and len(none["label"]) == 0
    finally:
        sim.close()


def test_catalogue_of_massless_groups_uses_unweighted_means(gpu):
    p = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [50.0, 0.0, 0.0], [51.0, 2.0, 0.0]])
    v = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 4.0], [2.0, 2.0, 2.0], [4.0, 4.0, 4.0]])
    m = np.array([0.0, 0.0, 0.0, 1.0, 3.0])
    sim = _bh(p, v, m)
    try:
        got = sim.group_catalogue(3.0, min_members=2)
        assert got["count"] == 2 and got["label"].tolist() == [0, 3] and got["members"].tolist() == [3, 2]
        assert got["mass"].tolist() == [0.0, 4.0]
        assert np.array_equal(got["center"], [[1.0 / 3.0, 1.0 / 3.0, 0.0], [50.75, 1.5, 0.0]])
        assert np.array_equal(got["velocity"], [[1.0 / 3.0, 1.0 / 3.0, 4.0 / 3.0], [3.5, 3.5, 3.5]])
    finally:
        sim.close()


def test_group_colours(gpu):
    p, v, m = _preset("galaxy", 4096, seed=3)
    b, mm = 12.0, 5
    lab = fr.fof(p, b)[0]
    sizes = fr.group_sizes(lab)
    assert (sizes >= mm).sum() >= 5 and (sizes < mm).sum() >= 5
    sim = _bh(p, v, m)
    try:
        sim.compute_colors(15.0)
        speed = sim.get_colors()
        sim.color_by_groups(b, min_members=mm)
        got = sim.get_colors()
        want = fr.group_colors(lab, mm)
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"group colours: max |delta| {err:.3e} (bound 2^-23 = {2.0 ** -23:.3e})")
        # t is exact (an integer over 2^24) and the ramp is the same float64 arithmetic: what is left is the float32
        # rounding of a colour in [0, 1], at most 2^-24 - the issue's bound is 2^-23
        assert err <= 2.0 ** -23
        assert len(np.unique(got, axis=0)) > 5
        assert sim.color_mode == "speed"
        sim.compute_colors(15.0)
        assert np.array_equal(sim.get_colors().view(np.uint32), speed.view(np.uint32))
    finally:
        sim.close()


def test_refusals_leave_handle_and_state_untouched(gpu):
    from nbody.gpu_backend import HIPBarnesHutSimulation, HIPDirectSimulation, HIPOwnerSimulation
    from nbody.sharded import let_capacities
    lib = gpu.load()
    rng = np.random.RandomState(1)
    n = 256
    p, v, m = rng.uniform(-10, 10, (n, 3)), np.zeros((n, 3)), np.ones(n)
    lab = np.empty(n, np.int32)
    mem = np.empty(n, np.int64)
    out = np.empty((n, 13))
    cnt = np.zeros(1, np.int64)

    def refused(call, *needles):
        rc = call()
        msg = gpu.last_error()
        assert rc == NBMI_ERR_ARG, (rc, msg)
        for s in needles:
            assert s in msg, (s, msg)

    def calls(sim, link=2.0, mm=1, cap=n):
        return (("nbmi_fof", lambda: lib.nbmi_fof(sim._h, link, gpu.ptr(lab), None, None)),
                ("nbmi_fof_catalogue", lambda: lib.nbmi_fof_catalogue(sim._h, link, mm, cap, gpu.ptr(lab), gpu.ptr(mem),
                                                                      gpu.ptr(out), gpu.ptr(cnt))),
                ("nbmi_compute_group_colors", lambda: lib.nbmi_compute_group_colors(sim._h, link, mm)))

    direct = HIPDirectSimulation(p, v, m, 0.07, 1.5, 1.0)
    cap, let_cap = let_capacities(n, 1)
    owner = HIPOwnerSimulation(p, v, m, np.arange(n, dtype=np.int32), cap, let_cap, 1, 0, 0.07, 1.5, 1.0)
    shard = HIPBarnesHutSimulation(p, v, m, 0.07, 1.5, 1.0, 0.5)
    bh = HIPBarnesHutSimulation(p, v, m, 0.07, 1.5, 1.0, 0.5)
    try:
        shard.set_shard(0, n // 2)
        for sim, needle in ((direct, "direct N^2"), (owner, "owner-mode"), (shard, "sharded")):
            for name, call in calls(sim):
                refused(call, name + ": ", needle)
        for sim in (direct, owner):  # the Python classes refuse on their own
            for call in (lambda: sim.find_groups(2.0), lambda: sim.group_catalogue(2.0), lambda: sim.color_by_groups(2.0)):
                with pytest.raises(ValueError):
                    call()
        with pytest.raises(ValueError, match="sharded"):
            shard.find_groups(2.0)
        bh.compute_colors(15.0)
        before = (bh.get_positions_f64(), bh.get_velocities(), bh.get_colors(), bh.step_count())
        for link in (0.0, -1.0, np.inf, np.nan):
            for name, call in calls(bh, link=link):
                refused(call, name + ": ", "linking length")
            with pytest.raises(ValueError, match="linking length"):
                bh.find_groups(link)
        for name, call in calls(bh, mm=0)[1:]:
            refused(call, name + ": ", "min_members = 0")
        refused(calls(bh, cap=-1)[1][1], "nbmi_fof_catalogue: ", "capacity = -1")
        with pytest.raises(ValueError, match="min_members"):
            bh.group_catalogue(2.0, min_members=0)
        with pytest.raises(ValueError, match="min_members"):
            bh.color_by_groups(2.0, min_members=-3)
        after = (bh.get_positions_f64(), bh.get_velocities(), bh.get_colors(), bh.step_count())
        for a, c in zip(before[:3], after[:3]):
            assert a.tobytes() == c.tobytes()
        assert before[3] == after[3] == 0 and bh.color_mode == "speed"
        # every handle goes on working
        direct.step(0.1)
        direct.sync()
        shard.set_shard(0, n)
        ref = fr.fof(p, 2.0)
        for sim in (shard, bh):
            _check_labels("after refusals", sim.find_groups(2.0), sim.n_groups, ref)
            sim.step(0.1)
            sim.sync()
    finally:
        for sim in (direct, owner, shard, bh):
            sim.close()


def test_empty_handle(gpu):
    sim = _bh(np.empty((0, 3)))
    try:
        assert len(sim.find_groups(1.0)) == 0 and sim.n_groups == 0
        assert sim.group_catalogue(1.0, min_members=1)["count"] == 0
        sim.color_by_groups(1.0)
    finally:
        sim.close()


def test_pruning_works(gpu):
    """a condition, not a benchmark: far fewer distances than all pairs"""
    p = _system("n4097")
    sim = _bh(p)
    try:
        lab, ev = sim.find_groups(8.0, evals=True)
        print(f"uniform n = 4 097, b = 8: {ev / len(p):.1f} distances per body")
        assert np.array_equal(lab, _reference("n4097", 8.0)[0])
        assert 0 < ev / len(p) < len(p) / 4
    finally:
        sim.close()


def test_recorder_groups_sessions_plain_and_pipelined(gpu, tmp_path):
    """quick_galaxy cut to 4 096 bodies x 5 frames with --groups 2 --linking-length auto: the plain and the pipelined loop
    write the same groups.jsonl, the length is in metadata.json, the lines are the restatement's of the states they
    describe, and the frame files are those of a session without --groups"""
    import json
    from tools import record as rec
    ap = rec.build_parser()
    base = ["--preset", "quick_galaxy", "--bodies", "4096", "--frames", "5"]
    groups = ["--groups", "2", "--linking-length", "auto", "--min-members", "5"]
    dirs = {}
    for name, extra in (("plain", groups), ("piped", groups + ["--pipeline"]), ("without", [])):
        cfg = rec.build_config(ap.parse_args(base + extra))
        dirs[name] = rec.record(dict(cfg, session_name=name), root=tmp_path, quiet=True, seed=1)
    text = (dirs["plain"] / rec.GROUPS_FILE).read_text()
    assert text == (dirs["piped"] / rec.GROUPS_FILE).read_text()
    assert not (dirs["without"] / rec.GROUPS_FILE).exists()
    for k in range(5):
        a = (dirs["without"] / f"frame_{k:04d}.npz").read_bytes()
        assert a == (dirs["plain"] / f"frame_{k:04d}.npz").read_bytes() == (dirs["piped"] / f"frame_{k:04d}.npz").read_bytes(), k
    metas = {k: rec.load_metadata(d) for k, d in dirs.items()}
    g = metas["plain"]["groups"]
    assert g == metas["piped"]["groups"] and g["every"] == 2 and g["min_members"] == 5 and "groups" not in metas["without"]
    # the length is the initial state's
    np.random.seed(1)
    cfg = rec.build_config(ap.parse_args(base))
    p, v, m = rec._generate_initial_conditions(cfg)
    assert g["link"] == 2.0 * float(np.median(np.sqrt(kr.knn(p, m, 1)[0])))
    rows = [json.loads(line) for line in text.splitlines()]
    assert [r["frame"] for r in rows] == [1, 3]
    from nbody.gpu_backend import HIPBarnesHutSimulation
    sim = HIPBarnesHutSimulation(p, v, m, cfg["G"], cfg["softening"], cfg["damping"], cfg.get("theta", 0.5))
    try:
        sim.step_many(cfg["dt_per_frame"] / cfg["substeps"], 2 * cfg["substeps"])
        x = sim.get_positions_f64()
    finally:
        sim.close()
    lab, ng = fr.fof(x, g["link"])
    cat = fr.catalogue(x, v, m, lab, 5)
    first = rows[0]
    assert first["link"] == g["link"] and first["min_members"] == 5 and first["n_groups"] == ng
    assert first["count"] == cat["count"] > 0 and len(first["groups"]) == min(cat["count"], rec.GROUPS_ROWS)
    assert [r["label"] for r in first["groups"]] == cat["label"][:rec.GROUPS_ROWS].tolist()
    assert [r["members"] for r in first["groups"]] == cat["members"][:rec.GROUPS_ROWS].tolist()
    assert first["groups"][0]["lo"] == cat["lo"][0].tolist() and first["groups"][0]["hi"] == cat["hi"][0].tolist()
    assert rec.show_status("plain", root=tmp_path)
