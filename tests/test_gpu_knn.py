"""nbmi_knn / nbmi_get_densities_f64 / density colours on the GPU against the NumPy brute force of tests/knn_ref.py
(include/nbmi.h).

r2_k is compared BIT FOR BIT: it is one of the float64 values d2(i, j), which the kernel and NumPy form with the same
three products and two sums.  mass_k is a sum of at most N masses in the walk's order: 1e-12 relative (N eps is 4e-12 at
20 000 bodies for a worst-case order; the sums here have a few dozen terms), and exact where the masses are integers.
"""
import numpy as np
import pytest

import knn_ref as kr
import query_cases as qc
from query_cases import bh as _bh, system as _system

pytestmark = pytest.mark.gpu

KS = (1, 8, 32, 64)
NBMI_ERR_ARG = -1


def _dist(dist, n, seed=7):
    R, G = {"galaxy": (800.0, 0.07), "cluster": (300.0, 0.05)}[dist]
    p, v, m = qc.preset(dist, n, seed, R, G)  # unequal masses: mass_k is not a count
    return p, v, m, G


_REF = {}


def _reference(name):
    """{k: (r2_k, mass_k)} of a named system for every k of KS it admits, computed once"""
    if name not in _REF:
        p, m = _system(name)
        _REF[name] = kr.knn_many(p, m, [k for k in KS if k <= len(p) - 1])
    return _REF[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check(label, got, ref, exact_mass=False):
    r2, mk = got
    bad = np.nonzero(_bits(r2) != _bits(ref[0]))[0]
    rel = np.abs(mk - ref[1]) / ref[1]
    print(f"{label}: r2_k mismatches {len(bad)} / {len(r2)}, mass_k max rel err {rel.max():.3e}")
    assert len(bad) == 0, (label, bad[:8], r2[bad[:8]], ref[0][bad[:8]])
    if exact_mass:
        assert np.array_equal(mk, ref[1]), (label, np.nonzero(mk != ref[1])[0][:8])
    else:
        assert rel.max() <= 1e-12, (label, rel.max())


CASES = [(s, k) for s in ("galaxy20k", "cluster20k", "n2049", "n4097", "trap", "far") for k in KS] + [("n9", 8), ("n65", 64)]


@pytest.mark.parametrize("name,k", CASES)
def test_exact_against_brute_force(gpu, name, k):
    p, m = _system(name)
    ref = _reference(name)[k]
    sim = _bh(p, m=m)
    try:
        _check(f"{name} k={k}", sim.knn(k), ref)
    finally:
        sim.close()


def test_ties_on_an_integer_lattice(gpu):
    """16^3 lattice, unit masses: most distances tie, so r2_k only comes out right if equal candidates are kept, and
    mass_k (an integer) only if subtrees AT the bound are never pruned"""
    p, m = qc.lattice(shuffle=False)
    ref = kr.knn_many(p, m, KS)
    sim = _bh(p, m=m)
    try:
        for k in KS:
            _check(f"lattice k={k}", sim.knn(k), ref[k], exact_mass=True)
    finally:
        sim.close()


def test_coincident_bodies(gpu):
    """4 096 bodies, every position held twice - and one of them by 70 bodies (more than a wave, more than k).
    Coincident bodies share all 42 key digits, so every pair hangs on a chain of cells down to level 42; the octree has
    4 N + 4 096 rows, like the reference's.  The positions are therefore drawn within 1e-9 of the origin (root half size
    10, level-42 cells 4.5e-12 wide): the pairs part from the others around level 35 and the tree needs 16 102 rows of
    the 20 480 (drawn in +-50 it would need 80 874, and every call would report NBMI_ERR_CAPACITY as a step does)."""
    rng = np.random.RandomState(9)
    base = rng.uniform(-1e-9, 1e-9, (2048, 3))
    p = np.concatenate([base, base])
    p[2049:2049 + 68] = p[0]  # rows 0, 2048 and 2049 .. 2116 hold one position; rows 1 .. 68 have lost their twins
    crowd = np.nonzero((p == p[0]).all(axis=1))[0]
    assert len(crowd) == 70
    m = rng.uniform(0.5, 1.5, len(p))
    ref = kr.knn_many(p, m, KS)
    assert (ref[1][0] == 0.0).sum() == len(p) - 68 and (ref[64][0] == 0.0).sum() == 70
    sim = _bh(p, m=m, eps=0.0)
    try:
        for k in KS:
            _check(f"coincident k={k}", sim.knn(k), ref[k])
            rho = sim.densities(k)
            zero = ref[k][0] == 0.0
            assert np.array_equal(rho == np.inf, zero)
            assert np.array_equal(_bits(rho[~zero]), _bits(kr.density(ref[k][0], sim.knn(k)[1])[~zero]))
        assert np.isinf(sim.densities(64)[crowd]).all()
    finally:
        sim.close()


def test_caller_order_before_and_after_steps_and_determinism(gpu):
    p, v, m, G = _dist("galaxy", 4096, seed=3)
    sim = _bh(p, v, m, G=G)
    try:
        for steps in (0, 5):
            if steps:
                sim.step_many(0.2, steps)
            x = sim.get_positions_f64()
            ref = kr.knn(x, m, 32)
            a = sim.knn(32)
            _check(f"after {steps} steps", a, ref)
            b = sim.knn(32)
            assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
            assert np.array_equal(_bits(sim.densities(32)), _bits(kr.density(*a)))
        ev = sim.knn(32, evals=True)[2]
        assert 2 * 32 * sim.n <= ev < sim.n * (sim.n - 1)  # both passes see at least the k neighbours; far from all pairs
    finally:
        sim.close()


def test_quadrupole_and_leapfrog_handles_give_the_same_bits(gpu):
    p, v, m, G = _dist("galaxy", 4096, seed=3)
    out = {}
    for tag, kw in (("plain", {}), ("quad", {"multipole": "quadrupole"}), ("leap", {"integrator": "leapfrog"})):
        sim = _bh(p, v, m, G=G, **kw)
        try:
            out[tag] = (sim.knn(8),)
        finally:
            sim.close()
    for tag in ("quad", "leap"):
        for a, b in zip(out[tag][0], out["plain"][0]):
            assert np.array_equal(_bits(a), _bits(b)), tag
    # after steps the three have moved differently (their forces and schemes differ): there the query is checked against
    # brute force on the handle's own positions
    sim = _bh(p, v, m, G=G, multipole="quadrupole", integrator="leapfrog")
    try:
        sim.step_many(0.2, 3)
        _check("quad+leap after steps", sim.knn(8), kr.knn(sim.get_positions_f64(), m, 8))
    finally:
        sim.close()


@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
def test_queries_do_not_disturb_the_run(gpu, integrator):
    p, v, m, G = _dist("galaxy", 20_000)

    def run(query):
        sim = _bh(p, v, m, G=G, integrator=integrator)
        try:
            sim.set_force_precision("auto")
            shares = []
            for i in range(12):
                if query and i % 3 == 0:
                    sim.knn(16)
                    sim.set_color_mode("density", k=8, log10_range=(-6.0, 2.0))
                    sim.compute_colors(15.0)
                    sim.set_color_mode("speed")
                sim.step(0.2)
                shares.append(sim.force_precision_share())
            return sim.get_positions_f64(), sim.get_velocities(), sim.step_count(), shares
        finally:
            sim.close()
    a, b = run(False), run(True)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert a[2] == b[2] == 12
    assert a[3] == b[3], (a[3], b[3])


@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
@pytest.mark.parametrize("multipole", ["monopole", "quadrupole"])
def test_side_builds_between_steps_do_not_disturb_the_run(gpu, multipole, integrator):
    """Every query that builds an octree of its own between two steps - the diagnostics' potential, the k-NN query, the
    density-coloured frame - on 4 099 bodies (64 waves and a ragged one), in both multipole orders: the quadrupole
    build always writes the query rows, and nbmi_frame_begin issues its query without waiting."""
    p, v, m, G = _dist("galaxy", 4099)

    def run(disturb):
        sim = _bh(p, v, m, G=G, multipole=multipole, integrator=integrator)
        try:
            sim.set_force_precision("auto")
            if disturb:
                sim.set_color_mode("density", k=8, log10_range=(-6.0, 2.0))
            shares = []
            for i in range(8):
                if disturb and i % 2 == 0:
                    sim.diagnostics(potential=True)
                    sim.knn(8)
                    slot = sim.frame_begin("f32", 15.0)
                    sim.frame_wait(slot)
                    sim.frame_release(slot)
                sim.step(0.2)
                shares.append(sim.force_precision_share())
            return sim.get_positions_f64(), sim.get_velocities(), sim.step_count(), shares
        finally:
            sim.close()
    a, b = run(False), run(True)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert a[2] == b[2] == 8
    assert a[3] == b[3], (a[3], b[3])


def test_density_colours(gpu):
    p, v, m, G = _dist("galaxy", 4096, seed=3)
    sim = _bh(p, v, m, G=G)
    try:
        assert sim.color_mode == "speed"
        sim.compute_colors(15.0)
        speed = sim.get_colors()
        slot = sim.frame_begin("f32", 15.0)
        pos_speed, col_speed = (a.copy() for a in sim.frame_wait(slot)[:2])
        sim.frame_release(slot)
        assert np.array_equal(col_speed, speed)

        rho = kr.density(*kr.knn(p, m, 16))
        lo, hi = kr.default_log10_range(rho)
        sim.set_color_mode("density", k=16, log10_range=(lo, hi))
        assert sim.color_mode == "density" and sim.color_settings == {"mode": "density", "k": 16, "log10_range": [lo, hi]}
        sim.compute_colors(123.0)  # max_speed is ignored
        got = sim.get_colors()
        want = kr.density_colors(rho, lo, hi)
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"density colours: max |delta| {err:.3e} (bound 2^-23 = {2.0 ** -23:.3e})")
        # the ramp is continuous with slope <= 50 and t differs by < 1e-11 (log10, mass_k): what is left is the float32
        # rounding, one ulp at 1.0
        assert err <= 2.0 ** -23
        assert len(np.unique(got, axis=0)) > 100  # the range spreads the bodies over the ramp

        slot = sim.frame_begin("f32", 15.0)
        pos_d, col_d = (a.copy() for a in sim.frame_wait(slot)[:2])
        sim.frame_release(slot)
        assert np.array_equal(col_d.view(np.uint32), got.view(np.uint32))
        assert np.array_equal(sim.get_colors().view(np.uint32), got.view(np.uint32))
        assert np.array_equal(pos_d.view(np.uint32), pos_speed.view(np.uint32))

        sim.set_color_mode("speed")
        sim.compute_colors(15.0)
        assert np.array_equal(sim.get_colors().view(np.uint32), speed.view(np.uint32))
        # rho = +inf colours as t = 1
        assert np.array_equal(kr.density_colors(np.array([np.inf]), lo, hi)[0], kr.ramp(np.array(1.0)))
    finally:
        sim.close()


def test_refusals_leave_the_handle_usable(gpu):
    from nbody.gpu_backend import HIPBarnesHutSimulation, HIPDirectSimulation, HIPOwnerSimulation
    from nbody.sharded import let_capacities
    lib = gpu.load()
    rng = np.random.RandomState(1)
    n = 256
    p, v, m = rng.uniform(-10, 10, (n, 3)), np.zeros((n, 3)), np.ones(n)
    out = np.empty(n)

    def refused(sim, call, *needles):
        rc = call()
        msg = gpu.last_error()
        assert rc == NBMI_ERR_ARG, (rc, msg)
        for s in needles:
            assert s in msg, (s, msg)

    def calls(sim, k=8):
        return (lambda: lib.nbmi_knn(sim._h, k, gpu.ptr(out), None, None),
                lambda: lib.nbmi_get_densities_f64(sim._h, k, gpu.ptr(out)),
                lambda: lib.nbmi_set_color_mode(sim._h, 1, k, -3.0, 3.0))

    direct = HIPDirectSimulation(p, v, m, 0.07, 1.5, 1.0)
    cap, let_cap = let_capacities(n, 1)
    owner = HIPOwnerSimulation(p, v, m, np.arange(n, dtype=np.int32), cap, let_cap, 1, 0, 0.07, 1.5, 1.0)
    shard = HIPBarnesHutSimulation(p, v, m, 0.07, 1.5, 1.0, 0.5)
    bh = HIPBarnesHutSimulation(p, v, m, 0.07, 1.5, 1.0, 0.5)
    try:
        shard.set_shard(0, n // 2)
        for sim, needle in ((direct, "direct N^2"), (owner, "owner-mode"), (shard, "sharded")):
            for call in calls(sim):
                refused(sim, call, needle)
        for sim in (direct, owner):  # the Python classes refuse on their own
            with pytest.raises(ValueError):
                sim.knn(8)
            with pytest.raises(ValueError):
                sim.densities(8)
            with pytest.raises(ValueError):
                sim.set_color_mode("density")
        with pytest.raises(ValueError, match="sharded"):
            shard.knn(8)
        for k in (0, 65, n):
            for call in calls(bh, k):
                refused(bh, call, f"k = {k}", f"N = {n}")
            with pytest.raises(ValueError, match=f"k = {k}"):
                bh.knn(k)
        for lo, hi in ((1.0, 1.0), (2.0, 1.0), (0.0, np.inf), (np.nan, 1.0)):
            refused(bh, lambda: lib.nbmi_set_color_mode(bh._h, 1, 8, lo, hi), "range")
        refused(bh, lambda: lib.nbmi_set_color_mode(bh._h, 7, 8, 0.0, 1.0), "colour mode")
        assert bh.color_mode == "speed"
        # every handle goes on working
        direct.step(0.1)
        direct.sync()
        shard.set_shard(0, n)
        for sim in (shard, bh):
            _check("after refusals", sim.knn(8), kr.knn(p, m, 8))
            sim.step(0.1)
            sim.sync()
    finally:
        for sim in (direct, owner, shard, bh):
            sim.close()


def test_recorder_density_sessions_plain_and_pipelined(gpu, tmp_path):
    """quick_galaxy cut to 4 096 bodies x 3 frames with --color density: the plain and the pipelined loop write the
    same files, the range is in metadata.json, and frame 0's colours are the restatement's under that range"""
    from tools import record as rec
    ap = rec.build_parser()
    base = ["--preset", "quick_galaxy", "--bodies", "4096", "--frames", "3", "--color", "density"]
    dirs = {}
    for name, extra in (("plain", []), ("piped", ["--pipeline"])):
        cfg = rec.build_config(ap.parse_args(base + extra))
        dirs[name] = rec.record(dict(cfg, session_name=name), root=tmp_path, quiet=True, seed=1)
    metas = {k: rec.load_metadata(d) for k, d in dirs.items()}
    color = metas["plain"]["color"]
    assert color["mode"] == "density" and color["k"] == 32 and color == metas["piped"]["color"]
    lo, hi = color["log10_range"]
    for k in range(3):
        a, b = dirs["plain"] / f"frame_{k:04d}.npz", dirs["piped"] / f"frame_{k:04d}.npz"
        assert a.read_bytes() == b.read_bytes(), k
    # the range is the initial state's; frame 0 is the state after the first frame interval
    np.random.seed(1)
    cfg = rec.build_config(ap.parse_args(base))
    p, v, m = rec._generate_initial_conditions(cfg)
    m = np.ones(len(p)) if m is None else m
    assert (lo, hi) == kr.default_log10_range(kr.density(*kr.knn(p, m, 32)))
    from nbody.gpu_backend import HIPBarnesHutSimulation
    sim = HIPBarnesHutSimulation(p, v, m, cfg["G"], cfg["softening"], cfg["damping"], cfg.get("theta", 0.5))
    try:
        sim.step_many(cfg["dt_per_frame"] / cfg["substeps"], cfg["substeps"])
        x = sim.get_positions_f64()
    finally:
        sim.close()
    pos0, col0 = rec.load_frame(dirs["plain"], 0)
    assert np.array_equal(pos0, x.astype(np.float32))
    want = kr.density_colors(kr.density(*kr.knn(x, m, 32)), lo, hi)
    assert np.abs(col0.astype(np.float64) - want).max() <= 2.0 ** -23
    assert rec.show_status("plain", root=tmp_path)
