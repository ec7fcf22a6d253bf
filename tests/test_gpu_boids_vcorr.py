"""bdmi_velocity_correlation (include/bdmi.h; csrc/bdmi.hip k_vc_quantise, k_vc_pairs, for_each_run_wide) against the NumPy
restatement tests/vcorr_ref.py on the inputs of tests/vcorr_cases.py.  Every comparison is equality of integers: pairs,
the sums S_k from their (hi, lo), evals and self5.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import boids_cases as BC
import boids_ref as R
import vcorr_cases as VC
import vcorr_ref as VR
from test_gpu_boids import RawFlock
from test_gpu_boids_periodic import PeriodicFlock
from test_gpu_boids_periodic_flocks import TorusStats
from test_gpu_boids_topological import TOPOLOGICAL, set_mode
from test_gpu_flockstats import Stats

pytestmark = pytest.mark.gpu

CALL = "bdmi_velocity_correlation"


def corr(f, edges, mean, nb=None, outputs=True):
    """The raw call on the handle of `f`, into arrays prefilled with -7: (rc, dict)."""
    edges = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
    nb = (len(edges) - 1 if edges is not None else 0) if nb is None else nb
    mean = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64)
    slots = 65 if edges is None else max(len(edges), 1)
    pairs, dot, s5, ev = np.full(slots, -7, np.int64), np.full((slots, 2), -7, np.int64), np.full(5, -7, np.int64), C.c_int64(-7)
    ptrs = [f.nat.ptr(pairs), f.nat.ptr(dot), f.nat.ptr(s5), C.addressof(ev)] if outputs else [None] * 4
    rc = f.lib.bdmi_velocity_correlation(f.h, nb, f.nat.ptr(edges), f.nat.ptr(mean), *ptrs)
    return rc, dict(pairs=pairs, dot=dot, self5=s5, evals=ev.value)


def decoded(res, nb):
    """pairs, S_k, evals, qsum, qsq as Python integers; (hi, lo) must be the unique form."""
    dot = res["dot"][:nb + 1]
    assert ((dot[:, 1] >= 0) & (dot[:, 1] < 2 ** 32)).all()
    assert 0 <= res["self5"][4] < 2 ** 32
    return dict(pairs=[int(x) for x in res["pairs"][:nb + 1]], dot=[VR.from_hi_lo(h, l) for h, l in dot], evals=int(res["evals"]),
                qsum=[int(x) for x in res["self5"][:3]], qsq=VR.from_hi_lo(res["self5"][3], res["self5"][4]))


def handle(nat, c):
    cls = PeriodicFlock if c["periodic"] else RawFlock
    return cls(nat, c["pos"], c["vel"], c["col"], c["params"])


@functools.lru_cache(maxsize=2)
def _table(key):
    c = CASES[key]()
    return c, VR.PairTable(c["pos"], c["params"], c["periodic"])


CASES = {
    "uniform_2049": lambda: VC.uniform(2049), "uniform_4097": lambda: VC.uniform(4097),
    "periodic_box_3": lambda: VC.periodic_box(3), "periodic_box_5": lambda: VC.periodic_box(5),
    "periodic_box_6": lambda: VC.periodic_box(6), "periodic_box_7": lambda: VC.periodic_box(7),
    "lattice_walled": lambda: VC.lattice16(False), "lattice_periodic": lambda: VC.lattice16(True),
    "corner_blob": VC.corner_blob, "twins": VC.twins, "crowded": VC.crowded,
}


def check(f, c, table, edges, mean, what, cut_allowed=False):
    """One call against the restatement; returns (decoded result, restatement)."""
    want = VR.correlate(c["pos"], c["vel"], c["params"], edges, mean, c["periodic"], table=table)
    rc, res = corr(f, edges, mean)
    assert rc == 0, (what, f.nat.last_error())
    got = decoded(res, len(edges) - 1)
    print(f"{what}: n={len(c['pos'])} nb={len(edges) - 1} reach={want['reach']} evals={got['evals']} pairs={sum(got['pairs'])} "
          f"cut={want['cut']}")
    assert got["pairs"] == [int(x) for x in want["pairs"]], what
    assert got["dot"] == want["dot"], what
    assert (got["evals"], got["qsum"], got["qsq"]) == (want["evals"], want["qsum"], want["qsq"]), what
    if not cut_allowed:
        assert want["cut"] == 0, what  # the candidate mask removed no pair in range
    return got, want


def run_case(nat, key, edge_list, mean=None, **kw):
    c, table = _table(key)
    mean = VC.mean_heading(c["vel"]) if mean is None else mean
    f = handle(nat, c)
    try:
        return [check(f, c, table, e, mean, f"{c['name']}[{k}]", **kw) for k, e in enumerate(edge_list)]
    finally:
        f.close()


def identity(got, n):
    """With a last edge that reaches every pair: 2 sum S_k == |sum q|^2 - Q, and every pair is counted."""
    assert sum(got["pairs"]) == n * (n - 1) // 2
    assert 2 * sum(got["dot"]) == sum(x * x for x in got["qsum"]) - got["qsq"]


# ---- walled, uniform -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (2049, 4097))
def test_walled_reach_1_2_3_and_the_whole_grid(gpu, n):
    edge_list = [np.linspace(0.0, 5.0 * m, 17) for m in (1, 2, 3)] + [np.linspace(0.0, VC.WHOLE_GRID, 33)]
    out = run_case(gpu, f"uniform_{n}", edge_list)
    assert [w["reach"] for _, w in out] == [1, 2, 3, 16]
    identity(out[3][0], n)


@pytest.mark.parametrize("n", (2049, 4097))
def test_walled_random_edge_sets(gpu, n):
    sets = VC.edge_sets(n)
    assert len(sets) == 20 and {len(e) - 1 for e in sets} >= {1, 64}
    run_case(gpu, f"uniform_{n}", sets)


def test_reach_1_walks_the_runs_of_the_link_kernel(gpu):
    """m = 1: evals equals bdmi_flocks' evals on the same state, and the single bin [0, link] holds its links."""
    c, table = _table("uniform_2049")
    f = Stats(gpu, c["pos"], c["vel"], c["col"], c["params"])
    try:
        for link in (5.0, 3.25):
            rc, fl = f.flocks(link)
            assert rc == 0
            got, _ = check(f, c, table, [0.0, link], np.zeros(3), f"link {link}")
            assert got["evals"] == fl["evals"] and got["pairs"][0] + got["pairs"][1] == fl["links"]
    finally:
        f.close()


# ---- periodic ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,reaches,refused", ((3, (1,), 2), (5, (1, 2), 3), (6, (1, 2), 3), (7, (1, 2, 3), 4)))
def test_periodic_boxes(gpu, dim, reaches, refused):
    c, table = _table(f"periodic_box_{dim}")
    mean = VC.mean_heading(c["vel"])
    f = TorusStats(gpu, c["pos"], c["vel"], c["col"], c["params"])
    try:
        for m in reaches:
            for edges in (np.linspace(0.0, 5.0 * m, 17), np.geomspace(0.05, 5.0 * m - 0.3, 9)):
                got, _ = check(f, c, table, edges, mean, f"box_{dim} m={m}")
        rc, fl = f.flocks(5.0)
        got, _ = check(f, c, table, [0.0, 5.0], mean, f"box_{dim} link")
        assert rc == 0 and got["evals"] == fl["evals"] and got["pairs"][0] + got["pairs"][1] == fl["links"]
        rc, res = corr(f, np.linspace(0.0, 5.0 * (refused - 1) + 0.5, 5), mean)  # one cell too far for this box
        msg = gpu.last_error()
        assert rc == -1 and msg.startswith(CALL + ": ") and f"= {refused} cells" in msg and f"dim = {dim}" in msg, msg
        assert f"last edge is {5 * (refused - 1)}" in msg, msg
        _untouched(res)
    finally:
        f.close()


@pytest.mark.parametrize("kind", ("face_pair", "face", "edge", "corner"))
def test_pairs_through_faces(gpu, kind):
    for c, reaches in ((VC.torus_pair(kind), (1,)), (VC.wide_pair(kind), (1, 2))):
        table = VR.PairTable(c["pos"], c["params"], True)
        f = handle(gpu, c)
        try:
            for m in reaches:
                last = 5.0 * m if kind != "face_pair" else (1.0 if m == 1 else 6.5)
                got, _ = check(f, c, table, [0.0, np.nextafter(last, 0.0), last], np.zeros(3), f"{c['name']} m={m}")
                assert sum(got["pairs"]) >= 1
                if kind == "face_pair":  # d == 1 exactly through the face: in the bin whose upper edge it is
                    assert got["pairs"][2] == (1 if m == 1 else 0) and (m == 1 or got["pairs"][1] == 1)
        finally:
            f.close()


def test_blob_across_a_corner(gpu):
    out = run_case(gpu, "corner_blob", [np.linspace(0.0, 5.0, 33), np.linspace(0.25, 10.0, 14)])
    identity(out[0][0], 300)  # a cube of side 2.5: every pair is closer than 5


# ---- the unit lattice ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic", (False, True))
def test_unit_lattice_at_and_one_ulp_below_its_distances(gpu, periodic):
    (got, want), = run_case(gpu, "lattice_periodic" if periodic else "lattice_walled", [VC.LATTICE_EDGES])
    assert want["reach"] == 3
    # a distance whose rounded root squares to at least itself sits in the bin between "one ulp below" and "at" (1, sqrt 2,
    # 2, 3); sqrt 3 squares to less than 3, so those pairs fall into the next bin: the edges are squared, not the distances
    assert sum(got["pairs"]) > 0 and got["pairs"][0] == got["pairs"][2] == 0
    if periodic:  # 6, 12 and 8 neighbours each
        assert got["pairs"][1] == 3 * 4096 and got["pairs"][3] == 6 * 4096 and got["pairs"][5] + got["pairs"][6] == 4 * 4096


# ---- the candidate boundary ----------------------------------------------------------------------------------------------
def test_pairs_on_the_candidate_boundary(gpu):
    for m in (1, 2, 3):
        c = VC.boundary(m)
        f = handle(gpu, c)
        try:
            got, want = check(f, c, VR.PairTable(c["pos"], c["params"], False), [0.0, 1.0, 5.0 * m], np.zeros(3), c["name"])
            # 0-1 at d = 5 m is counted; 1-2 is m + 1 cells apart: not a candidate, and out of range anyway
            assert got["pairs"] == [0, 1, 1] and got["evals"] == 2 and want["cut"] == 0
        finally:
            f.close()
    c = VC.boundary_face(2)
    f = handle(gpu, c)
    try:
        got, want = check(f, c, VR.PairTable(c["pos"], c["params"], True), [0.0, 1.0, 10.0], np.zeros(3), c["name"], cut_allowed=True)
        assert want["cut"] == 1 and got["evals"] == 2 and got["pairs"] == [0, 1, 1]  # the pair at exactly 10 is cut: the rule
    finally:
        f.close()


# ---- velocities ----------------------------------------------------------------------------------------------------------
def test_velocities_zero_and_equal(gpu):
    c0, table = _table("uniform_2049")
    n = len(c0["pos"])
    edges = np.linspace(0.0, 10.0, 9)
    mean = np.array([0.25, -0.5, 2.0 ** -24 * 1.5])  # the last one quantises at a tie: rint(-1.5) = -2
    c = VC.with_velocities(c0, np.zeros((n, 3)), "rest")
    f = handle(gpu, c)
    try:
        got, _ = check(f, c, table, edges, mean, c["name"])
        q = [-(1 << 22), 1 << 23, -2]
        assert got["qsum"] == [n * x for x in q] and got["qsq"] == n * sum(x * x for x in q)
        assert got["dot"] == [p * sum(x * x for x in q) for p in got["pairs"]]
    finally:
        f.close()
    v = np.tile([[3.0, -4.0, 12.0]], (n, 1))
    c = VC.with_velocities(c0, v, "equal")
    f = handle(gpu, c)
    try:
        got, _ = check(f, c, table, edges, v[0] / 13.0, c["name"])
        assert got["dot"] == [0] * 9 and got["qsq"] == 0 and sum(got["pairs"]) > 0
    finally:
        f.close()


def test_a_velocity_that_is_not_finite(gpu):
    c0, table = _table("uniform_2049")
    v = c0["vel"].copy()
    v[7] = [np.nan, 1.0, 2.0]
    v[8] = [np.inf, 1.0, 2.0]  # u = (nan, 0, 0): q = 0 in x only
    c = VC.with_velocities(c0, v, "nonfinite")
    f = handle(gpu, c)
    try:
        check(f, c, table, np.linspace(0.0, 10.0, 9), VC.mean_heading(c0["vel"]), c["name"])
    finally:
        f.close()


def _stepped(nat, periodic):
    if periodic:
        prm = BC.params(bounds=17.5)
        c = VC._case("noisy", np.random.default_rng(31).uniform(-17.5, 17.5, (2000, 3)), prm, 31, periodic=True)
        f = PeriodicFlock(nat, c["pos"], c["vel"], c["col"], c["params"])
        assert set_mode(f, TOPOLOGICAL, 7) == 0
        nat.check_arg(f.lib.bdmi_set_noise(f.h, 2.0, 5, -1), "bdmi_set_noise")
    else:
        c = VC.uniform(2049)
        f = RawFlock(nat, c["pos"], c["vel"], c["col"], c["params"])
    f.step(1.0 / 60.0, 50)
    return c, f


@pytest.mark.parametrize("periodic", (False, True))
def test_the_state_after_50_steps(gpu, periodic):
    c, f = _stepped(gpu, periodic)
    try:
        pos, vel, _ = f.state()
        s = dict(c, pos=pos, vel=vel)
        table = VR.PairTable(pos, c["params"], periodic)
        for edges in (np.linspace(0.0, 5.0, 17), np.linspace(0.0, 15.0, 17)):
            check(f, s, table, edges, VC.mean_heading(vel), f"stepped periodic={periodic}")
    finally:
        f.close()


# ---- sizes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0, 1, 2, 64, 65, 257))
def test_sizes(gpu, n):
    c = VC.sizes(n)
    f = handle(gpu, c)
    try:
        got, _ = check(f, c, VR.PairTable(c["pos"], c["params"], False), np.linspace(0.0, VC.WHOLE_GRID, 12), np.zeros(3), c["name"])
        identity(got, n)
        if n < 2:
            assert got["evals"] == 0 and sum(got["pairs"]) == 0
    finally:
        f.close()


def test_coincident_twins_and_a_crowded_cell(gpu):
    (got, _), = run_case(gpu, "twins", [np.array([0.0, 1.0, 5.0])], mean=np.zeros(3))
    assert got["pairs"][0] == 40
    out = run_case(gpu, "crowded", [np.linspace(0.0, 5.0, 17), np.geomspace(0.01, 10.0, 65)])
    assert out[0][0]["evals"] > 3000 * 2999 // 2


# ---- order and repeatability -----------------------------------------------------------------------------------------------
def test_caller_order_and_repetition(gpu):
    c, table = _table("uniform_2049")
    edges, mean = np.linspace(0.5, 10.0, 20), VC.mean_heading(c["vel"])
    f = handle(gpu, c)
    g = handle(gpu, VC.permuted(c))
    try:
        first = check(f, c, table, edges, mean, "first")[0]
        assert decoded(corr(f, edges, mean)[1], 19) == first and decoded(corr(g, edges, mean)[1], 19) == first
    finally:
        f.close()
        g.close()


_CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import conftest, nbmi_native as nat
import vcorr_cases as VC
from test_gpu_boids_vcorr import corr, decoded, handle
c = VC.periodic_box(7) if {periodic} else VC.uniform(2049)
f = handle(nat, c)
rc, res = corr(f, np.linspace(0.0, 15.0, 17), VC.mean_heading(c["vel"]))
assert rc == 0, nat.last_error()
print(json.dumps(decoded(res, 16)))
f.close()
"""


@pytest.mark.parametrize("periodic", (False, True))
def test_block_order_changes_nothing(gpu, periodic):
    """BDMI_XCD is read when a handle is made: the hardware block order in a fresh child process, the default one here."""
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, BDMI_XCD="0")
    out = subprocess.run([sys.executable, "-c", _CHILD.format(tests=tests, root=os.path.dirname(tests), periodic=periodic)], env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    c = VC.periodic_box(7) if periodic else VC.uniform(2049)
    f = handle(gpu, c)
    try:
        rc, res = corr(f, np.linspace(0.0, 15.0, 17), VC.mean_heading(c["vel"]))
        assert rc == 0 and decoded(res, 16) == json.loads(out.stdout.strip().splitlines()[-1])
    finally:
        f.close()


@pytest.mark.parametrize("periodic", (False, True))
def test_calls_between_steps_change_nothing(gpu, periodic):
    c = VC.periodic_box(7) if periodic else VC.uniform(2049)
    a, b = handle(gpu, c), handle(gpu, c)
    try:
        for k in range(12):
            a.step(1.0 / 60.0)
            b.step(1.0 / 60.0)
            if k % 3 == 2:
                rc, res = corr(b, np.linspace(0.0, 10.0, 17), np.zeros(3))
                rc0, res0 = corr(b, None, np.zeros(3))
                assert rc == 0 and rc0 == 0 and res["evals"] > 0
        for x, y in zip(a.state(), b.state()):
            assert R.same_bits(x, y)
    finally:
        a.close()
        b.close()


def test_grid_info_describes_the_query_grid(gpu):
    c = VC.uniform(2049)
    f = handle(gpu, c)
    try:
        assert corr(f, [0.0, 5.0], np.zeros(3))[0] == 0
        occ = C.c_int64(0)
        gpu.check(f.lib.bdmi_grid_info(f.h, None, None, C.addressof(occ)), "bdmi_grid_info")
        assert occ.value == len(np.unique(R.cell_index(c["pos"], c["params"])))
    finally:
        f.close()


# ---- nb == 0, refusals ---------------------------------------------------------------------------------------------------
def test_moments_alone(gpu):
    c = VC.uniform(2049)
    f = handle(gpu, c)
    try:
        for mean in (np.zeros(3), VC.mean_heading(c["vel"])):
            rc, res = corr(f, None, mean)
            assert rc == 0, gpu.last_error()
            qsum, qsq = VR.self5(VR.quantise(c["vel"], mean))
            assert [int(x) for x in res["self5"][:3]] == qsum and VR.from_hi_lo(*res["self5"][3:]) == qsq
            assert res["evals"] == 0 and (res["pairs"] == -7).all() and (res["dot"] == -7).all()
        assert corr(f, None, np.zeros(3), outputs=False)[0] == 0
    finally:
        f.close()


def _untouched(res):
    assert (res["pairs"] == -7).all() and (res["dot"] == -7).all() and (res["self5"] == -7).all() and res["evals"] == -7


def test_refusals_leave_the_outputs_alone(gpu):
    c = VC.uniform(2049)
    f = handle(gpu, c)
    ok = np.linspace(0.0, 10.0, 9)
    zero = np.zeros(3)
    try:
        def refused(rc_res, *words):
            rc, res = rc_res
            msg = gpu.last_error()
            assert rc == -1 and msg.startswith(CALL + ": ") and all(w in msg for w in words), (msg, words)
            _untouched(res)
        refused(corr(f, ok, zero, nb=-1), "nb = -1")
        refused(corr(f, np.linspace(0.0, 10.0, 67), zero, nb=65), "nb = 65")
        refused(corr(f, None, zero, nb=3), "null edges")
        refused(corr(f, ok, None), "null mean3")
        for k, bad in ((0, -1.0), (3, float("nan")), (8, float("inf")), (4, ok[3]), (5, 1.0), (8, 1e200)):
            e = ok.copy()
            e[k] = bad
            refused(corr(f, e, zero), f"edges[{k}]", f"{bad:g}")
        refused(corr(f, [0.0, 1e-200, 2e-200], zero), "edges[1]")  # the squares are not increasing
        refused(corr(f, [0.0, 80.5], zero), "= 17 cells", "dim = 7", "last edge is 80")
        for k, bad in ((0, 1.5), (1, -1.0000001), (2, float("nan")), (0, float("inf"))):
            m = zero.copy()
            m[k] = bad
            refused(corr(f, ok, m), f"mean3[{k}]")
            refused(corr(f, None, m), f"mean3[{k}]")
        rc = f.lib.bdmi_velocity_correlation(None, 0, None, gpu.ptr(zero), None, None, None, None)
        assert rc == -1 and gpu.last_error().startswith(CALL + ": null")
        assert corr(f, ok, zero)[0] == 0  # and the handle works on
    finally:
        f.close()


def test_slab_handle_refused(gpu):
    lib = gpu.load()
    n = 64
    rng = np.random.default_rng(0)
    pos, vel, col = rng.uniform(-20, 20, (n, 3)), rng.uniform(-5, 5, (n, 3)), rng.random((n, 3))
    ids = np.arange(n, dtype=np.int32)
    prm = BC.params(bounds=30.0)
    h = lib.bdmi_create_slab(n, gpu.ptr(pos), gpu.ptr(vel), gpu.ptr(col), gpu.ptr(ids), 2 * n, gpu.ptr(prm), -35.0, 35.0, 0, 0, 0)
    assert h, gpu.last_error()
    try:
        f = RawFlock.__new__(RawFlock)
        f.lib, f.nat, f.n, f.h = lib, gpu, n, h
        for edges in ([0.0, 5.0], None):
            rc, res = corr(f, edges, np.zeros(3))
            assert rc == -1 and gpu.last_error().startswith(CALL + ": refused on a slab handle"), gpu.last_error()
            _untouched(res)
    finally:
        lib.bdmi_destroy(h)


# ---- the Python layers ---------------------------------------------------------------------------------------------------
def _config_params():
    from config import boids as config
    return np.array([float(config.BOIDS[k]) for k in config.PARAM_ORDER], dtype=np.float64)


def test_flock_class_methods(gpu):
    from boids import Flock
    from boids.analysis import correlation_length, susceptibility, velocity_correlation_function
    for periodic in (False, True):
        fl = Flock(2000, seed=5, periodic=periodic)
        try:
            rng = np.random.default_rng(5)
            fl.set_state(positions=rng.uniform(-20, 20, (2000, 3)))
            fl.update(1.0 / 60.0, 3)
            pos, vel = fl.positions, fl.velocities
            prm = _config_params()
            edges = np.linspace(0.0, 3.0 * fl.box["cell_size"], 13)
            mom = fl.heading_moments()
            qsum, qsq = VR.self5(VR.quantise(vel, np.zeros(3)))
            assert mom == dict(qsum=qsum, qsq=qsq)
            res = fl.velocity_correlation(edges)
            assert res["mean"] == [x / (2000 * 2.0 ** 24) for x in qsum] and res["quantum"] == 2.0 ** -24 and res["reach"] == 3
            want = VR.correlate(pos, vel, prm, edges, res["mean"], periodic)
            assert [int(x) for x in res["pairs"]] == [int(x) for x in want["pairs"]] and res["dot"] == want["dot"]
            assert (res["evals"], res["qsum"], res["qsq"], res["n"]) == (want["evals"], want["qsum"], want["qsq"], 2000)
            r, cfun = velocity_correlation_function(res)
            assert len(r) == 13 and np.isfinite(cfun[1:]).all() and susceptibility(res)["chi"] >= 0
            correlation_length(res)
            with pytest.raises(ValueError, match="bdmi_velocity_correlation: "):
                fl.velocity_correlation(np.linspace(0.0, 1e4, 5))
            with pytest.raises(ValueError):
                fl.heading_moments((2.0, 0.0, 0.0))
        finally:
            fl.close()


@pytest.mark.parametrize("flags", ([], ["--periodic", "--noise", "1.5", "--neighbours", "topological"]))
def test_flock_video_correlations(gpu, tmp_path, monkeypatch, flags):
    """6 frames at 2 000 boids with --correlations 2: the three lines equal those recomputed from the fetched states, and
    the frames are the bytes of a run without the option."""
    from boids import Flock
    from boids.analysis import correlation_line
    from tools import flock_video
    monkeypatch.setitem(flock_video.RESOLUTION_PRESETS, "tiny", (64, 36))
    base = ["--boids", "2000", "--frames", "6", "--seed", "3", "--resolution", "tiny", "--format", "raw"] + flags
    states = []

    class Spy(Flock):
        def velocity_correlation(self, edges, mean=None):
            res = super().velocity_correlation(edges, mean)
            states.append((self.positions.copy(), self.velocities.copy(), res))
            return res

    def make(n, seed, device, **kw):
        return Spy(n, seed=seed, device=device, **kw)
    quiet = lambda *a, **k: None  # noqa: E731
    plain = flock_video.run(flock_video.build_parser().parse_args(base + ["-o", str(tmp_path / "plain.rgb")]), say=quiet)
    t = flock_video.run(flock_video.build_parser().parse_args(base + ["-o", str(tmp_path / "corr.rgb"), "--correlations", "2",
                                                                      "--correlation-edges", "auto"]), make_flock=make, say=quiet)
    assert plain["ok"] and t["ok"] and t["correlation_lines"] == 3 and "correlations" not in plain
    assert (tmp_path / "corr.rgb").read_bytes() == (tmp_path / "plain.rgb").read_bytes()
    lines = (tmp_path / "corr.correlation.jsonl").read_text().splitlines()
    assert len(lines) == 3 and len(states) == 3
    periodic = "--periodic" in flags
    for k, (line, (pos, vel, res)) in enumerate(zip(lines, states)):
        rec = json.loads(line)
        assert rec["frame"] == 2 * k and rec["steps"] == 2 * k + 1 and len(rec["edges"]) == 17
        assert set(rec) == {"frame", "steps", "edges", "pairs", "dot", "mean", "C", "xi", "chi"}
        prm = _config_params()
        cell = VR.grid_of(prm, periodic)[0]
        assert np.array_equal(rec["edges"], np.linspace(0.0, 4.0 * cell, 17))
        want = VR.correlate(pos, vel, prm, rec["edges"], rec["mean"], periodic)
        assert rec["pairs"] == [int(x) for x in want["pairs"]] and [int(x) for x in rec["dot"]] == want["dot"]
        assert line == correlation_line(2 * k, 2 * k + 1, dict(VR.result_dict(want, rec["edges"], 2000), mean=rec["mean"]))
    meta = json.loads((tmp_path / "corr.rgb.json").read_text())
    assert meta["correlations"]["file"] == "corr.correlation.jsonl" and meta["correlations"]["every"] == 2
    assert "correlations" not in json.loads((tmp_path / "plain.rgb.json").read_text())
