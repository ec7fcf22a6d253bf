"""nbmi_radial_profile and nbmi_mass_radii on the GPU against the NumPy restatement of tests/profile_ref.py (include/nbmi.h;
DESIGN.md section 4.26).

Every comparison is BIT FOR BIT - planes, stats and exponents; radius2, inside, mass_inside, total_mass: a quantity is a
function of float64 operations that the kernels and NumPy form in the same association, its integer is one rint of an
exact scaling, the sums are integers and the selection compares integers.
"""
import numpy as np
import pytest

import profile_cases as pc
import profile_ref as pr
import query_cases as qc

pytestmark = pytest.mark.gpu

NBMI_ERR_ARG = -1


def _profile(gpu, sims, tag, p, v, m, center, bulk, edges, quantities=pr.ALL, ref=None):
    """every handle of `sims` against the restatement of the state (p, v, m); returns the reference"""
    if ref is None:
        ref = pr.radial_profile(p, v, m, center, bulk, edges, quantities)
    for i, sim in enumerate(sims):
        rc, out, st, ex = pc.raw_profile(gpu, sim, center, bulk, edges, quantities)
        assert rc == 0, (tag, i, gpu.last_error())
        bad = int((out.view(np.int64) != ref[0].view(np.int64)).sum()) if out.shape == ref[0].shape else -1
        print(f"{tag} handle {i}: stats {st.tolist()} (reference {ref[1].tolist()}), exponents {ex.tolist()}, {bad} of {out.size} differ")
        assert bad == 0 and np.array_equal(st, ref[1]) and np.array_equal(ex, ref[2]), (tag, i)
    return ref


def _radii(gpu, sims, tag, p, m, center, fractions, ref=None):
    if ref is None:
        ref = pr.mass_radii(p, m, center, fractions)
    for i, sim in enumerate(sims):
        rc, r2, ins, mass, total, st, ex = pc.raw_radii(gpu, sim, center, fractions)
        assert rc == 0, (tag, i, gpu.last_error())
        print(f"{tag} handle {i}: radius2 {r2.tolist()} inside {ins.tolist()} total {total} stats {st.tolist()} e {ex}")
        assert pc.same_bits(r2, ref[0]) and np.array_equal(ins, ref[1]) and pc.same_bits(mass, ref[2]), (tag, i, ref)
        assert pc.same_bits([total], [ref[3]]) and np.array_equal(st, ref[4]) and ex == ref[5], (tag, i, ref)
    return ref


# ---- sizes, shell counts and selections ----
@pytest.mark.parametrize("n", pc.SIZES)
def test_sizes_shell_counts_and_quantities(gpu, n):
    p, v, m = pc.cloud(n)
    with pc.Handles(p, v, m) as sims:
        for nb in (1, 7, 256):
            for first in (0.0, 0.25):
                edges = pc.edges_for(nb, first=first)
                ref = _profile(gpu, sims, f"n {n} nb {nb} first {first} all", p, v, m, pc.CENTER, pc.BULK, edges)
                assert ref[1].sum() == n
                if n >= 1023:
                    assert ref[1][0] > 0 and ref[1][1] > 0, "the case lost its point: nobody beyond"
                if first:
                    continue
                for q in pr.SINGLE:  # a single quantity: the same planes, the same exponents
                    sel = pr.PLANES_OF[q]
                    _profile(gpu, sims, f"n {n} nb {nb} q {q}", p, v, m, pc.CENTER, pc.BULK, edges, q,
                             ref=(ref[0][sel], ref[1], ref[2][sel]))
        _profile(gpu, sims, f"n {n} no bulk velocity", p, v, m, pc.CENTER, None, pc.edges_for(7))
        ref = _radii(gpu, sims, f"n {n} radii", p, m, pc.CENTER, pc.FRACTIONS)
        if n:
            assert ref[1][5] == n and ref[0][5] == pr.radii2(p, pc.CENTER)[3].max()  # f = 1: everybody, the largest r2


# ---- edge membership, the centre, bodies that are skipped ----
@pytest.mark.parametrize("first", [0.0, 1.0])
def test_bodies_on_edges_at_the_centre_and_not_finite(gpu, first):
    edges = np.array([first, 2.0, 3.0, 4.5, 8.0, 16.0, 17.0])
    p = pc.on_edges(edges)
    p = np.concatenate([p, [[np.nan, 0.0, 0.0], [1e200, 0.0, 0.0], [0.0, -np.inf, 0.0]], pc.cloud(200, seed=2)[0]])
    rng = np.random.RandomState(3)
    v, m = rng.normal(size=p.shape), rng.uniform(0.5, 2.0, len(p))
    E = edges * edges
    r2 = pr.radii2(p, pc.CENTER)[3]
    assert all((r2 == e2).any() for e2 in E), "the case lost its point: no body exactly on an edge"
    with pc.Handles(p, v, m, kind="direct") as sims:  # (a direct handle: no tree has to hold these coordinates)
        ref = _profile(gpu, sims, f"on edges first {first}", p, v, m, pc.CENTER, pc.BULK, edges)
        assert ref[1][2] == 3 and ref[1][1] > 0
        # the upper edge belongs to the shell: the body on edges[k] alone is counted in slot k (the restatement's
        # membership is checked against the text in tests/test_profile_host.py)
        for k in range(len(edges)):
            one = pr.radial_profile(p[1 + 2 * k:2 + 2 * k], v[:1], m[:1], pc.CENTER, None, edges, pr.NUMBER)
            assert one[0][0].tolist() == [1.0 if s == k else 0.0 for s in range(len(edges))]
        ref = _radii(gpu, sims, f"on edges radii first {first}", p, m, pc.CENTER, pc.FRACTIONS)
        assert ref[4].tolist() == [len(p) - 3, 3]


def test_every_body_in_one_shell_and_every_body_beyond(gpu):
    rng = np.random.RandomState(4)
    d = rng.normal(size=(4097, 3))
    p = np.array(pc.CENTER) + d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(2.1, 2.9, 4097)[:, None]
    v, m = rng.normal(size=p.shape), rng.uniform(0.5, 2.0, len(p))
    with pc.Handles(p, v, m) as sims:
        for nb, edges in ((7, [0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 5.0, 6.0]), (1, [2.0, 3.0])):
            ref = _profile(gpu, sims, f"one shell nb {nb}", p, v, m, pc.CENTER, pc.BULK, edges)
            assert ref[1].tolist() == [4097, 0, 0] and np.count_nonzero(ref[0][0]) == 1
        ref = _profile(gpu, sims, "all beyond", p, v, m, pc.CENTER, pc.BULK, [0.0, 0.5, 1.0])
        assert ref[1].tolist() == [0, 4097, 0] and (ref[0] == 0.0).all() and (ref[2] != 0).all()  # the maxima count them
        ref = _profile(gpu, sims, "all in the inner ball", p, v, m, pc.CENTER, pc.BULK, [3.0, 4.0])
        assert ref[1].tolist() == [4097, 0, 0] and ref[0][0].tolist() == [4097.0, 0.0]


def test_masses_spanning_2_to_the_40(gpu):
    p, v, _ = pc.cloud(3000, seed=5)
    rng = np.random.RandomState(5)
    m = np.exp2(rng.uniform(-40.0, 0.0, 3000))
    m[::7] = np.exp2(-70.0)  # below half the quantum of either call: their k round to 0
    with pc.Handles(p, v, m) as sims:
        ref = _profile(gpu, sims, "masses 2^-70 .. 1", p, v, m, pc.CENTER, pc.BULK, pc.edges_for(7))
        assert np.exp2(-70.0) < 2.0 ** (int(ref[2][1]) - 1)
        rad = _radii(gpu, sims, "masses 2^-70 .. 1 radii", p, m, pc.CENTER, pc.FRACTIONS)
        assert np.exp2(-70.0) < 2.0 ** (rad[5] - 1) and rad[3] < m.sum()
    with pc.Handles(p, v, 0.0 * m) as sims:
        ref = _profile(gpu, sims, "masses 0", p, v, 0.0 * m, pc.CENTER, pc.BULK, pc.edges_for(7))
        assert ref[2][1:].tolist() == [0] * 7 and (ref[0][1:] == 0.0).all() and ref[2][0] != 0
        rad = _radii(gpu, sims, "masses 0 radii", p, 0.0 * m, pc.CENTER, pc.FRACTIONS)
        assert np.isnan(rad[0]).all() and (rad[1] == 0).all() and rad[3] == 0.0 and rad[4].tolist() == [3000, 0]


# ---- the selection ----
def test_radii_with_ties_and_thresholds_on_cumulative_values(gpu):
    """equal masses on shells of six bodies (+-x, +-y, +-z at equal radius): T lands exactly on cumulative values, and
    a run of ties enters together"""
    radii = np.array([1.0, 2.0, 3.0, 5.0, 8.0, 13.0, 21.0, 34.0, 55.0, 89.0])
    unit = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    p = np.array(pc.CENTER) + (radii[:, None, None] * unit[None]).reshape(-1, 3)
    p = p[np.random.RandomState(6).permutation(len(p))]
    v, m = np.zeros_like(p), np.full(len(p), 0.75)
    fractions = [0.5, 0.1, 0.1, 1.0, 0.125, 0.25, 0.75, 1e-12, 0.6]
    exact = [0, 3, 4, 5, 6, 7]  # the fractions whose T can be stated by hand: 30, 60, 7.5, 15, 45 bodies' worth and T = small
    with pc.Handles(p, v, m) as sims, pc.Handles(p, v, m, kind="direct") as direct:
        ref = _radii(gpu, sims, "ties", p, m, pc.CENTER, fractions)
        _radii(gpu, direct, "ties direct", p, m, pc.CENTER, fractions, ref=ref)
        assert ref[0][exact].tolist() == [64.0, 89.0 ** 2, 4.0, 9.0, 34.0 ** 2, 1.0]  # (0.5: T is exactly the 30th body's sum)
        assert ref[1][exact].tolist() == [30, 60, 12, 18, 48, 6] and ref[3] == 45.0
        assert ref[2][exact].tolist() == [22.5, 45.0, 9.0, 13.5, 36.0, 4.5]
    # every body at one radius: one run holds everything
    q = np.array(pc.CENTER) + np.tile(unit * 2.0, (700, 1))
    with pc.Handles(q, np.zeros_like(q), np.full(len(q), 1.0), kind="direct") as sims:  # (700 coincident bodies: no tree)
        ref = _radii(gpu, sims, "one run", q, np.full(len(q), 1.0), pc.CENTER, [0.001, 0.5, 1.0])
        assert ref[0].tolist() == [4.0] * 3 and ref[1].tolist() == [4200] * 3


# ---- order independence, handle types, repeated calls ----
def test_order_of_the_state_rows_and_handle_type(gpu):
    """a Barnes-Hut handle before any step, after 3 steps (state in key order), a direct handle given that state, a fresh
    Barnes-Hut handle given it in reversed body order: the same bits whenever the float64 state is the same, and twice
    the same bits from one handle"""
    p, v, m = qc.preset("galaxy", 6000, seed=3)
    edges = pc.edges_for(48, first=2.0, last=300.0)
    c, b = (3.0, -2.0, 1.0), (0.01, 0.0, -0.02)
    with pc.Handles(p, v, m) as stepped:
        _profile(gpu, stepped, "before any step", p, v, m, c, b, edges)
        _radii(gpu, stepped, "before any step radii", p, m, c, pc.FRACTIONS)
        for s in stepped:
            s.step_many(0.05, 3)
        x, w = stepped[0].get_positions_f64(), stepped[0].get_velocities()
        assert not np.array_equal(x, p)
        with pc.Handles(p, v, m, kind="direct") as direct, pc.Handles(x[::-1], w[::-1], m[::-1]) as fresh:
            for s in direct:
                s.set_state(x, w)
            ref = _profile(gpu, stepped, "stepped", x, w, m, c, b, edges)
            rad = _radii(gpu, stepped, "stepped radii", x, m, c, pc.FRACTIONS)
            for tag, sims in (("direct", direct), ("reversed", fresh), ("stepped again", stepped)):
                _profile(gpu, sims, tag, x, w, m, c, b, edges, ref=ref)
                _radii(gpu, sims, tag + " radii", x, m, c, pc.FRACTIONS, ref=rad)
            assert ref[1][0] > 0 and ref[1][1] > 0


@pytest.mark.parametrize("kind", ["plain", "leapfrog", "tracers"])
def test_calls_between_steps_change_nothing(gpu, kind):
    """5 steps with both calls between all steps against 5 steps without: positions, velocities and tracers bit for bit"""
    from nbody.gpu_backend import PROFILE_QUANTITIES
    p, v, m = qc.preset("galaxy", 6000, seed=4)
    tr = np.random.RandomState(6).normal(size=(100, 3)) * 200.0
    kw = {"integrator": "leapfrog"} if kind != "plain" else {}
    edges = pc.edges_for(48, first=2.0, last=3000.0)
    with pc.Handles(p, v, m, **kw) as sims, pc.Handles(p, v, m, **kw) as plain:
        for s in sims + plain:
            if kind == "tracers":
                s.set_tracers(tr)
        for step in range(5):
            for s in sims:
                got = s.radial_profile(edges, quantities=tuple(PROFILE_QUANTITIES))
                assert got["number"].sum() > 0
                assert np.isfinite(s.mass_radii(pc.FRACTIONS)["radius2"]).all()
                s.step(0.05)
            for s in plain:
                s.step(0.05)
        for s in sims:
            s.radial_profile(edges)
            s.mass_radii([0.5])
        want_x, want_v = plain[0].get_positions_f64(), plain[0].get_velocities()
        for s in sims + plain[1:]:
            assert np.array_equal(s.get_positions_f64(), want_x) and np.array_equal(s.get_velocities(), want_v)
            assert s.step_count() == 5
            if kind == "tracers":
                a, b = s.get_tracers(), plain[0].get_tracers()
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[0], tr)
        assert sims[0].force_precision_share() == plain[0].force_precision_share()


def test_after_every_other_analysis_call_a_fresh_handles_bits(gpu):
    """the property of DESIGN.md section 4.14.2 for the two new calls: whatever query ran before, they return what a
    fresh handle returns"""
    p, v, m = qc.preset("galaxy", 5000, seed=9)
    edges = pc.edges_for(16, first=2.0, last=3000.0)
    c = (3.0, -2.0, 1.0)
    ref = pr.radial_profile(p, v, m, c, pc.BULK, edges, pr.ALL)
    rad = pr.mass_radii(p, m, c, pc.FRACTIONS)
    before = {
        "diagnostics": lambda s: s.diagnostics(),
        "knn": lambda s: s.knn(8),
        "fof": lambda s: s.find_groups(5.0),
        "pair_counts": lambda s: s.pair_counts([1.0, 10.0, 100.0]),
        "field_at": lambda s: s.field_at(p[:50] + 0.5),
        "deposit": lambda s: s.deposit((-500.0,) * 3, (500.0,) * 3, (8, 8, 8)),
        "radial_profile": lambda s: s.radial_profile([1.0, 5.0], center="origin", bulk_velocity=None),
        "mass_radii": lambda s: s.mass_radii([0.3], center="origin"),
    }
    with pc.Handles(p, v, m) as sims:
        _profile(gpu, sims, "fresh", p, v, m, c, pc.BULK, edges, ref=ref)
        for name, call in before.items():
            for s in sims:
                call(s)
            _profile(gpu, sims, f"after {name}", p, v, m, c, pc.BULK, edges, ref=ref)
            for s in sims:
                call(s)
            _radii(gpu, sims, f"radii after {name}", p, m, c, pc.FRACTIONS, ref=rad)


# ---- the Python layer ----
def test_python_methods_equal_the_raw_calls(gpu):
    from nbody import profile as prof
    p, v, m = qc.preset("galaxy", 5000, seed=10)
    edges = prof.auto_edges(800.0, shells=24)
    with pc.Handles(p, v, m) as sims:
        for sim in sims:
            d = sim.diagnostics(potential=False)
            c, b = np.array(d.center_of_mass), np.array(d.momentum) / d.mass
            got = sim.radial_profile(edges, quantities=("mass", "angular_momentum", "number", "radial_kinetic"), stats=True)
            assert np.array_equal(got["center"], c) and np.array_equal(got["bulk_velocity"], b)
            rc, out, st, ex = pc.raw_profile(gpu, sim, c, b, edges, pr.NUMBER | pr.MASS | pr.RADIAL_KINETIC | pr.ANGULAR_MOMENTUM)
            assert rc == 0 and got["stats"] == tuple(st.tolist()) and np.array_equal(got["exponents"], ex)
            assert pc.same_bits(got["number"], out[0]) and pc.same_bits(got["mass"], out[1])
            assert pc.same_bits(got["radial_kinetic"], out[2]) and pc.same_bits(got["angular_momentum"], out[3:6])
            assert got["angular_momentum"].shape == (3, 25) and got["stats"][0] > 0
            zero = sim.radial_profile(edges, center=None, bulk_velocity="origin", quantities="kinetic")
            rc, out, st, ex = pc.raw_profile(gpu, sim, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), edges, pr.KINETIC)
            assert rc == 0 and pc.same_bits(zero["kinetic"], out[0]) and sorted(zero) == ["bulk_velocity", "center", "exponents", "kinetic"]
            given = sim.radial_profile(edges, center=(1.0, 2.0, 3.0), bulk_velocity=(0.5, 0.0, 0.0), quantities=("radial_momentum",))
            rc, out, st, ex = pc.raw_profile(gpu, sim, (1.0, 2.0, 3.0), (0.5, 0.0, 0.0), edges, pr.RADIAL_MOMENTUM)
            assert rc == 0 and pc.same_bits(given["radial_momentum"], out[0])
            mr = sim.mass_radii(pc.FRACTIONS)
            rc, r2, ins, mass, total, st2, e = pc.raw_radii(gpu, sim, c, pc.FRACTIONS)
            assert rc == 0 and pc.same_bits(mr["radius2"], r2) and np.array_equal(mr["inside"], ins)
            assert pc.same_bits(mr["mass_inside"], mass) and mr["total_mass"] == total and mr["stats"] == tuple(st2.tolist())
            assert mr["exponent"] == e
            lr = prof.lagrangian_radii(sim, fractions=pc.FRACTIONS)
            assert pc.same_bits(lr, np.sqrt(r2)) and (np.diff(np.sort(lr)) >= 0).all()
            dc = prof.density_center(sim, k=16)
            assert dc.shape == (3,) and np.isfinite(sim.mass_radii([0.5], center=dc)["radius2"]).all()
            for bad in ({"quantities": ("charge",)}, {"quantities": ()}, {"center": "middle"}, {"center": (1.0, 2.0)},
                        {"bulk_velocity": "fast"}):
                with pytest.raises(ValueError, match="radial_profile"):
                    sim.radial_profile(edges, **bad)
            with pytest.raises(ValueError, match="radial_profile"):
                sim.radial_profile([1.0])
            with pytest.raises(ValueError, match="mass_radii"):
                sim.mass_radii([])
            with pytest.raises(ValueError, match="mass_radii"):
                sim.mass_radii([0.5, 1.5])


# ---- refusals ----
def test_refusals_before_any_launch_leave_the_outputs_untouched(gpu):
    p, v, m = pc.cloud(300)
    nan, inf = np.nan, np.inf
    good = [0.5, 1.0, 2.0]
    many = np.arange(258, dtype=np.float64)
    bad = [  # (center, bulk, edges, nb or None, quantities, part of the message)
        ((nan, 0, 0), None, good, None, 3, "center[0]"), ((0, 0, inf), None, good, None, 3, "center[2]"),
        (pc.CENTER, (0, nan, 0), good, None, 3, "bulk_velocity[1]"), (pc.CENTER, (-inf, 0, 0), good, None, 3, "bulk_velocity[0]"),
        (pc.CENTER, None, good, 0, 3, "nb = 0"), (pc.CENTER, None, good, -1, 3, "nb = -1"), (pc.CENTER, None, many, 257, 3, "nb = 257"),
        (pc.CENTER, None, [-0.5, 1.0], None, 3, "edges[0] = -0.5"), (pc.CENTER, None, [0.5, nan, 2.0], None, 3, "edges[1] = nan"),
        (pc.CENTER, None, [0.5, 1.0, 1.0], None, 3, "edges[2] = 1"), (pc.CENTER, None, [0.5, 2.0, 1.0], None, 3, "edges[2] = 1"),
        (pc.CENTER, None, [0.5, inf], None, 3, "edges[1] = inf"), (pc.CENTER, None, [1.0, 1e200], None, 3, "square of edges[1]"),
        (pc.CENTER, None, [1e-170, 2e-170], None, 3, "square of edges[1]"),
        (pc.CENTER, None, good, None, 0, "quantities = 0"), (pc.CENTER, None, good, None, 64, "quantities = 64"),
        (pc.CENTER, None, good, None, 127, "quantities = 127"), (pc.CENTER, None, good, None, -1, "quantities = -1"),
    ]
    bad_radii = [  # (center, fractions, nf or None, part of the message)
        ((nan, 0, 0), [0.5], None, "center[0]"), (pc.CENTER, [0.5], 0, "nf = 0"), (pc.CENTER, [0.5] * 65, None, "nf = 65"),
        (pc.CENTER, [0.5, 0.0], None, "fractions[1] = 0"), (pc.CENTER, [1.5], None, "fractions[0] = 1.5"),
        (pc.CENTER, [0.5, 0.5, nan], None, "fractions[2] = nan"), (pc.CENTER, [-0.25], None, "fractions[0] = -0.25"),
    ]
    with pc.Handles(p, v, m) as sims, pc.Handles(p, v, m, kind="direct") as direct:
        for sim in sims + direct:
            for c, b, edges, nb, q, word in bad:
                rc, out, st, ex = pc.raw_profile(gpu, sim, c, b, edges, q, nb=nb)
                err = gpu.last_error()
                assert rc == NBMI_ERR_ARG and err.startswith("nbmi_radial_profile: ") and word in err, (c, b, edges, nb, q, rc, err)
                assert (out == pc.PROFILE_FILL).all() and (st == pc.INT_FILL).all() and (ex == pc.INT_FILL).all()
            for c, f, nf, word in bad_radii:
                got = pc.raw_radii(gpu, sim, c, f, nf=nf)
                err = gpu.last_error()
                assert got[0] == NBMI_ERR_ARG and err.startswith("nbmi_mass_radii: ") and word in err, (c, f, nf, got[0], err)
                assert pc.radii_untouched(got)
            lib = gpu.load()
            c, e, out = np.array(pc.CENTER), np.array(good), np.full(6, pc.PROFILE_FILL)
            for args, word in (((None, None, 2, gpu.ptr(e), 3, gpu.ptr(out)), "null center"),
                               ((gpu.ptr(c), None, 2, None, 3, gpu.ptr(out)), "null edges"),
                               ((gpu.ptr(c), None, 2, gpu.ptr(e), 3, None), "null out")):
                assert lib.nbmi_radial_profile(sim._h, *args, None, None) == NBMI_ERR_ARG
                assert gpu.last_error().startswith("nbmi_radial_profile: ") and word in gpu.last_error()
            assert (out == pc.PROFILE_FILL).all()
            assert lib.nbmi_radial_profile(sim._h, gpu.ptr(c), None, 2, gpu.ptr(e), 3, gpu.ptr(out), None, None) == 0  # NULL stats, exponents
            assert out[:3].sum() > 0
            f, r2 = np.array([0.5]), np.full(1, pc.PROFILE_FILL)
            for args, word in (((None, 1, gpu.ptr(f), gpu.ptr(r2)), "null center"), ((gpu.ptr(c), 1, None, gpu.ptr(r2)), "null fractions"),
                               ((gpu.ptr(c), 1, gpu.ptr(f), None), "null radius2")):
                assert lib.nbmi_mass_radii(sim._h, *args, None, None, None, None, None) == NBMI_ERR_ARG
                assert gpu.last_error().startswith("nbmi_mass_radii: ") and word in gpu.last_error()
            assert r2[0] == pc.PROFILE_FILL
            assert lib.nbmi_mass_radii(sim._h, gpu.ptr(c), 1, gpu.ptr(f), gpu.ptr(r2), None, None, None, None, None) == 0
            assert r2[0] > 0


def test_maxima_and_masses_that_are_not_finite_are_refused(gpu):
    p, v, m = pc.cloud(300)
    v[17, 1] = np.inf
    edges = pc.edges_for(7)
    with pc.Handles(p, v, m, kind="direct") as sims:
        for sim in sims:
            rc, out, st, ex = pc.raw_profile(gpu, sim, pc.CENTER, pc.BULK, edges, pr.MASS | pr.KINETIC)
            err = gpu.last_error()
            assert rc == NBMI_ERR_ARG and err.startswith("nbmi_radial_profile: ") and "plane 1 (KINETIC)" in err
            assert (out == pc.PROFILE_FILL).all() and (st == pc.INT_FILL).all() and (ex == pc.INT_FILL).all()
            rc, out, st, ex = pc.raw_profile(gpu, sim, pc.CENTER, pc.BULK, edges, pr.ANGULAR_MOMENTUM)
            assert rc == NBMI_ERR_ARG and "ANGULAR_MOMENTUM" in gpu.last_error() and (out == pc.PROFILE_FILL).all()
        _profile(gpu, sims, "mass beside an infinite velocity", p, v, m, pc.CENTER, pc.BULK, edges, pr.MASS | pr.NUMBER)
        _radii(gpu, sims, "radii beside an infinite velocity", p, m, pc.CENTER, pc.FRACTIONS)
    for value, word in ((-1.0, "negative"), (np.inf, "not finite"), (np.nan, "not finite")):
        mm = m.copy()
        mm[5] = value
        with pc.Handles(p, 0.0 * p, mm, kind="direct") as sims:
            for sim in sims:
                got = pc.raw_radii(gpu, sim, pc.CENTER, pc.FRACTIONS)
                err = gpu.last_error()
                assert got[0] == NBMI_ERR_ARG and err.startswith("nbmi_mass_radii: ") and word in err, (value, got[0], err)
                assert pc.radii_untouched(got)


def test_owner_mode_and_sharded_handles_refuse(gpu):
    from nbody.gpu_backend import HIPOwnerSimulation
    from nbody.sharded import let_capacities
    p, v, m = pc.cloud(256)
    called = []

    class NoLibrary:
        def __getattr__(self, name):
            called.append(name)
            raise AssertionError(name)
    owner = HIPOwnerSimulation.__new__(HIPOwnerSimulation)  # refused before the library is called
    owner._lib, owner._h = NoLibrary(), None
    with pytest.raises(ValueError, match="owner-mode"):
        owner.radial_profile([1.0, 2.0])
    with pytest.raises(ValueError, match="owner-mode"):
        owner.mass_radii([0.5])
    assert not called
    cap, let = let_capacities(256, 1)
    real = HIPOwnerSimulation(p, v, m, np.arange(256), cap, let, 1, 0, 1.0, 0.1, 1.0)
    try:
        rc, out, st, ex = pc.raw_profile(gpu, real, pc.CENTER, None, [1.0, 2.0], 3)
        assert rc == NBMI_ERR_ARG and "nbmi_radial_profile: owner-mode" in gpu.last_error() and (out == pc.PROFILE_FILL).all()
        got = pc.raw_radii(gpu, real, pc.CENTER, [0.5])
        assert got[0] == NBMI_ERR_ARG and "nbmi_mass_radii: owner-mode" in gpu.last_error() and pc.radii_untouched(got)
    finally:
        real.close()
    sim = pc.handle("bh", p, v, m)
    try:
        sim.set_shard(0, 128)
        with pytest.raises(ValueError, match="sharded"):
            sim.radial_profile([1.0, 2.0])
        with pytest.raises(ValueError, match="sharded"):
            sim.mass_radii([0.5])
        sim.set_shard(0, 256)
        assert sim.radial_profile([1.0, 20.0])["mass"].sum() > 0 and sim.mass_radii([0.5])["radius2"][0] > 0
    finally:
        sim.close()


# ---- the recorder ----
def test_recorder_writes_the_profile_lines_of_its_frames(gpu, tmp_path):
    """2 000 bodies, --profile 2, 6 frames: three lines, each equal to what a second handle that replays the steps
    returns for the state after that frame"""
    import json

    from nbody import profile as prof
    from nbody.gpu_backend import create_gpu_simulation
    from tools import record as rec
    argv = ["--preset", "quick_galaxy", "--bodies", "2000", "--frames", "6", "--profile", "2", "--profile-fractions", "0.5,0.1,0.9",
            "--root", str(tmp_path), "m"]
    config = rec.build_config(rec.build_parser().parse_args(argv))
    rec_dir = rec.record(dict(config), root=tmp_path, quiet=True, seed=5)
    lines = [json.loads(x) for x in (rec_dir / "profile.jsonl").read_text().splitlines()]
    assert [x["frame"] for x in lines] == [1, 3, 5]
    edges = config["profile"]["edges"]
    assert len(edges) == 49 and np.allclose(edges, prof.auto_edges(config["spawn_radius"]))
    np.random.seed(5)
    p, v, m = rec._generate_initial_conditions(config)
    sim = create_gpu_simulation(p, v, m, config["G"], config["softening"], config["damping"], theta=config.get("theta", 0.5),
                                force_gpu=True)
    try:
        dt = config["dt_per_frame"] / config["substeps"]
        for frame in range(6):
            sim.step_many(dt, config["substeps"])
            if frame % 2 == 1:
                line = lines[frame // 2]
                got = sim.radial_profile(edges, quantities=("number", "mass"))
                assert line["count"] == got["number"].astype(np.int64).tolist() and line["mass"] == got["mass"].tolist(), frame
                assert line["center"] == got["center"].tolist() and line["edges"] == list(edges)
                assert line["fractions"] == [0.5, 0.1, 0.9]
                assert line["lagrangian_radii"] == prof.lagrangian_radii(sim, [0.5, 0.1, 0.9]).tolist()
    finally:
        sim.close()
