"""nbmi_deposit on the GPU against the NumPy restatement of tests/deposit_ref.py (include/nbmi.h).

Every comparison is BIT FOR BIT - the planes, stats3 and the exponents: a contribution is a function of float64 products
that the kernel and NumPy form in the same association, its integer is one rint of an exact scaling, and the sums are
integers.  Every case runs on two handles of its own, created with NBMI_DEPOSIT_AGG 0 (one global atomic per
contribution) and 1 (combined per workgroup in LDS first), which must also agree with each other.
"""
import os

import numpy as np
import pytest

import deposit_ref as dr
import query_cases as qc

pytestmark = pytest.mark.gpu

NBMI_ERR_ARG = -1
SCHEMES = {dr.NGP: "ngp", dr.CIC: "cic"}
SINGLE = (dr.NUMBER, dr.MASS, dr.MOMENTUM, dr.KINETIC)
PLANES_OF = {dr.NUMBER: [0], dr.MASS: [1], dr.MOMENTUM: [2, 3, 4], dr.KINETIC: [5]}
GRIDS = {  # name -> (lo, hi, dims); the bodies of _cloud() reach beyond +-2 on every side
    "1x1x1": ((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), (1, 1, 1)),
    "5x3x2": ((-2.0, -1.5, -1.0), (2.0, 1.0, 3.0), (5, 3, 2)),
    "16x16x1 deep": ((-2.0, -2.0, -1e300), (2.0, 2.0, 1e300), (16, 16, 1)),
    "64x64x64": ((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), (64, 64, 64)),
}


def _handle(kind, p, v, m, agg, **kw):
    """a handle created with NBMI_DEPOSIT_AGG = agg (the knob is read at create)"""
    from nbody.gpu_backend import HIPBarnesHutSimulation, HIPDirectSimulation
    p, v, m = (np.ascontiguousarray(a, np.float64) for a in (p, v, m))
    old = os.environ.get("NBMI_DEPOSIT_AGG")
    os.environ["NBMI_DEPOSIT_AGG"] = str(agg)
    try:
        if kind == "direct":
            return HIPDirectSimulation(p, v, m, 0.07, 1.5, 1.0, **kw)
        return HIPBarnesHutSimulation(p, v, m, 0.07, 1.5, 1.0, 0.5, **kw)
    finally:
        if old is None:
            del os.environ["NBMI_DEPOSIT_AGG"]
        else:
            os.environ["NBMI_DEPOSIT_AGG"] = old


class _Both:
    """the two handles of a case, closed together"""
    def __init__(self, p, v, m, kind="bh", **kw):
        self.sims = []
        try:
            for agg in (0, 1):
                self.sims.append(_handle(kind, p, v, m, agg, **kw))
        except Exception:
            self.close()
            raise

    def __enter__(self):
        return self.sims

    def __exit__(self, *exc):
        self.close()

    def close(self):
        for s in self.sims:
            s.close()


def _raw(gpu, sim, lo, hi, dims, scheme, quantities, fill=0.0):
    """the C call itself: (rc, out (P, nz, ny, nx), stats3, exponents)"""
    planes = sum(len(PLANES_OF[q]) for q in SINGLE if quantities & q) if 0 < quantities < 16 else 1
    lo_, hi_ = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    d = np.array(dims, dtype=np.int32)
    shape = tuple(max(int(x), 1) for x in (planes, d[2], d[1], d[0]))
    out = np.full(shape if np.prod(shape, dtype=np.float64) < 1e7 else (16,), fill, dtype=np.float64)
    st, ex = np.full(3, -7, dtype=np.int64), np.full(planes, -7, dtype=np.int32)
    rc = gpu.load().nbmi_deposit(sim._h, gpu.ptr(lo_), gpu.ptr(hi_), gpu.ptr(d), int(scheme), int(quantities), gpu.ptr(out),
                                 gpu.ptr(st), gpu.ptr(ex))
    return rc, out, st, ex


def _same(tag, got, ref):
    out, st, ex = got
    assert out.dtype == np.float64 and out.shape == ref[0].shape, tag
    bad = int((out.view(np.int64) != ref[0].view(np.int64)).sum())
    print(f"{tag}: stats {st.tolist()} (reference {ref[1].tolist()}), exponents {ex.tolist()}, {bad} of {out.size} values differ")
    assert bad == 0 and np.array_equal(st, ref[1]) and np.array_equal(ex, ref[2]), tag


def _check(gpu, sims, tag, p, v, m, lo, hi, dims, scheme, quantities=dr.ALL, ref=None):
    """both handles against the restatement of the state (p, v, m); returns the reference"""
    if ref is None:
        ref = dr.deposit(p, v, m, lo, hi, dims, scheme, quantities)
    for agg, sim in enumerate(sims):
        rc, out, st, ex = _raw(gpu, sim, lo, hi, dims, scheme, quantities, fill=np.nan)
        assert rc == 0, (tag, gpu.last_error())
        _same(f"{tag} agg {agg}", (out, st, ex), ref)
    return ref


def _cloud(n, seed=1):
    rng = np.random.RandomState(seed)
    return rng.normal(size=(n, 3)) * 1.2, rng.normal(size=(n, 3)) * 3.0, rng.uniform(0.5, 2.0, n)


# ---- sizes around a wave and a workgroup, every grid, scheme and selection ----
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5000])
def test_sizes_grids_schemes_and_quantities(gpu, n):
    p, v, m = _cloud(n)
    with _Both(p, v, m) as sims:
        for name, (lo, hi, dims) in GRIDS.items():
            for scheme in (dr.NGP, dr.CIC):
                ref = _check(gpu, sims, f"n {n} {name} {SCHEMES[scheme]} all", p, v, m, lo, hi, dims, scheme)
                if n >= 63:
                    assert 0 < ref[1][0] < n or name == "16x16x1 deep", "the case lost its point: nobody outside"
                for q in SINGLE:  # a single quantity: the same planes, the same exponents
                    sel = PLANES_OF[q]
                    _check(gpu, sims, f"n {n} {name} {SCHEMES[scheme]} q {q}", p, v, m, lo, hi, dims, scheme, q,
                           ref=(ref[0][sel], ref[1], ref[2][sel]))
        if n:  # the Python call: names, shapes, the same bits
            lo, hi, dims = GRIDS["5x3x2"]
            ref = dr.deposit(p, v, m, lo, hi, dims, dr.CIC, dr.MASS | dr.MOMENTUM)
            got = sims[1].deposit(lo, hi, dims, scheme="cic", quantities=("momentum", "mass"), stats=True)
            assert sorted(got) == ["exponents", "mass", "momentum", "stats"]
            assert got["mass"].shape == (2, 3, 5) and got["momentum"].shape == (3, 2, 3, 5)
            assert np.array_equal(got["mass"], ref[0][0]) and np.array_equal(got["momentum"], ref[0][1:4])
            assert got["stats"] == tuple(ref[1].tolist()) and np.array_equal(got["exponents"], ref[2])


# ---- edge positions ----
def test_edge_positions(gpu):
    """bodies exactly on lo, on hi, on interior faces and on lo + h / 2 (the CIC fraction is 0), outside on every side,
    coordinates of 1e17 and coordinates that are not finite - on every axis, in every combination of a few values"""
    lo, hi, dims = (0.0, -4.0, 10.0), (4.0, 4.0, 12.0), (4, 8, 2)
    per_axis = []
    for a in range(3):
        h = (hi[a] - lo[a]) / dims[a]
        per_axis.append([lo[a], hi[a], lo[a] + h, lo[a] + 2 * h, lo[a] + 0.5 * h, hi[a] - 0.5 * h, lo[a] + 1.5 * h,
                         lo[a] - 0.25 * h, hi[a] + 0.25 * h, lo[a] - 3 * h, np.nextafter(lo[a], -np.inf),
                         np.nextafter(hi[a], -np.inf), 1e17, -1e17])
    p = np.stack(np.meshgrid(*per_axis, indexing="ij"), -1).reshape(-1, 3)
    extra = np.array([[np.nan, 0.0, 11.0], [1.0, np.inf, 11.0], [1.0, 0.0, -np.inf], [1e308, 0.0, 11.0], [-1e308, 0.0, 11.0]])
    p = np.concatenate([p, extra])
    rng = np.random.RandomState(2)
    v, m = rng.normal(size=p.shape), rng.uniform(0.5, 2.0, len(p))
    with _Both(p, v, m, kind="direct") as sims:  # (a direct handle: no tree has to hold these coordinates)
        for scheme in (dr.NGP, dr.CIC):
            ref = _check(gpu, sims, f"edges {SCHEMES[scheme]}", p, v, m, lo, hi, dims, scheme)
            assert ref[1][2] == 3 and 0 < ref[1][0] < len(p) - 3
        # the CIC fraction 0: a body on lo + h / 2 of every axis gives its cell everything and is 8 contributions
        one = np.array([[0.5, -3.5, 10.5]])
    with _Both(one, np.ones((1, 3)), np.array([3.0]), kind="direct") as sims:
        ref = _check(gpu, sims, "fraction 0", one, np.ones((1, 3)), np.array([3.0]), lo, hi, dims, dr.CIC)
        assert ref[1].tolist() == [1, 8, 0] and ref[0][1, 0, 0, 0] == 3.0 and ref[0][1].sum() == 3.0


# ---- contention ----
@pytest.mark.parametrize("cells", [1, 2])
def test_contention(gpu, cells):
    """4 096 bodies at one point, and 4 096 spread over two adjacent cells: every lane of every wave hits the same
    addresses"""
    rng = np.random.RandomState(3)
    p = np.tile([[0.3, 0.3, 0.3]], (4096, 1))
    if cells == 2:
        p[:, 0] += np.where(rng.randint(0, 2, 4096) == 1, 0.25, 0.0) + rng.uniform(0.0, 0.01, 4096)
    v, m = rng.normal(size=p.shape), rng.uniform(0.5, 2.0, len(p))
    lo, hi, dims = (0.0, 0.0, 0.0), (2.0, 2.0, 2.0), (8, 8, 8)
    with _Both(p, v, m) as sims:
        for scheme in (dr.NGP, dr.CIC):
            ref = _check(gpu, sims, f"contention {cells} {SCHEMES[scheme]}", p, v, m, lo, hi, dims, scheme)
            assert np.count_nonzero(ref[0][0]) == (cells if scheme == dr.NGP else 8 * (1 if cells == 1 else 1.5))


# ---- signed planes and scale ----
def test_signed_planes_cancel_exactly(gpu):
    rng = np.random.RandomState(4)
    half = rng.uniform(0.0, 4.0, (500, 3))
    vh, mh = rng.normal(size=(500, 3)) * 2.0, rng.uniform(0.5, 2.0, 500)
    p, v, m = np.concatenate([half, half]), np.concatenate([vh, -vh]), np.concatenate([mh, mh])
    lo, hi, dims = (0.0, 0.0, 0.0), (4.0, 4.0, 4.0), (4, 4, 4)
    with _Both(p, v, m) as sims:
        for scheme in (dr.NGP, dr.CIC):
            ref = _check(gpu, sims, f"cancel {SCHEMES[scheme]}", p, v, m, lo, hi, dims, scheme)
            assert (ref[0][2:5] == 0.0).all() and (ref[0][1] > 0).all() and (ref[0][5] > 0).all()
    # without the mirror bodies the momentum planes have both signs
    with _Both(half, vh, mh) as sims:
        ref = _check(gpu, sims, "signed", half, vh, mh, lo, hi, dims, dr.CIC)
        assert (ref[0][2:5] < 0).any() and (ref[0][2:5] > 0).any()


def test_scale_small_masses_vanish_and_zero_masses(gpu):
    rng = np.random.RandomState(5)
    p, v = rng.uniform(0.0, 4.0, (600, 3)), rng.normal(size=(600, 3))
    m = np.where(np.arange(600) % 2 == 0, 1.0, 1e-20)
    lo, hi, dims = (0.0, 0.0, 0.0), (4.0, 4.0, 4.0), (2, 2, 2)
    with _Both(p, v, m) as sims:
        ref = _check(gpu, sims, "masses 1 and 1e-20", p, v, m, lo, hi, dims, dr.NGP)
        assert ref[0][1].sum() == 300.0 and 1e-20 < 2.0 ** (int(ref[2][1]) - 1)  # the small ones vanish, as the header says
        assert ref[0][0].sum() == 600.0
    with _Both(p, v, 0.0 * m) as sims:
        for scheme in (dr.NGP, dr.CIC):
            ref = _check(gpu, sims, f"masses 0 {SCHEMES[scheme]}", p, v, 0.0 * m, lo, hi, dims, scheme)
            assert ref[2][1:].tolist() == [0] * 5 and (ref[0][1:] == 0.0).all() and ref[2][0] != 0


# ---- order independence on the device ----
def test_order_of_the_state_rows_and_handle_type(gpu):
    """a Barnes-Hut handle after 3 steps (state in key order), a direct handle given that state, a fresh Barnes-Hut
    handle given it in reversed body order: the same bits, and twice the same bits from one handle"""
    p, v, m = qc.preset("galaxy", 6000, seed=3)
    lo, hi, dims = (-400.0, -400.0, -100.0), (400.0, 400.0, 100.0), (32, 32, 8)
    with _Both(p, v, m) as stepped:
        for s in stepped:
            s.step_many(0.05, 3)
        x, w = stepped[0].get_positions_f64(), stepped[0].get_velocities()
        assert np.array_equal(x, stepped[1].get_positions_f64()) and not np.array_equal(x, p)
        with _Both(p, v, m, kind="direct") as direct, _Both(x[::-1], w[::-1], m[::-1]) as fresh:
            for s in direct:
                s.set_state(x, w)
            for scheme in (dr.NGP, dr.CIC):
                ref = _check(gpu, stepped, f"stepped {SCHEMES[scheme]}", x, w, m, lo, hi, dims, scheme)
                _check(gpu, direct, f"direct {SCHEMES[scheme]}", x, w, m, lo, hi, dims, scheme, ref=ref)
                _check(gpu, fresh, f"reversed {SCHEMES[scheme]}", x, w, m, lo, hi, dims, scheme, ref=ref)
                _check(gpu, stepped, f"stepped again {SCHEMES[scheme]}", x, w, m, lo, hi, dims, scheme, ref=ref)
                assert 0 < ref[1][0] < len(p)


# ---- no side effects ----
@pytest.mark.parametrize("integrator", ["kick_drift", "leapfrog"])
def test_a_deposit_between_steps_changes_nothing(gpu, integrator):
    """3 steps in precision "auto" with a deposit between every two against 3 steps without: positions, velocities and
    (leapfrog case: with tracers set) the tracers bit for bit"""
    p, v, m = qc.preset("galaxy", 6000, seed=4)
    tr = np.random.RandomState(6).normal(size=(100, 3)) * 200.0
    lo, hi, dims = (-400.0, -400.0, -400.0), (400.0, 400.0, 400.0), (16, 16, 16)
    with _Both(p, v, m, integrator=integrator) as sims, _Both(p, v, m, integrator=integrator) as plain:
        for s in sims + plain:
            if integrator == "leapfrog":
                s.set_tracers(tr)
        for step in range(3):
            for agg, s in enumerate(sims):
                for scheme in ("ngp", "cic"):
                    got = s.deposit(lo, hi, dims, scheme=scheme, quantities=("number", "mass", "momentum", "kinetic"))
                    assert got["number"].sum() > 0
                s.step(0.05)
            for s in plain:
                s.step(0.05)
        for s in sims:
            s.deposit(lo, hi, dims)
        want_x, want_v = plain[0].get_positions_f64(), plain[0].get_velocities()
        for s in sims + plain[1:]:
            assert np.array_equal(s.get_positions_f64(), want_x) and np.array_equal(s.get_velocities(), want_v)
            assert s.integrator == integrator
            if integrator == "leapfrog":
                a, b = s.get_tracers(), plain[0].get_tracers()
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[0], tr)
        assert sims[0].force_precision_share() == plain[0].force_precision_share()


# ---- NUMBER under NGP ----
def test_number_under_ngp_is_a_histogram(gpu):
    p, v, m = _cloud(5000, seed=8)
    lo, hi, dims = GRIDS["5x3x2"]
    u = [(p[:, a] - lo[a]) * (np.float64(dims[a]) / (np.float64(hi[a]) - np.float64(lo[a]))) for a in range(3)]
    want, _ = np.histogramdd(np.stack([np.floor(u[2]), np.floor(u[1]), np.floor(u[0])], 1),
                             bins=[np.arange(d + 1) - 0.5 for d in (dims[2], dims[1], dims[0])])
    with _Both(p, v, m) as sims:
        for agg, sim in enumerate(sims):
            got = sim.deposit(lo, hi, dims, scheme="ngp", quantities=("number",), stats=True)
            assert np.array_equal(got["number"], want) and got["number"].sum() == got["stats"][0], agg
            assert 0 < got["stats"][0] < 5000 and got["stats"][1] == got["stats"][0]


# ---- refusals ----
def test_refusals_before_any_launch_leave_the_output_untouched(gpu):
    p, v, m = _cloud(300)
    lo, hi, dims = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), (4, 4, 4)
    nan, inf = np.nan, np.inf
    bad = [  # (lo, hi, dims, scheme, quantities, part of the message)
        ((nan, -2, -2), hi, dims, 1, 2, "bounds"), (lo, (2, inf, 2), dims, 1, 2, "bounds"),
        (lo, (2, 2, -2.0), dims, 1, 2, "hi > lo"), (lo, (2, -3.0, 2), dims, 1, 2, "hi > lo"),
        ((-1e308, -2, -2), (1e308, 2, 2), dims, 1, 2, "not finite"), ((0.0, -2, -2), (5e-324, 2, 2), dims, 1, 2, "not finite"),
        (lo, hi, (4, 0, 4), 1, 2, "dims[1]"), (lo, hi, (4, 4, -1), 1, 2, "dims[2]"),
        (lo, hi, (1024, 1024, 257), 1, 2, "2^28"), (lo, hi, (1024, 1024, 64), 1, 15, "2^28"),
        (lo, hi, (2 ** 30, 2 ** 30, 2 ** 30), 0, 2, "2^28"),
        (lo, hi, dims, 2, 2, "scheme"), (lo, hi, dims, -1, 2, "scheme"),
        (lo, hi, dims, 1, 0, "quantities"), (lo, hi, dims, 1, 16, "quantities"), (lo, hi, dims, 1, 31, "quantities"),
    ]
    with _Both(p, v, m) as sims, _Both(p, v, m, kind="direct") as direct:
        for sim in sims + direct:
            for lo_, hi_, dims_, scheme, q, word in bad:
                rc, out, st, ex = _raw(gpu, sim, lo_, hi_, dims_, scheme, q, fill=-3.5)
                assert rc == NBMI_ERR_ARG and gpu.last_error().startswith("nbmi_deposit: ") and word in gpu.last_error(), \
                    (lo_, hi_, dims_, scheme, q, rc, gpu.last_error())
                assert (out == -3.5).all() and (st == -7).all() and (ex == -7).all()
            lib, out = gpu.load(), np.full(64, -3.5)
            lo_, hi_, d = np.array(lo), np.array(hi), np.array(dims, dtype=np.int32)
            for args, word in (((None, gpu.ptr(hi_), gpu.ptr(d), 1, 2, gpu.ptr(out)), "null lo"),
                               ((gpu.ptr(lo_), None, gpu.ptr(d), 1, 2, gpu.ptr(out)), "null hi"),
                               ((gpu.ptr(lo_), gpu.ptr(hi_), None, 1, 2, gpu.ptr(out)), "null dims"),
                               ((gpu.ptr(lo_), gpu.ptr(hi_), gpu.ptr(d), 1, 2, None), "null out")):
                assert lib.nbmi_deposit(sim._h, *args, None, None) == NBMI_ERR_ARG and word in gpu.last_error()
            assert (out == -3.5).all()
            assert lib.nbmi_deposit(sim._h, gpu.ptr(lo_), gpu.ptr(hi_), gpu.ptr(d), 1, 2, gpu.ptr(out), None, None) == 0  # NULL stats, exponents
            assert out.sum() > 0
            with pytest.raises(ValueError, match="deposit"):
                sim.deposit(lo, hi, dims, scheme="tsc")
            with pytest.raises(ValueError, match="deposit"):
                sim.deposit(lo, hi, dims, quantities=("charge",))
            with pytest.raises(ValueError, match="hi > lo"):
                sim.deposit(hi, lo, dims)


def test_an_infinite_velocity_is_refused_for_momentum_only(gpu):
    p, v, m = _cloud(300)
    v[17, 1] = np.inf
    lo, hi, dims = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), (4, 4, 4)
    with _Both(p, v, m, kind="direct") as sims:
        for sim in sims:
            rc, out, st, ex = _raw(gpu, sim, lo, hi, dims, dr.CIC, dr.MOMENTUM, fill=-3.5)
            assert rc == NBMI_ERR_ARG and "MOMENTUM y" in gpu.last_error() and "plane 1" in gpu.last_error()
            assert (out == -3.5).all()
            rc, out, st, ex = _raw(gpu, sim, lo, hi, dims, dr.CIC, dr.KINETIC, fill=-3.5)
            assert rc == NBMI_ERR_ARG and "KINETIC" in gpu.last_error() and (out == -3.5).all()
        _check(gpu, sims, "mass beside an infinite velocity", p, v, m, lo, hi, dims, dr.CIC, dr.MASS | dr.NUMBER)


def test_owner_mode_and_sharded_handles_refuse(gpu):
    from nbody.gpu_backend import HIPOwnerSimulation
    from nbody.sharded import let_capacities
    p, v, m = _cloud(256)
    lo, hi, dims = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), (4, 4, 4)
    called = []

    class NoLibrary:
        def __getattr__(self, name):
            called.append(name)
            raise AssertionError(name)
    owner = HIPOwnerSimulation.__new__(HIPOwnerSimulation)  # refused before the library is called
    owner._lib, owner._h = NoLibrary(), None
    with pytest.raises(ValueError, match="owner-mode"):
        owner.deposit(lo, hi, dims)
    assert not called
    cap, let = let_capacities(256, 1)
    real = HIPOwnerSimulation(p, v, m, np.arange(256), cap, let, 1, 0, 1.0, 0.1, 1.0)
    try:
        rc, out, st, ex = _raw(gpu, real, lo, hi, dims, dr.CIC, dr.MASS, fill=-3.5)
        assert rc == NBMI_ERR_ARG and "nbmi_deposit: owner-mode" in gpu.last_error() and (out == -3.5).all()
    finally:
        real.close()
    sim = _handle("bh", p, v, m, 0)
    try:
        sim.set_shard(0, 128)
        with pytest.raises(ValueError, match="sharded"):
            sim.deposit(lo, hi, dims)
        sim.set_shard(0, 256)
        assert sim.deposit(lo, hi, dims)["mass"].sum() > 0
    finally:
        sim.close()


# ---- one larger case ----
def test_galaxy_200k_on_64_cubed_all_planes(gpu):
    p, v, m = qc.preset("galaxy", 200_000, seed=11)
    lo, hi, dims = (-600.0, -600.0, -150.0), (600.0, 600.0, 150.0), (64, 64, 64)
    with _Both(p, v, m) as sims:
        ref = _check(gpu, sims, "galaxy 200k cic", p, v, m, lo, hi, dims, dr.CIC)
        assert 0.5 * len(p) < ref[1][0] < len(p)
        from nbody.grid import velocity_maps
        got = sims[1].deposit(lo, hi, dims, quantities=("mass", "momentum", "kinetic"))
        mean, sigma = velocity_maps(got)
        assert np.isnan(sigma[got["mass"] == 0.0]).all() and np.isfinite(sigma[got["mass"] > 0.0]).all()


# ---- the recorder ----
@pytest.mark.parametrize("pipeline", [False, True])
def test_recorder_writes_the_maps_of_its_frames(gpu, tmp_path, pipeline):
    """2 000 bodies, --density-map 2, 6 frames: three maps, each the surface density of the state after its frame - a
    second handle replays the steps - and the pipelined recorder writes the same files"""
    from nbody.gpu_backend import create_gpu_simulation
    from nbody.grid import surface_density
    from tools import record as rec
    argv = ["--preset", "quick_galaxy", "--bodies", "2000", "--frames", "6", "--density-map", "2", "--map-pixels", "64",
            "--root", str(tmp_path), "m"] + (["--pipeline"] if pipeline else [])
    config = rec.build_config(rec.build_parser().parse_args(argv))
    rec_dir = rec.record(dict(config), root=tmp_path, quiet=True, seed=5)
    names = sorted(q.name for q in rec_dir.glob("map_*.npy"))
    assert names == ["map_000001.npy", "map_000003.npy", "map_000005.npy"]
    meta = rec.load_metadata(rec_dir)
    assert rec.density_map_config(meta) == (2, 64, 1.5 * config["spawn_radius"], "z")
    np.random.seed(5)
    p, v, m = rec._generate_initial_conditions(config)
    sim = create_gpu_simulation(p, v, m, config["G"], config["softening"], config["damping"], theta=config.get("theta", 0.5),
                                force_gpu=True)
    try:
        dt = config["dt_per_frame"] / config["substeps"]
        for frame in range(6):
            sim.step_many(dt, config["substeps"])
            if frame % 2 == 1:
                want = surface_density(sim, half_width=1.5 * config["spawn_radius"], pixels=64).astype(np.float32)
                got = np.load(rec_dir / f"map_{frame:06d}.npy")
                assert got.dtype == np.float32 and got.shape == (64, 64) and want.sum() > 0
                assert np.array_equal(got, want), frame
    finally:
        sim.close()
