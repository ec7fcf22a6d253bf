"""The boids sweep kernel (csrc/bdmi.hip `k_flock`) at its edges, against the grid-free reference
(tests/boids_ref.py) and the CPU oracle.

For every constructed case (tests/boids_cases.py: lattice positions and velocities, integer colours
that encode the id), `bdmi_get_forces` (k_flock<false>) must give the reference's ali, coh and avg
bit for bit, since those sums are exact in any order, and a sep within boids_ref.sep_bound (summation
order is the only difference).  One `bdmi_step` (k_flock<true>) must then give exactly physics()
of the kernel's own forces.
"""
import numpy as np
import pytest

import boids_cases as BC
import boids_ref as R
from test_gpu_boids import RawFlock

pytestmark = pytest.mark.gpu


def _check_case(nat, c):
    pos, vel, col, prm, dt = c["pos"], c["vel"], c["col"], c["params"], c["dt"]
    f = RawFlock(nat, pos, vel, col, prm)
    try:
        assert np.array_equal(f.cells(), R.cell_index(pos, prm)), c["name"]
        sep, ali, coh, avg = f.forces()
        F = R.flocking(pos, vel, col, prm)
        for got, want, what in ((ali, F.ali, "ali"), (coh, F.coh, "coh"), (avg, F.avg, "avg")):
            bad = np.flatnonzero(np.any(got != want, axis=1))
            assert R.same_bits(got, want), (c["name"], what, len(bad), bad[:5], F.nb[bad[:5]])
        dmax, bmax = R.check_sep(sep, F, vel, prm, c["name"])
        f.step(dt)
        p, v, cl = f.state()
        ep, ev, ec = R.physics(pos, vel, col, (sep, ali, coh, avg), prm, dt)
        assert R.same_bits(p, ep) and R.same_bits(v, ev) and R.same_bits(cl, ec), c["name"]
        print(f"{c['name']}: n={len(pos)} max neighbours {F.nb.max()} sep diff {dmax:.2e} (bound up to {bmax:.2e})")
    finally:
        f.close()


_NAMES = ([f"run_length_{c}" for c in (4094, 4095, 4096, 4097)] + ["mixed_lanes", "hit_list", "thresholds"]
          + [f"grid_{d}" for d in (3, 4, 31, 32, 33, 34, 63, 64, 65)]
          + ["perception_2.5", "perception_7.25", "separation_above_perception", "max_force_clamps", "zero_weights",
             "blend_saturates"])


def _build(name):
    if name.startswith("run_length_"):
        return BC.run_length(int(name.rsplit("_", 1)[1]))
    if name.startswith("grid_"):
        return BC.grid_dims(int(name.split("_")[1]))
    if name in ("mixed_lanes", "hit_list", "thresholds"):
        return getattr(BC, name)()
    return next(x for x in BC.parameter_cases() if x["name"] == name)


@pytest.mark.parametrize("name", _NAMES)
def test_sweep_matches_reference(gpu, name):
    _check_case(gpu, _build(name))


def test_largest_grid(gpu):
    """Dimension 1290: cell ids up to 1290^3 - 1 = 2^31 - 794 809; forces against the reference only
    (the oracle's dense tables would need 17 GB)."""
    c = BC.largest_grid()
    assert R.cell_index(c["pos"], c["params"]).max() == 1290 ** 3 - 1
    _check_case(gpu, c)


def test_grid_1291_refused(gpu):
    lib = gpu.load()
    prm = BC.params(bounds=644.5, perception_radius=1.0)
    p = np.zeros((4, 3))
    h = lib.bdmi_create(4, gpu.ptr(p), gpu.ptr(p), gpu.ptr(p), gpu.ptr(prm), 0)
    if h:
        lib.bdmi_destroy(h)
    assert not h
    assert "grid dimension 1291 out of range" in gpu.last_error()


def _mean_candidates(pos, prm):
    return float(BC.grid_facts(pos, prm)["candidates"].mean())


def test_flocked_state(gpu, oracle):
    """Config 5 (2 M boids) after 1000 steps, on the lattice and recoloured: the kernel against the
    oracle (ali / coh / avg bit-exact, sep <= 1e-9), and against the reference's bound on ~20 k boids."""
    from boids import Flock
    prm = oracle.boids_params()
    dt = 1.0 / 60.0
    fl = Flock(2_000_000, seed=42)
    try:
        c0 = _mean_candidates(fl.positions, prm)
        fl.update(dt, substeps=1000)
        pos, vel = R.lattice(fl.positions, BC.PB), R.lattice(fl.velocities, BC.VB)
        col = R.id_colours(len(pos))
        c1 = _mean_candidates(pos, prm)
        print(f"mean candidates per boid: {c0:.1f} at t = 0, {c1:.1f} after 1000 steps")
        assert c1 >= 4 * c0  # the clustered regime (DESIGN: ~7 -> 53)
        fl.set_state(positions=pos, velocities=vel, colors=col)
        sep, ali, coh, avg = fl.forces()
        st = oracle.FlockStepper(pos, vel, col, prm, use_numpy_argsort=False)
        st.step(dt)
        assert R.same_bits(ali, st.ali) and R.same_bits(coh, st.coh) and R.same_bits(avg, st.avg)
        assert np.abs(sep - st.sep).max() <= 1e-9
        # ~20 k boids in a box around the median position; the box grown by the perception radius holds all
        # their neighbours
        cheb = np.abs(pos - np.median(pos, axis=0)).max(axis=1)
        h = np.partition(cheb, 20_000)[20_000]
        sub = np.flatnonzero(cheb < h + 5.0 * (1 + 1e-9))
        q = np.flatnonzero(cheb[sub] < h)
        F = R.flocking(pos[sub], vel[sub], col[sub], prm, query=q)
        qi = sub[q]
        assert R.same_bits(ali[qi], F.ali) and R.same_bits(coh[qi], F.coh) and R.same_bits(avg[qi], F.avg)
        dmax, bmax = R.check_sep(sep[qi], F, vel[qi], prm, "flocked")
        print(f"sample {len(qi)} boids, mean neighbours {F.nb.mean():.1f}, sep diff {dmax:.2e} (bound up to {bmax:.2e})")
        fl.update(dt)
        ep, ev, ec = R.physics(pos, vel, col, (sep, ali, coh, avg), prm, dt)
        assert R.same_bits(fl.positions, ep) and R.same_bits(fl.velocities, ev) and R.same_bits(fl.colors, ec)
        assert np.abs(fl.positions - st.pos).max() <= 1e-9 and np.abs(fl.velocities - st.vel).max() <= 1e-8
    finally:
        fl.close()


def _random_state(n, seed, bounds):
    rng = np.random.default_rng(seed)
    pos = R.lattice(rng.uniform(-bounds, bounds, (n, 3)), BC.PB)
    vel = R.lattice(rng.uniform(-12.5, 12.5, (n, 3)), BC.VB)
    return pos, vel, R.id_colours(n)


@pytest.mark.parametrize("n", [1, 255, 256, 257] + [256 * (16 + j) - 37 for j in range(1, 8)])
def test_block_order(gpu, oracle, monkeypatch, n):
    """BDMI_XCD=0 (hardware block order) against the default XCD-contiguous order: the same state after
    10 steps, bit for bit; block counts 1 .. 7 mod 8."""
    prm = oracle.boids_params(bounds=max(4.0, (n / 0.05) ** (1 / 3) / 2))
    pos, vel, col = _random_state(n, n, float(prm[0]))
    out = []
    for xcd in ("0", None):
        if xcd is None:
            monkeypatch.delenv("BDMI_XCD", raising=False)
        else:
            monkeypatch.setenv("BDMI_XCD", xcd)
        f = RawFlock(gpu, pos, vel, col, prm)
        f.step(1.0 / 60.0, 10)
        out.append(f.state())
        f.close()
    for a, b in zip(*out):
        assert R.same_bits(a, b)


@pytest.mark.parametrize("n", [65_536, 65_537, 524_288, 524_289])
def test_sort_tile_sizes(gpu, oracle, n):
    """The radix sort switches items per thread at n = 65 536 and 524 288 (radix.hip): one step
    on either side against the oracle."""
    prm = oracle.boids_params(bounds=(n / 0.002) ** (1 / 3) / 2)
    pos, vel, col = _random_state(n, n, float(prm[0]))
    f = RawFlock(gpu, pos, vel, col, prm)
    try:
        st = oracle.FlockStepper(pos, vel, col, prm, use_numpy_argsort=False)
        st.L.bdref_assign_cells(st.pos, st.cell_indices, st.cell, st.dim, st.offset, st.n)
        assert np.array_equal(f.cells(), st.cell_indices)
        sep, ali, coh, avg = f.forces()
        st.step(1.0 / 60.0)
        assert R.same_bits(ali, st.ali) and R.same_bits(coh, st.coh) and R.same_bits(avg, st.avg)
        assert np.abs(sep - st.sep).max() <= 1e-9
        f.step(1.0 / 60.0)
        p, v, c = f.state()
        assert np.abs(p - st.pos).max() <= 1e-9 and np.abs(v - st.vel).max() <= 1e-9
        assert np.abs(c - st.col).max() <= 1e-9 * np.abs(st.col).max()
    finally:
        f.close()
