"""The seeded vectorial noise of include/bdmi.h ("Noise"; csrc/bdmi.hip noise_xi and the FlockPN instances) against its
NumPy restatement (tests/noise_ref.py), bit for bit: the parity hook, noisy steps of walled and periodic handles, the step
counter, and the Flock class.
"""
import ctypes as C

import numpy as np
import pytest

import boids_cases as BC
import boids_ref as R
import noise_ref as N
import periodic_cases as PC
import periodic_ref as PR
import topo_ref as T
from test_gpu_boids import RawFlock
from test_gpu_boids_periodic import PeriodicFlock, _refused
from test_gpu_boids_topological import TOPOLOGICAL, same_state, set_mode

pytestmark = pytest.mark.gpu

SEEDS = (42, (1 << 32) + 42)
STEPS = (0, 1, (1 << 32) + 5)


def set_noise(f, eta, seed, step=-1):
    return f.lib.bdmi_set_noise(f.h, eta, seed, step)


def get_noise(f):
    eta, seed, step = C.c_double(-5), C.c_uint64(5), C.c_int64(-5)
    assert f.lib.bdmi_get_noise(f.h, C.addressof(eta), C.addressof(seed), C.addressof(step)) == 0, f.nat.last_error()
    return float(eta.value), int(seed.value), int(step.value)


def noise_vectors(f, step=-1):
    out = np.full((f.n, 3), -7.0)
    f.nat.check(f.lib.bdmi_noise_vectors(f.h, step, f.nat.ptr(out)), "bdmi_noise_vectors")
    return out


def _state(n, seed, bounds):
    rng = np.random.default_rng(seed)
    return (R.lattice(rng.uniform(-bounds, bounds, (n, 3)), BC.PB), R.lattice(rng.uniform(-12.5, 12.5, (n, 3)), BC.VB),
            R.id_colours(n))


@pytest.mark.parametrize("n", [1, 257, 4096])
def test_noise_vectors_match_restatement(gpu, n):
    prm = BC.params(bounds=12.0)
    pos, vel, col = _state(n, n, 12.0)
    f = RawFlock(gpu, pos, vel, col, prm)
    late = 0
    try:
        for seed in SEEDS:
            assert set_noise(f, 0.0, seed, 0) == 0  # the hook works with eta == 0
            for step in STEPS:
                want, attempt, _ = N.vectors(seed, step, np.arange(n))
                late += int((attempt >= 2).sum())
                assert R.same_bits(noise_vectors(f, step), want), (seed, step)
            assert set_noise(f, 0.0, seed, STEPS[2]) == 0
            assert R.same_bits(noise_vectors(f, -1), N.vectors(seed, STEPS[2], np.arange(n))[0])  # -1: the handle's step
    finally:
        f.close()
    if n == 4096:
        assert late >= 6, late  # boids accepted at the third block or later are in the population


def _topo_forces(pos, vel, col, prm, k, periodic):
    F = PR.flocking(pos, vel, col, prm, k) if periodic else T.flocking(pos, vel, col, prm, k)
    return F.sep, F.ali, F.coh, F.avg


def _ref_step(pos, vel, col, prm, k, dt, periodic, kick):
    forces = _topo_forces(pos, vel, col, prm, k, periodic)
    if periodic:
        return PR.physics(pos, vel, col, forces, prm, dt, kick)
    return N.physics_walled(pos, vel, col, forces, prm, dt, kick)


@pytest.mark.parametrize("periodic", [False, True], ids=["walled", "periodic"])
def test_noisy_steps_match_restatement(gpu, periodic):
    """One noisy topological step, then bdmi_step(dt, 3) = three restatement steps with the noise steps s, s + 1, s + 2."""
    n, k, eta, seed, s0 = 1500, 7, 0.75, SEEDS[1], (1 << 32) - 2  # the step counter crosses 2^32 on the way
    prm = BC.params(bounds=12.5)  # walls within reach of many boids; as a box: dim 5
    pos, vel, col = _state(n, 21, 12.5)
    f = (PeriodicFlock if periodic else RawFlock)(gpu, pos, vel, col, prm)
    try:
        assert set_mode(f, TOPOLOGICAL, k) == 0
        assert get_noise(f) == (0.0, 0, 0)
        assert set_noise(f, eta, seed, s0) == 0 and get_noise(f) == (eta, seed, s0)
        forces = f.forces()  # the four arrays do not contain the noise
        assert same_state(forces, _topo_forces(pos, vel, col, prm, k, periodic))
        assert get_noise(f)[2] == s0
        f.step(BC.DT)
        want = _ref_step(pos, vel, col, prm, k, BC.DT, periodic, N.kick(prm, eta, seed, s0, n))
        quiet = _ref_step(pos, vel, col, prm, k, BC.DT, periodic, None)
        assert same_state(f.state(), want) and not R.same_bits(want[1], quiet[1])
        assert get_noise(f) == (eta, seed, s0 + 1)
        between = noise_vectors(f, 7)  # the hook between steps changes nothing
        assert R.same_bits(between, N.vectors(seed, 7, np.arange(n))[0])
        f.step(BC.DT, 3)
        for s in range(s0 + 1, s0 + 4):
            want = _ref_step(*want, prm, k, BC.DT, periodic, N.kick(prm, eta, seed, s, n))
        assert same_state(f.state(), want)
        assert get_noise(f) == (eta, seed, s0 + 4)
        if periodic:
            assert np.all(np.abs(f.state()[0]) <= 12.5)
    finally:
        f.close()


def test_step_counter(gpu):
    prm = BC.params(bounds=12.0)
    pos, vel, col = _state(300, 5, 12.0)
    f = RawFlock(gpu, pos, vel, col, prm)
    try:
        f.step(BC.DT, 2)  # advances with eta == 0, on a handle that never heard of noise
        assert get_noise(f) == (0.0, 0, 2)
        assert set_noise(f, 0.5, 9, -1) == 0 and get_noise(f) == (0.5, 9, 2)  # step == -1 keeps the step
        f.step(BC.DT)
        f.lib.bdmi_set_state(f.h, gpu.ptr(pos), None, None)  # does not touch it
        assert get_noise(f) == (0.5, 9, 3)
        assert set_noise(f, 0.0, 9, 100) == 0 and get_noise(f) == (0.0, 9, 100)
        f.step(BC.DT, 0)
        assert get_noise(f)[2] == 100
        # each output may be null
        step = C.c_int64(0)
        assert f.lib.bdmi_get_noise(f.h, None, None, C.addressof(step)) == 0 and step.value == 100
        assert f.lib.bdmi_get_noise(f.h, None, None, None) == 0
    finally:
        f.close()
    e = RawFlock(gpu, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), prm)
    try:
        e.step(BC.DT, 3)
        assert get_noise(e)[2] == 3
        assert e.lib.bdmi_noise_vectors(e.h, 0, None) == 0
    finally:
        e.close()


def test_either_caller_order_matches_its_restatement(gpu):
    """Whatever the caller's order, two noisy steps are the restatement's on that order, bit for bit: nothing of the cell
    order or the block order enters.  (xi belongs to the caller id, so the same rows in another order draw other vectors:
    the permuted run is the restatement of the permuted input, not the permutation of the first run.)"""
    n, k, eta, seed = 1000, 7, 0.5, 42
    prm = BC.params(bounds=12.5)
    rng = np.random.default_rng(31)  # off the lattice: no d2 ties for the ids to break
    pos, vel, col = rng.uniform(-12.5, 12.5, (n, 3)), rng.uniform(-12.5, 12.5, (n, 3)), rng.random((n, 3))
    assert T.distinct_d2(PR.neighbours(pos, prm, k + 1)).all()
    perm = np.random.default_rng(3).permutation(n)
    out = []
    for order in (np.arange(n), perm):
        f = PeriodicFlock(gpu, pos[order], vel[order], col[order], prm, k)
        try:
            assert set_noise(f, eta, seed, 0) == 0
            f.step(BC.DT, 2)
            out.append(f.state())
        finally:
            f.close()
        want = pos[order], vel[order], col[order]
        for s in range(2):
            want = PR.step(*want, prm, k, BC.DT, N.kick(prm, eta, seed, s, n))
        assert same_state(out[-1], want)
    # without noise the permuted run is the permutation of the first; with it, it is not (row i draws xi_i either way)
    assert not R.same_bits(out[1][1], out[0][1][perm])


def test_eta_zero_is_the_step_without_noise(gpu):
    """After bdmi_set_noise(f, 0, seed, -1) a walled metric handle gives the state bits of a handle that never heard of
    noise; so does a handle whose noise was switched on and off again before the steps."""
    prm = BC.params(bounds=12.0)
    pos, vel, col = _state(1500, 3, 12.0)

    def run(before=None, hooks=False):
        f = RawFlock(gpu, pos, vel, col, prm)
        try:
            if before:
                before(f)
            for _ in range(3):
                f.step(BC.DT)
                if hooks:
                    noise_vectors(f, -1)
                    noise_vectors(f, 12345)
            return f.state()
        finally:
            f.close()

    fresh = run()
    assert same_state(run(lambda f: set_noise(f, 0.0, 77, -1)), fresh)
    assert same_state(run(lambda f: (set_noise(f, 2.0, 77, 5), set_noise(f, 0.0, 77, -1))), fresh)
    assert same_state(run(hooks=True), fresh)
    noisy = run(lambda f: set_noise(f, 0.25, 77, -1))
    assert not same_state(noisy, fresh)
    assert same_state(run(lambda f: set_noise(f, 0.25, 77, -1), hooks=True), noisy)  # the hook between noisy steps
    # a noisy METRIC step: everything but the separation sum's order is fixed, so the state is close to the restatement's
    F = R.flocking(pos, vel, col, prm)
    want = N.physics_walled(pos, vel, col, (F.sep, F.ali, F.coh, F.avg), prm, BC.DT, N.kick(prm, 0.25, 77, 0, len(pos)))
    f = RawFlock(gpu, pos, vel, col, prm)
    try:
        assert set_noise(f, 0.25, 77, -1) == 0
        sep = f.forces()[0]
        f.step(BC.DT)
        got = f.state()
    finally:
        f.close()
    R.check_sep(sep, F, vel, prm, "noisy metric")
    exact = N.physics_walled(pos, vel, col, (sep, F.ali, F.coh, F.avg), prm, BC.DT, N.kick(prm, 0.25, 77, 0, len(pos)))
    assert same_state(got, exact)  # bit for bit on the device's own separation sum
    assert np.abs(got[0] - want[0]).max() < 1e-9


def test_refusals(gpu):
    lib = gpu.load()
    prm = BC.params(bounds=30.0)
    n = 64
    pos, vel, col = _state(n, 6, 20.0)
    f = RawFlock(gpu, pos, vel, col, prm)
    ids = np.arange(n, dtype=np.int32)
    slab = lib.bdmi_create_slab(n, gpu.ptr(pos), gpu.ptr(vel), gpu.ptr(col), gpu.ptr(ids), 2 * n, gpu.ptr(prm), -35.0, 35.0,
                                0, 0, 0)
    assert slab, gpu.last_error()
    try:
        assert set_noise(f, 0.5, 9, 4) == 0
        for eta in (-1.0, -0.0 - 1e-300, float("nan"), float("inf"), float("-inf")):
            assert "eta" in _refused(gpu, set_noise(f, eta, 1, 0), "bdmi_set_noise")
        for step in (-2, -(1 << 40)):
            assert "step" in _refused(gpu, set_noise(f, 0.1, 1, step), "bdmi_set_noise")
        assert get_noise(f) == (0.5, 9, 4)  # settings untouched
        out = np.full((n, 3), -7.0)
        assert "step" in _refused(gpu, lib.bdmi_noise_vectors(f.h, -2, gpu.ptr(out)), "bdmi_noise_vectors")
        # null handles
        _refused(gpu, lib.bdmi_set_noise(None, 0.1, 1, 0), "bdmi_set_noise")
        _refused(gpu, lib.bdmi_get_noise(None, None, None, None), "bdmi_get_noise")
        _refused(gpu, lib.bdmi_noise_vectors(None, 0, gpu.ptr(out)), "bdmi_noise_vectors")
        # slab handles
        eta = C.c_double(-7)
        assert "slab" in _refused(gpu, lib.bdmi_set_noise(slab, 0.1, 1, 0), "bdmi_set_noise")
        assert "slab" in _refused(gpu, lib.bdmi_get_noise(slab, C.addressof(eta), None, None), "bdmi_get_noise")
        assert "slab" in _refused(gpu, lib.bdmi_noise_vectors(slab, 0, gpu.ptr(out)), "bdmi_noise_vectors")
        assert eta.value == -7 and (out == -7).all()
        gpu.check(lib.bdmi_step(slab, BC.DT, 1), "bdmi_step")  # the slab handle still steps
        gpu.check(lib.bdmi_sync(slab), "bdmi_sync")
    finally:
        f.close()
        lib.bdmi_destroy(slab)


def test_flock_class(gpu, monkeypatch):
    """boids.Flock: periodic=True, set_noise, .noise, noise_vectors, .box, one noisy periodic update, the ValueErrors."""
    import config.boids as bcfg
    from boids import Flock
    monkeypatch.delenv("BDMI_NEIGHBOURS", raising=False)
    saved = dict(bcfg.BOIDS)
    bcfg.BOIDS["bounds"] = 15.0
    try:
        fl = Flock(2048, seed=7, periodic=True)
        walled = Flock(64, seed=7)
        prm = np.array([float(bcfg.BOIDS[key]) for key in bcfg.PARAM_ORDER], dtype=np.float64)
        bcfg.BOIDS["bounds"] = 7.0
        with pytest.raises(ValueError, match="bdmi_create_periodic: .*dimension"):
            Flock(16, seed=1, periodic=True)
    finally:
        bcfg.BOIDS.clear()
        bcfg.BOIDS.update(saved)
    try:
        assert fl.periodic and not walled.periodic
        assert fl.box == dict(periodic=True, length=30.0, cell_size=5.0) and walled.box["periodic"] is False
        assert (fl.grid_dim, fl.cell_size, fl.num_cells, fl.grid_offset) == (6, 5.0, 216, 15.0)
        assert fl.noise == (0.0, 0, 0)
        fl.set_noise(0.5, seed=(1 << 40) + 3)
        assert fl.noise == (0.5, (1 << 40) + 3, 0)
        fl.set_neighbour_mode("topological", k=7)
        pos, vel, col = fl.positions.copy(), fl.velocities.copy(), fl.colors.copy()
        assert R.same_bits(fl.noise_vectors(), N.vectors((1 << 40) + 3, 0, np.arange(2048))[0])
        assert R.same_bits(fl.noise_vectors(step=9), N.vectors((1 << 40) + 3, 9, np.arange(2048))[0])
        fl.update(BC.DT)
        want = PR.step(pos, vel, col, prm, 7, BC.DT, N.kick(prm, 0.5, (1 << 40) + 3, 0, 2048))
        assert same_state((fl.positions, fl.velocities, fl.colors), want)
        assert fl.noise == (0.5, (1 << 40) + 3, 1)
        fl.set_noise(0.25, seed=5, step=40)
        assert fl.noise == (0.25, 5, 40)
        fl.set_noise(0.0)  # step=None keeps the step
        assert fl.noise == (0.0, 0, 40)
        with pytest.raises(ValueError, match="bdmi_set_noise: .*eta = -1"):
            fl.set_noise(-1.0)
        with pytest.raises(ValueError, match="bdmi_noise_vectors: .*step = -3"):
            fl.noise_vectors(step=-3)
        with pytest.raises(ValueError, match="bdmi_step: .*box length"):
            fl.update(2.0)
        with pytest.raises(ValueError, match="bdmi_flocks: .*periodic"):
            fl.flocks()
        bad = fl.positions.copy()
        bad[3, 0] = 15.5
        with pytest.raises(ValueError, match="bdmi_set_state: .*row 3"):
            fl.set_state(positions=bad)
        assert fl.diagnostics()[0] == 2048
    finally:
        fl.close()
        walled.close()
