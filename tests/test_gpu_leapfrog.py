"""The opt-in kick-drift-kick leapfrog integrator (include/nbmi.h nbmi_set_integrator) on the GPU:
order of convergence, agreement with a float64 KDK over the direct and the Barnes-Hut forces, every integrating walk
kernel, time reversibility, energy, the default left untouched, state rules, refusals and the recorder."""

import numpy as np
import pytest

import leapfrog_ref as lf

pytestmark = pytest.mark.gpu

T_KEPLER = 2.0 * np.pi


def _direct(x, v, m, G, eps, integrator="leapfrog", damping=1.0):
    from nbody.gpu_backend import HIPDirectSimulation
    return HIPDirectSimulation(x, v, m, G, eps, damping, integrator=integrator)


def _bh(x, v, m, G, eps, theta=0.5, integrator="leapfrog", damping=1.0):
    from nbody.gpu_backend import HIPBarnesHutSimulation
    return HIPBarnesHutSimulation(x, v, m, G, eps, damping, theta, integrator=integrator)


def _oracle_force(oracle, theta, G, eps):
    """F(x, m) of the oracle's float64 Barnes-Hut (uncapped, strict), and the node count of its last build."""
    last = {}

    def force(x, m):
        x = np.ascontiguousarray(x, dtype=np.float64)
        nd = oracle.NodeArrays.for_bodies(len(x))
        nn = oracle.build_octree(x, np.ascontiguousarray(m, dtype=np.float64), oracle.compute_bounds(x), nd,
                                 cap=oracle.UNCAPPED)
        last["num_nodes"] = nn
        return oracle.compute_forces_barnes_hut(x, np.ascontiguousarray(m, dtype=np.float64), nd, nn, theta, G, eps)
    return force, last


# ---- 1. order of convergence -------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["direct", "barnes_hut_f64"])
def test_kepler_order_of_convergence(gpu, method):
    """Circular Kepler pair (softening 0: the guarded kernels), a quarter period at T/200 and T/400: the errors of a
    second-order scheme shrink 4x, kick-drift's 2x (float64 NumPy: 4.00 and 2.00 / 1.98)."""
    x0, v0, m = lf.kepler_pair()
    xe, ve = lf.kepler_exact(T_KEPLER / 4)
    ratios = {}
    for integ in ("leapfrog", "kick_drift"):
        errs = []
        for steps in (50, 100):
            if method == "direct":
                s = _direct(x0, v0, m, 1.0, 0.0, integ)
            else:
                s = _bh(x0, v0, m, 1.0, 0.0, integrator=integ)
                s.set_force_precision("f64")
            s.step_many(T_KEPLER / 4 / steps, steps)
            errs.append((np.abs(s.get_positions_f64() - xe).max(), np.abs(s.get_velocities() - ve).max()))
            s.close()
        ratios[integ] = (errs[0][0] / errs[1][0], errs[0][1] / errs[1][1])
    print(method, "error ratios T/200 -> T/400 (x, v):", ratios)
    for r in ratios["leapfrog"]:
        assert 3.5 <= r <= 4.5
    for r in ratios["kick_drift"]:
        assert r < 2.5


# ---- 2. direct N^2 against a float64 KDK -----------------------------------------------------------------------
@pytest.mark.parametrize("equal_masses", [False, True], ids=["unequal-masses", "uniform-gm"])
def test_direct_against_float64_kdk(gpu, equal_masses):
    n, G, eps, dt = 4096, 1.0, 0.05, 0.01
    x, v, m = lf.plummer(n, 5)
    if equal_masses:
        m = np.full(n, 1.0 / n)
    force = lf.direct_force(G, eps)
    s = _direct(x, v, m, G, eps)
    assert s.integrator == "leapfrog"
    a0 = force(x, m)
    x1, v1, a1 = lf.leapfrog(x, v, m, force, dt, 1, a=a0)
    s.step(dt)
    gx, gv = s.get_positions_f64(), s.get_velocities()
    # test_direct_matches_oracle_mid_size: |a_gpu - a| <= 5e-5 |a| per body; one step moves x by a0 dt^2/2 and v by
    # (a0 + a1) dt/2
    na0, na1 = np.linalg.norm(a0, axis=1), np.linalg.norm(a1, axis=1)
    bx = 5e-5 * na0 * dt * dt / 2 + 1e-14
    bv = 5e-5 * (na0 + na1) * dt / 2 + 1e-14
    ex, ev = np.abs(gx - x1).max(axis=1), np.abs(gv - v1).max(axis=1)
    print(f"1 step: max x err / bound {np.max(ex / bx):.3f}, v {np.max(ev / bv):.3f}")
    assert np.all(ex <= bx) and np.all(ev <= bv)
    s.step_many(dt, 19)
    x20, v20, _ = lf.leapfrog(x1, v1, m, force, dt, 19, a=a1)
    scale = np.abs(x20).max()
    err = np.abs(s.get_positions_f64() - x20).max() / scale
    errv = np.abs(s.get_velocities() - v20).max() / np.abs(v20).max()
    print(f"20 steps: rel x err {err:.2e}, rel v err {errv:.2e}")
    assert err <= 1e-6 and errv <= 1e-5
    s.close()


# ---- 3. Barnes-Hut against the oracle ------------------------------------------------------------------------
def test_barnes_hut_against_oracle_kdk(gpu, oracle):
    """float64 KDK over the oracle's forces (cap=UNCAPPED, fast=False), the 200 k galaxy of test_force_precision_modes,
    20 steps: the same bounds as that test, the same octree."""
    from tools.presets import generate_distribution
    n, G, eps, theta, dt = 200_000, 0.07, 1.5, 0.5, 0.05
    np.random.seed(7)
    p, v, m = generate_distribution("galaxy", n, 800.0, G)
    m = m * np.random.uniform(0.5, 1.5, n)
    force, last = _oracle_force(oracle, theta, G, eps)
    xr, vr, _ = lf.leapfrog(p, v, m, force, dt, 20)
    scale, vscale = np.abs(xr).max(), np.abs(vr).max()
    err, errv = {}, {}
    for mode in ("f64", "auto", "f32"):
        s = _bh(p, v, m, G, eps, theta)
        s.set_force_precision(mode)
        s.step_many(dt, 20)
        err[mode] = np.abs(s.get_positions_f64() - xr).max() / scale
        errv[mode] = np.abs(s.get_velocities() - vr).max() / vscale
        assert s.tree_stats()["num_nodes"] == last["num_nodes"]
        s.close()
    print("leapfrog 200 k x 20 steps, rel position error:", err, "velocity:", errv)
    assert err["f64"] <= 1e-12 and errv["f64"] <= 1e-10
    assert err["auto"] <= 1e-7 and errv["auto"] <= 1e-5
    assert err["f32"] <= 1e-6 and errv["f32"] <= 1e-4


# ---- 4. every integrating walk kernel ---------------------------------------------------------------------------
WALK_CASES = [(30_000, "split K=16", {}), (60_000, "split K=8", {}), (120_000, "split K=4", {}),
              (250_000, "split K=2", {}), (320_000, "one wave, two cursors", {}),
              (120_000, "one wave, one cursor", {"NBMI_WALK_PAIR": "0", "NBMI_SPLIT_WAVES": "0"}),
              (320_000, "balance mode", {"NBMI_XCD_BALANCE": "2"})]


@pytest.mark.parametrize("n,kernel,env", WALK_CASES, ids=[c[1] for c in WALK_CASES])
def test_every_walk_kernel_one_leapfrog_step(gpu, oracle, monkeypatch, n, kernel, env):
    from tools.presets import generate_distribution
    np.random.seed(n)
    p, v, m = generate_distribution("galaxy", n, 500.0, 0.15)
    m = m * np.random.uniform(0.5, 1.5, n)
    G, eps, theta, dt = 0.15, 2.0, 0.6, 0.05
    force, last = _oracle_force(oracle, theta, G, eps)
    a0 = force(p, m)
    xr, vr, _ = lf.leapfrog(p, v, m, force, dt, 1, a=a0)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    s = _bh(p, v, m, G, eps, theta)
    for k in env:
        monkeypatch.delenv(k)
    s.step(dt)
    acc_scale = np.linalg.norm(a0, axis=1).max()
    ex = np.abs(s.get_positions_f64() - xr).max() / (acc_scale * dt * dt)
    ev = np.abs(s.get_velocities() - vr).max() / (acc_scale * dt)
    print(f"{kernel} (n={n}): acc-equivalent err x {ex:.2e}, v {ev:.2e}")
    assert ex <= 1e-4 and ev <= 1e-4
    assert s.tree_stats()["num_nodes"] == last["num_nodes"]
    s.close()


# ---- 5. time reversibility -----------------------------------------------------------------------------------
@pytest.mark.parametrize("system", ["kepler", "plummer512"])
def test_time_reversibility(gpu, system):
    """100 steps, v -> -v through set_state, 100 steps: leapfrog returns to (x0, -v0) (float64 NumPy: 8e-17), the
    reference's kick-drift misses by more than 1e-4 (NumPy: 0.06 on the pair, 8e-4 on the sphere)."""
    if system == "kepler":
        x0, v0, m = lf.kepler_pair()
        G, eps, dt = 1.0, 0.0, T_KEPLER / 200
    else:
        x0, v0, m = lf.plummer(512, 3)
        G, eps, dt = 1.0, 0.05, 0.01
    miss = {}
    for integ in ("leapfrog", "kick_drift"):
        s = _direct(x0, v0, m, G, eps, integ)
        s.step_many(dt, 100)
        s.set_state(s.get_positions_f64(), -s.get_velocities())
        s.step_many(dt, 100)
        x, v = s.get_positions_f64(), s.get_velocities()
        miss[integ] = (np.abs(x - x0).max() / np.abs(x0).max(), np.abs(-v - v0).max() / np.abs(v0).max())
        s.close()
    print(system, "reversal miss (x, v):", miss)
    assert miss["leapfrog"][0] <= 1e-9 and miss["leapfrog"][1] <= 1e-9
    assert miss["kick_drift"][0] > 1e-4


# ---- 6. energy ----------------------------------------------------------------------------------------------
def _max_energy_drift(s, dt, steps, every=1):
    e0 = s.diagnostics().total
    worst = 0.0
    for _ in range(steps // every):
        s.step_many(dt, every)
        worst = max(worst, abs(s.diagnostics().total / e0 - 1.0))
    return worst


def test_energy_error_is_second_order(gpu):
    x, v, m = lf.plummer(512, 3)
    drift = {}
    for integ in ("leapfrog", "kick_drift"):
        drift[integ] = []
        for dt in (0.01, 0.005):
            s = _direct(x, v, m, 1.0, 0.05, integ)
            drift[integ].append(_max_energy_drift(s, dt, int(round(1.0 / dt))))
            s.close()
    print("Plummer 512, t = 1: max |dE/E0| at dt 0.01, 0.005:", drift)
    assert drift["leapfrog"][0] / drift["leapfrog"][1] >= 3.0
    assert drift["kick_drift"][0] / drift["kick_drift"][1] < 2.5
    x, v, m = lf.kepler_pair()
    s = _direct(x, v, m, 1.0, 0.0)
    worst = _max_energy_drift(s, T_KEPLER / 200, 2000, every=10)
    s.close()
    print(f"Kepler pair, 10 periods at T/200: max |dE/E0| {worst:.2e}")
    assert worst < 1e-4


# ---- 7. the default is untouched ------------------------------------------------------------------------------
def test_kick_drift_choice_is_the_untouched_default(gpu):
    from tools.presets import generate_distribution
    np.random.seed(3)
    p, v, m = generate_distribution("galaxy", 200_000, 500.0, 0.15)
    for make in (lambda integ: _bh(p, v, m, 0.15, 3.0, integrator=integ),
                 lambda integ: _direct(p[:20_000], v[:20_000], m[:20_000], 0.15, 3.0, integ)):
        a, b = make("kick_drift"), make("kick_drift")
        b.set_integrator("kick_drift")
        assert a.integrator == b.integrator == "kick_drift"
        a.step_many(0.1, 20)
        b.step_many(0.1, 20)
        assert np.array_equal(a.get_positions_f64().view(np.uint64), b.get_positions_f64().view(np.uint64))
        assert np.array_equal(a.get_velocities().view(np.uint64), b.get_velocities().view(np.uint64))
        a.close(); b.close()


def test_switch_back_to_kick_drift_continues_from_the_state(gpu):
    x, v, m = lf.plummer(2048, 9)
    s = _direct(x, v, m, 1.0, 0.05)
    s.step_many(0.01, 5)
    s.set_integrator("kick_drift")
    fresh = _direct(s.get_positions_f64(), s.get_velocities(), m, 1.0, 0.05, "kick_drift")
    s.step_many(0.01, 5)
    fresh.step_many(0.01, 5)
    assert np.array_equal(s.get_positions_f64(), fresh.get_positions_f64())
    assert np.array_equal(s.get_velocities(), fresh.get_velocities())
    s.close(); fresh.close()


# ---- 8. state rules ----------------------------------------------------------------------------------------
def test_capacity_error_leaves_the_pre_step_state(gpu):
    """G = 0 colliding pairs of test_capacity_error_in_the_middle_of_step_many_is_sticky: in leapfrog the drift comes
    before the build, so the first substep's octree overflows and the state stays the initial one."""
    n_pairs, dt, sep = 1500, 0.1, 1.0
    rng = np.random.RandomState(7)
    base = rng.uniform(-50, 50, (n_pairs, 3))
    pos = np.concatenate([base, base + [sep, 0.0, 0.0]])
    vv = (sep - 1e-9) / (2 * dt)
    vel = np.concatenate([np.tile([vv, 0.0, 0.0], (n_pairs, 1)), np.tile([-vv, 0.0, 0.0], (n_pairs, 1))])
    s = _bh(pos, vel, np.ones(2 * n_pairs), 0.0, 0.1)
    s.step_many(dt, 3)
    with pytest.raises(RuntimeError, match="octree needs"):
        s.sync()
    assert np.array_equal(s.get_positions_f64(), pos)
    assert np.array_equal(s.get_velocities(), vel)
    s.set_state(pos, -vel)  # moving apart: the handle steps again
    s.step(dt)
    s.sync()
    assert np.array_equal(s.get_positions_f64(), pos + (-vel) * dt)
    assert np.array_equal(s.get_velocities(), -vel)
    s.close()


def test_diagnostics_and_accelerations_do_not_interfere(gpu):
    from nbody.gpu_backend import HIPBarnesHutSimulation
    res, all64_seen = [], []
    for every in (0, 5):
        s = HIPBarnesHutSimulation.generated("galaxy", 1_000_000, 500.0, 0.15, 3.0, 1.0, 0.5, seed=7,
                                             integrator="leapfrog")
        flags = []
        for k in range(60):
            s.step(0.02 if k < 30 else 0.25)  # the all-float64 switch is off at the short step and turns on at the long
            flags.append(s.force_precision_share())
            if every and (k + 1) % every == 0:
                s.diagnostics()
                s.accelerations()
        res.append((s.get_positions_f64(), s.get_velocities(), flags))
        all64_seen.append(any(f[1] for f in flags))
        s.close()
    a, b = res
    print("all-float64 switch inside the window:", all64_seen[0], [f for f in a[2][::10]])
    assert not a[2][0][1] and a[2][-1][1]
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
    assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    assert a[2] == b[2]


def test_tiny_systems(gpu):
    for make in (_bh, _direct):
        s = make(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), 1.0, 0.1)
        s.step_many(0.1, 3)
        s.sync()
        assert s.integrator == "leapfrog" and s.get_positions_f64().shape == (0, 3)
        s.close()
        x, v = np.array([[1.0, -2.0, 3.0]]), np.array([[0.25, 0.5, -1.0]])
        s = make(x, v, np.ones(1), 1.0, 0.1)
        s.step_many(0.1, 4)
        for _ in range(4):
            x = x + v * 0.1
        assert np.array_equal(s.get_positions_f64(), x) and np.array_equal(s.get_velocities(), v)
        s.close()


# ---- 9. refusals -----------------------------------------------------------------------------------------
def test_owner_and_sharded_handles_refuse_leapfrog(gpu):
    from nbody.gpu_backend import HIPBarnesHutSimulation, HIPOwnerSimulation
    from nbody.sharded import let_capacities
    import nbmi_native
    x, v, m = lf.plummer(4096, 1)
    cap, let_cap = let_capacities(len(x), 1)
    o = HIPOwnerSimulation(x, v, m, np.arange(len(x), dtype=np.int32), cap, let_cap, 1, 0, 1.0, 0.05, 1.0)
    with pytest.raises(ValueError, match="owner"):
        o.set_integrator("leapfrog")
    assert o._lib.nbmi_set_integrator(o._h, 1) == -1 and "owner-mode" in nbmi_native.last_error()
    assert o.integrator == "kick_drift"
    o.close()
    s = _bh(x, v, m, 1.0, 0.05, integrator="kick_drift")
    s.set_shard(0, 2048)
    with pytest.raises(ValueError, match="sharded"):
        s.set_integrator("leapfrog")
    s.set_shard(0, len(x))
    s.set_integrator("leapfrog")
    with pytest.raises(ValueError, match="cannot be sharded"):
        s.set_shard(0, 2048)
    s.step(0.01)  # still usable, unsharded, in leapfrog
    s.sync()
    assert s.integrator == "leapfrog"
    s.close()


# ---- 10. recorder --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["direct", "barnes_hut"])
def test_recorder_leapfrog_session_resumes_and_extends(gpu, tmp_path, monkeypatch, method):
    from tools import record as rec
    from tools.presets import get_preset_config
    monkeypatch.setenv("NBMI_METHOD", method)
    cfg = get_preset_config("quick_galaxy")
    cfg.update(num_bodies=3000, theta=0.5, substeps=2, integrator="leapfrog", diagnostics_every=10)
    u = rec.record(dict(cfg, total_frames=70, session_name="uninterrupted"), root=tmp_path, quiet=True, seed=42)
    d = rec.record(dict(cfg, total_frames=60, session_name="interrupted"), root=tmp_path, quiet=True, seed=42)
    assert (d / "state_0049.npz").exists()
    for k in range(50, 60):
        (d / f"frame_{k:04d}.npz").unlink()
    rec.record(dict(cfg, total_frames=60, session_name="interrupted"), resume=True, root=tmp_path, quiet=True)
    rec.extend_recording("interrupted", 10, root=tmp_path)
    assert rec.get_completed_frames(d) == 70
    scale = np.abs(rec.load_frame(u, 69)[0]).max()
    for k in range(50, 70):
        p, _ = rec.load_frame(d, k)
        q, _ = rec.load_frame(u, k)
        if method == "direct":
            assert np.array_equal(p, q), k
        else:
            assert np.abs(p - q).max() / scale < 1e-4, k
    meta = rec.load_metadata(d)
    assert meta["integrator"] == "leapfrog" and meta["total_frames"] == 70
    rows = rec.read_diagnostics(d / rec.DIAGNOSTICS_FILE)
    assert [r["frame"] for r in rows] == [-1] + list(range(9, 70, 10))
    assert all(r["integrator"] == "leapfrog" for r in rows)
    # a default session writes no such key
    plain = rec.record(dict(cfg, integrator="kick_drift", total_frames=2, diagnostics_every=1, session_name="plain"),
                       root=tmp_path, quiet=True, seed=42)
    cfg_default = {k: val for k, val in cfg.items() if k != "integrator"}
    plain2 = rec.record(dict(cfg_default, total_frames=2, diagnostics_every=1, session_name="plain2"),
                        root=tmp_path, quiet=True, seed=42)
    assert "integrator" not in rec.load_metadata(plain2)
    assert all("integrator" not in r for r in rec.read_diagnostics(plain2 / rec.DIAGNOSTICS_FILE))
    assert all("integrator" not in r for r in rec.read_diagnostics(plain / rec.DIAGNOSTICS_FILE))
    np.testing.assert_array_equal(rec.load_frame(plain, 1)[0], rec.load_frame(plain2, 1)[0])
