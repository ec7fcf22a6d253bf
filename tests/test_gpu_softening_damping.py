"""Softening 0, tiny softening and damping < 1 on the GPU, and every direct-N^2 kernel variant.

The other parity tests run at softening > 0 and damping 1.  Softening 0 (and a softening so small that the fp32
self-term G m eps^-3 overflows) selects the guarded kernels, k_walk<*, *, true> and k_direct<*, true, *, *>, which skip
the pairs with dist_sq <= eps^2 as the reference does (its own leaf, coincident bodies); damping enters the fused
kick-drift of every integrating kernel.  References: the strict-IEEE oracle (fast=False: -ffast-math would fold the
eps = 0 guards) and tests/direct_ref.py.

Stated tolerances
  * direct accelerations, per sampled body: 5e-5 |a_ref| (the bound of test_direct_matches_oracle_mid_size) plus the
    fp32 coordinate term of test_edge_cases summed over the body's pairs, 4 ulp32(max |x|) sum_j G m_j / max(d, eps)^3.
  * "f64" Barnes-Hut: 1e-12 of the largest coordinate after 10 steps (test_force_precision_modes); "auto" and "f32":
    1e-6 (that test's fp32 bound).
Inputs at softening 0 keep distinct bodies at least 0.5 apart (distinct sites of a unit lattice, jittered by at most
0.25 per coordinate) at coordinates below 1024, where the fp32 spacing is at most 6.1e-5: distinct in fp32 as well.
"""
import os

import numpy as np
import pytest

from direct_ref import direct_accelerations, pair_weights

pytestmark = pytest.mark.gpu

G_DIRECT, DT_DIRECT, DAMP_DIRECT = 0.05, 0.01, 0.99
MIN_SEP = 0.5


def _separated(p, rng, h=1.0):
    """Indices of bodies on distinct lattice sites of spacing h, and their positions jittered inside their site:
    any two are >= h / 2 apart."""
    sites = np.round(p / h)
    _, idx = np.unique(sites, axis=0, return_index=True)
    idx = np.sort(idx)
    return idx, (sites[idx] + rng.uniform(-0.25, 0.25, (len(idx), 3))) * h


def _direct_inputs(n, equal, seed, coincident=True):
    rng = np.random.RandomState(seed)
    idx, pos = _separated(rng.normal(0, 100, (n + n // 50 + 16, 3)), rng)
    assert len(idx) >= n
    pos = np.ascontiguousarray(pos[rng.permutation(len(pos))[:n]])
    dup = []
    if coincident and n >= 255:
        # exactly equal pairs in float64 (the rule skips them at every softening); one straddles the first tile edge
        dup = [(0, n - 1), (1, n // 2), (255 if n > 258 else n // 3, n - 2)]
        for a, b in dup:
            pos[b] = pos[a]
    assert np.abs(pos).max() < 1024.0
    m = np.full(n, 1.5) if equal else rng.uniform(0.5, 2.0, n)
    vel = rng.normal(0, 1, (n, 3))
    return pos, vel, m, dup


def _rows(n, dup, rng):
    if n <= 257:
        return np.arange(n)
    fixed = np.unique(np.concatenate([[0, 1, 255, 256, n // 2, n - 2, n - 1], np.ravel(dup)]))
    rest = np.setdiff1d(rng.choice(n, 128, replace=False), fixed)
    return np.concatenate([fixed, rest]).astype(np.int64)


def _direct_bound(pos, m, rows, eps, ref):
    coord = 4 * float(np.spacing(np.float32(np.abs(pos).max()))) * pair_weights(pos, m, rows, G_DIRECT, eps)
    return 5e-5 * np.linalg.norm(ref, axis=1) + coord


@pytest.mark.parametrize("eps", [1.0, 0.0, 1e-14], ids=["eps1", "eps0", "eps1e-14"])
@pytest.mark.parametrize("equal", [True, False], ids=["equal-masses", "unequal-masses"])
@pytest.mark.parametrize("n", [1, 2, 255, 257, 131_071, 131_073, 524_287, 524_289])
def test_direct_every_variant(gpu, oracle, n, equal, eps):
    """Bodies per thread 1 / 2 / 4 (switching at 131 072 and 524 288 integrated bodies), equal masses (G m outside the
    pair loop) or not, guarded (eps 0, 1e-14) or not; the force pass and one damped integrating step of each."""
    from nbody.gpu_backend import HIPDirectSimulation
    pos, vel, m, dup = _direct_inputs(n, equal, seed=n + 7 * equal)
    rows = _rows(n, dup, np.random.RandomState(n))
    sim = HIPDirectSimulation(pos, vel, m, G_DIRECT, eps, DAMP_DIRECT)
    acc = sim.accelerations()
    assert np.isfinite(acc).all()
    ref = direct_accelerations(pos, m, rows, G_DIRECT, eps)
    bound = _direct_bound(pos, m, rows, eps, ref)
    err = np.linalg.norm(acc[rows] - ref, axis=1)
    print(f"direct n={n} equal={equal} eps={eps}: worst err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all(), (rows[np.argmax(err - bound)], err.max())
    for a, b in dup:  # a coincident pair feels the same pull from everybody else
        assert np.array_equal(acc[a], acc[b])
    sim.step(DT_DIRECT)
    x1, v1 = sim.get_positions_f64(), sim.get_velocities()
    assert np.isfinite(x1).all() and np.isfinite(v1).all()
    xr, vr = np.ascontiguousarray(pos[rows]), np.ascontiguousarray(vel[rows])
    oracle.direct_update(xr, vr, np.ascontiguousarray(ref), DT_DIRECT, DAMP_DIRECT)
    tol_v = bound[:, None] * DT_DIRECT + 4 * np.spacing(np.abs(vr))
    tol_x = tol_v * DT_DIRECT + 4 * np.spacing(np.abs(xr))
    assert (np.abs(v1[rows] - vr) <= tol_v).all()
    assert (np.abs(x1[rows] - xr) <= tol_x).all()
    sim.close()


@pytest.mark.parametrize("eps", [1.0, 0.0], ids=["eps1", "eps0"])
@pytest.mark.parametrize("equal", [True, False], ids=["equal-masses", "unequal-masses"])
def test_direct_shards_pick_every_block_size_and_match_bit_for_bit(gpu, eps, equal):
    """700 000 bodies cut at indices that are not multiples of 256: the shards integrate 150 017 (two bodies per thread),
    539 984 (four) and 9 999 (one) bodies.  A body's sums run over the same tiles in the same order whatever the block
    size, so every integrated row equals the unsharded handle's bit for bit."""
    from nbody.gpu_backend import HIPDirectSimulation
    n = 700_000
    pos, vel, m, _ = _direct_inputs(n, equal, seed=70 + equal)
    full = HIPDirectSimulation(pos, vel, m, G_DIRECT, eps, DAMP_DIRECT)
    full.step(DT_DIRECT)
    xf, vf = full.get_positions_f64(), full.get_velocities()
    full.close()
    assert np.isfinite(xf).all()
    import torch
    differ = {}
    for b, e in ((0, 150_017), (150_017, 690_001), (690_001, n)):
        s = HIPDirectSimulation(pos, vel, m, G_DIRECT, eps, DAMP_DIRECT)
        s.set_shard(b, e)
        s.step(DT_DIRECT)
        # the shard's own rows {x, y, z, vx, vy, vz, m, id} as the exchange sends them (the rows outside the shard are
        # only defined once nbmi_import_ranks has supplied them, so the whole-state getters are not the measure here)
        rows = torch.empty((e - b, 8), dtype=torch.float64, device="cuda:0")
        s.export_shard(rows.data_ptr())
        r = rows.cpu().numpy()
        assert np.array_equal(r[:, 7], np.arange(b, e)) and np.array_equal(r[:, 6], m[b:e])
        bad = np.any(r[:, 0:3] != xf[b:e], axis=1) | np.any(r[:, 3:6] != vf[b:e], axis=1)
        differ[(b, e)] = int(bad.sum())
        s.close()
    print("rows that differ from the unsharded handle:", differ)
    assert all(c == 0 for c in differ.values()), differ


def _bh(pos, vel, mass, G, eps, theta, damping=1.0, mode=None):
    from nbody.gpu_backend import HIPBarnesHutSimulation
    sim = HIPBarnesHutSimulation(pos, vel, mass, G, eps, damping, theta)
    if mode is not None:
        sim.set_force_precision(mode)
    return sim


def _separated_galaxy(n, seed, R=800.0, G=0.07):
    from tools.presets import generate_distribution
    np.random.seed(seed)
    p, v, m = generate_distribution("galaxy", n + n // 20 + 64, R, G)
    idx, pos = _separated(p, np.random.RandomState(seed))
    assert len(idx) >= n
    pos = np.ascontiguousarray(pos[:n])
    assert np.abs(pos).max() < 1024.0
    return pos, np.ascontiguousarray(v[idx[:n]]), np.ascontiguousarray(m[idx[:n]])


@pytest.mark.parametrize("eps", [0.0, 1e-14], ids=["eps0", "eps1e-14"])
@pytest.mark.parametrize("n", [20_000, 320_000], ids=["split-walk-size", "one-wave-size"])
def test_barnes_hut_unsoftened_every_precision(gpu, oracle, n, eps):
    """Galaxy without close pairs at softening 0 and 1e-14: the counted walk's forces and accepted pairs, then 10 steps
    in each force precision against the oracle stepping at the same softening.  (dt 0.01: unsoftened bodies that meet
    during the run turn fp32 roundings into large differences; at dt 0.05 the 320 k galaxy's "f32" run ends 1.5e-6
    from the oracle, while "f64" stays at 3e-14.)"""
    G, theta, dt, steps = 0.07, 0.5, 0.01, 10
    p, v, m = _separated_galaxy(n, seed=n // 1000)
    b = oracle.compute_bounds(p)
    nd = oracle.NodeArrays(4 * n + 4096)
    nn = oracle.build_octree(p, m, b, nd, cap=oracle.UNCAPPED)
    ref, st = oracle.compute_forces_barnes_hut(p, m, nd, nn, theta, G, eps, stats=True)
    sim = _bh(p, v, m, G, eps, theta)
    acc = sim.accelerations()
    wc = sim.walk_counters()
    assert np.isfinite(acc).all()
    bound = 2e-4 * np.abs(ref).max() + 4 * np.spacing(np.float32(np.abs(p).max())) * G * m.max() / MIN_SEP ** 3
    print(f"n={n} eps={eps}: acc err {np.abs(acc - ref).max():.2e} (bound {bound:.2e}), accepts {wc['lane_accepts']} "
          f"vs {st['accepted']}")
    assert np.abs(acc - ref).max() <= bound
    assert wc["lane_accepts"] == st["accepted"]
    sim.close()
    o = oracle.BHStepper(p, v, m, theta, G, eps, 1.0, cap=oracle.UNCAPPED, rows=4 * n + 4096, fast=False)
    for _ in range(steps):
        o.step(dt)
    scale = np.abs(o.pos).max()
    err = {}
    for mode in ("f64", "auto", "f32"):
        s = _bh(p, v, m, G, eps, theta, mode=mode)
        s.step_many(dt, steps)
        x = s.get_positions_f64()
        assert np.isfinite(x).all() and np.isfinite(s.get_velocities()).all(), mode
        err[mode] = np.abs(x - o.pos).max() / scale
        assert s.tree_stats()["num_nodes"] == o.num_nodes
        s.close()
    print(f"   {steps} steps, max rel position error:", err)
    assert err["f64"] <= 1e-12
    assert err["auto"] <= 1e-6 and err["f32"] <= 1e-6


@pytest.mark.parametrize("eps", [0.0, 1e-14], ids=["eps0", "eps1e-14"])
@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_barnes_hut_coincident_bodies(gpu, oracle, mode, eps):
    """Exactly coincident bodies (which make the reference's own tree subdivide to its cap) at theta = 0, where every
    leaf is accepted and no cell is: the walk is the all-pairs sum, so direct_ref is its reference.  The coincident
    pairs are skipped (dist_sq = eps^2), everything stays finite, and one damped step follows the reference."""
    n, G, dt, damping = 3000, 0.05, 0.01, 0.99
    pos, vel, m, _ = _direct_inputs(n, False, seed=31, coincident=False)
    pos = pos * 0.5  # (coordinates ~50: shallower trees; separation still >= 0.25)
    dup = [(k, n - 1 - k) for k in range(0, 40, 4)]
    for a, b in dup:
        pos[b] = pos[a]
    rows = np.arange(n)
    ref = direct_accelerations(pos, m, rows, G, eps)
    sim = _bh(pos, vel, m, G, eps, 0.0, damping=damping, mode=mode)
    acc = sim.accelerations()
    wc = sim.walk_counters()
    assert np.isfinite(acc).all()
    assert wc["lane_accepts"] == n * (n - 1) - 2 * len(dup)
    coord = 4 * float(np.spacing(np.float32(np.abs(pos).max()))) * pair_weights(pos, m, rows, G, eps)
    bound = 5e-5 * np.linalg.norm(ref, axis=1) + coord
    assert (np.linalg.norm(acc - ref, axis=1) <= bound).all()
    sim.step(dt)
    x1, v1 = sim.get_positions_f64(), sim.get_velocities()
    assert np.isfinite(x1).all() and np.isfinite(v1).all()
    xr, vr = np.ascontiguousarray(pos.copy()), np.ascontiguousarray(vel.copy())
    oracle.direct_update(xr, vr, np.ascontiguousarray(ref), dt, damping)
    err = np.abs(x1 - xr).max() / np.abs(xr).max()
    print(f"coincident {mode} eps={eps}: one step, max rel position error {err:.2e}")
    if mode == "f64":
        assert err <= 1e-12
    else:
        tol_v = bound[:, None] * dt + 4 * np.spacing(np.abs(vr))
        assert (np.abs(v1 - vr) <= tol_v).all()
        assert (np.abs(x1 - xr) <= tol_v * dt + 4 * np.spacing(np.abs(xr))).all()
    sim.close()


@pytest.mark.parametrize("n,split,damping", [(30_000, True, 0.99), (320_000, True, 0.995), (30_000, False, 0.995)],
                         ids=["split-walk", "one-wave", "split-walk-off"])
def test_barnes_hut_damped_steps(gpu, oracle, n, split, damping):
    """Damping < 1 (ten of the reference's presets use 0.99 ... 0.999) through the fused kick-drift of the split walk, the
    one-wave walk and the one-wave walk at a split-walk size; 10 steps against the oracle."""
    from tools.presets import generate_distribution
    G, eps, theta, dt, steps = 0.07, 1.5, 0.5, 0.05, 10
    np.random.seed(n + int(split))
    p, v, m = generate_distribution("galaxy", n, 800.0, G)
    m = m * np.random.uniform(0.5, 1.5, n)
    o = oracle.BHStepper(p, v, m, theta, G, eps, damping, cap=oracle.UNCAPPED, fast=False)
    for _ in range(steps):
        o.step(dt)
    scale = np.abs(o.pos).max()
    err = {}
    for mode in ("f64", None):
        if not split:
            os.environ["NBMI_SPLIT_WAVES"] = "0"
        try:
            s = _bh(p, v, m, G, eps, theta, damping=damping, mode=mode)
        finally:
            os.environ.pop("NBMI_SPLIT_WAVES", None)
        s.step_many(dt, steps)
        err[mode or "default"] = np.abs(s.get_positions_f64() - o.pos).max() / scale
        vel_err = np.abs(s.get_velocities() - o.vel).max() / np.abs(o.vel).max()
        err[(mode or "default") + " vel"] = vel_err
        s.close()
    print(f"damping {damping}, n={n}, split={split}: {err}")
    assert err["f64"] <= 1e-12 and err["f64 vel"] <= 1e-10
    assert err["default"] <= 1e-6
