"""Device-side "spiral" and "filament" (cosmic web) initial conditions: statistical parity of nbmi_create_generated
with the NumPy generators of tools/presets.py (bit-identical to the reference's, tests/golden/ic_pins_more.npz), the
largest presets built on them, and recording them with device_ic from Python and from the command line."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
from scipy import stats

from conftest import PKG

pytestmark = pytest.mark.gpu

N = 200_000
SPIRAL = (600.0, 0.08, 2.0)      # R, G, softening of spiral_milkyway
WEB = (1200.0, 0.02, 5.0)        # R, G, softening of cosmic_web


def _host(dist, R, G, seed=42, n=N):
    from tools.presets import generate_distribution
    np.random.seed(seed)
    return generate_distribution(dist, n, R, G)


def _device(dist, R, G, eps, seed=42, n=N):
    from tools.presets import generate_distribution_device
    sim = generate_distribution_device(dist, n, R, G, eps, seed=seed)
    return sim, sim.get_positions_f64(), sim.get_velocities(), sim.get_masses()


def _ks(a, b):
    return stats.ks_2samp(a, b).statistic


def _binned_mean(r, v, edges):
    idx = np.digitize(r, edges)
    return np.array([v[idx == k].mean() for k in range(1, len(edges))])


def test_spiral_statistics_match_host_generator(gpu):
    R, G, eps = SPIRAL
    hp, hv, hm = _host("spiral", R, G)
    sim, dp, dv, dm = _device("spiral", R, G, eps)
    assert np.all(dm == 1.0) and np.isfinite(dp).all() and np.isfinite(dv).all()
    hr, dr = np.hypot(hp[:, 0], hp[:, 2]), np.hypot(dp[:, 0], dp[:, 2])
    assert _ks(hr, dr) < 0.01                                  # cylindrical radius
    assert _ks(hp[:, 1], dp[:, 1]) < 0.01                      # height

    def arm_phase(p, r):  # angle relative to the trailing log spiral, folded onto one of the 4 arms
        return np.mod(np.arctan2(p[:, 2], p[:, 0]) + np.log(r / (0.02 * R) + 1) / 0.35, np.pi / 2)
    ks_arm = _ks(arm_phase(hp, hr), arm_phase(dp, dr))
    assert ks_arm < 0.01

    def vtan(p, v):  # counter-clockwise in XZ
        r = np.hypot(p[:, 0], p[:, 2])
        return (p[:, 0] * v[:, 2] - p[:, 2] * v[:, 0]) / r

    def vrad(p, v):
        r = np.hypot(p[:, 0], p[:, 2])
        return (p[:, 0] * v[:, 0] + p[:, 2] * v[:, 2]) / r
    edges = np.quantile(hr, np.linspace(0.02, 0.98, 13))
    hc, dc = _binned_mean(hr, vtan(hp, hv), edges), _binned_mean(dr, vtan(dp, dv), edges)
    # the galaxy test's tolerance (tests/test_gpu_icgen.py)
    assert np.all(np.abs(dc - hc) < 0.01 * np.abs(hc).max() + 0.02 * np.abs(hc)) and hc.min() > 0
    vert = dv[:, 1].std() / hv[:, 1].std()
    plane = vrad(dp, dv).std() / vrad(hp, hv).std()
    assert abs(vert - 1) < 0.02 and abs(plane - 1) < 0.02
    assert np.abs(dv.mean(axis=0)).max() < 1e-10               # centre-of-mass velocity removed
    print(f"spiral 200k: KS radius {_ks(hr, dr):.4f} height {_ks(hp[:, 1], dp[:, 1]):.4f} arm phase {ks_arm:.4f}; "
          f"dispersion ratios vertical {vert:.4f} in-plane {plane:.4f}")


GRID = 8


def _grid(R):
    return np.linspace(-1.25 * R, 1.25 * R, GRID)


def _nearest_node(p, R):
    """(flat index of the nearest grid node, distance to it) per body."""
    g = _grid(R)
    idx = np.clip(np.rint((p + 1.25 * R) / (g[1] - g[0])), 0, GRID - 1).astype(int)
    return (idx[:, 0] * GRID + idx[:, 1]) * GRID + idx[:, 2], np.linalg.norm(p - g[idx], axis=1)


def _web_stats(p, R):
    """The ensemble statistics: quantiles of |x|, dense grid nodes, covariance eigenvalues."""
    s = 2.5 * R / GRID
    q = np.quantile(np.linalg.norm(p, axis=1), [0.1, 0.25, 0.5, 0.75, 0.9])
    node, d = _nearest_node(p, R)
    near = np.bincount(node[d < 0.3 * s], minlength=GRID ** 3)
    # nodes holding >= 0.05 % of the bodies within 0.3 s.  A threshold of 0.5 % finds no node in any host seed (the
    # densest node holds 0.2-0.3 % there), so it could not tell a wrong active fraction apart; 0.05 % counts the
    # active nodes (about 0.35 x 512 less the lightest) and moves with their probability and weights.
    dense = int((near >= 0.0005 * len(p)).sum())
    ev = np.linalg.eigvalsh(np.cov(p.T))
    return {"q10": q[0], "q25": q[1], "q50": q[2], "q75": q[3], "q90": q[4], "dense_nodes": dense,
            "ev0": ev[0], "ev1": ev[1], "ev2": ev[2]}


def test_filament_exact_properties_and_host_ensemble(gpu):
    R, G, eps = WEB
    s = 2.5 * R / GRID
    sim, dp, dv, dm = _device("filament", R, G, eps)
    assert np.all(dm == 0.1) and np.isfinite(dp).all() and np.isfinite(dv).all()
    # velocity = 0.05 x + N(0, 0.3) per component, exactly that law
    noise = dv - 0.05 * dp
    ks_v = [stats.kstest(noise[:, k], "norm", args=(0.0, 0.3)).statistic for k in range(3)]
    assert max(ks_v) < 0.01
    # each body lies in its node's cloud: 6 sigma along the axis (0.8 s) and across it (0.12 s, twice)
    _, d = _nearest_node(dp, R)
    assert d.max() <= 6 * 0.8 * s * np.sqrt(1.05)
    # The active nodes are themselves random, so one host seed is no reference for the device's node set: the
    # device's statistics must lie within the range 8 host seeds span, widened on each side by that range
    # (for a ninth draw of the same law, falling outside is a > 4-sigma event).
    ens = [_web_stats(_host("filament", R, G, seed=seed)[0], R) for seed in range(1, 9)]
    dev = _web_stats(dp, R)
    report = []
    for key, x in dev.items():
        vals = np.array([e[key] for e in ens], dtype=np.float64)
        lo, hi = vals.min(), vals.max()
        margin = hi - lo
        report.append(f"{key} {x:.4g} in [{lo:.4g}, {hi:.4g}] +- {margin:.3g}")
        assert lo - margin <= x <= hi + margin, report[-1]
    print("filament 200k: KS(v - 0.05x vs N(0,0.3)) " + " ".join(f"{k:.4f}" for k in ks_v)
          + f"; max node distance {d.max() / s:.2f} s; " + "; ".join(report))


@pytest.mark.parametrize("dist,params", [("spiral", SPIRAL), ("filament", WEB)])
def test_determinism_masses_ragged_sizes_and_stepping(gpu, dist, params):
    from nbody.gpu_backend import HIPBarnesHutSimulation
    R, G, eps = params
    mass = 0.1 if dist == "filament" else 1.0
    sim, p, v, m = _device(dist, R, G, eps, n=50_000)
    _, p2, v2, m2 = _device(dist, R, G, eps, n=50_000)
    assert np.array_equal(p, p2) and np.array_equal(v, v2) and np.array_equal(m, m2)
    _, p3, v3, _ = _device(dist, R, G, eps, n=50_000, seed=43)
    assert not np.array_equal(p, p3) and not np.array_equal(v, v3)
    assert m.shape == (50_000,) and np.all(m == mass)
    sim.step_many(0.05, 3)
    assert np.isfinite(sim.get_positions_f64()).all() and np.isfinite(sim.get_velocities()).all()
    assert np.all(sim.get_masses() == mass)
    sim.close()
    for n in (1, 255, 257, 100_003):
        h = HIPBarnesHutSimulation.generated(dist, n, R, G, eps, 1.0, seed=11)
        q, w = h.get_positions_f64(), h.get_velocities()
        assert q.shape == (n, 3) and np.isfinite(q).all() and np.isfinite(w).all()
        assert np.all(h.get_masses() == mass)
        if n > 1:
            assert len(np.unique(q[:, 0])) == n  # every body drew its own numbers
        h.step_many(0.05, 3)
        assert np.isfinite(h.get_positions_f64()).all()
        h.close()


@pytest.mark.parametrize("key", ["extreme_20m_spiral", "extreme_50m_web"])
def test_largest_presets_generate_and_step_on_one_gpu(gpu, key):
    from tools.presets import generate_distribution_device, get_preset_config
    c = get_preset_config(key)
    n = c["num_bodies"]
    t0 = time.perf_counter()
    sim = generate_distribution_device(c["distribution"], n, c["spawn_radius"], c["G"], c["softening"],
                                       theta=c["theta"], seed=42)
    sim.sync()
    t_gen = time.perf_counter() - t0
    sim.step_many(c["dt_per_frame"] / c["substeps"], 1)
    sim.sync()
    st = sim.tree_stats()
    assert n < st["num_nodes"] < 1.7 * n
    p = sim.get_positions()
    assert p.shape == (n, 3) and np.isfinite(p).all()
    sim.close()
    print(f"{key}: {n / 1e6:.0f} M {c['distribution']} bodies generated on the device in {1e3 * t_gen:.0f} ms "
          f"(handle creation included); {st['num_nodes']} nodes, depth {st['max_depth']}")


def test_record_filament_device_ic_checkpoint_masses_and_resume(gpu, tmp_path, monkeypatch):
    from tools import record as rec
    from tools.presets import get_preset_config
    monkeypatch.setattr(rec, "STATE_EVERY", 3)  # a checkpoint after frame 2 of 4
    cfg = get_preset_config("cosmic_web")
    cfg.update(num_bodies=20_000, total_frames=4, session_name="t_web_ic", device_ic=True)
    d = rec.record(cfg, root=tmp_path, quiet=True, seed=5)
    assert rec.get_completed_frames(d) == 4
    with np.load(d / "state_0002.npz") as st:
        assert st["masses"].shape == (20_000,) and np.all(st["masses"] == 0.1)
    last, _ = rec.load_frame(d, 3)
    (d / "frame_0003.npz").unlink()
    rec.record(dict(cfg), resume=True, root=tmp_path, quiet=True)
    assert rec.get_completed_frames(d) == 4
    again, _ = rec.load_frame(d, 3)
    assert np.array_equal(again, last)  # as tests/test_gpu_sharded_record.py's resume test


def test_record_command_line_with_device_ic(gpu, tmp_path):
    cmd = [sys.executable, "-m", "tools.record", "--preset", "cosmic_web", "-n", "20k", "-f", "3", "--device-ic",
           "--seed", "3", "--root", str(tmp_path)]
    r = subprocess.run(cmd, cwd=PKG.PACKAGE_DIR, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    from tools import record as rec
    d = tmp_path / "recordings" / "cosmic_web"
    assert rec.get_completed_frames(d) == 3 and not (d / "frame_0003.npz").exists()
    meta = rec.load_metadata(d)
    assert meta["num_bodies"] == 20_000 and meta["total_frames"] == 3 and meta["seed"] == 3
    assert meta["device_ic"] is True and meta["distribution"] == "filament"
    p, c = rec.load_frame(d, 2)
    assert p.shape == (20_000, 3) and np.isfinite(p).all()
