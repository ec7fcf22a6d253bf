"""Device-side initial conditions against their host replay (tests/icgen_ref.py), body by body.

Every case of icgen_ref.cases() - 1, 2, around one 256-thread block, past one 2048-item sort tile, 20 011, odd
collision halves; seeds 42 and 2^32 + 42 - is generated on the device and compared with the float64 replay:
masses exactly, positions within 256 max(E_ref, 2^-52) of R, velocities within the same multiple of the replay's
largest speed, where E_ref is the difference between the float64 and the extended-precision replay of that case
(tests/test_icgen_ref_host.py prints it and asserts the conditions - separated radii, floor ties, CDF margins -
under which no body needs to be left out; none is).  The factor 256 covers a device maths library that is allowed
a few ulp where the host's has under one, and a maximum over up to 20 011 bodies; every fault this test is for
(a draw in the wrong role or from the wrong half of its block, a dropped high word of seed or index, ranks one
disk off or wrong among floor ties, a single-precision constant, a mean over n - 1) is at least 1e-8.

Measured on the MI355X: see DESIGN.md, "Device-side initial conditions".
"""
import functools

import numpy as np
import pytest

import icgen_ref as ref

pytestmark = pytest.mark.gpu

FACTOR = 256.0
EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def _replays(dist, n, seed):
    return ref.generate(dist, seed, n), ref.generate(dist, seed, n, dtype=np.longdouble)


@functools.lru_cache(maxsize=None)
def _device(dist, n, seed):
    from nbody.gpu_backend import HIPBarnesHutSimulation
    R, G, eps = ref.PRESET[dist]
    sim = HIPBarnesHutSimulation.generated(dist, n, R, G, eps, 1.0, seed=seed)
    out = sim.get_positions_f64(), sim.get_velocities(), sim.get_masses()
    sim.close()
    for a in out:
        a.setflags(write=False)
    return out


def _case_id(c):
    return f"{c[0]}-{c[1]}-{'hi' if c[2] >> 32 else 'lo'}"


@pytest.mark.parametrize("case", ref.cases(), ids=_case_id)
def test_device_bodies_equal_the_replay(gpu, case):
    dist, n, seed = case
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, "np.longdouble is float64 on this machine"
    R = ref.PRESET[dist][0]
    lo, hi = _replays(dist, n, seed)
    e_pos, e_vel = ref.e_ref(lo, hi, R)
    vmax = ref.speed_scale(lo)
    dp, dv, dm = _device(dist, n, seed)
    assert dp.shape == (n, 3) and dv.shape == (n, 3) and dm.shape == (n,)
    assert np.array_equal(dm, lo["mass"]) and np.all(dm == (0.1 if dist == "filament" else 1.0))
    err_p = np.abs(dp - lo["pos"]).max(axis=1)
    err_v = np.abs(dv - lo["vel"]).max(axis=1)
    tol_p = FACTOR * max(e_pos, EPS) * R
    tol_v = FACTOR * max(e_vel, EPS) * vmax
    ip, iv = int(err_p.argmax()), int(err_v.argmax())
    print(f"{dist} n {n} seed {seed}: device - replay positions {err_p[ip] / R:.2e} R (body {ip}, bound "
          f"{tol_p / R:.2e}), velocities {err_v[iv] / vmax if vmax else err_v[iv]:.2e} vmax (body {iv}, bound "
          f"{tol_v / vmax if vmax else tol_v:.2e}); E_ref {e_pos:.1e} / {e_vel:.1e}")
    assert err_p[ip] <= tol_p, (ip, dp[ip], lo["pos"][ip], {k: v[ip] for k, v in hi.items()
                                                           if isinstance(v, np.ndarray) and len(v) == n})
    assert err_v[iv] <= tol_v, (iv, dv[iv], lo["vel"][iv], {k: v[iv] for k, v in hi.items()
                                                           if isinstance(v, np.ndarray) and len(v) == n})
    if dist == "filament":
        # the velocity law per body, on the device's own positions: v - 0.05 x is 0.3 times the replayed normals
        err_n = np.abs((dv - 0.05 * dp) - lo["noise"]).max()
        assert err_n <= tol_v + 0.05 * tol_p + 4 * EPS * vmax, err_n  # last term: the two subtractions' own rounding
        # and each body sits in the cloud of the replayed node: its offset from that node's centre is the replayed one
        T = lo["nodes"]
        off = lo["coef"][:, 0:1] * T["e"][lo["node"]] + lo["coef"][:, 1:2] * T["p1"][lo["node"]] \
            + lo["coef"][:, 2:3] * T["p2"][lo["node"]]
        assert np.abs((dp - T["centre"][lo["node"]]) - off).max() <= 2 * tol_p


@pytest.mark.parametrize("dist", ["galaxy", "spiral", "cluster", "filament"])
def test_positions_do_not_depend_on_n(gpu, dist):
    """A body's position is a function of (seed, index, R) alone, bit for bit; for the filament so is its velocity.
    (Disk and cluster velocities depend on n through the enclosed mass, the dispersion floor and the mean.)"""
    for seed in ref.SEEDS:
        big, small = _device(dist, 20011, seed), _device(dist, 257, seed)
        assert np.array_equal(big[0][:257], small[0])
        if dist == "filament":
            assert np.array_equal(big[1][:257], small[1])
        else:
            assert not np.array_equal(big[1][:257], small[1])


@pytest.mark.parametrize("dist", list(ref.PRESET))
def test_high_seed_word_changes_every_body(gpu, dist):
    for n in (257, 20011):
        a, b = _device(dist, n, ref.SEEDS[0]), _device(dist, n, ref.SEEDS[1])
        assert np.all(np.any(a[0] != b[0], axis=1)) and np.all(np.any(a[1] != b[1], axis=1))
