"""The host replay of the device initial conditions (tests/icgen_ref.py), checked without a GPU: its Philox
against the library's host entry, its distributions against the NumPy generator of tools/presets.py, the
conditions under which the GPU comparison (tests/test_gpu_icgen_replay.py) is unambiguous, and E_ref, the
float64-versus-extended-precision difference that the GPU tolerance is built from."""
import ctypes as C
import functools

import numpy as np
import pytest
from scipy import stats

import icgen_ref as ref

N_STAT = 20011
P_MIN = 1e-3
DISKS = ("galaxy", "spiral", "collision")


def _lib_philox(ctr, key):
    import nbmi_native
    lib = nbmi_native.load()
    c, k, o = (C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), (C.c_uint32 * 4)()
    lib.nbmi_philox4x32_10(c, k, o)
    return list(o)


def test_vectorised_philox_equals_the_library():
    kat = [([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
           ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
           ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
            [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1])]
    ctr = np.array([c for c, _, _ in kat], dtype=np.uint32)
    key = np.array([k for _, k, _ in kat], dtype=np.uint32)
    out = ref.philox4x32_10(ctr, key)
    for i, (c, k, want) in enumerate(kat):
        assert out[i].tolist() == want and _lib_philox(c, k) == want
    rng = np.random.RandomState(0)
    ctr = rng.randint(0, 2 ** 32, (10_000, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.randint(0, 2 ** 32, (10_000, 2), dtype=np.uint64).astype(np.uint32)
    out = ref.philox4x32_10(ctr, key)
    assert out.dtype == np.uint32 and out.shape == (10_000, 4)
    for i in range(10_000):
        assert out[i].tolist() == _lib_philox(ctr[i].tolist(), key[i].tolist()), i


def test_uniform_words_and_counter_layout():
    """uniform(k) of body i under a 64-bit seed, spelled out once by hand from the library's Philox."""
    seed, body = 2 ** 32 * 7 + 42, 2 ** 32 * 3 + 5
    d = ref.Draws(seed, [body])
    for k in (0, 1, 6, 7):
        w = _lib_philox([5, 3, k >> 1, ref.TAG_BODIES], [42, 7])
        a, b = (w[2], w[3]) if k & 1 else (w[0], w[1])
        assert d.uniform(k)[0] == (float(((a << 32) | b) >> 11) + 0.5) * 2.0 ** -53
    n0, n1 = d.normal2(3)
    u1, u2 = d.uniform(6)[0], d.uniform(7)[0]
    assert n0[0] == np.sqrt(-2 * np.log(u1)) * np.cos(ref.TWO_PI * u2)
    assert n1[0] == np.sqrt(-2 * np.log(u1)) * np.sin(ref.TWO_PI * u2)
    assert ref.TWO_PI == 2 * np.pi
    nodes = ref.Draws(seed, [body], tag=ref.TAG_NODES)
    assert nodes.uniform(0)[0] != d.uniform(0)[0]
    hi = ref.Draws(seed, [body], dtype=np.longdouble)
    assert hi.uniform(5).dtype == np.longdouble and hi.uniform(5)[0] == d.uniform(5)[0]


@functools.lru_cache(maxsize=None)
def _replay(dist, n, seed, wide=False):
    return ref.generate(dist, seed, n, dtype=np.longdouble if wide else np.float64)


def _host(dist, n, seed):
    from tools.presets import generate_distribution
    R, G, _ = ref.PRESET[dist]
    np.random.seed(seed)
    return generate_distribution(dist, n, R, G)


def _host_web_nodes(n, seed):
    """Centres of the nodes that presets._cosmic_web gave each body: its first three draws, taken again."""
    R = ref.PRESET["filament"][0]
    coords = np.linspace(-R * 1.25, R * 1.25, ref.WEB_GRID)
    centers = np.stack(np.meshgrid(coords, coords, coords, indexing="ij"), axis=-1).reshape(-1, 3)
    np.random.seed(seed)
    active = centers[np.random.random(len(centers)) < 0.35]
    weights = np.random.power(2.0, len(active))
    weights /= weights.sum()
    return active[np.random.choice(len(active), size=n, p=weights)], weights


def _statistics(dist, pos, vel, centre=None):
    """Named one-dimensional samples whose law does not depend on the random stream."""
    pos, vel = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    out = {"v_x": vel[:, 0], "v_y": vel[:, 1], "v_z": vel[:, 2]}
    if dist == "cluster":
        out["|x|"] = np.linalg.norm(pos, axis=1)
        out["|v|"] = np.linalg.norm(vel, axis=1)
        out["height"] = pos[:, 1]
    elif dist == "filament":
        # the set of active nodes is itself random, so compare what is not: the offset from the body's own node
        # and the velocity noise
        out = {"|x - node|": np.linalg.norm(pos - centre, axis=1)}
        noise = vel - 0.05 * pos
        out.update({"noise_x": noise[:, 0], "noise_y": noise[:, 1], "noise_z": noise[:, 2]})
    elif dist == "collision":
        half = len(pos) // 2
        sep = ref.PRESET[dist][0] * 0.5 * 3.5
        for tag, sl, x0 in (("a", slice(0, half), -sep / 2), ("b", slice(half, None), sep / 2)):
            out["radius_" + tag] = np.hypot(pos[sl, 0] - x0, pos[sl, 2])
            out["height_" + tag] = pos[sl, 1]
            out["v_x_" + tag] = vel[sl, 0]
    else:
        out["radius"] = np.hypot(pos[:, 0], pos[:, 2])
        out["height"] = pos[:, 1]
    return out


@pytest.mark.parametrize("dist", list(ref.PRESET))
def test_replay_is_statistically_the_numpy_generator(dist):
    hp, hv, hm = _host(dist, N_STAT, 42)
    rep = _replay(dist, N_STAT, 42)
    assert np.array_equal(rep["mass"], hm)
    if dist == "filament":
        h_centre, h_weights = _host_web_nodes(N_STAT, 42)
        T = rep["nodes"]
        a = _statistics(dist, hp, hv, h_centre)
        b = _statistics(dist, rep["pos"], rep["vel"], T["centre"][rep["node"]])
        # the node table's own laws: weight ~ power(2), active count ~ Binomial(512, 0.35) (6 sigma), picks ~ weights
        assert stats.ks_2samp(h_weights * len(h_weights), T["weight"] / T["weight"].mean()).pvalue > P_MIN
        assert abs(len(T["cdf"]) - 512 * 0.35) < 6 * np.sqrt(512 * 0.35 * 0.65)
        picks = np.bincount(rep["node"], minlength=len(T["cdf"]))
        expect = np.diff(np.concatenate([[0.0], T["cdf"]])) * N_STAT
        assert stats.chisquare(picks, expect * picks.sum() / expect.sum()).pvalue > P_MIN
        for v in ("e", "p1", "p2"):  # v / (|v| + 1e-10) is short of a unit vector by 1e-10 / |v|
            norm = np.linalg.norm(T[v], axis=1)
            assert norm.max() <= 1.0 and norm.min() > 1 - 1e-7
        # and e falls short likewise, so p1 keeps (p.e)(1 - |e|^2) / |p1| of it: 1e-6 allows |p.e| = 5 and norms of 0.03
        assert max(np.abs((T[u] * T[v]).sum(axis=1)).max() for u, v in (("e", "p1"), ("e", "p2"), ("p1", "p2"))) < 1e-6
        s = ref.PRESET[dist][0] * 2.5 / ref.WEB_GRID
        for col, sd in enumerate((0.8 * s, 0.12 * s, 0.12 * s)):  # along the axis and across it, twice
            assert stats.kstest(rep["coef"][:, col], "norm", args=(0.0, sd)).pvalue > P_MIN
    else:
        a, b = _statistics(dist, hp, hv), _statistics(dist, rep["pos"], rep["vel"])
    report = []
    for name in a:
        ks = stats.ks_2samp(a[name], b[name])
        report.append(f"{name} KS {ks.statistic:.4f} p {ks.pvalue:.3f}")
    print(f"{dist} replay vs NumPy generator, n {N_STAT}: " + "; ".join(report))
    for name in a:
        assert stats.ks_2samp(a[name], b[name]).pvalue > P_MIN, name
    if dist in ref.COM_REMOVED:
        assert np.abs(rep["vel"].mean(axis=0)).max() < 1e-12 * ref.speed_scale(rep)


def _disk_slices(dist, n):
    return [slice(0, n // 2), slice(n // 2, n)] if dist == "collision" else [slice(0, n)]


@pytest.mark.parametrize("dist", DISKS)
def test_disk_cases_have_separated_radii_and_floor_ties(dist):
    """A rank can be compared body by body only if no last-bit difference in a radius can move it: distinct radii
    of every disk case are at least 1e-10 apart (relative), in either precision, and both precisions rank alike.
    Bodies tied at the 0.001 R floor must exist from n = 4099 on, so that their index-order ranking is exercised."""
    R = ref.PRESET[dist][0]
    report = []
    for d, n, seed in ref.cases():
        if d != dist:
            continue
        lo, hi = _replay(dist, n, seed), _replay(dist, n, seed, True)
        assert np.array_equal(lo["rank"], hi["rank"])
        gaps, ties = [], []
        for sl in _disk_slices(dist, n):
            r = lo["radius"][sl]
            assert np.array_equal(np.sort(lo["rank"][sl]), np.arange(len(r)))
            ties.append(int((r == R * 0.001).sum()))
            assert np.array_equal((hi["radius"][sl] == np.longdouble(R) * 0.001), r == R * 0.001)
            u = np.unique(r)
            if len(u) > 1:
                gaps.append(float((np.diff(u) / u[1:]).min()))
            # tied bodies rank in index order, below every other body
            floor = np.flatnonzero(r == R * 0.001)
            assert np.array_equal(lo["rank"][sl][floor], np.arange(len(floor)))
        report.append(f"n {n} seed {seed}: gap {min(gaps) if gaps else float('inf'):.2e} ties {ties}")
        assert not gaps or min(gaps) >= 1e-10, report[-1]
        if n >= 4099:
            assert min(ties) >= 2, report[-1]
    print(f"{dist}: " + "; ".join(report))


def test_filament_picks_are_clear_of_the_cdf_edges():
    report = []
    for d, n, seed in ref.cases():
        if d != "filament":
            continue
        lo, hi = _replay(d, n, seed), _replay(d, n, seed, True)
        assert np.array_equal(lo["node"], hi["node"])
        assert np.array_equal(lo["nodes"]["grid_index"], hi["nodes"]["grid_index"])
        cdf = lo["nodes"]["cdf"]
        assert cdf[-1] == 1.0 and np.all(np.diff(cdf) > 0) and lo["node"].max() < len(cdf)
        margin = min(lo["cdf_margin"], hi["cdf_margin"])
        report.append(f"n {n} seed {seed}: {len(cdf)} nodes, margin {margin:.2e}")
        assert margin >= 1e-9, report[-1]
    print("filament: " + "; ".join(report))


def test_e_ref_of_every_case():
    """E_ref per case.  np.longdouble must be wider than float64, or E_ref would be 0 by construction."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, "np.longdouble is float64 on this machine"
    worst = {}
    for dist, n, seed in ref.cases():
        lo, hi = _replay(dist, n, seed), _replay(dist, n, seed, True)
        assert hi["pos"].dtype == np.longdouble and lo["pos"].dtype == np.float64
        ep, ev = ref.e_ref(lo, hi, ref.PRESET[dist][0])
        print(f"E_ref {dist} n {n} seed {seed}: positions {ep:.2e} velocities {ev:.2e}")
        w = worst.setdefault(dist, [0.0, 0.0])
        w[0], w[1] = max(w[0], ep), max(w[1], ev)
        # the device bound is 256 E_ref and the smallest fault it must catch is 1e-8 (a single-precision constant):
        # 256 x 2^-36 = 3.7e-9 keeps the bound below that in every case
        assert ep < 2.0 ** -36 and ev < 2.0 ** -36, (dist, n, seed, ep, ev)
    print("largest E_ref: " + "; ".join(f"{d} pos {w[0]:.2e} vel {w[1]:.2e}" for d, w in worst.items()))


def test_positions_do_not_depend_on_n_in_the_replay():
    for dist in ("galaxy", "spiral", "cluster", "filament"):
        a, b = _replay(dist, 20011, 42), _replay(dist, 257, 42)
        assert np.array_equal(a["pos"][:257], b["pos"])
        if dist == "filament":
            assert np.array_equal(a["vel"][:257], b["vel"])
        else:
            assert not np.array_equal(a["vel"][:257], b["vel"])
