"""Host restatement of force precision "auto" (include/nbmi.h, nbmi_set_force_precision).

With the bodies in sort-key order (rank r), p32 = (float)x, g32 = (float)(G m): a GROUP is 16 ranks aligned to the rank
index, a WAVE four groups.  dens of a group = fp32 sum of g32 over the volume of the group's fp32 bounding box with every
edge at least (float)eps; D_w = max over the wave's groups; flag_w = D_w > (float)(tau / dt^2); the system-wide verdict
is all64_rule on the flags' sum.  NumPy only, no GPU.

wave_values is the definition in float64 (on the fp32-rounded inputs), wave_values_f32 the same in the device's
arithmetic and association; thresholds() returns numbers that sit at least 1e-4 (relative) from every D_w, 150 x further
than the at most 11 fp32 roundings (11 * 2^-24 = 6.6e-7) can move one - so a count at such a threshold is exact
whichever of the two arithmetics produced the values."""
import numpy as np

MARGIN = 1e-4            # |threshold / D_w - 1| of every threshold handed out
ROUNDINGS = 11           # 4 in the sum, 3 differences, 2 products, 1 division, 1 conversion (eps or the threshold)
F32_BOUND = ROUNDINGS * 2.0 ** -24
ENTER_PM, LEAVE_PM = 333, 250

# the four DPP controls of k_gather_scan's row-of-16 reduction as lane permutations (lane i reads lane PERM[i])
_QUAD_1032 = np.array([(i & ~3) | [1, 0, 3, 2][i & 3] for i in range(16)])     # 0xB1  quad_perm [1,0,3,2]
_QUAD_2301 = np.array([(i & ~3) | [2, 3, 0, 1][i & 3] for i in range(16)])     # 0x4E  quad_perm [2,3,0,1]
_HALF_MIRROR = np.array([(i & 8) | (7 - (i & 7)) for i in range(16)])          # 0x141 row_half_mirror
_ROW_MIRROR = np.array([15 - i for i in range(16)])                            # 0x140 row_mirror
ROW16_STEPS = (_QUAD_1032, _QUAD_2301, _HALF_MIRROR, _ROW_MIRROR)


G, EPS, RADIUS, SEED = 0.15, 2.0, 500.0, 11
SIZES = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049)  # group, wave, 256-rank round, 2 048-rank tile edges


def cluster_input(n):
    """The tests' input: the "cluster" preset (radius 500, G 0.15) under a saved and restored NumPy seed, masses times
    uniform(0.5, 1.5) so that no two group sums are equal."""
    from tools.presets import generate_distribution
    state = np.random.get_state()
    try:
        np.random.seed(SEED)
        p, v, m = generate_distribution("cluster", n, RADIUS, G)
        m = m * np.random.uniform(0.5, 1.5, n)
    finally:
        np.random.set_state(state)
    return np.array(p, dtype=np.float64), np.array(v, dtype=np.float64), np.array(m, dtype=np.float64)


def planar_input(n=1000):
    """Bodies uniform in [-100, 100]^2 at z = 0: every group's box has volume 0 unless the softening floors it."""
    rng = np.random.default_rng(SEED)
    p = np.zeros((n, 3))
    p[:, :2] = rng.uniform(-100.0, 100.0, (n, 2))
    return p, np.zeros((n, 3)), rng.uniform(0.5, 1.5, n)


def key_order(pos):
    """Body indices along the device's sort-key order: the oracle's octant keys, relabelled along the Hilbert curve,
    ties by body index (the chain tests/test_gpu_nbody.py pins against the device)."""
    from hilbert_ref import hilbert_keys
    from oracle import pyref
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    hi, lo = pyref.body_keys(pos, pyref.compute_bounds(pos))
    shi, slo = hilbert_keys(hi, lo)
    return np.lexsort((np.arange(len(pos)), slo, shi)).astype(np.int32)


def _grouped(pos, mass, G, order, dtype):
    """(p [groups, 16, 3], g [groups, 16], present [groups, 16]) of the fp32-rounded inputs in `dtype`; the groups are
    padded to whole waves, absent ranks have g = 0."""
    pos = np.asarray(pos, dtype=np.float64)[order]
    gm = (float(G) * np.asarray(mass, dtype=np.float64))[order]
    n = len(pos)
    waves = (n + 63) // 64
    p = np.zeros((waves * 64, 3), dtype=dtype)
    g = np.zeros(waves * 64, dtype=dtype)
    present = np.zeros(waves * 64, dtype=bool)
    p[:n] = pos.astype(np.float32)
    g[:n] = gm.astype(np.float32)
    present[:n] = True
    return p.reshape(-1, 16, 3), g.reshape(-1, 16), present.reshape(-1, 16)


def _edges(p, present, eps, dtype):
    lo = np.where(present[..., None], p, np.inf).min(axis=1)
    hi = np.where(present[..., None], p, -np.inf).max(axis=1)
    with np.errstate(invalid="ignore"):
        d = (hi - lo).astype(dtype)  # (a group without bodies: -inf - inf, floored below, and its gsum is 0)
    d[~present.any(axis=1)] = 0
    return np.maximum(d, dtype(np.float32(eps)))


def _dens_to_waves(gsum, vol):
    with np.errstate(divide="ignore", invalid="ignore"):
        dens = np.where(gsum > 0, gsum / vol, gsum.dtype.type(0))
    return dens.reshape(-1, 4).max(axis=1).astype(np.float64)


def wave_values(pos, mass, G, eps, order):
    """D_w per wave, float64 arithmetic on the fp32-rounded p32 / g32 / eps: inf where a massive group's box has volume
    0, 0 for waves whose groups have no mass."""
    p, g, present = _grouped(pos, mass, G, order, np.float64)
    e = _edges(p, present, eps, np.float64)
    return _dens_to_waves(g.sum(axis=1), (e[:, 0] * e[:, 1]) * e[:, 2])


def nested_sum16(g):
    """fp32 sum over the last axis (16) in the device's association: ((w0+w1)+(w2+w3)) per quad, (q0+q1)+(q2+q3)."""
    g = np.asarray(g, dtype=np.float32)
    q = (g[..., 0::4] + g[..., 1::4]) + (g[..., 2::4] + g[..., 3::4])
    return (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])


def wave_values_f32(pos, mass, G, eps, order):
    """The same quantity with every operation in np.float32 and the device's association (returned widened)."""
    p, g, present = _grouped(pos, mass, G, order, np.float32)
    e = _edges(p, present, eps, np.float32)
    assert e.dtype == np.float32 and g.dtype == np.float32
    vol = (e[:, 0] * e[:, 1]) * e[:, 2]
    gsum = nested_sum16(g)
    assert vol.dtype == np.float32 and gsum.dtype == np.float32
    return _dens_to_waves(gsum, vol)


def row16_emulated(values, op):
    """The reduction as the kernel runs it: four times v = op(v, v[permutation]) over rows of 16 lanes (last axis).
    `op` works on np.float32 arrays (np.minimum, np.maximum, np.add); returns all 16 lanes."""
    v = np.array(values, dtype=np.float32)
    assert v.shape[-1] == 16
    for perm in ROW16_STEPS:
        v = op(v, v[..., perm])
        assert v.dtype == np.float32
    return v


def check_margins(thr, D, margin=MARGIN):
    """Raise unless every threshold is at least `margin` (relative) from every finite non-zero D_w."""
    D = np.asarray(D, dtype=np.float64)
    v = D[np.isfinite(D) & (D > 0)]
    thr = np.atleast_1d(np.asarray(thr, dtype=np.float64))
    if not (np.all(np.isfinite(thr)) and np.all(thr > 0)):
        raise ValueError(f"thresholds must be finite and positive: {thr}")
    if len(v) and len(thr):
        gap = np.abs(thr[:, None] / v[None, :] - 1.0).min()
        if gap < margin:
            raise ValueError(f"a threshold sits {gap:.3e} (relative) from a wave value, margin {margin:.1e}")


def thresholds(D):
    """fp32 thresholds that separate the distinct finite non-zero values of D: one below all of them, the geometric
    midpoints of adjacent ones, one above.  Raises (check_margins) where two values are too close to put a threshold
    between them at the margin.  No such value at all: [1]."""
    D = np.asarray(D, dtype=np.float64)
    v = np.unique(D[np.isfinite(D) & (D > 0)])
    if len(v) == 0:
        return np.array([1.0], dtype=np.float32)
    thr = np.concatenate([[v[0] / 2], np.sqrt(v[:-1] * v[1:]), [v[-1] * 2]]).astype(np.float32)
    check_margins(thr, D)
    return thr


def pick_thresholds(D, k):
    """k (or fewer, where the values allow no more) of the thresholds above, spread evenly over the sorted values:
    for inputs whose values lie too densely for all of them to be separated, at each target position the nearest
    candidate that keeps the margin.  The choice looks at the host's values only."""
    cand = separating_thresholds(D)
    targets = np.linspace(0, len(cand) - 1, k) if k > 1 else np.array([(len(cand) - 1) / 2])
    return cand[sorted({int(np.abs(np.arange(len(cand)) - t).argmin()) for t in targets})]


def separating_thresholds(D):
    """Every threshold of thresholds(D) that keeps twice the margin, ascending (never raises; the one below all values
    and the one above are always among them)."""
    D = np.asarray(D, dtype=np.float64)
    v = np.unique(D[np.isfinite(D) & (D > 0)])
    if len(v) == 0:
        return np.array([1.0], dtype=np.float32)
    cand = np.concatenate([[v[0] / 2], np.sqrt(v[:-1] * v[1:]), [v[-1] * 2]]).astype(np.float32)
    gap = np.abs(cand.astype(np.float64)[:, None] / v[None, :] - 1.0).min(axis=1)
    thr = cand[gap >= 2 * MARGIN]
    check_margins(thr, D)
    return thr


def tau_for(thr32, dt):
    """tau that makes the device's (float)(tau / dt^2) equal to thr32 - bit for bit when dt is a power of two (the
    product and the quotient are exact), within one fp32 rounding otherwise (which MARGIN covers)."""
    return float(np.float64(np.float32(thr32)) * np.float64(dt) * np.float64(dt))


def all64_rule(prev, ask, waves, enter_pm=ENTER_PM, leave_pm=LEAVE_PM):
    """csrc/nbmi.hip all64_rule in Python integers."""
    ask, waves = int(ask), int(waves)
    return 1000 * ask >= leave_pm * waves if prev else 1000 * ask > enter_pm * waves


def expected(pos, mass, G, eps, thr32, order=None):
    """(flags per wave, their sum, waves) at the fp32 threshold thr32."""
    if order is None:
        order = key_order(pos)
    flags = wave_values(pos, mass, G, eps, order) > np.float64(np.float32(thr32))
    return flags, int(flags.sum()), (len(order) + 63) // 64
