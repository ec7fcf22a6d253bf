"""The host restatement of force precision "auto" (tests/prec_ref.py) checked on its own, and the conditions under
which tests/test_gpu_prec_auto.py may compare counts exactly: every threshold it uses lies at least 1e-4 from every
wave value, fp32 rounding moves a wave value by less than 1e-5."""
import os
import re
import types

import numpy as np
import pytest

import prec_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the row-of-16 reduction -----------------------------------------------------------------------------------
def _row_cases():
    rng = np.random.default_rng(5)
    rows = [rng.uniform(-1e3, 1e3, 16), rng.uniform(0.0, 1.0, 16) * 10.0 ** rng.integers(-6, 6, 16)]
    for lane in range(16):  # one outlier at each lane in turn: a dropped or wrong permutation loses it from some lanes
        for out in (1e6, -1e6):
            r = rng.uniform(-1.0, 1.0, 16)
            r[lane] = out
            rows.append(r)
    return np.array(rows, dtype=np.float32)


def test_row16_permutations_are_the_four_dpp_controls():
    assert R.ROW16_STEPS[0].tolist() == [1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10, 13, 12, 15, 14]
    assert R.ROW16_STEPS[1].tolist() == [2, 3, 0, 1, 6, 7, 4, 5, 10, 11, 8, 9, 14, 15, 12, 13]
    assert R.ROW16_STEPS[2].tolist() == [7, 6, 5, 4, 3, 2, 1, 0, 15, 14, 13, 12, 11, 10, 9, 8]
    assert R.ROW16_STEPS[3].tolist() == [15 - i for i in range(16)]


def test_row16_reduction_reaches_every_lane_with_the_stated_association():
    rows = _row_cases()
    for op, want in ((np.minimum, rows.min(axis=1)), (np.maximum, rows.max(axis=1)), (np.add, R.nested_sum16(rows))):
        got = R.row16_emulated(rows, op)
        assert got.dtype == np.float32
        assert np.array_equal(_bits(got), np.repeat(_bits(want)[:, None], 16, axis=1)), op
    # the association matters: a plain left-to-right fp32 sum differs in bits for some of these rows
    seq = np.zeros(len(rows), dtype=np.float32)
    for k in range(16):
        seq = seq + rows[:, k]
    assert np.any(_bits(seq) != _bits(R.nested_sum16(rows)))
    # and every step is needed: without any one of the four, some lane misses the outlier
    for drop in range(4):
        v = rows.copy()
        for k, perm in enumerate(R.ROW16_STEPS):
            if k != drop:
                v = np.maximum(v, v[:, perm])
        assert np.any(v != rows.max(axis=1)[:, None]), drop


# ---- 2. the owner mode's floating-point restatement of the hysteresis ----------------------------------------------
def test_verdict_of_the_owner_mode_is_the_integer_rule_at_its_boundaries(monkeypatch):
    from nbody.sharded import LetBarnesHut
    monkeypatch.delenv("NBMI_ALL64_ENTER", raising=False)
    monkeypatch.delenv("NBMI_ALL64_LEAVE", raising=False)
    stepper = LetBarnesHut(types.SimpleNamespace(n_total=0), 0, 1)
    waves = np.arange(1, 200_001, dtype=np.int64)
    bad = []
    for base in (333 * waves // 1000, waves // 4):
        for d in (-1, 0, 1):
            ask = np.clip(base + d, 0, waves)
            for prev in (False, True):
                want = np.where(prev, 1000 * ask >= R.LEAVE_PM * waves, 1000 * ask > R.ENTER_PM * waves)
                for a, w, e in zip(ask.tolist(), waves.tolist(), want.tolist()):
                    stepper.all64 = prev
                    if stepper._verdict(a, w) != e:
                        bad.append((prev, a, w))
    assert not bad, bad[:10]
    # the vectorised expectation above is all64_rule itself
    for prev, a, w in [(0, 21, 64), (0, 22, 64), (1, 16, 64), (1, 15, 64), (0, 333, 1000), (0, 334, 1000), (1, 250, 1000),
                       (1, 249, 1000), (0, 0, 1), (0, 1, 1), (1, 0, 1)]:
        want = (1000 * a >= 250 * w) if prev else (1000 * a > 333 * w)
        assert R.all64_rule(prev, a, w) == want
    assert [R.all64_rule(*c) for c in [(0, 21, 64), (0, 22, 64), (1, 16, 64), (1, 15, 64)]] == [False, True, True, False]


# ---- 3. the gap conditions of every input the GPU tests use ----------------------------------------------------------
def _values(n):
    p, _, m = R.cluster_input(n)
    order = R.key_order(p)
    return p, m, order, R.wave_values(p, m, R.G, R.EPS, order)


def _min_ratio_gap(D):
    v = np.unique(D[np.isfinite(D) & (D > 0)])
    return np.inf if len(v) < 2 else (v[1:] / v[:-1]).min() - 1.0


def test_thresholds_refuse_values_that_are_too_close():
    D = np.array([1.0, 1.0 + 1.5e-4, 3.0])
    with pytest.raises(ValueError, match="margin"):
        R.thresholds(D)  # the midpoint would sit 7.5e-5 from both
    assert len(R.thresholds(np.array([1.0, 1.0 + 2.5e-4, 3.0, np.inf, 0.0, 3.0]))) == 4
    with pytest.raises(ValueError):
        R.check_margins([1.00005], D)
    assert R.thresholds(np.array([0.0, np.inf])).tolist() == [1.0]


def test_gap_conditions_of_the_sweep_and_hysteresis_inputs():
    _, _, _, D = _values(4099)
    assert len(D) == 65 and len(R.thresholds(D)) == 66
    gap = _min_ratio_gap(D)
    print("n = 4099: smallest ratio gap of adjacent wave values", gap)
    assert gap >= 1.5e-3
    _, _, _, D = _values(4096)
    assert len(D) == 64 and len(R.thresholds(D)) == 65
    gap = _min_ratio_gap(D)
    print("n = 4096: smallest ratio gap", gap)
    assert gap >= 4.5e-3
    desc = np.sort(D)[::-1]
    # the hysteresis test puts thresholds between the descending ranks 15/16/17 and 21/22/23 (1-based)
    ratios = [desc[14] / desc[15], desc[15] / desc[16], desc[20] / desc[21], desc[21] / desc[22]]
    print("n = 4096: ratios 15/16, 16/17, 21/22, 22/23:", ratios)
    assert min(ratios) >= 1.005


@pytest.mark.parametrize("n", R.SIZES)
def test_gap_conditions_of_the_size_edges(n):
    _, _, order, D = _values(n)
    assert len(D) == (n + 63) // 64 and len(order) == n
    thr = R.thresholds(D)
    assert len(thr) == len(np.unique(D[np.isfinite(D) & (D > 0)])) + 1
    assert _min_ratio_gap(D) >= 2.5e-4


def test_gap_conditions_of_the_isolation_and_floor_inputs():
    p, m, order, _ = _values(4099)
    rank = np.empty(len(p), dtype=np.int64)
    rank[order] = np.arange(len(p))
    masks = [(rank % 64) // 16 == q for q in range(4)] + [rank % 16 == (rank // 16) % 16]
    for k, mask in enumerate(masks):
        D = R.wave_values(p, np.where(mask, m, 0.0), R.G, R.EPS, order)
        assert np.count_nonzero(D > 0) >= 64, k
        thr = R.pick_thresholds(D, 8)
        counts = [int((D > t).sum()) for t in thr.astype(np.float64)]
        assert len(thr) == 8 and counts[0] == np.count_nonzero(D > 0) and counts[-1] == 0, (k, counts)
        assert len(set(counts)) == 8, (k, counts)
    assert np.all(R.wave_values(p, np.zeros_like(m), R.G, R.EPS, order) == 0.0)
    # every edge floored: the values are gsum / 1e9 and lie too densely to separate them all - three thresholds
    # (below, about the median, above) that keep the margin
    D = R.wave_values(p, m, R.G, 1e3, order)
    with pytest.raises(ValueError, match="margin"):
        R.thresholds(D)
    thr = R.pick_thresholds(D, 3)
    counts = [int((D > t).sum()) for t in thr.astype(np.float64)]
    assert counts[0] == 65 and 20 <= counts[1] <= 45 and counts[2] == 0, counts
    pp, _, pm = R.planar_input()
    po = R.key_order(pp)
    assert np.all(np.isinf(R.wave_values(pp, pm, R.G, 0.0, po)))
    assert np.all(R.wave_values(pp, np.zeros_like(pm), R.G, 0.0, po) == 0.0)
    one = np.tile([[3.0, -4.0, 5.0]], (40, 1))
    assert np.all(np.isinf(R.wave_values(one, np.ones(40), R.G, 0.0, R.key_order(one))))


def test_a_ragged_tail_and_absent_groups_follow_the_definition():
    # 17 bodies: group 0 full, group 1 one body (its box is the floor cube), groups 2 and 3 absent
    p, _, m = R.cluster_input(17)
    order = R.key_order(p)
    D = R.wave_values(p, m, R.G, R.EPS, order)
    g32 = (R.G * m[order]).astype(np.float32).astype(np.float64)
    p32 = p[order].astype(np.float32).astype(np.float64)
    e = np.maximum(p32[:16].max(axis=0) - p32[:16].min(axis=0), 2.0)
    want = max(g32[:16].sum() / (e[0] * e[1] * e[2]), g32[16] / 8.0)
    assert D.shape == (1,) and D[0] == want


# ---- 4. how far fp32 rounding moves a wave value --------------------------------------------------------------------
def _f32_deviation():
    worst = 0.0
    for n in (4099, 4096) + R.SIZES:
        p, m, order, D = _values(n)
        for eps in (R.EPS, 1e3, 1e-3):
            D64 = R.wave_values(p, m, R.G, eps, order)
            D32 = R.wave_values_f32(p, m, R.G, eps, order)
            ok = np.isfinite(D64) & (D64 > 0)
            assert np.array_equal(ok, np.isfinite(D32) & (D32 > 0))
            worst = max(worst, np.abs(D32[ok] / D64[ok] - 1.0).max())
    return worst


def test_fp32_rounding_moves_a_wave_value_far_less_than_the_margin():
    worst = _f32_deviation()
    print(f"largest |wave_values_f32 / wave_values - 1| = {worst:.3e} (bound {R.F32_BOUND:.2e}, margin {R.MARGIN:.0e})")
    assert worst < 1e-5
    assert worst <= R.F32_BOUND  # the derived bound: 11 roundings
    # DESIGN.md quotes the measured value
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as f:
        m = re.search(r"largest observed `\|wave_values_f32 / wave_values − 1\|` is ([0-9.]+)·10⁻⁷", f.read())
    assert m, "DESIGN.md section 4.2 must quote the measured deviation"
    assert abs(float(m.group(1)) * 1e-7 - worst) <= 0.05e-7, (m.group(1), worst)
