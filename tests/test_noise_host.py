"""The restatement of the noise of include/bdmi.h (tests/noise_ref.py) against written-out values, the library's own
Philox and the properties the header states; the bindings; the noise_sweep helpers and the flock_video flags with
stand-ins.  No GPU.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import boids_cases as BC
import boids_ref as R
import noise_ref as N
from conftest import ROOT
from icgen_ref import philox4x32_10
from test_flockstats_host import _FakeFlock, _FakeRenderer

U = 2.0 ** -53
SEED, STEP, DRAWS = 7, 3, 100_000  # the population of the statistical checks, fixed after looking (on the CPU)


@pytest.fixture(scope="module")
def population():
    return N.vectors(SEED, STEP, np.arange(DRAWS))


def test_written_out_vectors():
    """Two (seed, step, id) triples, computed once with this restatement and pasted in: a change of the counter layout,
    the key halves, the scaling or the pair order shows here."""
    xi, a, p = N.vectors(42, 0, [0])
    assert [float(v).hex() for v in xi[0]] == ["0x1.c1c87537cb2f3p-2", "-0x1.f453ffaac6bbfp-4", "0x1.c7b17f26fe758p-1"]
    assert (a[0], p[0]) == (0, 0)
    xi, a, p = N.vectors((1 << 32) + 42, (1 << 32) + 5, [4095])
    assert [float(v).hex() for v in xi[0]] == ["-0x1.fe0d6e16d8ae7p-2", "-0x1.8afbae51a16a7p-1", "-0x1.956ecf88f60e0p-2"]
    assert (a[0], p[0]) == (0, 1)  # pair 0 of this block is outside the disc


def test_first_draw_by_hand():
    """xi of (42, 0, 0) from the Philox block alone, in scalar Python floats."""
    w = philox4x32_10(np.array([0, 0, 0, 0], dtype=np.uint32), np.array([42, 0], dtype=np.uint32))
    x1 = (float(w[0]) + 0.5) * 2.0 ** -31 - 1.0
    x2 = (float(w[1]) + 0.5) * 2.0 ** -31 - 1.0
    s = x1 * x1 + x2 * x2
    assert s < 1.0
    t = float(np.sqrt(1.0 - s))
    want = np.array([(2.0 * x1) * t, (2.0 * x2) * t, 1.0 - 2.0 * s])
    assert R.same_bits(N.vectors(42, 0, [0])[0][0], want)


def test_counters_and_key_split_64_bit_values():
    c = N.counters([5, 6], (3 << 32) + 9, [0, 2])
    assert c.tolist() == [[5, 9, 3, 0], [6, 9, 3, 2]]
    assert N.key((7 << 32) + 1).tolist() == [1, 7]


def test_library_philox_agrees_on_the_counters_used():
    """nbmi_philox4x32_10 is a host function of the library: the very inline function the kernels call."""
    import nbmi_native
    lib = nbmi_native.load()
    for seed, step in ((42, 0), ((1 << 32) + 42, (1 << 32) + 5)):
        ctr = N.counters(np.arange(64), step, np.arange(64) % 3)
        want = philox4x32_10(ctr, N.key(seed)[None, :])
        k = np.ascontiguousarray(N.key(seed))
        for row, w in zip(ctr, want):
            c = np.ascontiguousarray(row)
            out = np.zeros(4, dtype=np.uint32)
            lib.nbmi_philox4x32_10(nbmi_native.ptr(c), nbmi_native.ptr(k), nbmi_native.ptr(out))
            assert out.tolist() == w.tolist()


def test_unit_length_is_a_rounding_bound(population):
    """|xi|^2 = three products and two sums of numbers at most 1 in size: within 8 * 2^-53 of 1."""
    xi = population[0]
    n2 = (xi[:, 0] * xi[:, 0] + xi[:, 1] * xi[:, 1]) + xi[:, 2] * xi[:, 2]
    err = np.abs(n2 - 1.0).max()
    print(f"max | |xi|^2 - 1 | = {err / U:.1f} u")
    assert err <= 8 * U


def test_component_means(population):
    """A uniform direction's component has variance 1/3: the mean of 10^5 lies within four standard deviations of 0."""
    m = population[0].mean(axis=0)
    print("component means", m)
    assert np.all(np.abs(m) <= 4 / np.sqrt(3 * DRAWS))


def test_population_reaches_every_acceptance_path(population):
    _, a, p = population
    assert ((a == 0) & (p == 0)).any() and ((a == 0) & (p == 1)).any() and (a == 1).any() and (a >= 2).any()
    # acceptance pi / 4 per pair: a fraction (1 - pi / 4)^2 of the boids goes on to a second block
    assert abs((a >= 1).mean() - (1 - np.pi / 4) ** 2) < 0.005


def test_steps_seeds_and_ids_are_independent_inputs():
    base = N.vectors(42, 5, np.arange(64))[0]
    assert not np.array_equal(base, N.vectors(42, 6, np.arange(64))[0])
    assert not np.array_equal(base, N.vectors(43, 5, np.arange(64))[0])
    assert not np.array_equal(base, N.vectors(42 + (1 << 32), 5, np.arange(64))[0])
    assert not np.array_equal(base, N.vectors(42, 5 + (1 << 32), np.arange(64))[0])
    perm = np.random.default_rng(0).permutation(64)
    assert R.same_bits(N.vectors(42, 5, perm)[0], base[perm])  # a function of the id, not of the row


def test_kick_and_walled_physics():
    prm = BC.params(bounds=12.0)
    rng = np.random.default_rng(1)
    n = 50
    pos, vel = R.lattice(rng.uniform(-12, 12, (n, 3)), BC.PB), R.lattice(rng.uniform(-12, 12, (n, 3)), BC.VB)
    col = R.id_colours(n)
    F = R.flocking(pos, vel, col, prm)
    forces = (F.sep, F.ali, F.coh, F.avg)
    # without a kick: boids_ref.physics itself ((a + b) + c is how NumPy evaluates a + b + c)
    assert all(R.same_bits(a, b) for a, b in zip(N.physics_walled(pos, vel, col, forces, prm, BC.DT),
                                                 R.physics(pos, vel, col, forces, prm, BC.DT)))
    k = N.kick(prm, 0.5, 42, 0, n)
    assert R.same_bits(k, (0.5 * 60.0) * N.vectors(42, 0, np.arange(n))[0])
    noisy = N.physics_walled(pos, vel, col, forces, prm, BC.DT, k)
    assert not R.same_bits(noisy[1], R.physics(pos, vel, col, forces, prm, BC.DT)[1])


# ---- bindings ---------------------------------------------------------------------------------------------------------
NEW_CALLS = {"bdmi_create_periodic": 6, "bdmi_get_box": 4, "bdmi_set_noise": 4, "bdmi_get_noise": 4, "bdmi_noise_vectors": 3}


def test_header_declares_and_table_binds_the_calls():
    import nbmi_native
    text = open(os.path.join(ROOT, "include", "bdmi.h")).read()
    lib = ctypes.CDLL(nbmi_native.LIB_PATH)
    for name, arity in NEW_CALLS.items():
        m = re.search(r"\b" + name + r"\(([^;]*)\);", text)
        assert m, name
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == arity == len(nbmi_native.PROTOTYPES[name][1]), name
        getattr(lib, name)
    assert nbmi_native.PROTOTYPES["bdmi_set_noise"][1][2] is ctypes.c_uint64
    for phrase in ("Equality does not shift", "(cx+a, cy+b, cz+c) mod dim", "max_speed * |dt| < L", "dim < 3 or dim > 1290",
                   "{i, (uint32)step, (uint32)(step >> 32), a}", "((double)u + 0.5) * 2^-31 - 1", "Marsaglia 1972",
                   "((sep_c + ali_c) + coh_c) + A * xi_c", "whether or not eta > 0", "bdmi_set_state does not touch it",
                   "do not contain the noise"):
        assert phrase in text, phrase


# ---- boids.analysis: order against noise ------------------------------------------------------------------------------
class _SweepFlock:
    """Polarisation 1 / (1 + eta * step): whatever noise_sweep sets and samples can be written down."""
    made = []

    def __init__(self):
        self.eta, self.steps, self.closed = None, 0, False
        self.noise = (0.0, 11, 0)
        _SweepFlock.made.append(self)

    def set_noise(self, eta, seed=0, step=None):
        self.eta, self.seed = eta, seed

    def update(self, dt, substeps=1):
        self.steps += substeps
        self.dt = dt

    def diagnostics(self):
        row = np.zeros(16)
        row[0], row[7], row[8], row[9] = 100, 1.0 / (1.0 + self.eta * self.steps), 2.0, 0.25
        return row

    def close(self):
        self.closed = True


def test_noise_sweep_and_binder_cumulant():
    from boids.analysis import binder_cumulant, noise_sweep, order_parameter_series
    rows = np.zeros((3, 16))
    rows[:, 7], rows[:, 8], rows[:, 9] = (0.5, 0.25, 1.0), 2.0, (0.1, 0.2, 0.3)
    s = order_parameter_series(rows)
    assert s["polarisation"].tolist() == [0.5, 0.25, 1.0] and s["milling"].tolist() == [0.1, 0.2, 0.3]
    assert s["mean_speed"].tolist() == [2.0] * 3
    with pytest.raises(ValueError):
        order_parameter_series(np.zeros((3, 15)))
    assert binder_cumulant([0.5, 0.5, 0.5]) == pytest.approx(2.0 / 3.0)  # no fluctuation: the ordered value
    phi = np.array([1.0, 2.0])
    assert binder_cumulant(phi) == pytest.approx(1 - (17 / 2) / (3 * (5 / 2) ** 2))
    assert np.isnan(binder_cumulant([])) and np.isnan(binder_cumulant([0.0, 0.0]))

    _SweepFlock.made.clear()
    out = noise_sweep(_SweepFlock, [0.0, 0.5], steps=10, discard=4, every=3, dt=0.02)
    assert [f.closed for f in _SweepFlock.made] == [True, True] and [f.eta for f in _SweepFlock.made] == [0.0, 0.5]
    assert all(f.steps == 10 and f.dt == 0.02 and f.seed == 11 for f in _SweepFlock.made)  # the flock's seed is kept
    assert [o["eta"] for o in out] == [0.0, 0.5] and [o["samples"] for o in out] == [2, 2]  # after updates 5 and 8
    assert out[0]["polarisation_mean"] == 1.0 and out[0]["polarisation_std"] == 0.0
    phi = np.array([1 / 3.5, 1 / 5.0])
    assert out[1]["polarisation_mean"] == pytest.approx(phi.mean()) and out[1]["polarisation_std"] == pytest.approx(phi.std())
    assert out[1]["binder"] == pytest.approx(binder_cumulant(phi))
    for bad in (dict(steps=0, discard=0, every=1), dict(steps=5, discard=5, every=1), dict(steps=5, discard=0, every=0)):
        with pytest.raises(ValueError):
            noise_sweep(_SweepFlock, [0.1], dt=0.02, **bad)


# ---- tools.flock_video: --periodic, --noise, --noise-seed -------------------------------------------------------------
class _BoxFlock(_FakeFlock):
    log = []

    def __init__(self, n, seed, device, periodic=False):
        super().__init__(n, seed, device)
        self.periodic = periodic
        _BoxFlock.log.append(("made", periodic))

    def set_noise(self, eta, seed=0, step=None):
        _BoxFlock.log.append(("noise", eta, seed))

    def update(self, dt, substeps=1):
        _BoxFlock.log.append(("update", substeps))
        return super().update(dt, substeps)

    def flocks(self, link=None):
        assert not self.periodic, "the flock finder is refused on a periodic flock"
        return super().flocks(link)

    def flock_catalogue(self, link=None, min_members=1, capacity=64):
        assert not self.periodic
        return super().flock_catalogue(link, min_members, capacity)

    def neighbour_stats(self, radius=None):
        assert not self.periodic
        return super().neighbour_stats(radius)


def _video(tmp_path, *flags):
    import tools.flock_video as fv
    _BoxFlock.log.clear()
    out = tmp_path / "clip.rgb"
    args = fv.build_parser().parse_args(["--boids", "64", "--frames", "4", "--format", "raw",
                                         "--diagnostics", "2", "--warmup", "3", "-o", str(out), *flags])
    t = fv.run(args, make_flock=_BoxFlock, make_renderer=_FakeRenderer, say=lambda *x: None)
    assert t["ok"]
    lines = [json.loads(l) for l in open(t["diagnostics"])]
    meta = json.loads((tmp_path / "clip.rgb.json").read_text())
    return lines, meta


def test_flock_video_periodic_and_noise_flags(tmp_path):
    import tools.flock_video as fv
    lines, meta = _video(tmp_path, "--periodic", "--noise", "0.5", "--noise-seed", "9")
    # both are set before the warm-up
    assert _BoxFlock.log[:3] == [("made", True), ("noise", 0.5, 9), ("update", 3)]
    assert meta["flock"]["periodic"] is True and meta["flock"]["noise"] == {"eta": 0.5, "seed": 9}
    assert len(lines) == 2
    for l in lines:  # the whole-flock row only
        assert l["periodic"] is True and l["noise"] == {"eta": 0.5, "seed": 9}
        assert "flocks" not in l and "n_flocks" not in l and "mean_neighbours" not in l and "global" in l
    assert "whole-flock row only" in " ".join(fv.build_parser().format_help().split())


def test_flock_video_records_the_flags_only_when_used(tmp_path):
    lines, meta = _video(tmp_path)
    assert _BoxFlock.log[:2] == [("made", False), ("update", 3)]
    assert "periodic" not in meta["flock"] and "noise" not in meta["flock"]
    assert all("periodic" not in l and "noise" not in l and "flocks" in l for l in lines)
    lines, meta = _video(tmp_path, "--noise", "0.25")
    assert ("noise", 0.25, 0) in _BoxFlock.log and meta["flock"]["noise"] == {"eta": 0.25, "seed": 0}
    assert all(l["noise"] == {"eta": 0.25, "seed": 0} and "periodic" not in l and "flocks" in l for l in lines)
    import tools.flock_video as fv
    with pytest.raises(ValueError, match="--noise"):
        fv.run(fv.build_parser().parse_args(["--frames", "1", "--noise", "-1"]), make_flock=_BoxFlock,
               make_renderer=_FakeRenderer, say=lambda *x: None)
