"""k-nearest-neighbour densities, host side: the NumPy restatement against the definition, ties and coincident bodies,
the colour ramp as a function of t, the C ABI's declarations, and the recorder's options and metadata with a stand-in
backend (no device)."""
import ctypes
import os
import re

import numpy as np
import pytest

import knn_ref as kr
from conftest import ROOT

KNN_CALLS = ("nbmi_knn", "nbmi_get_densities_f64", "nbmi_set_color_mode", "nbmi_get_color_mode")


def test_restatement_against_the_double_loop():
    rng = np.random.RandomState(2)
    p = rng.normal(size=(40, 3)) * 5.0
    m = rng.uniform(0.5, 1.5, 40)
    many = kr.knn_many(p, m, (1, 2, 7, 39), chunk=7)
    for k in (1, 2, 7, 39):
        r2, mk = kr.knn_naive(p, m, k)
        assert np.array_equal(many[k][0], r2)
        assert np.allclose(many[k][1], mk, rtol=1e-14, atol=0.0)
        assert np.array_equal(kr.knn(p, m, k)[0], r2)


def test_ties_and_coincident_bodies_by_hand():
    # bodies 0 and 1 coincide; 2, 3 and 4 are all at distance 1 from them; 5 is far
    p = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, -1], [10, 0, 0]], np.float64)
    m = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0])
    r2, mk = kr.knn(p, m, 1)
    assert r2[0] == 0.0 and r2[1] == 0.0      # the coincident OTHER body counts, self does not
    assert mk[0] == 3.0 and mk[1] == 3.0      # own mass + the twin
    assert r2[2] == 1.0 and mk[2] == 4.0 + 1.0 + 2.0   # both twins tie at distance 1: mass_k covers both
    r2, mk = kr.knn(p, m, 2)
    assert r2[0] == 1.0 and mk[0] == 1.0 + 2.0 + 4.0 + 8.0 + 16.0   # k = 2 reaches the three-way tie: all of it counts
    r2, mk = kr.knn(p, m, 4)
    assert r2[0] == 1.0 and mk[0] == 31.0     # ... and the value does not depend on which of the tied came "first"
    r2, mk = kr.knn(p, m, 5)
    assert r2[0] == 100.0 and mk[0] == 63.0
    rho = kr.density(*kr.knn(p, m, 1))
    assert rho[0] == np.inf and rho[1] == np.inf
    assert rho[2] == 7.0 / kr.SPHERE
    a, b = kr.knn(p, m, 3), kr.knn(p[::-1], m[::-1], 3)  # the order of the bodies changes nothing
    assert np.array_equal(a[0], b[0][::-1]) and np.array_equal(a[1], b[1][::-1])


def test_ramp_is_continuous_at_every_breakpoint_and_bounded_in_slope():
    for b in kr.BREAKPOINTS:
        below, at = kr.ramp(np.nextafter(b, 0.0)), kr.ramp(b)
        assert np.abs(below - at).max() < 1e-13, (b, below, at)
    t = np.linspace(0.0, 1.0, 20001)
    c = kr.ramp(t)
    assert ((c >= -1e-15) & (c <= 1.0)).all()  # ((1 - 0.99) / 0.01 rounds to 1 + 9e-16: green ends at -4e-16)
    slope = np.abs(np.diff(c, axis=0)).max() / (t[1] - t[0])
    assert slope <= 50.0 * (1.0 + 1e-9), slope
    assert np.array_equal(kr.ramp(0.0), [0.4, 0.2, 0.8]) and np.allclose(kr.ramp(1.0), [1.0, 0.0, 0.0], rtol=0.0, atol=1e-15)
    # the density colours: clamped position of log10 rho in the range; +inf is the top of the ramp
    assert np.array_equal(kr.density_t(np.array([1e-9, 1.0, 10.0, 1e9, np.inf, 0.0]), 0.0, 2.0), [0.0, 0.0, 0.5, 1.0, 1.0, 0.0])
    assert np.array_equal(kr.density_colors(np.array([np.inf]), -1.0, 1.0)[0], kr.ramp(1.0))


def test_ramp_restates_the_library_source():
    """every constant of color_ramp_t appears in the restatement's pieces (a drifted copy would pass its own tests)"""
    src = open(os.path.join(ROOT, "3d-spatial-sim-for-boid-and-nbody_amd", "csrc", "nbmi.hip")).read()
    body = src[src.index("void color_ramp_t("):src.index("__device__ __forceinline__ void color_ramp(double vx")]
    for piece in ("t < 0.55", "t < 0.15", "t < 0.30", "s < 0.6", "t < 0.90", "t < 0.95", "t < 0.99", "(t - 0.30) / 0.25",
                  "(s - 0.6) / 0.4", "(t - 0.99) / 0.01"):
        assert piece in body, piece
    assert "color_ramp_t(t, out_r, out_g, out_b)" in src  # the speed path goes through it


def test_header_declares_and_library_exports_the_knn_calls():
    import nbmi_native
    text = open(os.path.join(ROOT, "include", "nbmi.h")).read()
    for name in KNN_CALLS:
        assert re.search(r"^int %s\(nbmi_sim \*sim" % name, text, re.M), f"include/nbmi.h does not declare {name}"
        assert name in nbmi_native.PROTOTYPES
    assert re.search(r"^#define NBMI_COLOR_SPEED 0$", text, re.M) and re.search(r"^#define NBMI_COLOR_DENSITY 1$", text, re.M)
    assert len(nbmi_native.PROTOTYPES["nbmi_knn"][1]) == 5
    lib = ctypes.CDLL(nbmi_native.LIB_PATH)
    for name in KNN_CALLS:
        assert hasattr(lib, name), f"libnbmi.so lacks {name}"


def test_python_classes_refuse_without_a_device():
    from nbody.gpu_backend import COLOR_MODES, HIPDirectSimulation, HIPOwnerSimulation, _HIPSimulation
    assert COLOR_MODES == {"speed": 0, "density": 1}
    for cls, word in ((HIPDirectSimulation, "direct"), (HIPOwnerSimulation, "owner")):
        sim = cls.__new__(cls)  # no handle: the refusal must come before any library call
        sim._h = None
        for call in (lambda: sim.knn(8), lambda: sim.densities(), lambda: sim.set_color_mode("density")):
            with pytest.raises(ValueError, match=word):
                call()
    with pytest.raises(ValueError, match="color mode"):
        _HIPSimulation.__new__(_HIPSimulation).set_color_mode("temperature")
    from nbody.sharded import create_sharded_simulation
    with pytest.raises(ValueError, match="only speed colours"):
        create_sharded_simulation(None, None, None, 1.0, 0.1, 1.0, color="density")


# ---- the recorder ----------------------------------------------------------------------------------------------------
def _args(*extra):
    from tools import record as rec
    return rec.build_parser().parse_args(["--preset", "quick_galaxy", *extra])


def test_recorder_options():
    from tools import record as rec
    assert "color" not in rec.build_config(_args())                       # the default writes no key
    assert "color" not in rec.build_config(_args("--color", "speed"))
    assert rec.build_config(_args("--color", "density"))["color"] == {"mode": "density", "k": 32}
    cfg = rec.build_config(_args("--color", "density", "--density-k", "8", "--density-range", "-4.5", "1"))
    assert cfg["color"] == {"mode": "density", "k": 8, "log10_range": [-4.5, 1.0]}
    assert rec.color_config(cfg) == ("density", 8, (-4.5, 1.0))
    assert rec.color_config({}) == ("speed", 32, None)
    for bad in (("--density-k", "8"), ("--density-range", "0", "1"), ("--color", "speed", "--density-k", "8"),
                ("--color", "density", "--density-k", "0"), ("--color", "density", "--density-k", "65"),
                ("--color", "density", "--density-range", "1", "1"), ("--color", "density", "--density-range", "2", "1"),
                ("--color", "density", "--bodies", "9", "--density-k", "9")):
        with pytest.raises(ValueError):
            rec.build_config(_args(*bad))
    with pytest.raises(SystemExit):
        _args("--color", "temperature")


class FakeSim:
    """densities / set_color_mode of the backend object; rho spans eight decades"""

    def __init__(self, n=1000):
        self.rho = np.logspace(-6.0, 2.0, n)
        self.rho[::97] = np.inf  # coincident bodies: not part of the range
        self.calls = []

    def densities(self, k=32):
        self.calls.append(("densities", k))
        return self.rho.copy()

    def set_color_mode(self, mode, k=32, log10_range=(0.0, 1.0)):
        self.calls.append(("set_color_mode", mode, k, tuple(log10_range)))


def test_recorder_metadata_round_trip_and_status(tmp_path, capsys):
    from tools import record as rec
    cfg = rec.build_config(_args("--color", "density", "--density-k", "16"))
    d = rec.get_recording_dir("dens", tmp_path)
    rec.save_metadata(d, cfg, 0.0)
    sim = FakeSim()
    out = rec.apply_color_mode(sim, cfg, d)
    lo, hi = out["color"]["log10_range"]
    fin = np.log10(sim.rho[np.isfinite(sim.rho)])
    assert lo == np.percentile(fin, 1.0) and hi == np.percentile(fin, 99.9) + 1.0
    assert (lo, hi) == kr.default_log10_range(sim.rho)
    assert sim.calls == [("densities", 16), ("set_color_mode", "density", 16, (lo, hi))]
    meta = rec.load_metadata(d)
    assert meta["color"] == {"mode": "density", "k": 16, "log10_range": [lo, hi]}
    assert meta["start_time"] == 0.0 and meta["num_bodies"] == cfg["num_bodies"]  # the rest of the file is kept
    # --resume / --extend: the range comes from metadata.json, the state is not asked again
    again = FakeSim()
    again.rho *= 100.0
    assert rec.apply_color_mode(again, meta, d)["color"] == meta["color"]
    assert again.calls == [("set_color_mode", "density", 16, (lo, hi))]
    assert rec.load_metadata(d) == meta
    # an explicit range is used as given; a speed session touches nothing
    given = FakeSim()
    rec.apply_color_mode(given, rec.build_config(_args("--color", "density", "--density-range", "-3", "2")), None)
    assert given.calls == [("set_color_mode", "density", 32, (-3.0, 2.0))]
    plain = FakeSim()
    assert rec.apply_color_mode(plain, rec.build_config(_args()), None) == rec.build_config(_args()) and plain.calls == []
    capsys.readouterr()
    assert rec.show_status("dens", root=tmp_path)
    text = capsys.readouterr().out
    assert "Color: density (k = 16" in text and f"{lo:.3f} .. {hi:.3f}" in text
    rec.save_metadata(rec.get_recording_dir("plain", tmp_path), rec.build_config(_args()), 0.0)
    assert rec.show_status("plain", root=tmp_path) and "Color: speed" in capsys.readouterr().out
    empty = FakeSim()
    empty.rho[:] = np.inf
    with pytest.raises(ValueError, match="no finite density"):
        rec.apply_color_mode(empty, cfg, None)
