"""nbmi_deposit, host side (no device): the NumPy restatement of the header (tests/deposit_ref.py) against the properties
the header states - order independence, conservation, the per-cell error bound against a plain float64 deposit -, the
derived fields of nbody/grid.py, and the recorder's --density-map options, metadata and map files with a stand-in
backend."""
import math
import re

import numpy as np
import pytest

import deposit_ref as dr
from conftest import ROOT
from test_record_streams_host import FRAMES, Handle, World, _config, _files

N = 5000
LO, HI, DIMS = (-6.0, -6.0, -6.0), (6.0, 6.0, 6.0), (8, 8, 8)


def _gaussian(seed=3):
    rng = np.random.RandomState(seed)
    p = rng.normal(size=(N, 3))
    v = rng.normal(size=(N, 3)) * 3.0
    m = rng.uniform(0.5, 2.0, N)
    assert np.abs(p).max() < 4.5            # every body at least one cell (1.5) inside the box
    assert (v != 0.0).all() and (m > 0).all()  # every selected quantity is nonzero on every body
    return p, v, m


_REF = {}


def _reference(scheme):
    if scheme not in _REF:
        p, v, m = _gaussian()
        _REF[scheme] = dr.deposit(p, v, m, LO, HI, DIMS, scheme, dr.ALL)
    return _REF[scheme]


@pytest.mark.parametrize("scheme", [dr.NGP, dr.CIC])
def test_a_permuted_input_gives_the_same_bits(scheme):
    p, v, m = _gaussian()
    out, stats, e = _reference(scheme)
    perm = np.random.RandomState(9).permutation(N)
    out2, stats2, e2 = dr.deposit(p[perm], v[perm], m[perm], LO, HI, DIMS, scheme, dr.ALL)
    assert out.shape == (6, 8, 8, 8) and out.dtype == np.float64
    assert np.array_equal(out.view(np.int64), out2.view(np.int64))
    assert np.array_equal(stats, stats2) and np.array_equal(e, e2)
    assert stats.tolist() == [N, N * (8 if scheme == dr.CIC else 1), 0]
    # the exponent rule: frexp of the largest |q|, the bit length of N
    q = dr.plane_quantities(m, v, dr.ALL)
    want = [int(np.frexp(np.abs(q[k]).max())[1]) + N.bit_length() - 62 for k in range(6)]
    print(f"scheme {scheme}: exponents {e.tolist()}")
    assert e.tolist() == want and e[0] == 1 + 13 - 62


@pytest.mark.parametrize("scheme", [dr.NGP, dr.CIC])
def test_the_total_is_conserved(scheme):
    p, v, m = _gaussian()
    out, stats, e = _reference(scheme)
    total, want = math.fsum(out[1].ravel()), math.fsum(m)
    bound = 0.5 * 2.0 ** int(e[1]) * 8 * N
    print(f"scheme {scheme}: grid sum - sum m = {total - want:.3e}, bound {bound:.3e} (e = {e[1]})")
    assert abs(total - want) <= bound
    assert out[0].sum() == N if scheme == dr.NGP else abs(math.fsum(out[0].ravel()) - N) <= 0.5 * 2.0 ** int(e[0]) * 8 * N


@pytest.mark.parametrize("scheme", [dr.NGP, dr.CIC])
def test_within_the_derived_bound_of_a_float64_deposit(scheme):
    p, v, m = _gaussian()
    out, stats, e = _reference(scheme)
    S, cnt, A = dr.deposit_float(p, v, m, LO, HI, DIMS, scheme, dr.ALL)
    assert cnt.sum() == stats[1]
    for k in range(6):
        bound = 0.5 * 2.0 ** int(e[k]) * cnt + cnt * 2.0 ** -53 * A[k]
        err = np.abs(out[k].ravel() - S[k])
        print(f"scheme {scheme} plane {k}: largest error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert (err <= bound).all()
    assert (S[2:5] < 0).any() and (S[2:5] > 0).any()  # the signed planes are signed


def test_edges_of_the_grid_and_of_the_cells():
    """Bodies on lo, on hi, on interior faces and on lo + h / 2; outside on every side; coordinates of 1e17 and not
    finite ones: which cells take part, by hand."""
    lo, hi, dims = (0.0, 0.0, 0.0), (4.0, 4.0, 4.0), (4, 4, 1)
    rows = [[0.0, 0.5, 0.5],      # on lo: NGP cell 0; CIC s = -0.5: cell -1 dropped, cell 0 gets 0.5
            [4.0, 0.5, 0.5],      # on hi: NGP cell 4 dropped; CIC s = 3.5: cell 3 gets 0.5, cell 4 dropped
            [2.0, 0.5, 0.5],      # on an interior face: NGP cell 2; CIC halves to cells 1 and 2
            [0.5, 0.5, 0.5],      # on lo + h / 2: the CIC fraction is 0, cell 0 whole and cell 1 a contribution of 0
            [-1.0, 0.5, 0.5], [5.0, 0.5, 0.5], [0.5, -1.0, 0.5], [0.5, 5.0, 0.5], [0.5, 0.5, -1.0], [0.5, 0.5, 5.0],
            [1e17, 0.5, 0.5], [0.5, -1e17, 0.5],
            [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5]]
    p = np.array(rows)
    v, m = np.zeros_like(p), np.ones(len(p))
    ngp, st, e = dr.deposit(p, v, m, lo, hi, dims, dr.NGP, dr.MASS)
    want = np.zeros((1, 4, 4))
    want[0, 0, 0], want[0, 0, 2] = 2.0, 1.0
    assert np.array_equal(ngp[0], want) and st.tolist() == [3, 3, 2]
    cic, st, e = dr.deposit(p, v, m, lo, hi, dims, dr.CIC, dr.MASS)
    # y = 0.5 is on lo + h / 2 too: row 0 whole (weight 1), row 1 a contribution of 0; z has one cell (weight 1)
    want = np.zeros((1, 4, 4))
    want[0, 0] = [0.5 + 1.0, 0.5, 0.5, 0.5]
    assert np.array_equal(cic[0], want)
    # contributions: body 0: 1 x 2, body 1: 1 x 2, body 2: 2 x 2, body 3: 2 x 2; x = -1: s = -1.5 -> cells -2, -1: none
    # x = 5: s = 4.5 -> none; y = -1 / 5: none; z outside: none; the 1e17 bodies: none
    assert st.tolist() == [4, 12, 2]


def test_number_under_ngp_is_a_histogram():
    p, v, m = _gaussian()
    lo, hi, dims = (-2.0, -1.5, -1.0), (2.0, 1.0, 3.0), (5, 3, 2)
    out, st, e = dr.deposit(p, v, m, lo, hi, dims, dr.NGP, dr.NUMBER)
    u = [(p[:, a] - lo[a]) * (np.float64(dims[a]) / (np.float64(hi[a]) - np.float64(lo[a]))) for a in range(3)]
    h, _ = np.histogramdd(np.stack([np.floor(u[2]), np.floor(u[1]), np.floor(u[0])], 1),
                          bins=[np.arange(dims[2] + 1) - 0.5, np.arange(dims[1] + 1) - 0.5, np.arange(dims[0] + 1) - 0.5])
    assert np.array_equal(out[0], h) and out[0].sum() == st[0] and 0 < st[0] < N


def test_small_bodies_vanish_and_zero_planes_read_exponent_zero():
    p = np.array([[0.5, 0.5, 0.5]] * 4)
    v = np.array([[1.0, 0.0, 0.0]] * 4)
    m = np.array([1.0, 1e-20, 1.0, 1e-20])
    out, st, e = dr.deposit(p, v, m, (0, 0, 0), (1, 1, 1), (1, 1, 1), dr.NGP, dr.MASS)
    assert out[0, 0, 0, 0] == 2.0 and 1e-20 < 2.0 ** (int(e[0]) - 1)   # below half a quantum: nothing, as the header says
    out, st, e = dr.deposit(p, v, 0.0 * m, (0, 0, 0), (1, 1, 1), (1, 1, 1), dr.CIC, dr.ALL)
    assert e.tolist()[1:] == [0] * 5 and (out[1:] == 0.0).all() and out[0, 0, 0, 0] == 4.0
    out, st, e = dr.deposit(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), (0, 0, 0), (1, 1, 1), (2, 2, 2), dr.CIC, dr.ALL)
    assert out.shape == (6, 2, 2, 2) and (out == 0.0).all() and e.tolist() == [0] * 6 and st.tolist() == [0, 0, 0]
    v[2, 0] = np.inf
    with pytest.raises(ValueError):
        dr.deposit(p, v, m, (0, 0, 0), (1, 1, 1), (1, 1, 1), dr.NGP, dr.MOMENTUM)
    assert dr.deposit(p, v, m, (0, 0, 0), (1, 1, 1), (1, 1, 1), dr.NGP, dr.MASS)[0][0, 0, 0, 0] == 2.0


# ---- nbody/grid.py ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["ngp", "cic"])
def test_power_spectrum_of_one_cosine(scheme):
    from nbody.grid import density_contrast, power_spectrum
    n, L, j, A = 32, 10.0, 5, 0.3
    x = (np.arange(n) + 0.5) * (L / n)
    g = np.broadcast_to(1.0 + A * np.cos(2.0 * np.pi * j * x / L)[None, None, :], (n, n, n))
    d = density_contrast(g)
    assert abs(d.mean()) < 1e-14 and abs(d.max() - A) < 1e-2
    k, pk, modes = power_spectrum(g, L, scheme)
    assert len(k) == len(pk) == len(modes) == n // 2
    power = np.where(modes > 0, pk * modes, 0.0)
    share = power[j - 1] / power.sum()
    print(f"{scheme}: share of the power in the bin of k_j {share:.6f}, k there {k[j - 1]:.4f}")
    assert share > 0.99
    assert abs(k[j - 1] - 2.0 * np.pi * j / L) < 0.5 * 2.0 * np.pi / L
    assert modes[0] == 6 + 12  # |k| in [0.5, 1.5) fundamentals: the 6 axis modes and the 12 face diagonals (1.414)


def test_velocity_maps_two_streams_and_empty_cells():
    from nbody.grid import velocity_maps
    # cell 0: two equal streams +-v0 along x, drifting at w along y; cell 1: empty
    v0, w = 3.0, 0.5
    p = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]])
    v = np.array([[v0, w, 0.0], [-v0, w, 0.0]])
    m = np.array([2.0, 2.0])
    out, st, e = dr.deposit(p, v, m, (0, 0, 0), (2, 1, 1), (2, 1, 1), dr.NGP, dr.MASS | dr.MOMENTUM | dr.KINETIC)
    mean, sigma = velocity_maps({"mass": out[0], "momentum": out[1:4], "kinetic": out[4]})
    assert mean.shape == (3, 1, 1, 2) and sigma.shape == (1, 1, 2)
    assert mean[:, 0, 0, 0].tolist() == [0.0, w, 0.0] and sigma[0, 0, 0] == v0
    assert np.isnan(mean[:, 0, 0, 1]).all() and np.isnan(sigma[0, 0, 1])


def test_map_box_and_surface_density_with_a_stand_in():
    from nbody.grid import map_box, surface_density
    lo, hi, dims = map_box("y", (1.0, 2.0, 3.0), 4.0, 16)
    assert dims == [16, 1, 16] and lo[0] == -3.0 and hi[2] == 7.0 and lo[1] < -1e299 and hi[1] > 1e299
    assert np.isfinite(1.0 / (hi[1] - lo[1]))
    with pytest.raises(ValueError):
        map_box("w")
    p, v, m = _gaussian()
    sim = _StandIn(p, v, m)
    s = surface_density(sim, axis="z", half_width=6.0, pixels=8)
    assert s.shape == (8, 8) and abs(s.sum() * 1.5 * 1.5 - m.sum()) < 1e-9
    thin = surface_density(sim, axis="z", half_width=6.0, pixels=8, depth=0.1)
    assert 0 < thin.sum() < 0.2 * s.sum()


class _StandIn:
    """The backend's deposit() through the restatement: what the helpers and the recorder need of a handle."""
    def __init__(self, p, v, m):
        self.p, self.v, self.m = p, v, m

    def deposit(self, lo, hi, dims, scheme="cic", quantities=("mass",), stats=False):
        assert tuple(quantities) == ("mass",)
        out, st, e = dr.deposit(self.p, self.v, self.m, lo, hi, dims, {"ngp": dr.NGP, "cic": dr.CIC}[scheme], dr.MASS)
        return {"mass": out[0], "exponents": e}


# ---- the recorder ----------------------------------------------------------------------------------------------------
def test_recorder_options_metadata_and_map_files(tmp_path, capsys):
    from tools import record as rec
    parse = rec.build_parser().parse_args
    cfg = rec.build_config(parse(["--preset", "quick_galaxy", "--density-map", "2"]))
    assert cfg["density_map"] == {"every": 2, "pixels": 512, "half_width": 1.5 * cfg["spawn_radius"], "axis": "z"}
    assert "density_map" not in rec.build_config(parse(["--preset", "quick_galaxy"]))
    cfg = rec.build_config(parse(["--preset", "quick_galaxy", "--density-map", "3", "--map-pixels", "64",
                                  "--map-half-width", "250", "--map-axis", "x"]))
    assert rec.density_map_config(cfg) == (3, 64, 250.0, "x")
    for bad in (["--map-pixels", "64"], ["--map-axis", "x"], ["--density-map", "0"], ["--density-map", "2", "--map-pixels", "0"],
                ["--density-map", "2", "--map-half-width", "-1"]):
        with pytest.raises(ValueError):
            rec.build_config(parse(["--preset", "quick_galaxy"] + bad))
    # metadata.json carries the settings: a resume or an extend reads them back
    rec.save_metadata(tmp_path, cfg, 1000.0)
    assert rec.density_map_config(rec.load_metadata(tmp_path)) == (3, 64, 250.0, "x")
    # the writer both loops call: a map where one is due, after the lines, equal to surface_density
    from nbody.grid import surface_density
    p, v, m = _gaussian()
    sim = _StandIn(p, v, m)
    seen = []
    due, write = rec._with_maps(sim, tmp_path, (2, 8, 6.0, "z"), lambda f: f == 0, lambda f: seen.append(f))
    assert [due(f) for f in range(4)] == [True, True, False, True]
    for f in range(6):
        write(f)
    assert seen == list(range(6))
    assert sorted(q.name for q in tmp_path.glob("map_*.npy")) == ["map_000001.npy", "map_000003.npy", "map_000005.npy"]
    got = np.load(tmp_path / "map_000003.npy")
    assert got.dtype == np.float32 and np.array_equal(got, surface_density(sim, half_width=6.0, pixels=8).astype(np.float32))
    assert rec.map_frames(tmp_path, 6) == [1, 3, 5] and rec.map_frames(tmp_path, 5) == [1, 3]
    assert not list(tmp_path.glob(".*.part"))


class MapHandle(Handle):
    """the recorder's stand-in handle with deposit() through the restatement"""
    def deposit(self, lo, hi, dims, scheme="cic", quantities=("mass",), stats=False):
        return _StandIn(self.x, self.v, self.m).deposit(lo, hi, dims, scheme, quantities, stats)


class MapWorld(World):
    def create(self, positions, velocities, masses, G, softening, damping, **kw):
        self.handles.append(MapHandle(self, positions, velocities, masses))
        return self.handles[-1]


MAP_EVERY = 4


def _map_config(name, pipeline=False, frames=FRAMES):
    cfg = _config(name, False, pipeline, frames)
    for key in ("diagnostics_every", "groups", "pairs"):
        del cfg[key]
    cfg["density_map"] = {"every": MAP_EVERY, "pixels": 16, "half_width": 15.0, "axis": "z"}
    return cfg


def _map_frames(d):
    return sorted(int(q.stem.split("_")[1]) for q in d.glob("map_*.npy"))


@pytest.mark.parametrize("pipeline", [False, True])
def test_recorder_session_interrupt_resume_extend_and_status(tmp_path, monkeypatch, capsys, pipeline):
    from nbody.grid import surface_density
    from tools import record as rec
    world = MapWorld(monkeypatch)
    whole = rec.record(_map_config("whole", pipeline), root=tmp_path, quiet=True)
    assert _map_frames(whole) == [f for f in range(FRAMES) if (f + 1) % MAP_EVERY == 0]
    assert not list(whole.glob(".*.part")) and world.handles[0].closed == 1
    # the last map is the surface density of the state after its frame: the stand-in moves on straight lines
    h, last = world.handles[0], _map_frames(whole)[-1]
    cfg = _map_config("whole")
    back = MapHandle(world, h.x - h.v * cfg["dt_per_frame"] * (FRAMES - 1 - last), h.v, h.m)
    want = surface_density(back, half_width=15.0, pixels=16).astype(np.float32)
    got = np.load(whole / f"map_{last:06d}.npy")
    assert want.sum() > 0 and np.allclose(got, want, rtol=0, atol=1e-6 * want.max())
    # an interrupt, then a resume that reads the settings from metadata.json: the same files
    cut_world = MapWorld(monkeypatch)
    cut_world.interrupt_at = 30
    with pytest.raises(KeyboardInterrupt):
        rec.record(_map_config("cut", pipeline), root=tmp_path, quiet=True)
    d = rec.get_recording_dir("cut", tmp_path)
    assert 0 < len(_map_frames(d)) < len(_map_frames(whole))
    rec.record(rec.load_metadata(d), resume=True, root=tmp_path, quiet=True)
    assert _files(d, "map_*") == _files(whole, "map_*")
    # --extend goes on with the same settings
    short = rec.record(_map_config("short", pipeline, frames=FRAMES - 9), root=tmp_path, quiet=True)
    assert rec.extend_recording("short", 9, root=tmp_path) == short
    assert _files(short, "map_*") == _files(whole, "map_*")
    capsys.readouterr()
    assert rec.show_status("short", root=tmp_path)
    out = capsys.readouterr().out
    assert f"Density maps: every {MAP_EVERY} frames, 16 x 16 pixels along z" in out
    assert f"{len(_map_frames(whole))} maps, the last after frame {last}" in out
    # a session without the key writes no map and says nothing about maps
    plain = _map_config("plain", pipeline)
    del plain["density_map"]
    d = rec.record(plain, root=tmp_path, quiet=True)
    assert not list(d.glob("map_*")) and "density_map" not in rec.load_metadata(d)
    capsys.readouterr()
    assert rec.show_status("plain", root=tmp_path) and "Density maps" not in capsys.readouterr().out


def test_header_declares_the_call_and_the_python_table_binds_it():
    import nbmi_native
    text = open(f"{ROOT}/include/nbmi.h").read()
    assert re.search(r"int nbmi_deposit\(nbmi_sim \*sim, const double lo\[3\], const double hi\[3\], const int32_t dims\[3\]", text)
    for name, value in (("NGP", 0), ("CIC", 1), ("NUMBER", 1), ("MASS", 2), ("MOMENTUM", 4), ("KINETIC", 8)):
        assert re.search(rf"#define NBMI_DEPOSIT_{name} {value}\b", text)
    assert len(nbmi_native.PROTOTYPES["nbmi_deposit"][1]) == 9
    from nbody import gpu_backend as gb
    assert gb.DEPOSIT_QUANTITIES == {"number": 1, "mass": 2, "momentum": 4, "kinetic": 8} and gb.DEPOSIT_SCHEMES == {"ngp": 0, "cic": 1}
    # owner-mode handles are refused before the library is called; direct handles are not
    with pytest.raises(ValueError, match="owner-mode"):
        gb.HIPOwnerSimulation._query_refuse(gb.HIPOwnerSimulation, "deposit", tree=False)
    gb.HIPDirectSimulation._query_refuse(gb.HIPDirectSimulation, "deposit", tree=False)
    with pytest.raises(ValueError, match="no tree"):
        gb.HIPDirectSimulation._query_refuse(gb.HIPDirectSimulation, "knn(1)")
