"""nbmi_radial_profile and nbmi_mass_radii, host side (no device): the NumPy restatement of the header
(tests/profile_ref.py) against an independent plain computation - np.histogram with weights, a brute force over every
candidate radius - and against the properties the header states; the header, the exports and the Python table; the
formulas of nbody/profile.py on hand-made planes; the recorder's --profile options and its line stream with a stand-in
backend."""
import ctypes
import json
import math
import re

import numpy as np
import pytest

import profile_cases as pc
import profile_ref as pr
from conftest import ROOT
from test_record_streams_host import FRAMES, Handle, World, _config, _files

N = 5000
EDGES = pc.edges_for(12, first=0.25, last=6.0)


def _state(seed=3):
    return pc.cloud(N, seed=seed)


_REF = {}


def _reference():
    if "all" not in _REF:
        p, v, m = _state()
        _REF["all"] = pr.radial_profile(p, v, m, pc.CENTER, pc.BULK, EDGES, pr.ALL)
    return _REF["all"]


# ---- the profile ----
def test_profile_within_the_derived_bound_of_a_weighted_histogram():
    """np.histogram on rho = sqrt(r2) with weights q: per slot the error is at most 0.5 * 2^e * (bodies in it) from the
    roundings to the quantum plus count * eps * sum |q| of the float summation; the slots differ from the histogram's
    bins only where sqrt moves a body across an edge, which this cloud does not have (asserted)."""
    p, v, m = _state()
    out, stats, e = _reference()
    q, r2 = pr.body_quantities(p, v, m, pc.CENTER, pc.BULK)
    rho = np.sqrt(r2)
    E = pr.squared_edges(EDGES)
    assert not np.isin(r2, E).any() and not np.isin(rho, EDGES).any()
    bins = np.concatenate([[0.0], EDGES])  # [0, e0), [e0, e1), ... against (.., e0], (e0, e1], ...: equal without ties
    A, cnt = pr.profile_float(p, v, m, pc.CENTER, pc.BULK, EDGES, pr.ALL)
    assert cnt.sum() == stats[0] and stats.tolist() == [int((rho <= EDGES[-1]).sum()), int((rho > EDGES[-1]).sum()), 0]
    assert stats[1] > 0 and (cnt > 0).sum() >= 10
    for k in range(8):
        want, _ = np.histogram(rho, bins=bins, weights=q[k])
        bound = 0.5 * 2.0 ** int(e[k]) * cnt + cnt * 2.0 ** -52 * A[k]
        err = np.abs(out[k] - want)
        print(f"plane {k} ({pr.PLANE_NAMES[k]}): e {e[k]}, largest error / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
        assert (err <= bound).all()
    assert (out[2] < 0).any() and (out[2] > 0).any() and (out[5:] < 0).any()  # the signed planes are signed


def test_number_plane_exact_counts_exponents_and_selections():
    p, v, m = _state()
    out, stats, e = _reference()
    rho = np.sqrt(pr.radii2(p, pc.CENTER)[3])
    want, _ = np.histogram(rho, bins=np.concatenate([[0.0], EDGES]))
    assert np.array_equal(out[0], want) and out[0].sum() == stats[0] and stats.sum() == N
    q, r2 = pr.body_quantities(p, v, m, pc.CENTER, pc.BULK)
    assert e.tolist() == [int(np.frexp(np.abs(q[k]).max())[1]) + N.bit_length() - 62 for k in range(8)] and e[0] == 1 + 13 - 62
    for sel in pr.SINGLE + (pr.MASS | pr.KINETIC, pr.NUMBER | pr.ANGULAR_MOMENTUM):
        one = pr.radial_profile(p, v, m, pc.CENTER, pc.BULK, EDGES, sel)
        rows = pr.planes_of(sel)
        assert pc.same_bits(one[0], out[rows]) and np.array_equal(one[2], e[rows]) and np.array_equal(one[1], stats)
    none = pr.radial_profile(p, v, m, pc.CENTER, None, EDGES, pr.KINETIC)  # no bulk velocity: w = v
    zero = pr.radial_profile(p, v, m, pc.CENTER, (0.0, 0.0, 0.0), EDGES, pr.KINETIC)
    assert pc.same_bits(none[0], zero[0]) and not pc.same_bits(none[0], out[4:5])


def test_a_permuted_input_gives_the_same_bits():
    p, v, m = _state()
    out, stats, e = _reference()
    perm = np.random.RandomState(9).permutation(N)
    out2, stats2, e2 = pr.radial_profile(p[perm], v[perm], m[perm], pc.CENTER, pc.BULK, EDGES, pr.ALL)
    assert pc.same_bits(out, out2) and np.array_equal(stats, stats2) and np.array_equal(e, e2)
    a = pr.mass_radii(p, m, pc.CENTER, pc.FRACTIONS)
    b = pr.mass_radii(p[perm], m[perm], pc.CENTER, pc.FRACTIONS)
    assert pc.same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and pc.same_bits(a[2], b[2]) and a[3:4] == b[3:4] and a[5] == b[5]


@pytest.mark.parametrize("first", [0.0, 1.0])
def test_edge_membership_the_centre_and_skipped_bodies(first):
    """r2 == E[k] belongs to slot k (the upper edge belongs to the shell), just above it to slot k + 1; the centre and,
    with edges[0] == 0, only the centre is in slot 0; NaN and overflowing bodies are skipped, the maxima included"""
    edges = np.array([first, 2.0, 3.0, 4.5, 8.0, 16.0, 17.0])
    c = np.array(pc.CENTER)
    on = np.array([c + [0.0, -e, 0.0] for e in edges])
    above = np.array([c + [0.0, 0.0, e + 2.0 ** -20] for e in edges[1:]])  # (an offset that survives the sum with c)
    assert (pr.radii2(on, c)[3] == edges * edges).all() and (pr.radii2(above, c)[3] > (edges * edges)[1:]).all()
    for k in range(len(edges)):
        one = pr.radial_profile(on[k:k + 1], np.ones((1, 3)), [2.0], c, None, edges, pr.NUMBER | pr.MASS)
        assert one[0][0].tolist() == [1.0 if s == k else 0.0 for s in range(7)] and one[0][1][k] == 2.0 and one[1].tolist() == [1, 0, 0]
    for k in range(len(edges) - 1):
        one = pr.radial_profile(above[k:k + 1], np.ones((1, 3)), [2.0], c, None, edges, pr.NUMBER)
        if k + 2 < len(edges):
            assert one[0][0].tolist() == [1.0 if s == k + 2 else 0.0 for s in range(7)]
        else:
            assert (one[0] == 0.0).all() and one[1].tolist() == [0, 1, 0] and one[2][0] != 0  # beyond: counted, and in the maxima
    centre = pr.radial_profile(c[None, :], [[1.0, 2.0, 3.0]], [2.0], c, None, edges, pr.ALL)
    assert centre[0][:, 0].tolist() == [1.0, 2.0, 0.0, 0.0, 28.0, 0.0, 0.0, 0.0] and (centre[0][:, 1:] == 0.0).all()  # rho == 0: vr = 0
    p = np.concatenate([on, [[np.nan, 0.0, 0.0], [1e200, 0.0, 0.0], [0.0, np.inf, 0.0]]])
    v = np.ones_like(p)
    v[-2] = 1e300  # a skipped body's quantities take no part in the maxima
    got = pr.radial_profile(p, v, np.ones(len(p)), c, None, edges, pr.ALL)
    assert got[1].tolist() == [7, 0, 3] and got[0][0].tolist() == [1.0] * 7
    assert got[2][4] == int(np.frexp(3.0)[1]) + 4 - 62


def test_profile_zero_planes_empty_state_and_refusals():
    p, v, m = pc.cloud(40)
    out, st, e = pr.radial_profile(p, v, 0.0 * m, pc.CENTER, pc.BULK, EDGES, pr.ALL)
    assert e.tolist()[1:] == [0] * 7 and (out[1:] == 0.0).all() and out[0].sum() == st[0]
    out, st, e = pr.radial_profile(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), pc.CENTER, None, EDGES, pr.ALL)
    assert out.shape == (8, 13) and (out == 0.0).all() and e.tolist() == [0] * 8 and st.tolist() == [0, 0, 0]
    m2 = np.where(np.arange(40) % 2 == 0, 1.0, 1e-20)
    out, st, e = pr.radial_profile(p, v, m2, pc.CENTER, pc.BULK, [0.0, 100.0], pr.MASS)
    assert out[0, 1] == 20.0 and 1e-20 < 2.0 ** (int(e[0]) - 1)  # below half a quantum: nothing, as the header says
    for bad in ([1.0], [-1.0, 2.0], [1.0, 1.0], [2.0, 1.0], [1.0, np.nan], [1.0, np.inf], [1.0, 1e200], [1e-170, 2e-170],
                np.arange(258.0)):
        with pytest.raises(ValueError):
            pr.radial_profile(p, v, m, pc.CENTER, None, bad, pr.MASS)
    for q in (0, 64, -1):
        with pytest.raises(ValueError):
            pr.radial_profile(p, v, m, pc.CENTER, None, EDGES, q)
    with pytest.raises(ValueError):
        pr.radial_profile(p, v, m, (np.nan, 0, 0), None, EDGES, pr.MASS)
    with pytest.raises(ValueError):
        pr.radial_profile(p, v, m, pc.CENTER, (0, np.inf, 0), EDGES, pr.MASS)
    v[3, 0] = np.inf
    with pytest.raises(ValueError, match="KINETIC"):
        pr.radial_profile(p, v, m, pc.CENTER, None, EDGES, pr.MASS | pr.KINETIC)
    assert pr.radial_profile(p, v, m, pc.CENTER, None, EDGES, pr.MASS)[0].sum() > 0


# ---- the mass radii ----
def _brute(p, m, center, fractions):
    """every candidate R = a body's own r2, Python integers: the smallest one whose bodies with r2 <= R reach T"""
    r2 = pr.radii2(p, center)[3]
    e, k = pr.mass_quantum(m)
    take = np.isfinite(r2)
    r2, k = r2[take], [int(x) for x in k[take]]
    total = sum(k)
    res = []
    for f in fractions:
        T = max(1, int(math.ceil(float(np.float64(f) * np.float64(total)))))
        best = None
        for R in r2:
            if best is not None and R >= best[0]:
                continue
            inside = r2 <= R
            s = sum(x for x, i in zip(k, inside) if i)
            if s >= T:
                best = (R, int(inside.sum()), s)
        res.append(best)
    return res, total, e


@pytest.mark.parametrize("case", ["cloud", "ties", "spanning"])
def test_mass_radii_against_a_brute_force(case):
    rng = np.random.RandomState(7)
    if case == "cloud":
        p, _, m = pc.cloud(300, seed=7)
    elif case == "ties":  # few distinct radii: bodies at +-x, +-y, +-z enter together
        unit = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
        p = np.array(pc.CENTER) + (rng.randint(1, 9, 50)[:, None, None] * unit[None]).reshape(-1, 3)
        m = np.full(len(p), 0.75)
    else:  # masses over 2^40 and some below the quantum, one body skipped
        p, _, _ = pc.cloud(300, seed=8)
        m = np.exp2(rng.uniform(-40.0, 0.0, 300))
        m[::5] = np.exp2(-80.0)
        p[17, 0] = np.nan
    fractions = list(pc.FRACTIONS) + [k / 8.0 for k in range(1, 9)]
    got = pr.mass_radii(p, m, pc.CENTER, fractions)
    want, total, e = _brute(p, m, pc.CENTER, fractions)
    assert got[5] == e and got[3] == math.ldexp(total, e) and total < 2 ** 53
    for i, w in enumerate(want):
        assert (got[0][i], got[1][i], got[2][i]) == (w[0], w[1], math.ldexp(w[2], e)), (case, fractions[i])
    assert got[4].tolist() == ([299, 1] if case == "spanning" else [len(p), 0])
    r2 = pr.radii2(p, pc.CENTER)[3]
    assert got[0][5] == np.nanmax(r2) and got[1][5] == got[4][0]  # f = 1 gives the largest r2 and everybody taking part
    if case == "ties":  # a run of equal r2 enters together: inside counts whole runs
        assert all(n == (r2 <= R).sum() and n % 6 == 0 for R, n in zip(got[0], got[1]))
        assert len(set(r2.tolist())) <= 8


def test_mass_radii_thresholds_on_cumulative_values_and_empty_cases():
    p = np.array(pc.CENTER) + np.array([[1.0, 0, 0], [2.0, 0, 0], [3.0, 0, 0], [4.0, 0, 0]])
    m = np.ones(4)
    got = pr.mass_radii(p, m, pc.CENTER, [0.25, 0.5, 0.75, 1.0, 0.26, 0.74, 1e-30])
    assert got[0].tolist() == [1.0, 4.0, 9.0, 16.0, 4.0, 9.0, 1.0] and got[1].tolist() == [1, 2, 3, 4, 2, 3, 1]  # T on a sum: that body
    assert got[2].tolist() == [1.0, 2.0, 3.0, 4.0, 2.0, 3.0, 1.0] and got[3] == 4.0 and got[5] == 1 + 3 - 53
    for pp, mm in ((p, 0.0 * m), (np.zeros((0, 3)), np.zeros(0)), (p * np.nan, m)):
        got = pr.mass_radii(pp, mm, pc.CENTER, [0.5, 1.0])
        assert np.isnan(got[0]).all() and got[1].tolist() == [0, 0] and got[2].tolist() == [0.0, 0.0] and got[3] == 0.0
    assert pr.mass_radii(p * np.nan, m, pc.CENTER, [0.5])[4].tolist() == [0, 4]
    for bad in ([], [0.0], [1.5], [np.nan], [-0.5], [0.5] * 65):
        with pytest.raises(ValueError):
            pr.mass_radii(p, m, pc.CENTER, bad)
    for bad in (-1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            pr.mass_radii(p, np.array([1.0, bad, 1.0, 1.0]), pc.CENTER, [0.5])
    # the mass quantum is not the profile's: 9 bits coarser, so that K_total stays below 2^53
    assert pr.mass_quantum(m)[0] - pr.radial_profile(p, 0 * p, m, pc.CENTER, None, [0.0, 9.0], pr.MASS)[2][0] == 9


# ---- the header, the library, the Python table ----
def test_header_declares_library_exports_and_the_python_table_binds_both_calls():
    import nbmi_native
    text = open(f"{ROOT}/include/nbmi.h").read()
    decl = {name: re.search(rf"int {name}\(([^;]*)\);", text) for name in ("nbmi_radial_profile", "nbmi_mass_radii")}
    assert all(decl.values())
    arity = {name: len(re.sub(r"/\*.*?\*/", "", d.group(1), flags=re.S).split(",")) for name, d in decl.items()}
    assert arity == {"nbmi_radial_profile": 9, "nbmi_mass_radii": 10}
    for name, n in arity.items():
        assert len(nbmi_native.PROTOTYPES[name][1]) == n and nbmi_native.PROTOTYPES[name][0] is ctypes.c_int
    for name, value in (("NUMBER", 1), ("MASS", 2), ("RADIAL_MOMENTUM", 4), ("RADIAL_KINETIC", 8), ("KINETIC", 16),
                        ("ANGULAR_MOMENTUM", 32)):
        assert re.search(rf"#define NBMI_PROFILE_{name} {value}\b", text)
    assert "tests/profile_ref.py" in text
    lib = ctypes.CDLL(nbmi_native.LIB_PATH)
    assert lib.nbmi_radial_profile and lib.nbmi_mass_radii
    from nbody import gpu_backend as gb
    assert gb.PROFILE_QUANTITIES == {"number": 1, "mass": 2, "radial_momentum": 4, "radial_kinetic": 8, "kinetic": 16,
                                     "angular_momentum": 32}
    # owner-mode handles are refused before the library is called; direct handles are not
    for what in ("radial_profile", "mass_radii"):
        with pytest.raises(ValueError, match="owner-mode"):
            gb.HIPOwnerSimulation._query_refuse(gb.HIPOwnerSimulation, what, tree=False)
        gb.HIPDirectSimulation._query_refuse(gb.HIPDirectSimulation, what, tree=False)


# ---- nbody/profile.py ----
def test_profile_formulas_on_hand_made_planes():
    from nbody import profile as prof
    e = prof.auto_edges(100.0)
    assert len(e) == 49 and e[0] == 100.0 / 256 and e[-1] == 400.0 and (np.diff(e) > 0).all()
    assert np.allclose(e[1:] / e[:-1], 2.0 ** (10.0 / 48.0)) and len(prof.auto_edges(1.0, shells=3)) == 4
    for bad in ((0.0, 48), (-1.0, 48), (1.0, 0), (1.0, 257), (np.inf, 4)):
        with pytest.raises(ValueError):
            prof.auto_edges(*bad)
    edges = [1.0, 2.0, 4.0]
    vol = prof.shell_volumes(edges)
    assert np.allclose(vol, 4.0 / 3.0 * np.pi * np.array([1.0, 7.0, 56.0])) and prof.shell_volumes([0.0, 1.0])[0] == 0.0
    planes = {"mass": np.array([2.0, 0.0, 4.0]), "radial_momentum": np.array([2.0, 0.0, -4.0]),
              "radial_kinetic": np.array([10.0, 0.0, 8.0]), "kinetic": np.array([34.0, 0.0, 8.0]),
              "angular_momentum": np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 12.0], [4.0, 0.0, -16.0]])}
    rho, enclosed = prof.density_profile(planes, edges)
    assert np.allclose(rho, [2.0 / vol[0], 0.0, 4.0 / vol[2]]) and enclosed.tolist() == [2.0, 2.0, 6.0]
    assert np.isnan(prof.density_profile({"mass": np.array([1.0, 1.0])}, [0.0, 1.0])[0][0])
    vel = prof.velocity_profile(planes)
    # slot 0: <vr> = 1, <vr^2> = 5, <w^2> = 17: sigma_r^2 = 4, sigma_t^2 = 12, beta = 1 - 12 / 8
    assert vel["mean_vr"][0] == 1.0 and vel["sigma_r2"][0] == 4.0 and vel["sigma_t2"][0] == 12.0 and vel["beta"][0] == -0.5
    assert vel["sigma_r"][0] == 2.0 and vel["sigma_t"][0] == math.sqrt(12.0)
    # slot 2: <vr> = -1, <vr^2> = 2 = <w^2>: purely radial, sigma_t^2 = 0 (clamped), beta = 1
    assert vel["mean_vr"][2] == -1.0 and vel["sigma_r2"][2] == 1.0 and vel["sigma_t2"][2] == 0.0 and vel["beta"][2] == 1.0
    assert all(np.isnan(vel[k][1]) for k in vel)  # the empty shell
    j, jm = prof.rotation_profile(planes)
    assert j[:, 0].tolist() == [0.0, 0.0, 2.0] and j[:, 2].tolist() == [0.0, 3.0, -4.0] and jm.tolist()[::2] == [2.0, 5.0]
    assert np.isnan(j[:, 1]).all() and np.isnan(jm[1])

    class Sim:
        def mass_radii(self, fractions, center="com"):
            assert center == "origin"
            return {"radius2": np.array([4.0, 9.0, np.nan])}

        def densities(self, k):
            return np.array([1.0, 3.0, np.inf, 5.0])

        def get_positions_f64(self):
            return np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 8.0], [100.0, 0.0, 0.0], [np.nan, 0.0, 0.0]])
    lr = prof.lagrangian_radii(Sim(), (0.1, 0.5, 0.9), center="origin")
    assert lr[:2].tolist() == [2.0, 3.0] and np.isnan(lr[2])
    assert prof.density_center(Sim(), k=2).tolist() == [3.0, 0.0, 6.0]  # the infinite density and the NaN row are left out


# ---- the recorder ----
def _args(*more):
    from tools import record as rec
    return rec.build_parser().parse_args(["--preset", "quick_galaxy", *more])


def test_recorder_options_and_metadata(tmp_path):
    from nbody.profile import auto_edges
    from tools import record as rec
    assert "profile" not in rec.build_config(_args())  # the default writes no key
    assert rec.LINE_STREAMS.index(rec.PROFILE) == rec.LINE_STREAMS.index(rec.GROUPS) + 1 == rec.LINE_STREAMS.index(rec.PAIRS) - 1
    cfg = rec.build_config(_args("--profile", "5"))
    assert cfg["profile"] == {"every": 5, "edges": [float(x) for x in auto_edges(cfg["spawn_radius"])],
                              "fractions": [0.1, 0.25, 0.5, 0.75, 0.9]}
    assert rec.profile_config(cfg) == (5, cfg["profile"]["edges"], cfg["profile"]["fractions"]) and len(cfg["profile"]["edges"]) == 49
    assert rec.build_config(_args("--profile", "5", "--profile-edges", "AUTO"))["profile"] == cfg["profile"]
    cfg = rec.build_config(_args("--profile", "2", "--profile-edges", "0,1.5,3,6", "--profile-fractions", "0.5,1,0.01"))
    assert cfg["profile"] == {"every": 2, "edges": [0.0, 1.5, 3.0, 6.0], "fractions": [0.5, 1.0, 0.01]}
    assert rec.build_config(_args("--profile", "2", "--pairs", "3"))["pairs"]["every"] == 3
    for bad, word in ((("--profile-edges", "1,2"), "need --profile"), (("--profile-fractions", "0.5"), "need --profile"),
                      (("--profile", "0"), "--profile"), (("--profile", "-2"), "--profile"),
                      (("--profile", "2", "--profile-edges", "1"), "--profile-edges"),
                      (("--profile", "2", "--profile-edges", "2,1"), "--profile-edges"),
                      (("--profile", "2", "--profile-edges", "1,1"), "--profile-edges"),
                      (("--profile", "2", "--profile-edges=-1,1"), "--profile-edges"),
                      (("--profile", "2", "--profile-edges", "1,inf"), "--profile-edges"),
                      (("--profile", "2", "--profile-edges", "1,wide"), "--profile-edges"),
                      (("--profile", "2", "--profile-edges", ",".join(str(k) for k in range(258))), "--profile-edges"),
                      (("--profile", "2", "--profile-fractions", "0"), "--profile-fractions"),
                      (("--profile", "2", "--profile-fractions", "0.5,1.5"), "--profile-fractions"),
                      (("--profile", "2", "--profile-fractions", "half"), "--profile-fractions"),
                      (("--profile", "2", "--profile-fractions", ",".join(["0.5"] * 65)), "--profile-fractions")):
        with pytest.raises(ValueError, match=re.escape(word)):
            rec.build_config(_args(*bad))
    rec.save_metadata(tmp_path, cfg, 1000.0)
    assert rec.profile_config(rec.load_metadata(tmp_path)) == (2, [0.0, 1.5, 3.0, 6.0], [0.5, 1.0, 0.01])
    assert "--profile" in rec.build_parser().format_help() and "--profile-fractions" in rec.build_parser().epilog


class ProfileHandle(Handle):
    """the recorder's stand-in handle with radial_profile() and mass_radii() through the restatement"""
    def _center(self, center):
        d = self.diagnostics(potential=False)
        return np.array(d.center_of_mass) if isinstance(center, str) and center == "com" else np.array(center, dtype=np.float64)

    def radial_profile(self, edges, center="com", bulk_velocity="com", quantities=("number", "mass"), stats=False):
        d = self.diagnostics(potential=False)
        c = self._center(center)
        b = np.array(d.momentum) / d.mass if isinstance(bulk_velocity, str) else np.array(bulk_velocity, dtype=np.float64)
        bits = {"number": 1, "mass": 2, "radial_momentum": 4, "radial_kinetic": 8, "kinetic": 16}
        out, st, e = pr.radial_profile(self.x, self.v, self.m, c, b, edges, sum(bits[q] for q in quantities))
        res = {q: out[i] for i, q in enumerate(q for q in bits if q in quantities)}
        res.update(center=c, bulk_velocity=b, exponents=e)
        return res

    def mass_radii(self, fractions, center="com"):
        c = self._center(center)
        r2, inside, mass, total, st, e = pr.mass_radii(self.x, self.m, c, fractions)
        return {"radius2": r2, "inside": inside, "mass_inside": mass, "total_mass": total, "center": c, "stats": tuple(st), "exponent": e}


class ProfileWorld(World):
    def create(self, positions, velocities, masses, G, softening, damping, **kw):
        self.handles.append(ProfileHandle(self, positions, velocities, masses))
        return self.handles[-1]


PROFILE_EVERY = 4


def _profile_config(name, pipeline=False, frames=FRAMES):
    cfg = _config(name, False, pipeline, frames)
    for key in ("diagnostics_every", "groups", "pairs"):
        del cfg[key]
    cfg["profile"] = {"every": PROFILE_EVERY, "edges": [0.0, 2.0, 5.0, 10.0, 20.0], "fractions": [0.9, 0.5]}
    return cfg


def _lines(d):
    return [json.loads(x) for x in (d / "profile.jsonl").read_text().splitlines()]


@pytest.mark.parametrize("pipeline", [False, True])
def test_recorder_session_interrupt_resume_extend_and_status(tmp_path, monkeypatch, capsys, pipeline):
    from nbody import profile as prof
    from tools import record as rec
    world = ProfileWorld(monkeypatch)
    whole = rec.record(_profile_config("whole", pipeline), root=tmp_path, quiet=True)
    lines = _lines(whole)
    assert [x["frame"] for x in lines] == [f for f in range(FRAMES) if (f + 1) % PROFILE_EVERY == 0]
    assert not list(whole.glob(".*.part")) and world.handles[0].closed == 1
    # the last line describes the state after its frame: the stand-in moves on straight lines
    h, last = world.handles[0], lines[-1]
    cfg = _profile_config("whole")
    back = ProfileHandle(world, h.x - h.v * cfg["dt_per_frame"] * (FRAMES - 1 - last["frame"]), h.v, h.m)
    want = json.loads(rec.profile_line(back, last["frame"], cfg["profile"]["edges"], cfg["profile"]["fractions"]))
    assert sorted(last) == ["beta", "bulk_velocity", "center", "count", "density", "edges", "fractions", "frame",
                            "lagrangian_radii", "mass", "mean_vr", "sigma_r", "sigma_t"]
    assert last["edges"] == cfg["profile"]["edges"] and last["fractions"] == [0.9, 0.5] and sum(last["count"]) > 0
    assert last["count"] == want["count"] and np.allclose(last["mass"], want["mass"], rtol=1e-9)
    assert np.allclose(last["lagrangian_radii"], want["lagrangian_radii"], rtol=1e-9) and last["density"][0] is None  # a ball of radius 0
    got = back.radial_profile(cfg["profile"]["edges"])
    assert np.allclose(last["center"], got["center"], rtol=1e-9, atol=1e-9)
    assert np.allclose(last["lagrangian_radii"], prof.lagrangian_radii(back, [0.9, 0.5]), rtol=1e-9)
    # an interrupt, then a resume that reads the settings from metadata.json: the same file
    cut_world = ProfileWorld(monkeypatch)
    cut_world.interrupt_at = 30
    with pytest.raises(KeyboardInterrupt):
        rec.record(_profile_config("cut", pipeline), root=tmp_path, quiet=True)
    d = rec.get_recording_dir("cut", tmp_path)
    assert 0 < len(_lines(d)) < len(lines)
    rec.record(rec.load_metadata(d), resume=True, root=tmp_path, quiet=True)
    assert _files(d, "profile.jsonl") == _files(whole, "profile.jsonl")
    # --extend goes on with the same settings
    short = rec.record(_profile_config("short", pipeline, frames=FRAMES - 9), root=tmp_path, quiet=True)
    assert rec.extend_recording("short", 9, root=tmp_path) == short
    assert _files(short, "profile.jsonl") == _files(whole, "profile.jsonl")
    capsys.readouterr()
    assert rec.show_status("short", root=tmp_path)
    out = capsys.readouterr().out
    assert f"Profile: every {PROFILE_EVERY} frames, 4 shells from 0 to 20, 2 Lagrangian radii" in out
    assert f"frame {last['frame']}: r(0.5 M) = {last['lagrangian_radii'][1]:.6g}, central density = " in out
    # a session without the key writes no file and says nothing about profiles
    plain = _profile_config("plain", pipeline)
    del plain["profile"]
    d = rec.record(plain, root=tmp_path, quiet=True)
    assert not (d / "profile.jsonl").exists() and "profile" not in rec.load_metadata(d)
    capsys.readouterr()
    assert rec.show_status("plain", root=tmp_path) and "Profile" not in capsys.readouterr().out
