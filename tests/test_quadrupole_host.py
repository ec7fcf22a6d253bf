"""Host half of quadrupole mode: the float64 restatement the GPU tests compare against (a = -grad phi
term by term, the closed-form two-mass case, how much force error the second moments remove on this project's octree and
opening rule), the C-ABI names, the Python refusals that need no device and the recorder's CLI / metadata round trip."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import quadrupole_ref as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("eps", [0.0, 1.5])
def test_term_is_minus_the_gradient_of_its_potential(eps):
    rng = np.random.RandomState(5)
    k = 64
    A = rng.normal(size=(k, 3, 3))
    S = np.einsum("kij,klj->kil", A, A) * 0.3  # symmetric positive semi-definite, like a second moment
    P6 = np.stack([S[:, i, j] for i, j in qr.PAIRS], axis=1)
    gm = rng.uniform(0.5, 2.0, k)
    c = rng.normal(size=(k, 3)) * 3.0
    x = c + rng.normal(size=(k, 3)) * 4.0 + 5.0

    def phi_at(y):
        d = c - y
        return qr.term(d, (d * d).sum(1) + eps * eps, gm, P6)[1]

    d = c - x
    a, _, q, _ = qr.term(d, (d * d).sum(1) + eps * eps, gm, P6)
    h = 1e-4
    grad = np.zeros((k, 3))
    for j in range(3):
        e = np.zeros(3)
        e[j] = h
        grad[:, j] = (phi_at(x + e) - phi_at(x - e)) / (2 * h)
    err = np.abs(a + grad).max(1) / np.abs(a).max(1)
    print(f"eps={eps}: a + grad phi, worst relative {err.max():.2e}; |q|/|a| up to {np.abs(q).max() / np.abs(a).max():.2e}")
    assert err.max() <= 1e-6


def test_two_masses_on_a_line_in_closed_form():
    """Two masses m at +-s on the x axis seen from distance r on that axis, eps = 0: monopole 2 G m / r^2, the
    correction 2 G m 3 s^2 / r^4 towards the pair, and the exact pull G m [(r - s)^-2 + (r + s)^-2] up to O(s^4 / r^6)."""
    G, m, s, r = 0.7, 1.3, 0.2, 9.0
    P6 = np.array([[2 * G * m * s * s, 0, 0, 0, 0, 0.0]])
    d = np.array([[-r, 0.0, 0.0]])  # centre of the pair minus the body at (r, 0, 0)
    a, phi, q, qphi = qr.term(d, np.array([r * r]), np.array([2 * G * m]), P6)
    assert np.allclose(q[0], [-2 * G * m * 3 * s * s / r ** 4, 0, 0], rtol=1e-13, atol=0)
    exact = -G * m * ((r - s) ** -2 + (r + s) ** -2)
    assert abs(a[0, 0] - exact) <= 6 * abs(exact) * (s / r) ** 4
    assert abs(-2 * G * m / r ** 2 - exact) > 100 * abs(a[0, 0] - exact)
    exact_phi = -G * m * (1 / (r - s) + 1 / (r + s))
    assert abs(phi[0] - exact_phi) <= 2 * abs(exact_phi) * (s / r) ** 4


def test_moments_body_by_body_match_the_definition(oracle):
    rng = np.random.RandomState(3)
    n, G = 300, 0.07
    pos = rng.normal(size=(n, 3)) * 40.0
    mass = rng.uniform(0.5, 1.5, n)
    nd, nn = qr.build_tree(oracle, pos, mass)
    P = qr.cell_moments(nd, nn, pos, mass, G)
    # the root holds every body
    d = pos - nd.com[0]
    want = np.array([(G * mass * d[:, i] * d[:, j]).sum() for i, j in qr.PAIRS])
    assert np.allclose(P[0], want, rtol=1e-12, atol=0)
    leaf = nd.leaf[:nn].astype(bool)
    assert not P[leaf].any()
    tp = qr.tol_p(nd, nn, G)
    assert (np.abs(P[~leaf]).max(1) <= tp[~leaf] * 2.0 ** 20 * (1 + 1e-12)).all()  # |P_ab| <= G M (2 hs)^2


def _rms_rel(a, ref):
    e = np.linalg.norm(a - ref, axis=1) / np.linalg.norm(ref, axis=1)
    return float(np.sqrt((e * e).mean()))


CASES = {"galaxy": (800.0, 0.07, 1.5), "collision": (800.0, 0.07, 1.5), "cluster": (300.0, 0.05, 1.0)}


def error_table(oracle, dist, n, thetas, seed=7):
    """{(theta, multipole): (rms relative force error against the float64 direct sum, applied terms per body)}"""
    from tools.presets import generate_distribution
    R, G, eps = CASES[dist]
    np.random.seed(seed)
    p, v, m = generate_distribution(dist, n, R, G)
    p, m = np.ascontiguousarray(p, np.float64), np.ascontiguousarray(m, np.float64)
    ref = oracle.direct_forces(p, m, G, eps)
    tree = qr.build_tree(oracle, p, m)
    P = qr.cell_moments(tree[0], tree[1], p, m, G)
    out = {}
    for theta in thetas:
        for mp in ("monopole", "quadrupole"):
            a = np.zeros((n, 3))
            terms = 0
            for r0 in range(0, n, 4000):  # (chunks of bodies: the frontier of all 20 000 holds 10^7 pairs)
                rows = np.arange(r0, min(n, r0 + 4000))
                w = qr.walk(oracle, p, m, G, eps, theta, tree=tree, rows=rows, multipole=mp, P=P)
                a[rows] = w["a"]
                terms += w["terms"]
            out[(theta, mp)] = (_rms_rel(a, ref), terms / n)
    return out


@pytest.mark.parametrize("dist", ["galaxy", "collision", "cluster"])
def test_second_moments_remove_most_of_the_truncation_error(oracle, dist):
    """DESIGN 4.13's table on the restatement alone, 20 000 bodies; the conditions it meets with room."""
    n = 20_000
    t = error_table(oracle, dist, n, (0.5, 0.7, 0.8))
    for theta in (0.5, 0.7, 0.8):
        mo, qu = t[(theta, "monopole")], t[(theta, "quadrupole")]
        print(f"{dist} {n} theta {theta}: monopole rms {mo[0]:.3e} ({mo[1]:.0f} terms/body), quadrupole {qu[0]:.3e} "
              f"({qu[1]:.0f}), ratio {qu[0] / mo[0]:.3f}")
        assert mo[1] == qu[1]  # the accepted sets are the same
    r5 = t[(0.5, "quadrupole")][0] / t[(0.5, "monopole")][0]
    r8 = t[(0.8, "quadrupole")][0] / t[(0.8, "monopole")][0]
    if dist == "cluster":
        assert r5 <= 0.40 and r8 <= 0.65
        x = t[(0.7, "quadrupole")][0] / t[(0.5, "monopole")][0]
        print(f"   quadrupole theta 0.7 over monopole theta 0.5: {x:.3f}")
        assert x <= 1.25
    else:
        assert r5 <= 0.15 and r8 <= 0.30
        x = t[(0.8, "quadrupole")][0] / t[(0.5, "monopole")][0]
        print(f"   quadrupole theta 0.8 over monopole theta 0.5: {x:.3f}")
        assert x <= 1.0


def test_header_declares_and_library_exports_the_calls():
    import nbmi_native
    from nbody.gpu_backend import MULTIPOLES
    hdr = open(os.path.join(ROOT, "include", "nbmi.h")).read()
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define NBMI_MULTIPOLE_(\w+) (\d+)", hdr)}
    assert codes == MULTIPOLES == {"monopole": 0, "quadrupole": 1}
    names = ("nbmi_set_multipole", "nbmi_get_multipole", "nbmi_get_cell_moments")
    for name in names:
        assert name in nbmi_native.PROTOTYPES and re.search(r"\b%s\(" % name, hdr)
    syms = subprocess.run(["nm", "-D", "--defined-only", nbmi_native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in names:
        assert re.search(r"\bT %s\b" % name, syms), name


def test_python_refusals_without_a_device(monkeypatch):
    from nbody import gpu_backend as gb
    from nbody import sharded
    monkeypatch.setattr(gb._nat, "load", lambda: pytest.fail("a device call before the argument check"))
    x = np.zeros((4, 3))
    with pytest.raises(ValueError, match="multipole must be one of"):
        gb.HIPBarnesHutSimulation(x, x, np.ones(4), 1.0, 0.1, 1.0, 0.5, multipole="octupole")
    with pytest.raises(ValueError, match="multipole must be one of"):
        gb.HIPBarnesHutSimulation.generated("galaxy", 64, 10.0, 1.0, 0.1, 1.0, multipole="octupole")
    with pytest.raises(ValueError, match="monopole"):
        sharded.create_sharded_simulation(x, x, np.ones(4), 1.0, 0.1, 1.0, multipole="quadrupole")
    with pytest.raises(ValueError, match="monopole"):
        sharded.HipShardEngine(x, x, np.ones(4), 1.0, 0.1, 1.0, 0.5, 0, multipole="quadrupole")
    with pytest.raises(ValueError, match="monopole"):
        sharded.HipLetEngine(x, x, np.ones(4), 1.0, 0.1, 1.0, 0.5, 0, 0, 1, multipole="quadrupole")


def test_record_cli_and_metadata_round_trip(tmp_path, capsys):
    from tools import record as rec
    ap = rec.build_parser()
    cfg = rec.build_config(ap.parse_args(["--preset", "quick_galaxy", "--multipole", "quadrupole"]))
    assert cfg["multipole"] == "quadrupole"
    plain = rec.build_config(ap.parse_args(["--preset", "quick_galaxy"]))
    assert "multipole" not in plain  # a default recording's metadata keeps its keys
    assert rec.build_config(ap.parse_args(["--preset", "quick_galaxy", "--multipole", "monopole"]))["multipole"] == "monopole"
    with pytest.raises(SystemExit):
        ap.parse_args(["--preset", "quick_galaxy", "--multipole", "octupole"])
    capsys.readouterr()
    for name, c in (("quad", cfg), ("plain", plain)):
        d = tmp_path / "recordings" / name
        d.mkdir(parents=True)
        rec.save_metadata(d, dict(c, session_name=name), 0.0)
        meta = json.loads((d / "metadata.json").read_text())
        assert meta.get("multipole") == ("quadrupole" if name == "quad" else None)
        assert rec.load_metadata(d).get("multipole", "monopole") == ("quadrupole" if name == "quad" else "monopole")
        assert rec.show_status(name, root=tmp_path)
        out = capsys.readouterr().out
        assert ("Multipole: quadrupole" if name == "quad" else "Multipole: monopole") in out
