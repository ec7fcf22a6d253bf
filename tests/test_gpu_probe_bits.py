"""The float64 probe family - potentials, nbmi_field_at, nbmi_tidal_at, nbmi_get_tidal_f64, tracers, on a tree and by
the direct sums - gives the bits recorded in tests/golden/probe_bits.json.

The tree calls share one walk (field_walk), one probe scratch and one side-tree helper, the direct
calls one tile loop (DESIGN.md sections 4.9, 4.18, 4.19, 4.27), so a test that compares the field with the potential, or
tidal() with tidal_at(), compares a function with itself.  The fixture pins the family to
the commit named in the file instead: for every case below a SHA-256 over the bytes of each float64 array and the int32
term counts as they are.  It was written by scripts/gen_probe_bits_golden.py with the library built at that commit; a
differing value is a defect of the library under test, never a reason to write the fixture again.  A lane's result
depends on the probe and the tree alone (section 4.18), not on chunks or wave membership, so the fixture is stable.

4 097 bodies: 65 waves, more than one block, and the last wave holds one body.  Softening 0 puts the band at its cap,
where the near-pair rule of the walk is live.  The points of a field call: row 0 is a body's position, then bodies'
positions, points inside the root cube and points far outside it in turn - a call of one point has pmax <= maxabs (the
band of the build), every longer call pmax > maxabs (the widened band).
"""
import hashlib
import json
import os

import numpy as np
import pytest

N = 4097
G, EPS, THETA, DT, STEPS, RADIUS = 0.15, 2.0, 0.6, 0.05, 10, 500.0
FIELD_M = (1, 64, 65, 1000)
TRACER_M = (65, 1000)
DISTS = {"galaxy": 11, "cluster": 12}  # distribution -> seed
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probe_bits.json")
MORTON = {"NBMI_HILBERT": "0"}
UNSORTED = {"NBMI_FIELD_SORT": "0"}


def _cases():
    c = {}
    for dist in DISTS:
        for mp in ("monopole", "quadrupole"):
            for curve, env in (("hilbert", {}), ("morton", MORTON)):
                for tag, eps in (("eps", EPS), ("eps0", 0.0)):
                    c[f"field_{dist}_{mp}_{curve}_{tag}"] = dict(kind="field", dist=dist, multipole=mp, env=env, eps=eps)
                    c[f"tidal_{dist}_{mp}_{curve}_{tag}"] = dict(kind="tidal", dist=dist, multipole=mp, env=env, eps=eps)
    c["field_unsorted"] = dict(kind="field", dist="galaxy", multipole="monopole", env=UNSORTED, eps=EPS)
    c["tidal_unsorted"] = dict(kind="tidal", dist="galaxy", multipole="monopole", env=UNSORTED, eps=EPS)
    for dist in DISTS:  # the direct sums: the potential's tile loop, the probes' and the tidal tensor's
        for tag, eps in (("eps", EPS), ("eps0", 0.0)):
            c[f"direct_{dist}_{tag}"] = dict(kind="direct", dist=dist, multipole="monopole", env={}, eps=eps, direct=True)
    for mp in ("monopole", "quadrupole"):
        for integ in ("kick_drift", "leapfrog"):
            for m in TRACER_M:
                c[f"tracers_{mp}_{integ}_{m}"] = dict(kind="tracers", dist="galaxy", multipole=mp, env={}, eps=EPS,
                                                      integrator=integ, m=m, direct=False)
    c["tracers_eps0"] = dict(kind="tracers", dist="cluster", multipole="monopole", env={}, eps=0.0, integrator="kick_drift",
                             m=1000, direct=False)
    c["tracers_morton"] = dict(kind="tracers", dist="cluster", multipole="quadrupole", env=MORTON, eps=EPS,
                               integrator="leapfrog", m=1000, direct=False)
    c["tracers_unsorted"] = dict(kind="tracers", dist="galaxy", multipole="monopole", env=UNSORTED, eps=EPS,
                                 integrator="kick_drift", m=1000, direct=False)
    for integ in ("kick_drift", "leapfrog"):
        for m in TRACER_M:
            c[f"tracers_direct_{integ}_{m}"] = dict(kind="tracers", dist="galaxy", multipole="monopole", env={}, eps=EPS,
                                                    integrator=integ, m=m, direct=True)
    return c


CASES = _cases()
# the order of the walk decides speed, never a bit
SORT_TWINS = {"field_unsorted": "field_galaxy_monopole_hilbert_eps", "tidal_unsorted": "tidal_galaxy_monopole_hilbert_eps",
              "tracers_unsorted": "tracers_monopole_kick_drift_1000"}


def make_input(dist):
    """(pos, vel, mass, points, tracer velocities) of one distribution: float64, drawn on the host, read-only"""
    from tools.presets import generate_distribution
    state = np.random.get_state()
    try:
        np.random.seed(DISTS[dist])
        p, v, m = generate_distribution(dist, N, RADIUS, G)
    finally:
        np.random.set_state(state)
    pos, vel, mass = (np.ascontiguousarray(a, np.float64) for a in (p, v, m))
    rng = np.random.default_rng(DISTS[dist])
    mmax = max(FIELD_M)
    bounds = np.abs(pos).max() * 1.1 + 10.0  # the root cube's half size
    u = rng.normal(size=(mmax, 3))
    u /= np.sqrt((u * u).sum(1))[:, None]
    far = np.where(np.arange(mmax)[:, None] % 2 == 0, 3.0, 100.0) * bounds * u
    pts = np.where(np.arange(mmax)[:, None] % 3 == 0, pos[rng.choice(N, mmax, replace=False)],
                   np.where(np.arange(mmax)[:, None] % 3 == 1, far, rng.uniform(-bounds, bounds, (mmax, 3))))
    tv = rng.normal(size=(mmax, 3)) * 0.3
    out = (pos, vel, mass, np.ascontiguousarray(pts), tv)
    for a in out:
        a.setflags(write=False)
    return out


def _sha(a, dtype=np.float64):
    a = np.ascontiguousarray(a)
    assert a.dtype == dtype
    return hashlib.sha256(a.tobytes()).hexdigest()


def run_case(case, inputs):
    """Everything the fixture holds for one case, computed by the library that nbmi_native loads.  The case's knobs are
    in the environment from before nbmi_create until the handle is closed."""
    from nbody.gpu_backend import HIPBarnesHutSimulation, HIPDirectSimulation
    pos, vel, mass, pts, tv = inputs
    saved = {k: os.environ.get(k) for k in case["env"]}
    os.environ.update(case["env"])
    sim = None
    try:
        if case.get("direct"):
            sim = HIPDirectSimulation(pos, vel, mass, G, case["eps"], 1.0, integrator=case.get("integrator", "kick_drift"))
        else:
            sim = HIPBarnesHutSimulation(pos, vel, mass, G, case["eps"], 1.0, THETA, multipole=case["multipole"],
                                         integrator=case.get("integrator", "kick_drift"))
        out = {}
        if case["kind"] in ("tidal", "direct"):
            t6, norm = sim.tidal(norm=True)
            out["t6_bodies"], out["norm_bodies"] = _sha(t6), _sha(norm)
            for m in FIELD_M:
                t6, terms = sim.tidal_at(pts[:m], terms=True)
                assert terms.dtype == np.int32
                out[f"tidal_m{m}"] = {"t6": _sha(t6), "terms": [int(t) for t in terms]}
        if case["kind"] in ("field", "direct"):
            out["phi_bodies"] = _sha(sim.potentials())
            d = sim.diagnostics()
            out["terms_bodies"] = d.terms
            out["potential"] = float(d.potential).hex()
            for m in FIELD_M:
                acc, phi, terms = sim.field_at(pts[:m], terms=True)
                assert terms.dtype == np.int32
                out[f"m{m}"] = {"acc": _sha(acc), "phi": _sha(phi), "terms": [int(t) for t in terms]}
        if case["kind"] == "tracers":
            m = case["m"]
            sim.set_tracers(pts[:m], tv[:m])
            for _ in range(STEPS):
                sim.step(DT)
            p, v = sim.get_tracers()
            out["positions"], out["velocities"] = _sha(p), _sha(v)
            out["moved"] = int((p != pts[:m]).any(axis=1).sum())
        return out
    finally:
        if sim is not None:
            sim.close()
        for k, old in saved.items():
            if old is None:
                del os.environ[k]
            else:
                os.environ[k] = old


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN_PATH) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def inputs():
    return {dist: make_input(dist) for dist in DISTS}


def test_fixture_covers_every_case(recorded):
    assert sorted(recorded["cases"]) == sorted(CASES)
    assert len(recorded["commit"]) == 40
    assert (recorded["n"], recorded["steps"]) == (N, STEPS)
    assert set(SORT_TWINS) | set(SORT_TWINS.values()) <= set(CASES)
    for name, twin in SORT_TWINS.items():
        assert recorded["cases"][name] == recorded["cases"][twin], (name, twin)
    for name, case in CASES.items():
        got = recorded["cases"][name]
        if case["kind"] in ("field", "direct"):
            assert all(len(got[f"m{m}"]["terms"]) == m and min(got[f"m{m}"]["terms"]) > 0 for m in FIELD_M), name
        if case["kind"] == "tidal":  # the tensor's walk accepts what the field's accepts
            field = recorded["cases"]["field" + name[len("tidal"):]]
            assert all(got[f"tidal_m{m}"]["terms"] == field[f"m{m}"]["terms"] for m in FIELD_M), name
        if case["kind"] == "direct":
            assert all(got[f"tidal_m{m}"]["terms"] == got[f"m{m}"]["terms"] for m in FIELD_M), name
        if case["kind"] == "tracers":
            assert got["moved"] == case["m"], name  # every tracer was carried


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_same_bits_as_recorded(gpu, recorded, inputs, name):
    got = run_case(CASES[name], inputs[CASES[name]["dist"]])
    want = recorded["cases"][name]
    for key in sorted(want):  # every figure before the assertion
        print(name, key, "same" if got.get(key) == want[key] else f"differs: {got.get(key)} != {want[key]}")
    assert got == want
