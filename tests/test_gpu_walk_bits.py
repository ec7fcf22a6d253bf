"""The tree walks give the same bits as the commit recorded in tests/golden/walk_bits.json.

Every walk kernel shares its opening decision, its float64 monopole, its lane prologue and its launch code with the
others ("Shared pieces of the walks").  The fixture holds, for every case below, one SHA-256 over
the float64 positions and velocities after 3 steps and, where the case asks for them, over accelerations() and
potentials(), plus diagnostics() and the integer walk_counters().  It was written by scripts/gen_walk_bits_golden.py
with the library built at the commit named in the file; a differing hash is a defect of the library under test, never a
reason to write the fixture again.

4 099 bodies: not a multiple of 64 (the last wave has lanes without a body), 65 waves (the per-wave float64 flags
are read beyond one block), and few enough for the split walk (K waves per group when tree groups * K * 2 <=
NBMI_SPLIT_WAVES; 65 groups here).
"""
import hashlib
import json
import os

import numpy as np
import pytest

N = 4099
GROUPS = (N + 63) // 64
G, EPS, THETA, DT, STEPS, RADIUS = 0.15, 2.0, 0.6, 0.05, 3, 500.0
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "walk_bits.json")
ONE_WAVE = {"NBMI_SPLIT_WAVES": "0"}


def _case(env=None, eps=EPS, prec=None, integrator="kick_drift", multipole="monopole", want=()):
    return dict(env=dict(env or {}), eps=eps, prec=prec, integrator=integrator, multipole=multipole, want=tuple(want))


def _cases():
    c = {}
    # one-wave walk: one cursor / two cursors cut in the middle / cut at the wave's home leaf, every force precision
    for pair in (0, 1, 2):
        for prec in ("f32", "f64", "auto"):
            c[f"wave_pair{pair}_{prec}"] = _case(dict(ONE_WAVE, NBMI_WALK_PAIR=str(pair)), prec=prec)
    for prec in ("f32", "f64"):  # softening 0: the guarded instantiations, guard_visit64
        c[f"guard_{prec}"] = _case(ONE_WAVE, eps=0.0, prec=prec)
    for k in (2, 4, 8, 16):  # split walk: seek, the float64 span loop, the offset conversion
        for prec in ("f32", "f64"):
            c[f"split{k}_{prec}"] = _case({"NBMI_SPLIT_WAVES": str(GROUPS * k)}, prec=prec)
    c["leap_wave"] = _case(ONE_WAVE, integrator="leapfrog")
    c["leap_split4"] = _case({"NBMI_SPLIT_WAVES": str(GROUPS * 4)}, integrator="leapfrog")
    for prec in ("f32", "f64"):
        for tag, eps in (("eps", EPS), ("eps0", 0.0)):
            for integ in ("kick_drift", "leapfrog"):
                c[f"quad_{prec}_{tag}_{integ}"] = _case(eps=eps, prec=prec, integrator=integ, multipole="quadrupole",
                                                        want=("acc", "accepts"))
    c["count_eps"] = _case(want=("acc", "counters"))
    c["count_eps0"] = _case(eps=0.0, want=("acc", "counters"))
    for prec in ("f32", "auto"):  # the same bits as wave_pair1_<prec>: BALANCE_TWINS
        c[f"balance_{prec}"] = _case(dict(ONE_WAVE, NBMI_WALK_PAIR="1", NBMI_XCD_BALANCE="2"), prec=prec)
    for mp in ("monopole", "quadrupole"):
        for tag, eps in (("eps", EPS), ("eps0", 0.0)):  # eps 0: the near-pair branch of the potential's decision
            c[f"pot_{mp}_{tag}"] = _case(eps=eps, multipole=mp, want=("phi", "diag"))
    return c


CASES = _cases()
BALANCE_TWINS = {"balance_f32": "wave_pair1_f32", "balance_auto": "wave_pair1_auto"}
SPLIT_TWINS = {f"split{k}_{prec}": f"wave_pair1_{prec}" for k in (2, 4, 8, 16) for prec in ("f32", "f64")}
COUNTERS = ("wave_visits", "lane_visits", "lane_accepts", "jumps", "band_visits")  # (xcd_visits: where a wave ran)


def make_input(seed):
    """Plummer sphere (its core is dense against its halo) with unequal masses, drawn on the host."""
    from tools.presets import generate_distribution
    state = np.random.get_state()
    try:
        np.random.seed(seed)
        p, v, m = generate_distribution("cluster", N, RADIUS, G)
        m = m * np.random.uniform(0.5, 1.5, N)
    finally:
        np.random.set_state(state)
    return p, v, m


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        assert a.dtype == np.float64
        h.update(a.tobytes())
    return h.hexdigest()


def run_case(case, inputs, tau):
    """Everything the fixture holds for one case, computed by the library that nbmi_native loads.  The case's knobs
    are in the environment from before nbmi_create until the handle is closed."""
    from nbody.gpu_backend import HIPBarnesHutSimulation
    p, v, m = inputs
    saved = {k: os.environ.get(k) for k in case["env"]}
    os.environ.update(case["env"])
    sim = None
    try:
        sim = HIPBarnesHutSimulation(p, v, m, G, case["eps"], 1.0, THETA, integrator=case["integrator"],
                                     multipole=case["multipole"])
        if case["prec"] == "auto":
            sim.set_force_precision("auto", tau)
        elif case["prec"]:
            sim.set_force_precision(case["prec"])
        out = {}
        want = case["want"]
        if "acc" in want:
            out["acc"] = _sha(sim.accelerations())
            wc = sim.walk_counters()
            if "counters" in want:
                out["counters"] = {k: wc[k] for k in COUNTERS}
                out["counters"]["window_misses"] = {str(k): n for k, n in wc["window_misses"].items()}
            else:
                out["accepts"] = wc["lane_accepts"]
        if "phi" in want:
            out["phi"] = _sha(sim.potentials())
            d = sim.diagnostics()
            out["terms"] = d.terms
            out["potential"] = float(d.potential).hex()
        for _ in range(STEPS):
            sim.step(DT)
        if case["prec"] == "auto":
            out["share"] = sim.force_precision_share()[0]
        out["state"] = _sha(sim.get_positions_f64(), sim.get_velocities())
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
def inputs(recorded):
    return make_input(recorded["seed"])


@pytest.fixture(scope="module")
def computed():
    return {}


def test_fixture_covers_every_case(recorded):
    assert sorted(recorded["cases"]) == sorted(CASES)
    assert len(recorded["commit"]) == 40
    assert recorded["cases"]["count_eps"]["counters"]["band_visits"] > 0  # the float64 re-decision is reached
    for twin_of in (BALANCE_TWINS, SPLIT_TWINS):
        assert set(twin_of) | set(twin_of.values()) <= set(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_same_bits_as_recorded(gpu, recorded, inputs, computed, name):
    got = run_case(CASES[name], inputs, recorded["tau"])
    computed[name] = got
    share = got.pop("share", None)
    if share is not None:
        assert 0.0 < share < 1.0, share  # some waves in float64, some in fp32
    want = recorded["cases"][name]
    print(name, got)
    assert got == want


@pytest.mark.gpu
def test_balance_mode_changes_no_bit_and_split_changes_the_last(gpu, recorded, inputs, computed):
    def state(name):
        if name not in computed:
            computed[name] = run_case(CASES[name], inputs, recorded["tau"])
        return computed[name]["state"]
    for name, twin in BALANCE_TWINS.items():
        assert state(name) == state(twin), (name, twin)
    for name, twin in SPLIT_TWINS.items():  # the split cases really ran split: their sums associate differently
        assert state(name) != state(twin), (name, twin)
