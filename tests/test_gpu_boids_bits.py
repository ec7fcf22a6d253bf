"""The boids sweep and the flock analysis give the bits recorded in tests/golden/boids_bits.json.

tests/test_gpu_boids_sweep.py holds the metric sweep's `sep` to boids_ref.sep_bound only, because the kernel sums its
separation terms in another order than the reference: a change that reorders the candidates of `k_flock` would pass it.
The fixture pins the order instead: for every case below a SHA-256 over the raw bytes of the four arrays of
bdmi_get_forces on the initial state, of the state after STEPS steps, of bdmi_neighbour_stats' counts and nn_d2 and of
bdmi_flocks' labels, with the link and evaluation counts as they are.  It was written by scripts/gen_boids_bits_golden.py
with the library built at the commit named in the file; a differing value is a defect of the library under test, never a
reason to write the fixture again.  A boid's sums depend on the cell order alone (a stable sort by cell of the row order),
not on blocks or timing, so the fixture is stable.

The cases are the smallest of tests/boids_cases.py and tests/slab_cases.py at which each path of the sweep is live:
  run_length_4095 / _4096  the last run whose offsets fit the 16-bit notes, and the first that takes its candidates one by one
  mixed_lanes              both kinds of lane in one wave
  hit_list                 more than 32 neighbours: the hit list is flushed in the middle of the walk
  grid_32 / grid_33        rows inside one occupancy word, and rows that straddle two
  grid_3                   every row clipped in x, y and z
  thresholds               distances at the perception and separation radii and at the 0.0001 floor
  slab_faces_3             three slab handles, the middle one with ghosts on both faces (the ghost branch of the sweep);
                           the stepped state only: the analysis calls are refused on slabs
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import boids_cases as BC
import slab_cases as SC

STEPS = 3
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boids_bits.json")
CASES = {
    "run_length_4095": lambda: BC.run_length(4095),
    "run_length_4096": lambda: BC.run_length(4096),
    "mixed_lanes": BC.mixed_lanes,
    "hit_list": BC.hit_list,
    "grid_32": lambda: BC.grid_dims(32),
    "grid_33": lambda: BC.grid_dims(33),
    "grid_3": lambda: BC.grid_dims(3),
    "thresholds": BC.thresholds,
    "slab_faces_3": lambda: SC.faces(3),
}
FLOCK_KEYS = ("sep", "ali", "coh", "avg", "positions", "velocities", "colours", "nb_count", "nb_nn_d2", "nb_evals",
              "labels", "n_flocks", "links", "evals")
SLAB_KEYS = ("state",)


def _sha(a, dtype=np.float64):
    a = np.ascontiguousarray(a)
    assert a.dtype == dtype
    return hashlib.sha256(a.tobytes()).hexdigest()


def _run_flock(nat, c):
    from test_gpu_boids import RawFlock
    prm = c["params"]
    f = RawFlock(nat, c["pos"], c["vel"], c["col"], prm)
    try:
        lib, n, out = f.lib, f.n, {}
        for key, a in zip(("sep", "ali", "coh", "avg"), f.forces()):
            out[key] = _sha(a)
        # the widest radius the calls take (the perception radius = the cell) and the separation radius as the link
        count, nn, ev = np.full(n, -7, dtype=np.int32), np.full(n, -7.0), C.c_int64(-7)
        nat.check(lib.bdmi_neighbour_stats(f.h, float(prm[5]), nat.ptr(count), nat.ptr(nn), C.addressof(ev)),
                  "bdmi_neighbour_stats")
        out["nb_count"], out["nb_nn_d2"], out["nb_evals"] = _sha(count, np.int32), _sha(nn), int(ev.value)
        labels, res = np.full(n, -7, dtype=np.int32), [C.c_int64(-7) for _ in range(3)]
        nat.check(lib.bdmi_flocks(f.h, float(min(prm[5], prm[6])), nat.ptr(labels), *[C.addressof(x) for x in res]),
                  "bdmi_flocks")
        out["labels"] = _sha(labels, np.int32)
        out["n_flocks"], out["links"], out["evals"] = (int(x.value) for x in res)
        f.step(c["dt"], STEPS)
        for key, a in zip(("positions", "velocities", "colours"), f.state()):
            out[key] = _sha(a)
        return out
    finally:
        f.close()


def _run_slab(nat, c):
    import test_gpu_boids_slab as TS
    engs = TS._engines(nat, c)
    try:
        for _ in range(STEPS):
            TS._exchange(engs)
            for e in engs:
                e.op_step(c["dt"])
        state, _ = TS._gather(engs, len(c["pos"]))
        return {"state": _sha(state)}
    finally:
        TS._close(engs)


def run_case(nat, name):
    """Everything the fixture holds for one case, computed by the library that nbmi_native loads."""
    c = CASES[name]()
    return _run_slab(nat, c) if name.startswith("slab_") else _run_flock(nat, c)


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN_PATH) as f:
        return json.load(f)


def test_fixture_covers_every_case(recorded):
    assert sorted(recorded["cases"]) == sorted(CASES)
    assert len(recorded["commit"]) == 40 and recorded["steps"] == STEPS
    for name, got in recorded["cases"].items():
        assert sorted(got) == sorted(SLAB_KEYS if name.startswith("slab_") else FLOCK_KEYS), name
    # the two run lengths are different inputs, and both were recorded
    assert recorded["cases"]["run_length_4095"] != recorded["cases"]["run_length_4096"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_same_bits_as_recorded(gpu, recorded, name):
    got = run_case(gpu, name)
    want = recorded["cases"][name]
    for key in sorted(want):  # every figure before the assertion
        print(name, key, "same" if got.get(key) == want[key] else f"differs: {got.get(key)} != {want[key]}")
    assert got == want
