"""Balance mode of the tree walk: the device's cut kernel against its host restatement, and walks on chosen wave times.

In balance mode (from 2 M bodies on by default, NBMI_XCD_BALANCE=2 from 8 walk blocks on) a workgroup of k_walk takes its
logical block from the nine XCD bounds that k_xcd_bounds cut from the previous walk's wave times.  A block that no range
covers keeps the other buffer's stale state, a block two ranges cover is integrated twice: silent either way.  Here

  * nbmi_debug_xcd_bounds runs the product's cut kernel on tables of our choosing and must give xcd_ref.bounds,
  * nbmi_debug_wave_times puts such a table into a live handle, so that the next walk runs on bounds no hardware timing
    would produce (every clamp of the cut rule), and reports how many walks ran balanced - a run that silently fell
    back to the plain mapping fails here, it does not pass,
  * every balanced run has a twin in the same test: a second handle with NBMI_XCD_BALANCE=0 and otherwise the same knobs
    and calls, whose float64 positions and velocities must have the same SHA-256.

Everything is compared exactly.  The knobs NBMI_XCD_CHUNK, NBMI_WALK_BLOCK and NBMI_FUSE_MAXABS decide which workgroup
walks which bodies and which bounds the next build starts from; "speed only, never correctness" is checked the same way.
"""
import contextlib
import ctypes as C
import json
import os

import numpy as np
import pytest

import test_gpu_walk_bits as W
import xcd_ref as X

NBMI_ERR_ARG = -1
ONE_WAVE = {"NBMI_SPLIT_WAVES": "0"}
BALANCED = dict(ONE_WAVE, NBMI_XCD_BALANCE="2")
TWIN = dict(ONE_WAVE, NBMI_XCD_BALANCE="0")
CUT_NB = (8, 9, 15, 16, 17, 1023, 1024, 1025, 2047, 2049, 8192, 39_063)  # chunk 1, 2, 3, 8 and 39; idle threads below 1 024
UNTOUCHED = -77


@pytest.fixture(scope="module")
def recorded():
    with open(W.GOLDEN_PATH) as f:
        return json.load(f)


_inputs = {}


def inputs_for(n, recorded):
    """4 099 bodies: the Plummer sphere of test_gpu_walk_bits; otherwise a galaxy with unequal masses."""
    if n not in _inputs:
        if n == W.N:
            _inputs[n] = W.make_input(recorded["seed"])
        else:
            from tools.presets import generate_distribution
            state = np.random.get_state()
            try:
                np.random.seed(recorded["seed"] + n)
                p, v, m = generate_distribution("galaxy", n, W.RADIUS, W.G)
                m = m * np.random.uniform(0.5, 1.5, n)
            finally:
                np.random.set_state(state)
            _inputs[n] = (p, v, m)
    return _inputs[n]


@contextlib.contextmanager
def handle(env, inputs, prec=None, tau=0.0, integrator="kick_drift", multipole="monopole"):
    """A handle whose knobs stand in the environment from before nbmi_create until it is closed (one of them is read at
    every walk)."""
    from nbody.gpu_backend import HIPBarnesHutSimulation
    knobs = ("NBMI_XCD_BALANCE", "NBMI_SPLIT_WAVES", "NBMI_XCD_CHUNK", "NBMI_WALK_BLOCK", "NBMI_FUSE_MAXABS", "NBMI_WALK_PAIR")
    saved = {k: os.environ.pop(k, None) for k in knobs}
    os.environ.update(env)
    sim = None
    try:
        p, v, m = inputs
        sim = HIPBarnesHutSimulation(p, v, m, W.G, W.EPS, 1.0, W.THETA, integrator=integrator, multipole=multipole)
        if prec == "auto":
            sim.set_force_precision("auto", tau)
        elif prec:
            sim.set_force_precision(prec)
        yield sim
    finally:
        if sim is not None:
            sim.close()
        for k in knobs:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def state_sha(sim):
    return W._sha(sim.get_positions_f64(), sim.get_velocities())


def wave_times(nat, sim, table=None):
    """nbmi_debug_wave_times -> (rc, bounds, nb, jmax, balanced_walks); the outputs start at UNTOUCHED."""
    b = np.full(9, UNTOUCHED, dtype=np.int32)
    nb, jm, walks = C.c_int32(UNTOUCHED), C.c_int32(UNTOUCHED), C.c_int64(UNTOUCHED)
    rc = nat.load().nbmi_debug_wave_times(sim._h, nat.ptr(table), 0 if table is None else table.size, nat.ptr(b),
                                          C.addressof(nb), C.addressof(jm), C.addressof(walks))
    return rc, [int(x) for x in b], nb.value, jm.value, walks.value


def cut_on_device(nat, table, nb=None):
    b = np.full(9, UNTOUCHED, dtype=np.int32)
    jm = C.c_int32(UNTOUCHED)
    rc = nat.load().nbmi_debug_xcd_bounds(len(table) if nb is None else nb, nat.ptr(table), nat.ptr(b), C.addressof(jm))
    return rc, [int(x) for x in b], jm.value


# ---- the cut kernel ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("nb", CUT_NB)
def test_cut_kernel_equals_the_restatement(gpu, nb):
    for name, table in X.patterns(nb):
        rc, got, jm = cut_on_device(gpu, table)
        assert rc == 0, (nb, name, gpu.last_error())
        assert jm == X.jmax(nb), (nb, jm)
        assert got == X.bounds(table), (nb, name)
        assert X.covers_once(got, nb, jm), (nb, name, got)


# ---- walks on injected times ------------------------------------------------------------------------------------------

def stepped_hashes(sim, steps, before_step=None):
    out = []
    for k in range(steps):
        if before_step:
            before_step(k)
        sim.step(W.DT)
        out.append(state_sha(sim))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n,prec,integrator", [(2048, "f32", "kick_drift"), (2049, "f32", "kick_drift"),
                                               (W.N, "f32", "kick_drift"), (W.N, "auto", "kick_drift"),
                                               (W.N, "f32", "leapfrog"), (262_145, "f32", "kick_drift")])
def test_walk_on_injected_times_equals_the_twin(gpu, recorded, n, prec, integrator):
    """Inject a pattern, step, inject the next, step: after every step the bits of the twin, and every walk balanced.
    (A leapfrog handle walks once more than it steps: the first step primes a = F(x) with a walk of its own, which is
    the one that runs on the first injected table; that step's closing walk runs on the cut of the priming walk's
    measured times.)"""
    inputs = inputs_for(n, recorded)
    nb = (n + 255) // 256
    pats = X.patterns(nb)
    kw = dict(prec=prec, tau=recorded["tau"], integrator=integrator)
    with handle(TWIN, inputs, **kw) as twin:
        want = stepped_hashes(twin, len(pats))
        assert wave_times(gpu, twin)[4] == 0
        share = twin.force_precision_share()[0]
    with handle(BALANCED, inputs, **kw) as sim:
        def inject(k):
            name, table = pats[k]
            rc, b, got_nb, jm, _ = wave_times(gpu, sim, table)
            assert rc == 0, gpu.last_error()
            assert (got_nb, jm) == (nb, X.jmax(nb))
            assert b == X.bounds(table), (name, b)
        got = stepped_hashes(sim, len(pats), inject)
        rc, b, _, jm, walks = wave_times(gpu, sim)
        assert rc == 0 and X.covers_once(b, nb, jm), (rc, b)  # (the cut from the last step's measured times)
        assert walks == len(pats) + (1 if integrator == "leapfrog" else 0), walks
        assert sim.force_precision_share()[0] == share
        assert share > 0.0 if prec == "auto" else share == 0.0  # "auto": float64 waves among the balanced ones
    bad = [pats[k][0] for k in range(len(pats)) if got[k] != want[k]]
    assert not bad, f"first differing step: the one on pattern {bad[0]!r} (all: {bad})"


@pytest.mark.gpu
def test_walks_on_measured_times_with_two_blocks_per_thread(gpu, recorded):
    """1 025 blocks: the cut kernel's threads hold 2 blocks each, and from the second step on the walk runs on a cut
    from the hardware's own times.  Their values are the hardware's; that they cover every block once is ours."""
    n, steps = 262_145, 4
    nb = (n + 255) // 256
    inputs = inputs_for(n, recorded)
    with handle(TWIN, inputs, prec="f32") as twin:
        want = stepped_hashes(twin, steps)
    with handle(BALANCED, inputs, prec="f32") as sim:
        rc, b, got_nb, jm, walks = wave_times(gpu, sim)
        assert (rc, b, got_nb, jm, walks) == (0, [-1] * 9, nb, X.jmax(nb), 0)  # nothing cut yet
        got = []
        for k in range(steps):
            sim.step(W.DT)
            rc, b, _, jm, walks = wave_times(gpu, sim)
            print("measured cut after step", k + 1, b)
            assert rc == 0 and walks == k + 1
            assert X.covers_once(b, nb, jm), (k, b)
            got.append(state_sha(sim))
    assert got == want


@pytest.mark.gpu
def test_side_stream_cut_survives_calls_in_between(gpu, recorded):
    """step, accelerations(), diagnostics() with potential, set_state, step on one balanced handle: the second walk waits
    for the cut that the first one left on the side stream, whatever the main stream did since."""
    p, v, m = inputs = inputs_for(W.N, recorded)
    nb = (W.N + 255) // 256
    table = dict(X.patterns(nb))["back_heavy"]

    def session(sim, balanced):
        out = {}
        if balanced:
            rc, b, *_ = wave_times(gpu, sim, table)
            assert rc == 0 and b == X.bounds(table), (rc, b)
        sim.step(W.DT)
        out["acc"] = W._sha(sim.accelerations())
        d = sim.diagnostics(potential=True)
        out["potential"], out["terms"] = float(d.potential).hex(), d.terms
        out["first"] = state_sha(sim)
        sim.set_state(0.9 * p, -v)
        sim.step(W.DT)
        out["second"] = state_sha(sim)
        return out

    with handle(TWIN, inputs, prec="f32") as twin:
        want = session(twin, False)
    with handle(BALANCED, inputs, prec="f32") as sim:
        got = session(sim, True)
        rc, b, _, jm, walks = wave_times(gpu, sim)
        assert rc == 0 and walks == 2 and X.covers_once(b, nb, jm), (rc, walks, b)
    assert got == want


# ---- the gate ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_fewer_than_8_blocks_never_run_balanced(gpu, recorded):
    """1 000 bodies are 4 blocks: the cut rule has no answer for them (tests/test_xcd_bounds_host.py), so the knobs that
    ask for balance mode get the plain mapping, and both hooks refuse."""
    n = 1000
    inputs = inputs_for(n, recorded)
    with handle(TWIN, inputs, prec="f32") as twin:
        want = stepped_hashes(twin, 3)
    with handle(BALANCED, inputs, prec="f32") as sim:
        got = stepped_hashes(sim, 3)
        rc, b, nb, jm, walks = wave_times(gpu, sim)
        assert (rc, b, nb, walks) == (0, [-1] * 9, 4, 0), (rc, b, nb, walks)
        table = np.zeros((4, 4), dtype=np.uint32)
        rc, b, nb, jm, walks = wave_times(gpu, sim, table)
        assert rc == NBMI_ERR_ARG and gpu.last_error().startswith("nbmi_debug_wave_times: fewer than 8"), gpu.last_error()
        assert (b, nb, jm, walks) == ([UNTOUCHED] * 9, UNTOUCHED, UNTOUCHED, UNTOUCHED)
        assert state_sha(sim) == got[-1]
    assert got == want


@pytest.mark.gpu
def test_hooks_refuse_before_they_launch(gpu, recorded):
    table = np.zeros((16, 4), dtype=np.uint32)
    for nb in range(8):
        rc, b, jm = cut_on_device(gpu, table, nb=nb)
        assert rc == NBMI_ERR_ARG and gpu.last_error().startswith("nbmi_debug_xcd_bounds: "), (nb, rc)
        assert b == [UNTOUCHED] * 9 and jm == UNTOUCHED, (nb, b, jm)
    for nb in (-1, -(2 ** 31), 2 ** 31 - 1, 1_500_000_000):  # negative; 8 jmax = 1.5 nb + 8 beyond an int
        rc, b, jm = cut_on_device(gpu, table, nb=nb)
        assert rc == NBMI_ERR_ARG and b == [UNTOUCHED] * 9 and jm == UNTOUCHED, (nb, rc, b)
    lib = gpu.load()
    b = np.full(9, UNTOUCHED, dtype=np.int32)
    jm = C.c_int32(UNTOUCHED)
    assert lib.nbmi_debug_xcd_bounds(16, None, gpu.ptr(b), C.addressof(jm)) == NBMI_ERR_ARG
    assert lib.nbmi_debug_xcd_bounds(16, gpu.ptr(table), None, C.addressof(jm)) == NBMI_ERR_ARG
    assert lib.nbmi_debug_xcd_bounds(16, gpu.ptr(table), gpu.ptr(b), None) == NBMI_ERR_ARG
    assert (b == UNTOUCHED).all() and jm.value == UNTOUCHED
    assert lib.nbmi_debug_wave_times(None, None, 0, gpu.ptr(b), None, None, None) == NBMI_ERR_ARG
    # a live handle: a table of the wrong length, a null output, a sharded handle, a walk block other than 256
    inputs = inputs_for(W.N, recorded)
    nb = (W.N + 255) // 256
    with handle(BALANCED, inputs) as sim:
        short = np.zeros((nb - 1, 4), dtype=np.uint32)
        rc, b, *rest = wave_times(gpu, sim, short)
        assert rc == NBMI_ERR_ARG and "count" in gpu.last_error() and b == [UNTOUCHED] * 9 and rest == [UNTOUCHED] * 3
        assert lib.nbmi_debug_wave_times(sim._h, None, 0, None, None, None, None) == NBMI_ERR_ARG
        sim.set_shard(0, 2048)
        rc, b, *rest = wave_times(gpu, sim)
        assert rc == NBMI_ERR_ARG and "sharded" in gpu.last_error() and b == [UNTOUCHED] * 9 and rest == [UNTOUCHED] * 3
        sim.set_shard(0, W.N)
        assert wave_times(gpu, sim)[0] == 0
    with handle(dict(BALANCED, NBMI_WALK_BLOCK="64"), inputs) as sim:
        rc, b, *rest = wave_times(gpu, sim, np.zeros((4 * ((W.N + 63) // 64)), dtype=np.uint32))
        assert rc == NBMI_ERR_ARG and "walk block" in gpu.last_error() and b == [UNTOUCHED] * 9
        assert wave_times(gpu, sim)[2:] == ((W.N + 63) // 64, X.jmax((W.N + 63) // 64), 0)


# ---- the knobs no other test names --------------------------------------------------------------------------------------

_plain = {}


def plain_run(key, make):
    if key not in _plain:
        _plain[key] = make()
    return _plain[key]


def three_steps(env, inputs, set_state_before_third=False, **kw):
    p, v, _ = inputs
    with handle(env, inputs, **kw) as sim:
        def before(k):
            if k == 2 and set_state_before_third:
                sim.set_state(1.1 * p, 0.5 * v)
        return stepped_hashes(sim, 3, before)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [W.N, 20_000])
@pytest.mark.parametrize("walk", ["one_wave", "split4", "quadrupole"])
@pytest.mark.parametrize("chunk", [-1, 1, 3])
def test_xcd_chunk_changes_no_bit(gpu, recorded, n, walk, chunk):
    """logical_block at its three call sites (k_walk, k_walk_split, k_walk_quad): 17 / 79 blocks of 256 bodies and
    65 / 313 groups of 64, so that chunk 1 and 3 leave a tail behind the last complete round of 8 chunks."""
    inputs = inputs_for(n, recorded)
    env = {"one_wave": ONE_WAVE, "split4": {"NBMI_SPLIT_WAVES": str(((n + 63) // 64) * 4)}, "quadrupole": {}}[walk]
    kw = dict(prec="f32", multipole="quadrupole" if walk == "quadrupole" else "monopole")
    want = plain_run(("chunk", n, walk), lambda: three_steps(env, inputs, **kw))
    assert three_steps(dict(env, NBMI_XCD_CHUNK=str(chunk)), inputs, **kw) == want


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "f64", "auto"])
@pytest.mark.parametrize("block", [64, 128])
def test_walk_block_changes_no_bit(gpu, recorded, prec, block):
    inputs = inputs_for(W.N, recorded)
    kw = dict(prec=prec, tau=recorded["tau"])
    want = plain_run(("block", prec), lambda: three_steps(ONE_WAVE, inputs, **kw))
    assert three_steps(dict(ONE_WAVE, NBMI_WALK_BLOCK=str(block)), inputs, **kw) == want


@pytest.mark.gpu
@pytest.mark.parametrize("walk", ["default", "one_wave"])
def test_unfused_maxabs_changes_no_bit(gpu, recorded, walk):
    """NBMI_FUSE_MAXABS=0: every build finds its bounds with a pass of its own, not from what the last walk published -
    also for the build after a set_state, which must not use a published value either way."""
    inputs = inputs_for(W.N, recorded)
    env = ONE_WAVE if walk == "one_wave" else {}
    want = plain_run(("maxabs", walk), lambda: three_steps(env, inputs, set_state_before_third=True))
    assert three_steps(dict(env, NBMI_FUSE_MAXABS="0"), inputs, set_state_before_third=True) == want
