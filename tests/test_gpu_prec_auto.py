"""Force precision "auto" on the device against its host restatement (tests/prec_ref.py; the rule: include/nbmi.h at
nbmi_set_force_precision).

Every comparison of a count is exact.  It can be: the thresholds come from prec_ref.thresholds / pick_thresholds, which
hand out only numbers at least 1e-4 (relative) from every wave value of the input, while fp32 rounding moves a wave
value by less than 6.6e-7 (tests/test_prec_ref_host.py asserts both for every input used here).  With dt = 2^-10 the
device's (float)(tau / dt^2) is the fp32 threshold bit for bit.

Unless stated otherwise: the "cluster" input of prec_ref.cluster_input, G 0.15, softening 2, theta 0.6, velocities 0,
dt = 2^-10, one step per measurement."""
import os

import numpy as np
import pytest

import prec_ref as R

pytestmark = pytest.mark.gpu

THETA = 0.6
DT = 2.0 ** -10
N = 4099


class _Env:
    def __init__(self, **env):
        self.env = {k: str(v) for k, v in env.items()}

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, old in self.saved.items():
            if old is None:
                del os.environ[k]
            else:
                os.environ[k] = old


def _sim(p, v, m, eps=R.EPS, **kw):
    from nbody.gpu_backend import HIPBarnesHutSimulation
    return HIPBarnesHutSimulation(p, v, m, R.G, eps, 1.0, THETA, **kw)


class Case:
    """An input with the host's key order and wave values (computed once, never changed)."""

    def __init__(self, p, v, m, eps=R.EPS):
        self.p, self.v, self.m, self.eps = p, v, m, eps
        self.zero = np.zeros_like(p)
        self.n = len(p)
        self.order = R.key_order(p)
        self.D = R.wave_values(p, m, R.G, eps, self.order)
        self.waves = (self.n + 63) // 64
        for a in (self.p, self.v, self.m, self.zero, self.order, self.D):
            a.setflags(write=False)

    def with_masses(self, m, eps=None):
        return Case(self.p.copy(), self.v.copy(), np.array(m, dtype=np.float64), self.eps if eps is None else eps)

    def count(self, thr):
        return int((self.D > np.float64(np.float32(thr))).sum())

    def open(self):
        """A handle at rest on this input whose device key order is the host's."""
        sim = _sim(self.p, self.zero, self.m, self.eps)
        sim.build_tree()
        assert np.array_equal(sim.key_order(), self.order)
        return sim

    def measure(self, sim, thr, dt=DT):
        """(share, all64) of one step from this input's positions at rest, at the fp32 threshold thr."""
        R.check_margins([thr], self.D)
        sim.set_state(self.p, self.zero)
        sim.set_force_precision("auto", R.tau_for(thr, dt))
        sim.step(dt)
        return sim.force_precision_share()

    def want(self, thr):
        """(share, all64) the rule gives for a first step at thr."""
        c = self.count(thr)
        return c / self.waves, bool(R.all64_rule(0, c, self.waves))


@pytest.fixture(scope="module")
def cluster(gpu):
    return Case(*R.cluster_input(N))


@pytest.fixture(scope="module")
def cluster64(gpu):
    return Case(*R.cluster_input(4096))


# ---- 1. sweep ------------------------------------------------------------------------------------------------------
def test_sweep_pins_every_wave_value(cluster):
    """66 thresholds, one between every two adjacent wave values of the host: the device's count at each is the host's,
    so the sorted list of the device's 65 values interleaves with the host's."""
    thr = R.thresholds(cluster.D)
    assert len(thr) == 66 and [cluster.count(t) for t in thr] == list(range(65, -1, -1))
    sim = cluster.open()
    try:
        got = [cluster.measure(sim, t) for t in thr]
    finally:
        sim.close()
    want = [cluster.want(t) for t in thr]
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert [w[1] for w in want] == [c > 21 for c in range(65, -1, -1)]  # 1000 * 22 > 333 * 65 > 1000 * 21


# ---- 2. sizes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SIZES)
def test_group_wave_round_and_tile_edges(gpu, n):
    """Ragged groups (n % 16), ragged waves, the 256-rank round and the 2 048-rank tile with one body more and less,
    and the round that starts at r0 == n."""
    case = Case(*R.cluster_input(n))
    thr = R.thresholds(case.D)
    picks = [thr[0], thr[-1]] + ([thr[len(thr) // 2]] if case.waves >= 2 else [])
    sim = case.open()
    try:
        for t in picks:
            assert case.measure(sim, t) == case.want(t), (n, t, case.count(t))
    finally:
        sim.close()
    assert case.count(thr[0]) == case.waves and case.count(thr[-1]) == 0


# ---- 3. group and lane isolation ------------------------------------------------------------------------------------
def _rank_of(case):
    rank = np.empty(case.n, dtype=np.int64)
    rank[case.order] = np.arange(case.n)
    return rank


ISOLATION = ["quarter0", "quarter1", "quarter2", "quarter3", "diagonal"]


@pytest.mark.parametrize("which", ISOLATION)
def test_mass_in_one_group_or_one_lane_per_group(cluster, which):
    """Masses do not move keys.  quarter q: mass only in group q of every wave - a max over the groups that skips one
    (a missing __shfl_xor) loses those waves.  diagonal: one massive body per group, at lane (group index) % 16 - a
    row reduction that misses a lane loses that group's sum."""
    rank = _rank_of(cluster)
    mask = rank % 16 == (rank // 16) % 16 if which == "diagonal" else (rank % 64) // 16 == int(which[-1])
    case = cluster.with_masses(np.where(mask, cluster.m, 0.0))
    assert np.array_equal(case.order, cluster.order)
    thr = R.pick_thresholds(case.D, 8)
    assert len(thr) == 8
    sim = case.open()
    try:
        got = [case.measure(sim, t) for t in thr]
    finally:
        sim.close()
    assert got == [case.want(t) for t in thr], (got, [case.count(t) for t in thr])


def test_no_mass_no_float64(cluster):
    """All masses 0 (nbmi_create accepts them): every group's dens is 0 by definition, whatever its box."""
    case = cluster.with_masses(np.zeros(N))
    assert np.all(case.D == 0.0)
    sim = case.open()
    try:
        for t in R.pick_thresholds(cluster.D, 3):
            sim.set_state(case.p, case.zero)
            sim.set_force_precision("auto", R.tau_for(t, DT))
            sim.step(DT)
            assert sim.force_precision_share() == (0.0, False)
    finally:
        sim.close()


# ---- 4. the softening floor and degenerate boxes -------------------------------------------------------------------
FINITE = [np.float32(1e-30), np.float32(1.0), np.float32(1e30)]


def _shares(case, thrs, tau_dt=None):
    sim = case.open()
    try:
        out = []
        for t in thrs:
            sim.set_state(case.p, case.zero)
            tau, dt = tau_dt if tau_dt else (R.tau_for(t, DT), DT)
            sim.set_force_precision("auto", tau)
            sim.step(dt)
            out.append(sim.force_precision_share())
        return out
    finally:
        sim.close()


def test_planar_bodies_without_softening_have_infinite_density(gpu):
    case = Case(*R.planar_input(), eps=0.0)
    assert case.waves == 16 and np.all(np.isinf(case.D))
    assert _shares(case, FINITE) == [(1.0, True)] * 3
    # no mass: 0, not 0 / 0
    assert _shares(case.with_masses(np.zeros(case.n)), FINITE) == [(0.0, False)] * 3
    # tau / dt^2 = 1e60 becomes +inf in fp32, and inf > inf is false
    assert _shares(case, [None], tau_dt=(1.0, 1e-30)) == [(0.0, False)]


def test_every_edge_floored(cluster):
    """Softening 1e3 exceeds every group's extent: the values are gsum / 1e9.  With the floor ignored (or applied to
    the volume) they would be the softening-2 values, orders of magnitude higher."""
    case = cluster.with_masses(cluster.m, eps=1e3)
    thr = R.pick_thresholds(case.D, 3)
    assert len(thr) == 3 and case.D.max() < cluster.D.min()
    sim = case.open()
    try:
        got = [case.measure(sim, t) for t in thr]
    finally:
        sim.close()
    assert got == [case.want(t) for t in thr], got
    assert [case.count(t) for t in thr][0] == 65 and [case.count(t) for t in thr][2] == 0


def test_coincident_bodies_without_softening(gpu):
    p = np.tile([[3.0, -4.0, 5.0]], (40, 1))
    case = Case(p, np.zeros_like(p), np.ones(40), eps=0.0)
    assert case.waves == 1 and np.isinf(case.D[0])
    assert _shares(case, FINITE) == [(1.0, True)] * 3


# ---- 5. hysteresis ---------------------------------------------------------------------------------------------------
def test_hysteresis_over_steps_and_its_reset(cluster64):
    """64 waves, one handle, no set_state between the steps: ask 21, 22, 16, 15, 21, 22 waves of 64 give all64 F, T, T, F,
    F, T (22 / 64 = 343.75 per mille enters, 16 / 64 is the >= edge of staying).  Then set_state and 16: F."""
    case = cluster64
    desc = np.sort(case.D)[::-1]
    thr_for = {k: np.float32(np.sqrt(desc[k - 1] * desc[k])) for k in (15, 16, 21, 22)}
    sim = case.open()
    try:
        sim.set_state(case.p, case.zero)
        prev, got, want = 0, [], []
        for ask in (21, 22, 16, 15, 21, 22):
            # precondition (host only): the bodies have moved by ~1e-8, the thresholds of step 0 still separate
            pos = sim.get_positions_f64()
            order = R.key_order(pos)
            D = R.wave_values(pos, case.m, R.G, case.eps, order)
            R.check_margins([thr_for[ask]], D)
            assert int((D > np.float64(thr_for[ask])).sum()) == ask
            sim.set_force_precision("auto", R.tau_for(thr_for[ask], DT))
            sim.step(DT)
            prev = R.all64_rule(prev, ask, 64)
            got.append(sim.force_precision_share())
            want.append((ask / 64, bool(prev)))
        assert [w[1] for w in want] == [False, True, True, False, False, True]
        assert got == want, got
        assert case.measure(sim, thr_for[16]) == (16 / 64, False)  # a new state: the history is the old system's
    finally:
        sim.close()


# ---- 6. the walk honours the flags, wave by wave ----------------------------------------------------------------------
WALK_DT = 0.05


def _one_step(case, mode, thr, multipole, dt=WALK_DT):
    sim = _sim(case.p, case.v, case.m, case.eps, multipole=multipole)
    try:
        if mode == "auto":
            sim.set_force_precision("auto", R.tau_for(thr, dt))
        else:
            sim.set_force_precision(mode)
        sim.step(dt)
        return np.concatenate([sim.get_positions_f64(), sim.get_velocities()], axis=1).view(np.uint64), sim.force_precision_share()
    finally:
        sim.close()


@pytest.mark.parametrize("multipole", ["monopole", "quadrupole"])
@pytest.mark.parametrize("walk", ["one_wave", "default"])
def test_walk_computes_each_wave_in_the_flagged_precision(cluster, walk, multipole):
    """Three handles step once from the same state: "auto", "f32", "f64".  With 21 of the 65 waves asking (the most
    that leaves the system-wide verdict off) every wave of the key order ends with the bits of the f64 handle if the
    host flags it and with the bits of the f32 handle if not - all 64 bodies, positions and velocities.  At the median
    threshold 32 waves ask, more than a third: every body ends with the f64 handle's bits."""
    case = cluster
    thr = R.thresholds(case.D)
    part, many = thr[65 - 21], thr[len(thr) // 2]
    R.check_margins([part, many], case.D, margin=2e-4)  # tau / dt^2 is rounded once more at this dt
    flags = case.D > np.float64(part)
    assert case.count(part) == 21 and case.count(many) == 32
    with _Env(**({"NBMI_SPLIT_WAVES": 0} if walk == "one_wave" else {})):
        b32, s32 = _one_step(case, "f32", None, multipole)
        b64, s64 = _one_step(case, "f64", None, multipole)
        auto, sa = _one_step(case, "auto", part, multipole)
        allw, sw = _one_step(case, "auto", many, multipole)
    assert s32 == (0.0, False) and s64 == (1.0, True)
    assert sa == (21 / 65, False) and sw == (32 / 65, True)
    bad = []
    for w in range(case.waves):
        rows = case.order[64 * w:64 * w + 64]
        assert np.any(b32[rows] != b64[rows]), f"wave {w}: fp32 and float64 forces give the same bits, nothing to tell"
        is64 = np.all(auto[rows] == b64[rows], axis=1)
        is32 = np.all(auto[rows] == b32[rows], axis=1)
        if not (is64.all() if flags[w] else is32.all()):
            bad.append((w, bool(flags[w]), int(is64.sum()), int(is32.sum()), len(rows)))
    assert not bad, bad
    assert np.array_equal(allw, b64)


def test_leapfrog_decides_on_the_drifted_positions(cluster):
    """A leapfrog step builds its tree after the drift: the flags are those of the positions the step ends with.  Its
    first step also primes a = F(x) with a build of its own on the initial positions - two builds, two applications of
    the hysteresis."""
    case = cluster
    # the drifted positions do not depend on the threshold beyond the priming forces' precision: take them from a probe
    sim = _sim(case.p, case.v, case.m, case.eps, integrator="leapfrog")
    try:
        sim.set_force_precision("auto", R.tau_for(np.float32(1e30), DT))
        sim.step(DT)
        probe = sim.get_positions_f64()
    finally:
        sim.close()
    assert not np.array_equal(probe, case.p)
    Dp = R.wave_values(probe, case.m, R.G, case.eps, R.key_order(probe))
    thr = R.thresholds(Dp)
    for t in (thr[len(thr) // 2], thr[65 - 10]):  # about half of the waves ask (every wave float64); 10 ask
        sim = _sim(case.p, case.v, case.m, case.eps, integrator="leapfrog")
        try:
            sim.set_force_precision("auto", R.tau_for(t, DT))
            sim.step(DT)
            pos, got = sim.get_positions_f64(), sim.force_precision_share()
        finally:
            sim.close()
        D1 = R.wave_values(pos, case.m, R.G, case.eps, R.key_order(pos))
        R.check_margins([t], D1)
        R.check_margins([t], case.D)
        ask0, ask1 = case.count(t), int((D1 > np.float64(t)).sum())
        assert got == (ask1 / 65, bool(R.all64_rule(R.all64_rule(0, ask0, 65), ask1, 65))), (got, ask0, ask1)


# ---- 7. API ----------------------------------------------------------------------------------------------------------
def _flag_everything_and_close(case):
    """A handle that flags every wave, closed: its flag memory is likely to be handed to the next handle of this size."""
    sim = _sim(case.p, case.zero, case.m, case.eps)
    try:
        sim.set_force_precision("auto", R.tau_for(R.separating_thresholds(case.D)[0], DT))  # below every value
        sim.step(DT)
        assert sim.force_precision_share() == (1.0, True)
    finally:
        sim.close()


def test_api_of_the_modes(cluster):
    case = cluster
    thr = R.thresholds(case.D)
    mid = thr[len(thr) // 2]
    _flag_everything_and_close(case)
    sim = case.open()
    try:
        assert sim.force_precision_share() == (0.0, False)  # before the first step: nothing has asked
        assert case.measure(sim, mid) == case.want(mid)
        # tau = 0 keeps the tau
        sim.set_state(case.p, case.zero)
        sim.set_force_precision("auto", 0.0)
        sim.step(DT)
        assert sim.force_precision_share() == case.want(mid)
        # builds that are not part of a step leave the flags and the verdict alone
        before = sim.force_precision_share()
        sim.set_force_precision("auto", R.tau_for(thr[0], DT))
        sim.build_tree()
        sim.accelerations()
        assert sim.force_precision_share() == before
        sim.set_force_precision("f32")
        assert sim.force_precision_share() == (0.0, False)
        sim.set_force_precision("f64")
        assert sim.force_precision_share() == (1.0, True)
    finally:
        sim.close()
    with _Env(NBMI_PREC_TAU=repr(R.tau_for(thr[10], DT))):
        sim = case.open()
    try:
        sim.step(DT)
        assert sim.force_precision_share() == case.want(thr[10]) and case.count(thr[10]) == 55
    finally:
        sim.close()


# ---- 8. owner mode -----------------------------------------------------------------------------------------------------
def _owner_run(case, thr, world=3, mode="auto", set_dt=True):
    """One LetBarnesHut.step(DT) over `world` thread-ranks; returns per rank (ids, recorded step facts or None, (share,
    all64)) and the gathered state."""
    from nbody.sharded import HipLetEngine, LetBarnesHut
    from test_gpu_sharded_record import _ThreadComm, _run_ranks
    comm = _ThreadComm(world)
    engines = [HipLetEngine(case.p, case.zero, case.m, R.G, case.eps, 1.0, THETA, 0, r, world) for r in range(world)]
    try:
        seen = [None] * world
        for r, e in enumerate(engines):
            if mode != "auto":
                e.sim.set_force_precision(mode)
            elif thr is not None:
                e.sim.set_force_precision("auto", R.tau_for(thr, DT))
            if not set_dt:
                e.op_begin = lambda dt: None  # the caller that never announces its dt

            def facts(e=e, r=r):
                seen[r] = np.array(e.sim.owner_step_facts(), dtype=np.int64)
                return seen[r]
            e.step_facts = facts
        steppers = [LetBarnesHut(e, r, world, comm.bind(r) if world > 1 else None) for r, e in enumerate(engines)]
        out = _run_ranks(steppers, comm, DT, 1)
        return [(e.sim.ids().astype(np.int32), seen[r], e.sim.force_precision_share()) for r, e in enumerate(engines)], out[0]
    finally:
        for e in engines:
            e.sim.close()


def test_owner_mode_votes_rank_by_rank_and_decides_once(cluster):
    """World 3: every rank's (asking, waves) is the host's on that rank's rows taken 64 at a time from its own first
    row, and every rank's verdict is the rule on the sums - for one threshold on either side of a third."""
    case = cluster
    # the partition does not depend on the threshold: learn it, then choose thresholds that keep the margin from the
    # RANKS' wave values (their waves are not the single handle's: they start at each rank's first row)
    ranks, _ = _owner_run(case, None, mode="f32")
    parts = [ids for ids, _, _ in ranks]
    assert np.array_equal(np.concatenate(parts), case.order)
    assert all(len(ids) > 0 for ids in parts)
    Dr = [R.wave_values(case.p, case.m, R.G, case.eps, ids) for ids in parts]
    pooled = np.concatenate(Dr)
    waves = len(pooled)
    assert waves == sum((len(ids) + 63) // 64 for ids in parts)
    thr = R.separating_thresholds(pooled)  # ascending: the counts descend
    asks = [int((pooled > np.float64(t)).sum()) for t in thr]
    above = [t for t, a in zip(thr, asks) if 1000 * a > 333 * waves][-1]
    below = [t for t, a in zip(thr, asks) if 1000 * a <= 333 * waves][0]
    print("owner mode: waves", waves, "asking at the two thresholds", int((pooled > above).sum()), int((pooled > below).sum()))
    for t, verdict in ((above, True), (below, False)):
        ranks, _ = _owner_run(case, t)
        total = 0
        for r, (ids, facts, share) in enumerate(ranks):
            assert np.array_equal(ids, parts[r])
            flags, ask, w = R.expected(case.p, case.m, R.G, case.eps, t, order=ids)
            assert (int(facts[0]), int(facts[1])) == (ask, w), (r, facts, ask, w)
            assert share == (ask / w, verdict), (r, share)
            total += ask
        assert bool(R.all64_rule(0, total, waves)) == verdict


def test_owner_mode_without_a_dt_computes_in_fp32(gpu):
    """nbmi_owner_step on an "auto" handle whose dt was never set reads wave flags that no build has written: they are
    cleared at allocation, so the forces are fp32 - the bits of an "f32" owner handle.  (Before the flags were cleared
    this depended on what the allocator returned; the handle opened and closed first makes stale flags likely.  A
    regression guard, not a proof.)"""
    case = Case(*R.cluster_input(N))
    from nbody.sharded import let_capacities
    big = Case(*R.cluster_input(let_capacities(N, 1)[0]))  # as many rows as the owner handle's capacity
    _flag_everything_and_close(big)
    ranks, auto = _owner_run(case, None, world=1, set_dt=False)
    assert ranks[0][2] == (0.0, False)
    _, f32 = _owner_run(case, None, world=1, mode="f32")
    _, f64 = _owner_run(case, None, world=1, mode="f64")
    assert not np.array_equal(f32[1], f64[1])
    assert np.array_equal(auto[0], f32[0]) and np.array_equal(auto[1], f32[1])
