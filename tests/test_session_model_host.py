"""The session model (tests/session_model.py) and the committed seeds (tests/session_cases.py) on the host: the generators
cover what the GPU tests rely on.  These are conditions, not measurements: the seed list was chosen so that they hold.
"""
import collections
import dataclasses

import numpy as np
import pytest

import session_cases as SC
import session_model as SM

NBODY_SYSTEMS = ("n1", "n2", "n65", "n257", "n2049", "n4097")
ALL_KINDS = [SC.nbody_kind(label, system) for label in SC.NBODY_KINDS for system in NBODY_SYSTEMS + ("far", "trap")]
ALL_KINDS += [SC.boids_kind(label, n) for label in SC.BOIDS_KINDS for n in SC.BOIDS_SIZES]
MID_KINDS = [k for k in ALL_KINDS if k.n == 257]  # one of every handle kind, at a size that admits every op
IDS = lambda k: k.label  # noqa: E731


def observations(kind, ops):
    return [op for op in ops if not SM.is_state(kind, op)]


@pytest.mark.parametrize("kind", [k for k in ALL_KINDS if k.n in (65, 257, 2049)], ids=IDS)
def test_pair_walk_covers_every_ordered_pair_once(kind):
    ops = SM.walk_ops(kind)
    walk = SM.pair_walk(kind)
    obs = observations(kind, walk)
    assert len(obs) == len(ops) ** 2 + 1 and obs[0] == obs[-1]  # closed
    pairs = collections.Counter(zip(obs, obs[1:]))
    assert set(pairs) == {(a, b) for a in ops for b in ops} and set(pairs.values()) == {1}
    # a state op after every 25 observations, from the fixed cycle, and nothing else
    states = [i for i, op in enumerate(walk) if SM.is_state(kind, op)]
    assert len(states) == (len(obs) - 1) // SM.STATE_EVERY
    seen = 0
    for i, op in enumerate(walk):
        if SM.is_state(kind, op):
            assert seen and seen % SM.STATE_EVERY == 0 and op in SM.STATE_CYCLE[kind.family], (i, op)
        else:
            seen += 1
    assert not SM.invalid(kind, walk)
    # every observation of the table that the kind admits is in the walk (cell_moments: on the quadrupole kind)
    names = {s.name for s in SM.applicable(kind, SM.OBS)} - ({"cell_moments"} if kind.multipole != "quadrupole" else set())
    assert {op.name for op in ops} == names


def test_pair_sequence_is_the_eulerian_circuit():
    for m in (1, 2, 3, 7, 31):
        seq = SM.pair_sequence(m)
        assert len(seq) == m * m
        assert collections.Counter(zip(seq, seq[1:] + seq[:1])) == {(a, b): 1 for a in range(m) for b in range(m)}


def test_the_walks_the_issue_asks_for_see_every_observation():
    """a Barnes-Hut walk holds every N-body observation but cell_moments, the quadrupole one that too; a walled and a
    periodic boids walk together hold every boids observation"""
    table = {s.name for s in SM.NBODY if s.kind == SM.OBS}
    assert {op.name for op in SM.walk_ops(SC.nbody_kind("bh", "n65"))} == table - {"cell_moments"}
    assert {op.name for op in SM.walk_ops(SC.nbody_kind("bh_quadrupole", "n65"))} == table
    both = {op.name for label in ("walled_metric", "periodic_metric") for op in SM.walk_ops(SC.boids_kind(label, 257))}
    assert both == {s.name for s in SM.BOIDS if s.kind == SM.OBS}


@pytest.mark.parametrize("kind", MID_KINDS, ids=IDS)
def test_every_op_appears_three_times_over_the_seeds(kind):
    count = collections.Counter(op.name for seed in SC.SEEDS for op in SM.random_session(kind, seed))
    want = [s.name for s in SM.applicable(kind)]
    assert set(count) <= set(want)
    # cell_moments needs quadrupole mode: on a kind that is not created in it, only after a set_multipole("quadrupole")
    # and before the next set_multipole("monopole") - at least once there, three times and more on the quadrupole kind
    if kind.family == "nbody" and kind.tree and kind.multipole != "quadrupole":
        assert count["cell_moments"] >= 1
        want.remove("cell_moments")
    assert all(count[name] >= 3 for name in want), {name: count[name] for name in want if count[name] < 3}


def test_every_op_of_both_tables_is_applicable_somewhere():
    for family, table in SM.TABLES.items():
        seen = {s.name for k in MID_KINDS if k.family == family for s in SM.applicable(k)}
        assert seen == set(table), set(table) - seen


@pytest.mark.parametrize("kind", MID_KINDS, ids=IDS)
def test_every_state_op_is_followed_by_every_class_of_observation(kind):
    classes = {s.cls for s in SM.applicable(kind, SM.OBS)}
    after = collections.defaultdict(set)
    for seed in SC.SEEDS:
        ops = SM.random_session(kind, seed)
        for i, op in enumerate(ops):
            if SM.is_state(kind, op):
                after[op.name] |= {SM.spec_of(kind, o).cls for o in ops[i + 1:] if not SM.is_state(kind, o)}
    for s in SM.applicable(kind, SM.STATE):
        assert after[s.name] == classes, (s.name, classes - after[s.name])


@pytest.mark.parametrize("kind", ALL_KINDS, ids=IDS)
def test_every_emitted_call_satisfies_its_precondition(kind):
    for seed in SC.SEEDS:
        ops = SM.random_session(kind, seed)
        assert len(ops) == SM.MAX_LENGTH and not SM.invalid(kind, ops), (seed, SM.invalid(kind, ops))
        for op in ops:  # restated, apart from the model's own bookkeeping
            if op.name in ("knn", "densities"):
                assert kind.tree and 1 <= op.args[0] <= kind.n - 1
            if op.name in ("tree_stats", "morton_keys", "sort_keys", "cells", "cell_moments", "key_order", "build_tree",
                           "set_force_precision", "force_precision_share", "find_groups", "group_catalogue", "pair_counts",
                           "color_by_groups"):
                assert kind.tree
            if op.name == "set_multipole" and op.args[0] == "quadrupole":
                assert kind.tree
            if op.name.startswith("periodic_"):
                assert kind.periodic
            if op.name in ("flocks", "flock_catalogue", "neighbour_stats"):
                assert not kind.periodic and SM._link_of(kind, op.args[0]) <= kind.perception
            if op.name == "velocity_correlation":
                nb, m = op.args
                edges = SM.vcorr_edges(kind, nb, m)
                assert len(edges) == nb + 1 and (np.diff(edges) > 0).all() and int(np.ceil(edges[-1] / kind.cell)) == m <= 16
                assert not kind.periodic or (2 * m + 1 <= kind.dim and edges[-1] < kind.length / 2)
            if op.name == "update" and kind.periodic:
                assert kind.max_speed * abs(op.args[0]) < kind.length
            if op.name == "topological_neighbours":
                assert 1 <= op.args[0] <= 16
    assert not SM.invalid(kind, SM.pair_walk(kind))


def test_preconditions_follow_the_state_ops():
    kind = SC.nbody_kind("bh", "n65")
    assert SM.invalid(kind, [SM.Op("frame_delta")]) == [0]
    assert SM.invalid(kind, [SM.Op("frame_keyframe"), SM.Op("frame_delta")]) == []
    assert SM.invalid(kind, [SM.Op("cell_moments")]) == [0]
    assert SM.invalid(kind, [SM.Op("set_multipole", ("quadrupole",)), SM.Op("cell_moments")]) == []
    assert SM.invalid(SC.nbody_kind("direct", "n65"), [SM.Op("knn", (1,)), SM.Op("get_masses")]) == [0]
    assert SM.invalid(SC.nbody_kind("bh", "n2"), [SM.Op("knn", (1,)), SM.Op("knn", (8,))]) == [1]
    assert SM.invalid(SC.boids_kind("periodic_metric", 257), [SM.Op("flocks", ("link",)), SM.Op("periodic_flocks", ("link",)),
                                                              SM.Op("velocity_correlation", (12, 2))]) == [0, 2]  # dim 3: reach 1


@pytest.mark.parametrize("kind", MID_KINDS, ids=IDS)
def test_generators_are_deterministic_and_seeds_differ(kind):
    sessions = [SM.random_session(kind, seed) for seed in SC.SEEDS]
    assert sessions == [SM.random_session(kind, seed) for seed in SC.SEEDS]
    assert len({tuple(s) for s in sessions}) == len(SC.SEEDS)
    assert SM.pair_walk(kind) == SM.pair_walk(kind)
    assert len(SM.random_session(kind, SC.SEEDS[0], 5)) == 5


def test_the_sizes_of_a_kind_run_every_seed_and_every_state_op():
    assert len(set(SC.SEEDS)) == len(SC.SEEDS)
    for label in SC.NBODY_KINDS:
        ran = [(SC.nbody_kind(label, s), seed) for i, s in enumerate(NBODY_SYSTEMS) for seed in SC.seeds_of(i)]
        assert {seed for _, seed in ran} == set(SC.SEEDS)
        names = {op.name for kind, seed in ran for op in SM.random_session(kind, seed) if SM.is_state(kind, op)}
        assert names == {s.name for s in SM.applicable(SC.nbody_kind(label, "n257"), SM.STATE)}, label
    for label in SC.BOIDS_KINDS:
        ran = [(SC.boids_kind(label, n), seed) for i, n in enumerate(SC.BOIDS_SIZES) for seed in SC.seeds_of(i)]
        assert {seed for _, seed in ran} == set(SC.SEEDS)
        names = {op.name for kind, seed in ran for op in SM.random_session(kind, seed) if SM.is_state(kind, op)}
        assert names == {s.name for s in SM.BOIDS if s.kind == SM.STATE}, label


def test_size_arguments_grow_shrink_and_grow():
    """over the seeds and the kinds of a family every value of every size set is drawn"""
    kind = SC.nbody_kind("bh", "n257")
    drawn = collections.defaultdict(set)
    for k in MID_KINDS:
        for seed in SC.SEEDS:
            for op in SM.random_session(k, seed):
                drawn[k.family, op.name].add(op.args)
    drawn = collections.defaultdict(set, {name: v for (family, name), v in drawn.items() if family == "nbody"})
    assert {a[0] for a in drawn["knn"]} == set(SM.KNN_K) and {a[0] for a in drawn["field_at"]} == set(SM.FIELD_M)
    assert {a[0] for a in drawn["deposit"]} == set(SM.DEPOSIT_DIMS) and {a[1] for a in drawn["deposit"]} == {"ngp", "cic"}
    assert {a[0] for a in drawn["pair_counts"]} == set(SM.PAIR_NB) and {a[1] for a in drawn["group_catalogue"]} == set(SM.CAPACITIES)
    assert {a[0] for a in drawn["set_tracers"]} == set(SM.TRACER_M) and {a[1] for a in drawn["step_many"]} == set(SM.SUBSTEPS)
    assert [SM.field_size(kind, w) for w in SM.FIELD_M] == [1, 63, 3 * 257 + 5]
    assert [SM.tracer_size(kind, w) for w in SM.TRACER_M] == [0, 1, 260]
    assert [SM.capacity_of(w, 257) for w in SM.CAPACITIES] == [0, 1, 64, 260]
    drawn.clear()
    for k in MID_KINDS:
        for seed in SC.SEEDS:
            for op in SM.random_session(k, seed):
                if k.family == "boids":
                    drawn[op.name].add(op.args)
    assert {a[0] for a in drawn["velocity_correlation"]} == set(SM.PAIR_NB) and drawn["heading_moments"]  # (nb = 0)
    assert {a[0] for a in drawn["topological_neighbours"]} == set(SM.TOPO_K)
    assert {a[2] for a in drawn["flock_catalogue"]} == set(SM.CAPACITIES) and {a[1] for a in drawn["update"]} == set(SM.SUBSTEPS)


def test_describe_round_trips():
    for kind in MID_KINDS:
        for ops in (SM.random_session(kind, SC.SEEDS[0]), SM.pair_walk(kind)[:60]):
            text = SM.describe(ops)
            assert SM.parse(text) == ops and SM.describe(SM.parse(text)) == text
            assert all(isinstance(op, SM.Op) for op in SM.parse(text))
    assert SM.parse(SM.describe([])) == []


def test_the_comparison_is_of_bits():
    @dataclasses.dataclass
    class D:
        x: float
        y: tuple
    nan = np.array([np.nan, 1.0])
    assert SM.same_bits(nan, nan.copy()) and SM.same_bits(float("nan"), float("nan"))
    assert not SM.same_bits(np.array([0.0]), np.array([-0.0])) and not SM.same_bits(0.0, -0.0)
    assert not SM.same_bits(np.float32([1.0]), np.float64([1.0])) and not SM.same_bits(np.zeros(2), np.zeros(3))
    assert SM.same_bits(np.float32([np.nan, -0.0]), np.float32([np.nan, -0.0]))
    assert not SM.same_bits(np.float32([0.0]), np.float32([-0.0]))
    a = {"r": (np.arange(3), D(1.0, (np.ones(2), None))), "n": 3}
    b = {"r": (np.arange(3), D(1.0, (np.ones(2), None))), "n": 3}
    assert SM.same_bits(a, b)
    b["r"][1].y[0][1] = np.nextafter(1.0, 2.0)
    d = SM.differences(a, b)
    assert len(d) == 1 and "['r'][1]['y'][0]" in d[0] and "flat index 1" in d[0], d
    assert SM.differences((1, 2), (1, 2, 3)) and SM.differences({"a": 1}, {"b": 1}) and SM.differences(1, "1")
    assert SM.same_bits(np.int64(3), 3) and SM.same_bits([None, "x", True], [None, "x", True])


def test_replay_and_the_rule_on_a_fake_handle():
    """check_session with a handle made of Python: an observation that leaves something behind is caught, with a message
    that holds the op list"""
    class Fake:
        def __init__(self, leaky):
            self.x, self.seen, self.leaky = 0, 0, leaky

        def close(self):
            pass

    specs = {"bump": SM.Spec("bump", SM.STATE, "", lambda h, c, k: setattr(h, "x", h.x + k), lambda kind: (1,), None),
             "peek": SM.Spec("peek", SM.OBS, "state", lambda h, c: h.x + (h.seen if h.leaky else 0), lambda kind: (), None),
             "look": SM.Spec("look", SM.OBS, "state", lambda h, c: setattr(h, "seen", h.seen + 1), lambda kind: (), None)}
    kind = SM.Kind("fake", "fake", 1)
    SM.TABLES["fake"] = specs
    try:
        ops = [SM.Op("peek"), SM.Op("bump", (2,)), SM.Op("peek"), SM.Op("look"), SM.Op("peek"), SM.Op("bump", (1,)), SM.Op("peek")]
        for leaky in (False, True):
            class factory:
                def __call__(self):
                    return Fake(leaky)

                def state(self, h):
                    return {"x": h.x}
            ctx = SM.Ctx(kind, {})
            assert SM.replay(factory(), ctx, ops, 6) == 3 + 0 and SM.state_prefix(kind, ops, 6) == (ops[1], ops[5])
            if not leaky:
                assert SM.check_session(factory(), ctx, ops, "fake") == 4  # peek at three prefixes, look at one: cached
            else:
                with pytest.raises(AssertionError) as e:
                    SM.check_session(factory(), ctx, ops, "seed 0")
                msg = str(e.value)
                assert "fake n=1 seed 0: op 4 peek()" in msg and SM.describe(ops[:5]) in msg
    finally:
        del SM.TABLES["fake"]
