"""Sessions on one N-body handle (tests/session_model.py, tests/session_cases.py): whatever ran
before, every read-only call gives the bits of a fresh handle that has seen the same state ops and no other observation,
and the state at the end is that of a handle which ran the state ops alone.  test_gpu_query_shared.py asserts this for
three queries in six orders; here it is every public call of HIPBarnesHutSimulation / HIPDirectSimulation after every
other one (the pair walk), mixed with every state op (the random sessions), and the scratch that grows and shrinks.

Up to 257 bodies every observation that has an exact host reference is also compared with it, after its history, so an
answer that is wrong the same way on both handles still fails.  A failure's message holds the op list that reproduces it:
paste it into EXPLICIT below.
"""
import pytest

import session_cases as SC
import session_model as SM

pytestmark = pytest.mark.gpu

SYSTEMS = ("n1", "n2", "n65", "n257", "n2049", "n4097")
WALKS = [("bh_quadrupole", "n65"), ("bh_quadrupole", "n2049"), ("bh", "n65"), ("bh", "n2049"), ("bh_auto", "n65"),
         ("bh_auto", "n2049"), ("direct", "n65"), ("direct", "n2049")]
WALK_PARTS = 4  # pieces of a walk (SM.split_walk), each a test of its own: a whole walk is a thousand calls
RANDOM = [(label, system, i) for label in SC.NBODY_KINDS for i, system in enumerate(SYSTEMS)]
RANDOM += [("bh", "far", 6), ("bh_quadrupole", "far", 7), ("bh", "trap", 8)]

# Op lists that failed once, reduced by hand: name -> (kind label, system, SM.parse text or a list of ops)
EXPLICIT = {}


def check(label, system, ops, what, anchor=True):
    ctx = SC.nbody_ctx(label, system)
    use = SC.nbody_anchor(ctx) if anchor and ctx.kind.n <= SC.ANCHOR_MAX_N else None
    try:
        made = SM.check_session(SC.NBodyFactory(ctx), ctx, ops, what, anchor=use)
    except RuntimeError as e:  # a HIP error, not a mismatch: nothing more is started on a device that may have faulted
        pytest.exit(f"{ctx.kind.label} {what}: {e}\nthe session was SM.parse('''{SM.describe(ops)}''')", returncode=3)
    print(f"{ctx.kind.label} {what}: {len(ops)} ops, {made} replays")


@pytest.mark.parametrize("system", ("n65", "n257", "n2049", "n4097", "far", "trap"))
def test_the_cases_have_their_point(gpu, system):
    """groups, pairs and occupied deposit cells exist and are not everything: a call that returned nothing would be noticed"""
    ctx = SC.nbody_ctx("bh", system)
    h = SC.NBodyFactory(ctx)()
    try:
        n = ctx.kind.n
        h.find_groups(ctx.kind.link)
        counts, below = h.pair_counts(SM.pair_edges(ctx, 12))
        cat = h.group_catalogue(ctx.kind.link, 2)
        dep = SM.call(h, ctx, SM.Op("deposit", ((4, 5, 6), "cic")))
        vis = SM.call(h, ctx, SM.Op("visible_points"))
        print(f"{system}: groups {h.n_groups}, catalogue {cat['count']}, pairs {counts.sum()} + {below}, visible {len(vis[0])}")
        lost = (system, "the case lost its point")
        assert 1 < h.n_groups < n and cat["count"] >= 1, lost
        # ("far": one body 1e6 away sets the scale of the edges, the grid and the camera; the ball is a dot in them)
        assert counts.sum() > n and (counts > 0).sum() >= (1 if system == "far" else 6), lost
        assert dep["stats"][0] == n and (dep["number"] > 0).sum() > (1 if system == "far" else 60), lost
        assert len(vis[0]) < n and (len(vis[0]) > 0 or system == "far"), lost
    finally:
        h.close()


@pytest.mark.parametrize("part", range(WALK_PARTS))
@pytest.mark.parametrize("label,system", WALKS)
def test_pair_walk(gpu, label, system, part):
    """every observation after every other one, a state op after every 25"""
    kind = SC.nbody_kind(label, system)
    check(label, system, SM.split_walk(kind, SM.pair_walk(kind), WALK_PARTS)[part], f"pair walk, part {part} of {WALK_PARTS}")


@pytest.mark.parametrize("label,system,index", RANDOM)
def test_random_sessions(gpu, label, system, index):
    kind = SC.nbody_kind(label, system)
    for seed in SC.seeds_of(index):
        check(label, system, SM.random_session(kind, seed), f"random session, seed {seed}")


@pytest.mark.parametrize("system", ("n1", "n2"))
@pytest.mark.parametrize("label", ("bh", "direct"))
def test_every_op_on_one_and_two_bodies(gpu, label, system):
    """each call once, in table order, twice over"""
    kind = SC.nbody_kind(label, system)
    ops = SM.fixed_tour(kind)
    assert {op.name for op in ops} == {s.name for s in SM.applicable(kind)} and len(ops) >= 2 * len(SM.applicable(kind))
    assert ("knn" in {op.name for op in ops}) == (kind.tree and system == "n2")  # k <= n - 1
    check(label, system, ops, "every op, twice")


REGROW = {
    # grow, shrink, grow of one call's size argument with another call in between
    "field_at": [("field_at", ("one",)), ("knn", (8,)), ("field_at", ("many",)), ("deposit", ((16, 16, 16), "cic")),
                 ("field_at", ("some",)), ("knn", (32,)), ("potentials", ()), ("field_at", ("many",))],
    "group_catalogue": [("group_catalogue", (2, "one")), ("pair_counts", (12,)), ("group_catalogue", (1, "all")),
                        ("find_groups", ()), ("group_catalogue", (2, "zero")), ("knn", (1,)), ("group_catalogue", (1, "64"))],
    "tracers": [("set_tracers", ("many",)), ("get_tracers", ()), ("step_many", (SM.DT_NBODY, 1)), ("set_tracers", ("one",)),
                ("field_at", ("some",)), ("tracer_positions_f32", ()), ("set_tracers", ("none",)), ("get_tracers", ()),
                ("step_many", (SM.DT_NBODY, 1)), ("set_tracers", ("many",)), ("step_many", (SM.DT_NBODY, 3)), ("get_tracers", ())],
}


AUTO = [  # force precision "auto": the wave flags and the all64 hysteresis are the last STEP's, whatever built a tree since
    ("force_precision_share", ()), ("step_many", (SM.DT_NBODY, 1)), ("force_precision_share", ()), ("knn", (8,)),
    ("force_precision_share", ()), ("accelerations", ()), ("force_precision_share", ()), ("potentials", ()),
    ("build_tree", ()), ("force_precision_share", ()), ("step_many", (SM.DT_NBODY, 3)), ("field_at", ("some",)),
    ("force_precision_share", ()), ("set_state", (1,)), ("find_groups", ()), ("force_precision_share", ()),
    ("step_many", (SM.DT_NBODY, 1)), ("pair_counts", (12,)), ("force_precision_share", ()),
    ("set_force_precision", ("auto", "high")), ("step_many", (SM.DT_NBODY, 1)), ("diagnostics", (True,)),
    ("force_precision_share", ()), ("set_force_precision", ("auto", "case")), ("step_many", (SM.DT_NBODY, 1)),
    ("deposit", ((4, 5, 6), "cic")), ("force_precision_share", ()),
]


@pytest.mark.parametrize("system", ("n65", "n2049", "trap"))
def test_auto_precision_is_the_last_steps(gpu, system):
    ctx = SC.nbody_ctx("bh_auto", system)
    h = SC.NBodyFactory(ctx)()
    try:
        h.step_many(SM.DT_NBODY, 1)
        share, all64 = h.force_precision_share()
    finally:
        h.close()
    print(f"{ctx.kind.label}: tau {ctx.kind.tau:.3e}, share {share:.3f}, all64 {all64}")
    assert share > 0.0, (system, "the case lost its point: no wave asks for float64")
    check("bh_auto", system, [SM.Op(*o) for o in AUTO], "auto precision")


@pytest.mark.parametrize("system", ("n257", "n2049"))
@pytest.mark.parametrize("name", sorted(REGROW))
def test_scratch_regrowth(gpu, name, system):
    check("bh", system, [SM.Op(*o) for o in REGROW[name]], f"regrowth of {name}")


def test_explicit_cases(gpu):
    for name, (label, system, ops) in sorted(EXPLICIT.items()):
        check(label, system, SM.parse(ops) if isinstance(ops, str) else [SM.Op(*o) for o in ops], name)
