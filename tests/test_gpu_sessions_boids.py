"""Sessions on one boids.Flock (tests/session_model.py, tests/session_cases.py): the rule of
test_gpu_sessions_nbody.py for the boids handle, walled and periodic, metric and topological, with and without noise.
One handle carries one staging buffer of 12 N doubles through every getter, one "last built grid" that eight calls
rebuild, and scratch that grows with k: whatever ran before, every read-only call gives the bits of a fresh Flock that has
seen the same state ops and no other observation.

Up to 257 boids every observation that has an exact host reference is also compared with it, after its history.  A
failure's message holds the op list that reproduces it: paste it into EXPLICIT below.
"""
import numpy as np
import pytest

import session_cases as SC
import session_model as SM

pytestmark = pytest.mark.gpu

WALKS = [(label, n) for label in ("walled_metric", "periodic_metric", "walled_topological_noise", "periodic_topological_noise")
         for n in (257, 2049)]
WALK_PARTS = 3  # pieces of a walk (SM.split_walk), each a test of its own
RANDOM = [(label, n, i) for label in SC.BOIDS_KINDS for i, n in enumerate(SC.BOIDS_SIZES)]

# Op lists that failed once, reduced by hand: name -> (kind label, n, SM.parse text or a list of ops)
EXPLICIT = {}


def check(label, n, ops, what, anchor=True):
    ctx = SC.boids_ctx(label, n)
    use = SC.boids_anchor(ctx) if anchor and n <= SC.ANCHOR_MAX_N else None
    try:
        made = SM.check_session(SC.BoidsFactory(ctx), ctx, ops, what, anchor=use)
    except RuntimeError as e:  # a HIP error, not a mismatch: nothing more is started on a device that may have faulted
        pytest.exit(f"{ctx.kind.label} {what}: {e}\nthe session was SM.parse('''{SM.describe(ops)}''')", returncode=3)
    print(f"{ctx.kind.label} {what}: {len(ops)} ops, {made} replays")


@pytest.mark.parametrize("n", (257, 2049, 4097))
@pytest.mark.parametrize("label", ("walled_metric", "periodic_metric"))
def test_the_cases_have_their_point(gpu, label, n):
    """flocks, links, full neighbour rows and correlation bins are not empty, and not everything"""
    ctx = SC.boids_ctx(label, n)
    k = ctx.kind
    f = SC.BoidsFactory(ctx)()
    try:
        fl = (f.periodic_flocks if k.periodic else f.flocks)(k.link)
        cat = (f.periodic_flock_catalogue if k.periodic else f.flock_catalogue)(k.link, 2, 64)
        topo = f.topological_neighbours(7)
        vc = SM.call(f, ctx, SM.Op("velocity_correlation", tuple(SM.spec_of(k, SM.Op("velocity_correlation")).fixed(k))))
        vis = SM.call(f, ctx, SM.Op("visible_vertices", (True,)))
        print(f"{k.label}: flocks {fl['n_flocks']} links {fl['links']} catalogue {cat['count']} full rows "
              f"{int((topo['count'] == 7).sum())} pairs {vc['pairs'].tolist()} visible {len(vis[0]) // 6}")
        lost = (k.label, "the case lost its point")
        assert 1 < fl["n_flocks"] < n and fl["links"] > n // 8 and cat["count"] > 1, lost
        # (the periodic cases are dense, about 40 boids within sight of each: every row is full; the walled ones have
        # boids with fewer than 7 in sight, whose rows are padded)
        assert (topo["count"] == 7).sum() > n // 8 and (k.periodic or (topo["count"] < 7).any()), lost
        assert (vc["pairs"][1:] > 0).all() and any(vc["dot"]), lost
        assert 0 < len(vis[0]) // 6 < n, lost
    finally:
        f.close()


@pytest.mark.parametrize("part", range(WALK_PARTS))
@pytest.mark.parametrize("label,n", WALKS)
def test_pair_walk(gpu, label, n, part):
    """every observation after every other one, a state op after every 25"""
    kind = SC.boids_kind(label, n)
    check(label, n, SM.split_walk(kind, SM.pair_walk(kind), WALK_PARTS)[part], f"pair walk, part {part} of {WALK_PARTS}")


@pytest.mark.parametrize("label,n,index", RANDOM)
def test_random_sessions(gpu, label, n, index):
    kind = SC.boids_kind(label, n)
    for seed in SC.seeds_of(index):
        check(label, n, SM.random_session(kind, seed), f"random session, seed {seed}")


@pytest.mark.parametrize("n", (1, 2))
@pytest.mark.parametrize("label", ("walled_metric", "periodic_metric"))
def test_every_op_on_one_and_two_boids(gpu, label, n):
    """each call once, in table order, twice over"""
    kind = SC.boids_kind(label, n)
    ops = SM.fixed_tour(kind)
    assert {op.name for op in ops} == {s.name for s in SM.applicable(kind)} and len(ops) >= 2 * len(SM.applicable(kind))
    check(label, n, ops, "every op, twice")


def _catalogue(kind):
    return "periodic_flock_catalogue" if kind.periodic else "flock_catalogue"


def regrow(kind, name):
    """grow, shrink, grow of one call's size argument with another call in between"""
    reach = min(2, SM.max_reach(kind))
    return {
        "topological_neighbours": [("topological_neighbours", (1,)), ("forces", ()), ("topological_neighbours", (16,)),
                                   ("cell_indices", ()), ("topological_neighbours", (7,)), ("velocity_correlation", (12, 1)),
                                   ("topological_neighbours", (16,))],
        "flock_catalogue": [(_catalogue(kind), ("link", 1, "one")), ("topological_neighbours", (7,)),
                            (_catalogue(kind), ("link", 1, "all")), ("diagnostics", ()), (_catalogue(kind), ("sight", 2, "zero")),
                            ("forces", ()), (_catalogue(kind), ("link", 2, "64"))],
        "velocity_correlation": [("velocity_correlation", (64, reach)), ("positions", ()), ("heading_moments", ()),
                                 ("forces", ()), ("velocity_correlation", (1, 1)), ("noise_vectors", (None,)),
                                 ("velocity_correlation", (64, reach))],
    }[name]


@pytest.mark.parametrize("n", (257, 2049))
@pytest.mark.parametrize("label", ("walled_metric", "periodic_topological_noise"))
@pytest.mark.parametrize("name", ("flock_catalogue", "topological_neighbours", "velocity_correlation"))
def test_scratch_regrowth(gpu, name, label, n):
    kind = SC.boids_kind(label, n)
    ops = [SM.Op(*o) for o in regrow(kind, name)]
    # between a step and a state upload too: the grid a call finds is the step's, then none
    ops = ops + [SM.Op("update", (SM.DT_BOIDS, 3))] + ops + [SM.Op("set_state", (2,))] + ops
    check(label, n, ops, f"regrowth of {name}")


def test_explicit_cases(gpu):
    for name, (label, n, ops) in sorted(EXPLICIT.items()):
        check(label, n, SM.parse(ops) if isinstance(ops, str) else [SM.Op(*o) for o in ops], name)


def test_the_python_state_cache_is_dropped(gpu):
    """Flock keeps the last fetched state; an update or an upload must drop it (SM's factory fetches afresh, so this is
    the one place where the cached arrays themselves are looked at)"""
    ctx = SC.boids_ctx("walled_metric", 257)
    f = SC.BoidsFactory(ctx)()
    try:
        before = f.positions.copy()
        assert f.positions is f.positions
        f.update(SM.DT_BOIDS, 1)
        assert not np.array_equal(f.positions, before)
        f.set_state(before)
        assert np.array_equal(f.positions, before)
    finally:
        f.close()
