"""A model of one handle's session: which public methods of HIPBarnesHutSimulation /
HIPDirectSimulation (nbody/gpu_backend.py) and of Flock (boids/flock.py) change what later calls may see (STATE ops) and
which must change nothing (OBSERVATIONS), what each needs to be a valid call, and two generators of valid op lists.  A
plain helper module like query_cases.py: no fixtures, no GPU, nothing imported from the package.

    Op(name, args)      one call; the arguments are plain literals (numbers, strings, tuples).  Arrays are named, not
                        held: set_state(3) is "the third prepared state", field_at(63) "the 63 prepared points" - the
                        binding (`call` of the op's Spec) makes them from the Kind and the case's base arrays, always
                        the same way, so an op list printed by describe() is the whole reproduction.
    Kind                the static facts of a handle kind that the preconditions need (size, tree or not, box, ...).
    pair_walk(kind)     every ordered pair (A, then B) of the kind's observations exactly once, a state op from a short
                        fixed cycle after every 25 observations.  No seed.
    random_session(kind, seed, length)
                        at most 32 ops, state ops and observations mixed, the size arguments drawn from small sets that
                        grow, shrink and grow the scratch again.
    run / replay        a session on one handle; one op on a fresh handle that saw the state ops before it and nothing else
    same_bits / differences   the bit-exact comparison
    describe / parse    an op list as Python text, and back

The rule the GPU tests assert with these (tests/test_gpu_sessions_*.py): every observation of a session equals, bit for
bit, replay() of it; at the end the state equals that of a handle that ran the state ops alone.

Three calls are modelled as what a caller has to do to use them at all, because what they return is by their own
definition a fact about an earlier call:
    the tree getters (tree_stats, morton_keys, sort_keys, cells, cell_moments, key_order) describe "the last built tree"
        and refuse without one: each is build_tree() followed by the getter;
    grid_info's `occupied` describes the last built grid: grid_dim and num_cells are compared, `occupied` is not;
    timers() reports times and the steps since enable_timers(): the keys are compared, the values are not.
frame_begin / frame_wait / frame_release are one state op, `frame_async`: a begun frame that is never released would make
a later begin a refusal, and no session contains a call that is meant to be refused.
"""
import ast
import dataclasses
import random
from typing import NamedTuple

import numpy as np

STATE, OBS = "state", "obs"
MAX_LENGTH = 32     # of a random session
STATE_EVERY = 25    # pair walk: observations between two state ops
DT_NBODY, DT_BOIDS = 0.05, 1.0 / 60.0


class Op(NamedTuple):
    name: str
    args: tuple = ()


@dataclasses.dataclass(frozen=True)
class Kind:
    """What the preconditions may ask about a handle.  `label` names the kind in messages and test ids."""
    family: str                 # "nbody" | "boids"
    label: str
    n: int
    # nbody
    tree: bool = True           # Barnes-Hut (False: direct)
    integrator: str = "kick_drift"
    multipole: str = "monopole"
    precision: str = ""         # "" = the handle's default; else set_force_precision(precision, tau) at creation
    tau: float = 0.0            # the threshold of force precision "auto" at which about the denser waves of the case ask
                                # for float64 at dt = DT_NBODY (the library's default is far above these cases' densities)
    link: float = 1.0           # linking length of find_groups / group_catalogue / color_by_groups (<= perception for boids)
    # boids
    periodic: bool = False
    mode: str = "metric"
    eta: float = 0.0
    perception: float = 5.0
    dim: int = 0                # cells per side of the handle's grid
    cell: float = 5.0
    length: float = 0.0         # box length 2 * bounds
    max_speed: float = 25.0


@dataclasses.dataclass(frozen=True)
class Spec:
    name: str
    kind: str                   # STATE | OBS
    cls: str                    # the class of an observation ("state", "force", "tree", "query", ...), "" for state ops
    call: object                # (handle, ctx, *args) -> result
    fixed: object               # (Kind) -> args of the pair walk / of the fixed tests
    draw: object                # (rng, Kind, model) -> args of a random session
    ok: object = None           # (Kind, model, args) -> bool; None: always
    effect: object = None       # (model, args): what a state op changes in the generator's model of the handle
    more: tuple = ()            # further fixed argument tuples that the pair walk visits as ops of their own

    def valid(self, kind, model, args):
        return self.ok is None or bool(self.ok(kind, model, args))


# ---- bit-exact comparison -------------------------------------------------------------------------------------------------
def _words(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    return a


def differences(got, want, where="result"):
    """[] if the two results are the same bits, else a list of where they differ.  float64 is compared through uint64
    views, float32 through uint32 (a NaN equals the same NaN, -0.0 differs from +0.0); tuples, lists, dicts and dataclasses
    member by member; Python floats through their 64 bits."""
    if dataclasses.is_dataclass(got) and not isinstance(got, type):
        if type(got) is not type(want):
            return [f"{where}: {type(got).__name__} != {type(want).__name__}"]
        got, want = dataclasses.asdict(got), dataclasses.asdict(want)
    if isinstance(got, dict):
        if not isinstance(want, dict) or set(got) != set(want):
            return [f"{where}: keys differ"]
        return [d for k in sorted(got) for d in differences(got[k], want[k], f"{where}[{k!r}]")]
    if isinstance(got, (tuple, list)):
        if not isinstance(want, (tuple, list)) or len(got) != len(want):
            return [f"{where}: lengths differ"]
        return [d for i, (g, w) in enumerate(zip(got, want)) for d in differences(g, w, f"{where}[{i}]")]
    if isinstance(got, np.ndarray) or isinstance(want, np.ndarray):
        g, w = np.asarray(got), np.asarray(want)
        if g.dtype != w.dtype or g.shape != w.shape:
            return [f"{where}: {g.dtype}{g.shape} != {w.dtype}{w.shape}"]
        bad = np.flatnonzero(_words(g).reshape(-1) != _words(w).reshape(-1))
        if len(bad):
            i = int(bad[0])
            return [f"{where}: {len(bad)} of {g.size} differ, first at flat index {i}: {g.reshape(-1)[i]!r} != {w.reshape(-1)[i]!r}"]
        return []
    if isinstance(got, float) and isinstance(want, float):
        return [] if np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64) else [f"{where}: {got!r} != {want!r}"]
    if type(got) is not type(want) and not (isinstance(got, (int, np.integer)) and isinstance(want, (int, np.integer))):
        return [f"{where}: {type(got).__name__} != {type(want).__name__}"]
    return [] if got == want else [f"{where}: {got!r} != {want!r}"]


def same_bits(got, want):
    return not differences(got, want)


# ---- describe / parse ---------------------------------------------------------------------------------------------------------
def describe(ops):
    """The op list as Python text: paste it into a test as `SM.parse('''...''')` (or as the literal it is) for an explicit
    case."""
    return "[\n" + "".join(f"    ({op.name!r}, {tuple(op.args)!r}),\n" for op in ops) + "]"


def parse(text):
    return [Op(name, tuple(args)) for name, args in ast.literal_eval(text)]


# ---- the arrays an op names -------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Ctx:
    """A Kind and the base arrays of its case: nbody p, v, m; boids pos, vel, col, params."""
    kind: Kind
    base: dict


def _span(p):
    lo, hi = p.min(axis=0), p.max(axis=0)
    pad = np.where(hi > lo, 0.0625 * (hi - lo), 1.0)
    return lo - pad, hi + pad


def nbody_state(ctx, j):
    """The j-th prepared state: the base rows rotated by j (every body gets another body's place, so the masses meet
    other positions), shifted by j / 64, at half the base velocities rotated the other way."""
    p, v = ctx.base["p"], ctx.base["v"]
    return np.roll(p, j, axis=0) + j / 64.0, 0.5 * np.roll(v, -j, axis=0)


def probe_points(ctx, m, salt=0):
    """m points in the (padded) bounding box of the base positions, the same for the same (case, m, salt)."""
    lo, hi = _span(ctx.base["p"])
    return lo + (hi - lo) * np.random.RandomState(1000 + 7 * salt + m).uniform(size=(m, 3))


def field_size(kind, which):
    return {"one": 1, "some": 63, "many": 3 * kind.n + 5}[which]


def tracer_size(kind, which):
    return {"none": 0, "one": 1, "many": kind.n + 3}[which]


def precision_tau(kind, which):
    """tau of set_force_precision: "keep" the handle's, "case" the kind's (some waves ask), "high" one that no wave reaches"""
    return {"keep": 0.0, "case": kind.tau, "high": 1.0e-3}[which]


def pair_edges(ctx, nb):
    lo, hi = _span(ctx.base["p"])
    return np.linspace(0.0, 0.5 * float(np.linalg.norm(hi - lo)), nb + 1)


def deposit_box(ctx):
    lo, hi = _span(ctx.base["p"])
    return lo, hi


def camera(ctx):
    """Some visible, some not.  N-body: a camera outside the system looking at its centre through a narrow frustum.  Boids
    (whose frustum is wide): a camera at the centre of the flock, so that what lies behind it is not drawn."""
    boids = "pos" in ctx.base
    lo, hi = _span(ctx.base["pos"] if boids else ctx.base["p"])
    c, r = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    return dict(cam_pos=c if boids else c - np.array([0.0, 0.0, 2.0 * r]), cam_forward=(0.0, 0.0, 1.0),
                cam_right=(1.0, 0.0, 0.0), cam_up=(0.0, 1.0, 0.0))


def previous_frame(ctx, j):
    p = np.roll(ctx.base["p"], j, axis=0).astype(np.float32)
    c = np.linspace(0.0, 1.0, 3 * len(p), dtype=np.float32).reshape(-1, 3)
    return p, c


def boids_state(ctx, j):
    """The j-th prepared state: the base rows rotated by j (a rotation keeps every position inside a periodic box),
    velocities rotated the other way, colours as they are."""
    b = ctx.base
    return np.roll(b["pos"], j, axis=0), np.roll(b["vel"], -j, axis=0), b["col"]


def vcorr_edges(kind, nb, reach):
    """nb bins up to just inside `reach` cells"""
    return np.linspace(0.0, kind.cell * (reach - 0.125), nb + 1)


def capacity_of(which, count_bound):
    """catalogue capacities: 0, 1, 64, more than there can be groups"""
    return {"zero": 0, "one": 1, "64": 64, "all": count_bound + 3}[which]


# ---- N-body table -----------------------------------------------------------------------------------------------------------
def _copy2(t):
    return tuple(np.array(a, copy=True) for a in t)


def _built(getter):
    def call(h, ctx, *a):
        h.build_tree()
        return getter(h)
    return call


def _frame_async(h, ctx, kind, max_speed):
    slot = h.frame_begin(kind, max_speed)
    out = _copy2(h.frame_wait(slot))
    h.frame_release(slot)
    return out


def _deposit(h, ctx, dims, scheme):
    lo, hi = deposit_box(ctx)
    return h.deposit(lo, hi, dims, scheme, ("number", "mass", "momentum", "kinetic"), stats=True)


def _catalogue_cap(kind, which):
    return capacity_of(which, kind.n)


def _knn_ok(kind, model, a):
    return kind.tree and 1 <= a[0] <= min(64, kind.n - 1)


def _tree(kind, model, a):
    return kind.tree


def _have_prev(kind, model, a):
    return model["have_prev"]


def _set(key, value=None, index=None):
    def effect(model, a):
        model[key] = value if index is None else a[index]
    return effect


def _pick(*choices):
    return lambda rng, kind, model: rng.choice(choices)


def _none(*_):
    return ()


_N = lambda kind: ()  # noqa: E731
KNN_K = (1, 8, 32)
FIELD_M = ("one", "some", "many")
DEPOSIT_DIMS = ((1, 1, 1), (4, 5, 6), (16, 16, 16))
PAIR_NB = (1, 12, 64)
CAPACITIES = ("zero", "one", "64", "all")
TRACER_M = ("none", "one", "many")
SUBSTEPS = (1, 3)
TOPO_K = (1, 7, 16)


def _fixed_k(kind):
    return (min(8, max(kind.n - 1, 1)),)


NBODY = [
    # ---- state ops
    Spec("step_many", STATE, "", lambda h, c, dt, k: h.step_many(dt, k), lambda kind: (DT_NBODY, 1),
         lambda rng, kind, model: (DT_NBODY, rng.choice(SUBSTEPS))),
    Spec("set_state", STATE, "", lambda h, c, j: h.set_state(*nbody_state(c, j)), lambda kind: (1,),
         lambda rng, kind, model: (rng.choice((1, 2, 5)),)),
    Spec("set_integrator", STATE, "", lambda h, c, name: h.set_integrator(name), lambda kind: ("leapfrog",),
         _pick(("kick_drift",), ("leapfrog",))),
    Spec("set_multipole", STATE, "", lambda h, c, name: h.set_multipole(name),
         lambda kind: ("quadrupole",) if kind.tree else ("monopole",),
         _pick(("monopole",), ("quadrupole",)), ok=lambda kind, model, a: kind.tree or a[0] == "monopole",
         effect=_set("multipole", index=0)),
    Spec("set_force_precision", STATE, "", lambda h, c, mode, which: h.set_force_precision(mode, precision_tau(c.kind, which)),
         lambda kind: ("f64", "keep"), _pick(("auto", "keep"), ("auto", "case"), ("auto", "high"), ("f32", "keep"), ("f64", "keep")),
         ok=_tree),
    Spec("set_tracers", STATE, "",
         lambda h, c, which: h.set_tracers(probe_points(c, tracer_size(c.kind, which), 1),
                                           0.25 * probe_points(c, tracer_size(c.kind, which), 2)),
         lambda kind: ("many",), lambda rng, kind, model: (rng.choice(TRACER_M),)),
    Spec("compute_colors", STATE, "", lambda h, c, s: h.compute_colors(s), lambda kind: (15.0,), _pick((15.0,), (2.0,))),
    Spec("set_color_mode", STATE, "",
         lambda h, c, mode, k: h.set_color_mode(mode, k, (-6.0, 0.0)), lambda kind: ("speed", 8),
         lambda rng, kind, model: rng.choice((("speed", 8), ("density", 1), ("density", 8))),
         ok=lambda kind, model, a: a[0] == "speed" or _knn_ok(kind, model, (a[1],))),
    Spec("color_by_groups", STATE, "", lambda h, c, mm: h.color_by_groups(c.kind.link, mm), lambda kind: (2,),
         _pick((1,), (2,)), ok=_tree),
    Spec("frame_keyframe", STATE, "", lambda h, c: h.frame_keyframe(), _N, _none, effect=_set("have_prev", True)),
    Spec("frame_delta", STATE, "", lambda h, c: h.frame_delta(), _N, _none, ok=_have_prev),
    Spec("frame_set_previous", STATE, "", lambda h, c, j: h.frame_set_previous(*previous_frame(c, j)), lambda kind: (1,),
         _pick((0,), (1,)), effect=_set("have_prev", True)),
    Spec("frame_async", STATE, "", _frame_async, lambda kind: ("f32", 15.0),
         lambda rng, kind, model: (rng.choice(("f32", "key", "delta")), 15.0),
         ok=lambda kind, model, a: a[0] != "delta" or model["have_prev"],
         effect=lambda model, a: model.__setitem__("have_prev", model["have_prev"] or a[0] == "key")),
    # ---- observations
    Spec("get_positions", OBS, "state", lambda h, c: h.get_positions(), _N, _none),
    Spec("get_positions_f64", OBS, "state", lambda h, c: h.get_positions_f64(), _N, _none),
    Spec("get_velocities", OBS, "state", lambda h, c: h.get_velocities(), _N, _none),
    Spec("get_colors", OBS, "state", lambda h, c: h.get_colors(), _N, _none),
    Spec("get_masses", OBS, "state", lambda h, c: h.get_masses(), _N, _none),
    Spec("accelerations", OBS, "force", lambda h, c: h.accelerations(), _N, _none),
    Spec("diagnostics", OBS, "force", lambda h, c, pot: h.diagnostics(potential=pot), lambda kind: (True,),
         _pick((True,), (False,)), more=((False,),)),
    Spec("potentials", OBS, "force", lambda h, c: h.potentials(), _N, _none),
    Spec("field_at", OBS, "probe",
         lambda h, c, which: h.field_at(probe_points(c, field_size(c.kind, which)), potential=True, terms=True),
         lambda kind: ("some",), lambda rng, kind, model: (rng.choice(FIELD_M),)),
    Spec("get_tracers", OBS, "probe", lambda h, c: h.get_tracers(), _N, _none),
    Spec("tracer_positions_f32", OBS, "probe", lambda h, c: h.tracer_positions_f32(), _N, _none),
    Spec("deposit", OBS, "grid", _deposit, lambda kind: ((4, 5, 6), "cic"),
         lambda rng, kind, model: (rng.choice(DEPOSIT_DIMS), rng.choice(("ngp", "cic")))),
    Spec("knn", OBS, "query", lambda h, c, k: h.knn(k), _fixed_k, lambda rng, kind, model: (rng.choice(KNN_K),), ok=_knn_ok),
    Spec("densities", OBS, "query", lambda h, c, k: h.densities(k), _fixed_k, lambda rng, kind, model: (rng.choice(KNN_K),),
         ok=_knn_ok),
    Spec("find_groups", OBS, "query", lambda h, c: (h.find_groups(c.kind.link), h.n_groups), _N, _none, ok=_tree),
    Spec("group_catalogue", OBS, "query",
         lambda h, c, mm, cap: h.group_catalogue(c.kind.link, mm, _catalogue_cap(c.kind, cap)), lambda kind: (2, "64"),
         lambda rng, kind, model: (rng.choice((1, 2)), rng.choice(CAPACITIES)), ok=_tree),
    Spec("pair_counts", OBS, "query", lambda h, c, nb: h.pair_counts(pair_edges(c, nb)), lambda kind: (12,),
         lambda rng, kind, model: (rng.choice(PAIR_NB),), ok=_tree),
    Spec("visible_points", OBS, "state", lambda h, c: _copy2(h.visible_points(tan_h=0.25, tan_v=0.25, far_dist=1e12, **camera(c))),
         _N, _none),
    Spec("build_tree", OBS, "tree", lambda h, c: h.build_tree(), _N, _none, ok=_tree),
    Spec("tree_stats", OBS, "tree", _built(lambda h: h.tree_stats()), _N, _none, ok=_tree),
    Spec("morton_keys", OBS, "tree", _built(lambda h: h.morton_keys()), _N, _none, ok=_tree),
    Spec("sort_keys", OBS, "tree", _built(lambda h: h.sort_keys()), _N, _none, ok=_tree),
    Spec("cells", OBS, "tree", _built(lambda h: h.cells()), _N, _none, ok=_tree),
    Spec("cell_moments", OBS, "tree", _built(lambda h: h.cell_moments()), _N, _none,
         ok=lambda kind, model, a: kind.tree and model["multipole"] == "quadrupole"),
    Spec("key_order", OBS, "tree", _built(lambda h: h.key_order()), _N, _none, ok=_tree),
    Spec("force_precision_share", OBS, "meta", lambda h, c: h.force_precision_share(), _N, _none, ok=_tree),
    Spec("step_count", OBS, "meta", lambda h, c: h.step_count(), _N, _none),
    Spec("enable_timers", OBS, "meta", lambda h, c, on: h.enable_timers(on), lambda kind: (True,), _pick((True,), (False,))),
    Spec("timers", OBS, "meta", lambda h, c, reset: sorted(h.timers(reset)), lambda kind: (False,), _pick((True,), (False,))),
]


# ---- boids table --------------------------------------------------------------------------------------------------------------
def _periodic(kind, model, a):
    return kind.periodic


def _walled(kind, model, a):
    return not kind.periodic


def _view(x):
    return np.array(x, copy=True)


def _flock_cap(kind, which):
    return capacity_of(which, kind.n)


def _vcorr(h, c, nb, reach):
    return h.velocity_correlation(vcorr_edges(c.kind, nb, reach))


def max_reach(kind):
    """the largest reach (cells) a correlation may have on this kind: 16, on a periodic handle 2 m + 1 <= dim and the last
    edge below half the box"""
    if not kind.periodic:
        return min(16, max(kind.dim, 1))
    return max(0, min(16, (kind.dim - 1) // 2))


def _vcorr_ok(kind, model, a):
    nb, reach = a
    return 1 <= nb <= 64 and 1 <= reach <= max_reach(kind)


def _grid_info(h, c):
    g = h.grid_info()
    return {"grid_dim": g["grid_dim"], "num_cells": g["num_cells"]}


def _visible(h, c, cam):
    if not cam:
        return _copy2(h.visible_vertices())
    return _copy2(h.visible_vertices(fov=40.0, aspect=1.0, **camera(c)))


def _link_of(kind, which):
    return {"link": kind.link, "sight": kind.perception}[which]


def _link_args(kind):
    return ("link",)


_LINKS = _pick(("link",), ("sight",))


def _update_ok(kind, model, a):
    return not kind.periodic or kind.max_speed * abs(a[0]) < kind.length


BOIDS = [
    Spec("update", STATE, "", lambda h, c, dt, k: h.update(dt, k), lambda kind: (DT_BOIDS, 1),
         lambda rng, kind, model: (DT_BOIDS, rng.choice(SUBSTEPS)), ok=_update_ok),
    Spec("set_state", STATE, "", lambda h, c, j: h.set_state(*boids_state(c, j)), lambda kind: (1,),
         lambda rng, kind, model: (rng.choice((1, 2, 5)),)),
    Spec("set_neighbour_mode", STATE, "", lambda h, c, mode, k: h.set_neighbour_mode(mode, k), lambda kind: ("topological", 7),
         lambda rng, kind, model: (rng.choice(("metric", "topological")), rng.choice(TOPO_K))),
    Spec("set_noise", STATE, "", lambda h, c, eta, seed, step: h.set_noise(eta, seed, step), lambda kind: (0.5, 9, None),
         lambda rng, kind, model: (rng.choice((0.0, 0.5, 2.0)), rng.choice((0, 9, 2 ** 40 + 1)), rng.choice((None, None, 0, 5)))),
    Spec("positions", OBS, "state", lambda h, c: _view(h.positions), _N, _none),
    Spec("velocities", OBS, "state", lambda h, c: _view(h.velocities), _N, _none),
    Spec("colors", OBS, "state", lambda h, c: _view(h.colors), _N, _none),
    Spec("cell_indices", OBS, "grid", lambda h, c: h.cell_indices(), _N, _none),
    Spec("forces", OBS, "force", lambda h, c: h.forces(), _N, _none),
    Spec("grid_info", OBS, "grid", _grid_info, _N, _none),
    Spec("flocks", OBS, "flocks", lambda h, c, w: h.flocks(_link_of(c.kind, w)), _link_args, _LINKS, ok=_walled),
    Spec("flock_catalogue", OBS, "flocks",
         lambda h, c, w, mm, cap: h.flock_catalogue(_link_of(c.kind, w), mm, _flock_cap(c.kind, cap)),
         lambda kind: ("link", 2, "64"),
         lambda rng, kind, model: (rng.choice(("link", "sight")), rng.choice((1, 2)), rng.choice(CAPACITIES)), ok=_walled),
    Spec("diagnostics", OBS, "flocks", lambda h, c: h.diagnostics(), _N, _none),
    Spec("neighbour_stats", OBS, "flocks", lambda h, c, w: h.neighbour_stats(_link_of(c.kind, w)), _link_args, _LINKS, ok=_walled),
    Spec("periodic_flocks", OBS, "flocks", lambda h, c, w: h.periodic_flocks(_link_of(c.kind, w)), _link_args, _LINKS,
         ok=_periodic),
    Spec("periodic_flock_catalogue", OBS, "flocks",
         lambda h, c, w, mm, cap: h.periodic_flock_catalogue(_link_of(c.kind, w), mm, _flock_cap(c.kind, cap)),
         lambda kind: ("link", 2, "64"),
         lambda rng, kind, model: (rng.choice(("link", "sight")), rng.choice((1, 2)), rng.choice(CAPACITIES)), ok=_periodic),
    Spec("periodic_neighbour_stats", OBS, "flocks", lambda h, c, w: h.periodic_neighbour_stats(_link_of(c.kind, w)),
         _link_args, _LINKS, ok=_periodic),
    Spec("heading_moments", OBS, "correlation", lambda h, c: h.heading_moments(), _N, _none),  # the correlation with nb = 0
    Spec("velocity_correlation", OBS, "correlation", _vcorr, lambda kind: (12, min(2, max_reach(kind))),
         lambda rng, kind, model: (rng.choice(PAIR_NB), rng.choice(tuple(range(1, min(3, max_reach(kind)) + 1)) or (1,))),
         ok=_vcorr_ok),
    Spec("topological_neighbours", OBS, "topological", lambda h, c, k: h.topological_neighbours(k), lambda kind: (7,),
         lambda rng, kind, model: (rng.choice(TOPO_K),)),
    Spec("noise_vectors", OBS, "noise", lambda h, c, step: h.noise_vectors(step), lambda kind: (None,), _pick((None,), (3,))),
    Spec("noise", OBS, "noise", lambda h, c: h.noise, _N, _none),
    Spec("neighbour_mode", OBS, "meta", lambda h, c: h.neighbour_mode, _N, _none),
    Spec("box", OBS, "meta", lambda h, c: h.box, _N, _none),
    Spec("visible_vertices", OBS, "state", _visible, lambda kind: (True,), _pick((True,), (False,))),
    Spec("enable_timers", OBS, "meta", lambda h, c, on: h.enable_timers(on), lambda kind: (True,), _pick((True,), (False,))),
    Spec("timers", OBS, "meta", lambda h, c, reset: sorted(h.timers(reset)), lambda kind: (False,), _pick((True,), (False,))),
]

TABLES = {"nbody": {s.name: s for s in NBODY}, "boids": {s.name: s for s in BOIDS}}
# the short fixed cycle of state ops of the pair walk (names; the arguments are each op's `fixed`, except where given)
STATE_CYCLE = {
    "nbody": [Op("step_many", (DT_NBODY, 1)), Op("step_many", (DT_NBODY, 3)), Op("set_state", (1,)), Op("set_multipole", ("quadrupole",)),
              Op("step_many", (DT_NBODY, 1)), Op("set_tracers", ("many",)), Op("set_integrator", ("leapfrog",)),
              Op("step_many", (DT_NBODY, 1)), Op("compute_colors", (15.0,)), Op("set_multipole", ("monopole",)),
              Op("set_force_precision", ("f64", "keep")), Op("step_many", (DT_NBODY, 1)), Op("frame_keyframe", ()),
              Op("set_integrator", ("kick_drift",)), Op("set_force_precision", ("auto", "case")), Op("set_tracers", ("none",))],
    "boids": [Op("update", (DT_BOIDS, 1)), Op("update", (DT_BOIDS, 3)), Op("set_state", (1,)), Op("set_neighbour_mode", ("topological", 7)),
              Op("update", (DT_BOIDS, 1)), Op("set_noise", (0.5, 9, None)), Op("update", (DT_BOIDS, 1)),
              Op("set_neighbour_mode", ("metric", 7)), Op("set_noise", (0.0, 0, None))],
}


def new_model(kind):
    return {"have_prev": False, "multipole": kind.multipole} if kind.family == "nbody" else {}


def spec_of(kind, op):
    return TABLES[kind.family][op.name]


def apply_effect(kind, model, op):
    s = spec_of(kind, op)
    if s.kind == STATE and s.effect:
        s.effect(model, op.args)


def applicable(kind, which=None):
    """The specs of the kind's family that have at least one valid call on this kind (in a model where everything a
    state op can switch on is on), in table order; `which`: STATE or OBS only."""
    model = new_model(kind)
    model.update(have_prev=True, multipole="quadrupole" if kind.tree else "monopole")
    out = []
    for s in TABLES[kind.family].values():
        if which and s.kind != which:
            continue
        if s.valid(kind, model, tuple(s.fixed(kind))):
            out.append(s)
    return out


def invalid(kind, ops):
    """The positions of the ops whose precondition does not hold where they stand (the model follows the state ops)."""
    model, bad = new_model(kind), []
    for i, op in enumerate(ops):
        if op.name not in TABLES[kind.family] or not spec_of(kind, op).valid(kind, model, op.args):
            bad.append(i)
        else:
            apply_effect(kind, model, op)
    return bad


# ---- generators ---------------------------------------------------------------------------------------------------------------
def pair_sequence(m):
    """A cyclic sequence of length m * m over 0 .. m - 1 in which every ordered pair (a, b), a == b included, is adjacent
    exactly once: the Lyndon words of length 1 and 2 in order (a; a b for b > a), the Eulerian circuit of the complete
    digraph with loops.  A stretch of 25 holds about 13 different symbols, not 25, which is what keeps the replays few."""
    seq = []
    for a in range(m):
        seq.append(a)
        for b in range(a + 1, m):
            seq += [a, b]
    return seq


def walk_ops(kind):
    """The observations of the pair walk: every applicable one at its fixed arguments (and at its `more`); cell_moments
    only on a kind that is created in quadrupole mode."""
    out = []
    for s in applicable(kind, OBS):
        if s.name == "cell_moments" and kind.multipole != "quadrupole":
            continue
        out += [Op(s.name, tuple(a)) for a in (tuple(s.fixed(kind)),) + tuple(s.more)]
    return out


def pair_walk(kind, ops=None):
    """The closed walk over the kind's observations at their fixed arguments (or over `ops`), a state op of STATE_CYCLE
    after every STATE_EVERY observations (those that are valid for the kind where they stand; others are passed over)."""
    model = new_model(kind)
    if ops is None:
        ops = walk_ops(kind)
    seq = pair_sequence(len(ops))
    out, cycle, c = [], STATE_CYCLE[kind.family], 0
    for i, a in enumerate(seq + seq[:1]):
        if i and i % STATE_EVERY == 0:
            for _ in range(len(cycle)):
                st = cycle[c % len(cycle)]
                c += 1
                # a walk that contains cell_moments stays in quadrupole mode: the walk's ops keep their preconditions
                keeps = not (st.name == "set_multipole" and any(o.name == "cell_moments" for o in ops))
                if keeps and spec_of(kind, st).valid(kind, model, st.args):
                    out.append(st)
                    apply_effect(kind, model, st)
                    break
        out.append(ops[a])
    return out


def split_walk(kind, walk, parts):
    """The walk cut into `parts` sessions of about the same number of observations, for tests that have to stay short.  A
    piece starts with the state ops that stand before it in the walk (a handle that has seen them and nothing else) and
    with the last observation of the piece before it, so no ordered pair is lost at a cut."""
    obs = [i for i, op in enumerate(walk) if not is_state(kind, op)]
    cuts = [obs[len(obs) * k // parts] for k in range(parts)] + [len(walk)]
    out = []
    for k in range(parts):
        first = cuts[k]
        if k:
            first = max(i for i in obs if i < cuts[k])  # the observation before the cut, again
        out.append(list(state_prefix(kind, walk, first)) + walk[first:cuts[k + 1]])
    return out


def fixed_tour(kind, rounds=2):
    """Every op of the kind's table that is valid where it stands, once, in table order, at its fixed arguments (and its
    `more`), `rounds` times over."""
    model, out = new_model(kind), []
    for _ in range(rounds):
        for s in TABLES[kind.family].values():
            for args in (tuple(s.fixed(kind)),) + tuple(s.more):
                if s.valid(kind, model, args):
                    out.append(Op(s.name, args))
                    apply_effect(kind, model, out[-1])
    return out


def random_session(kind, seed, length=MAX_LENGTH):
    """`length` (at most 32) valid ops.  Two decks, the applicable state ops and the applicable observations, each
    shuffled by the seed and dealt in turn (two observations to one state op, reshuffled when a deck runs out); an op that
    is not valid where it stands goes to the bottom of its deck.  The arguments are drawn by each op's `draw`.  Everything
    comes from random.Random(seed): the same seed gives the same list."""
    assert 0 < length <= MAX_LENGTH
    rng = random.Random(f"{kind.label}/{seed}")  # (a string seeds through SHA-512: the same on every machine)
    decks = {STATE: [s.name for s in applicable(kind, STATE)], OBS: [s.name for s in applicable(kind, OBS)]}
    piles = {STATE: [], OBS: []}
    model, out = new_model(kind), []
    pattern = rng.choice(((OBS, OBS, STATE), (OBS, STATE, OBS), (STATE, OBS, OBS)))
    while len(out) < length:
        which = pattern[len(out) % 3]
        for _ in range(4 * len(decks[which])):
            if not piles[which]:
                piles[which] = list(decks[which])
                rng.shuffle(piles[which])
            name = piles[which].pop()
            s = TABLES[kind.family][name]
            args = tuple(s.draw(rng, kind, model))
            if s.valid(kind, model, args):
                out.append(Op(name, args))
                apply_effect(kind, model, out[-1])
                break
        else:
            raise AssertionError(f"{kind.label}: no valid {which} op")
    return out


# ---- running ------------------------------------------------------------------------------------------------------------------
def is_state(kind, op):
    return spec_of(kind, op).kind == STATE


def state_prefix(kind, ops, upto):
    return tuple(op for op in ops[:upto] if is_state(kind, op))


def call(handle, ctx, op):
    return spec_of(ctx.kind, op).call(handle, ctx, *op.args)


def run(handle_factory, ctx, ops, each=None):
    """The ops in order on one handle of `handle_factory()`; each(position, op, result, handle) after every op (default:
    collect).  Returns (results, final) - `final` is handle_factory.state(handle) - and closes the handle."""
    h = handle_factory()
    results = []
    try:
        for i, op in enumerate(ops):
            r = call(h, ctx, op)
            if each:
                each(i, op, r, h)
            else:
                results.append(r)
        return results, handle_factory.state(h)
    finally:
        h.close()


def replay(handle_factory, ctx, ops, upto, with_state=False):
    """ops[upto] on a fresh handle on which only the state ops before position `upto` were applied.  with_state: also
    handle_factory.state() of that handle, fetched after the op (for the host references)."""
    h = handle_factory()
    try:
        for op in state_prefix(ctx.kind, ops, upto):
            call(h, ctx, op)
        r = call(h, ctx, ops[upto])
        return (r, handle_factory.state(h)) if with_state else r
    finally:
        h.close()


class Replays:
    """replay() cached per (state-op prefix, op): the pair walk asks for the same one many times."""

    def __init__(self, handle_factory, ctx, with_state=False):
        self.factory, self.ctx, self.with_state, self.cache = handle_factory, ctx, with_state, {}

    def get(self, ops, upto):
        key = (state_prefix(self.ctx.kind, ops, upto), ops[upto])
        fresh = key not in self.cache
        if fresh:
            self.cache[key] = replay(self.factory, self.ctx, ops, upto, self.with_state)
        return self.cache[key], fresh


def failure(ctx, what, position, ops, diffs):
    """The assertion message: the reproduction itself."""
    return (f"{ctx.kind.label} n={ctx.kind.n} {what}: op {position} {ops[position].name}{ops[position].args} differs from a fresh "
            f"handle's: {'; '.join(diffs[:3])}\nreproduce with SM.parse('''{describe(ops[:position + 1])}''')")


def check_session(handle_factory, ctx, ops, what, replays=None, anchor=None):
    """The rule.  Every observation of the session against replay(); the values the state ops return and the final state
    against a handle that ran the state ops alone.  anchor(op, result, state): the host reference of an observation, called
    once per new replay with the replay handle's state.  Returns the number of replays made."""
    kind = ctx.kind
    assert not invalid(kind, ops), (kind.label, what, invalid(kind, ops))
    replays = replays or Replays(handle_factory, ctx, with_state=anchor is not None)
    made = [0]
    state_results = []

    def each(i, op, r, h):
        if is_state(kind, op):
            state_results.append((i, r))
            return
        want, fresh = replays.get(ops, i)
        made[0] += fresh
        state = None
        if replays.with_state:
            want, state = want
        d = differences(r, want)
        assert not d, failure(ctx, what, i, ops, d)
        if fresh and anchor is not None:
            anchor(op, want, state, failure(ctx, what + " (host reference)", i, ops, ["see above"]))
    _, final = run(handle_factory, ctx, ops, each)
    alone = [(i, op) for i, op in enumerate(ops) if is_state(kind, op)]
    want_results, want_final = run(handle_factory, ctx, [op for _, op in alone])
    for (i, r), w in zip(state_results, want_results):
        d = differences(r, w)
        assert not d, failure(ctx, what + " (state op's own result)", i, ops, d)
    d = differences(final, want_final, "state")
    assert not d, failure(ctx, what + " (final state against the state ops alone)", len(ops) - 1, ops, d)
    return made[0]
