"""The handle kinds, inputs, handle factories and host references of the session tests (tests/session_model.py,
tests/test_gpu_sessions_nbody.py, tests/test_gpu_sessions_boids.py, tests/test_session_model_host.py).  A plain helper
module: the kinds and inputs need NumPy only, the factories import the package when they are called.

Sizes (no larger than these): N-body 1, 2, 65 (two waves), 257, 2049 (one body past the 2 048-body sort tile), 4097, and
the 4 096 of query_cases.trap; boids 1, 2, 257, 2049 (the 2 048-boid cell-table tile), 4097 (the 4 096-member reduction
chunk).
"""
import numpy as np

import boids_cases as BC
import periodic_ref as PR
import query_cases as qc
import session_model as SM
import torus_cases as TC

# the seeds of the random sessions: a committed list, chosen so that tests/test_session_model_host.py's conditions hold
SEEDS = (2, 11, 12, 13, 14, 15, 36, 53, 150, 207, 224, 16)
SEEDS_PER_TEST = 3
ANCHOR_MAX_N = 257  # up to here every observation with an exact host reference is also compared with it

# ---- N-body -------------------------------------------------------------------------------------------------------------------
G, EPS, THETA = 0.07, 1.5, 0.5  # query_cases.bh's constants
NBODY_SYSTEMS = {  # name -> (system of query_cases or None, linking length of test_gpu_fof.CASES where it has one)
    "n1": 1.0, "n2": 5.0, "n65": 30.0, "n257": 20.0, "n2049": 8.0, "n4097": 8.0, "far": 5.0, "trap": 50.0,
}
NBODY_SIZES = {"n1": 1, "n2": 2, "n65": 65, "n257": 257, "n2049": 2049, "n4097": 4097, "far": 4097, "trap": 4096}
NBODY_KINDS = {  # label -> (tree, integrator, multipole, precision)
    "bh": (True, "kick_drift", "monopole", ""),
    "bh_leapfrog": (True, "leapfrog", "monopole", ""),
    "bh_quadrupole": (True, "kick_drift", "quadrupole", ""),
    "bh_auto": (True, "kick_drift", "monopole", "auto"),
    "bh_f64": (True, "kick_drift", "monopole", "f64"),
    "direct": (False, "kick_drift", "monopole", ""),
    "direct_leapfrog": (False, "leapfrog", "monopole", ""),
}
_NB = {}


def nbody_base(system):
    """p, v, m of a system, made once (read only).  The systems of query_cases are at rest: the velocities here are a
    fixed normal draw, a few units against positions of +-100."""
    if system not in _NB:
        p, m = qc.uniform(257, 7) if system == "n257" else qc.system(system)
        v = np.random.RandomState(900 + len(p)).normal(0.0, 2.0, (len(p), 3))
        _NB[system] = dict(p=np.ascontiguousarray(p, np.float64), v=v, m=np.ascontiguousarray(m, np.float64))
    return _NB[system]


def case_tau(system):
    """G rho dt^2 at the mean density of the quarter of the bodies nearest the median position (their bounding box): the
    "auto" rule looks at the densest quarter of each wave, so on these cases some waves lie above it and some below"""
    b = nbody_base(system)
    p, m = b["p"], b["m"]
    if len(p) < 8:
        return 1.0e-9
    if system in ("trap", "far"):  # two scales: the mean density of the whole box separates the ball from the rest
        return float(G * m.sum() / np.prod(p.max(axis=0) - p.min(axis=0)) * SM.DT_NBODY ** 2)
    near =np.argsort(np.abs(p - np.median(p, axis=0)).max(axis=1))[:len(p) // 4]
    ext = np.maximum(p[near].max(axis=0) - p[near].min(axis=0), 1e-300)
    return float(G * m[near].sum() / np.prod(ext) * SM.DT_NBODY ** 2)


def nbody_kind(label, system):
    tree, integrator, multipole, precision = NBODY_KINDS[label]
    return SM.Kind("nbody", f"{label}/{system}", NBODY_SIZES[system], tree=tree, integrator=integrator, multipole=multipole,
                   precision=precision, tau=case_tau(system), link=NBODY_SYSTEMS[system])


def nbody_ctx(label, system):
    return SM.Ctx(nbody_kind(label, system), nbody_base(system))


class NBodyFactory:
    """A fresh handle of the kind on the case's base state; state(): what a session must leave as the state ops alone do."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __call__(self):
        from nbody.gpu_backend import HIPBarnesHutSimulation, HIPDirectSimulation
        k, b = self.ctx.kind, self.ctx.base
        if k.tree:
            h = HIPBarnesHutSimulation(b["p"], b["v"], b["m"], G, EPS, 1.0, THETA, integrator=k.integrator, multipole=k.multipole)
            if k.precision:
                h.set_force_precision(k.precision, k.tau)
        else:
            h = HIPDirectSimulation(b["p"], b["v"], b["m"], G, EPS, 1.0, integrator=k.integrator)
        return h

    def state(self, h):
        out = dict(positions=h.get_positions_f64(), velocities=h.get_velocities(), colors=h.get_colors(),
                   tracers=h.get_tracers(), step_count=h.step_count())
        if self.ctx.kind.tree:
            out["force_precision_share"] = h.force_precision_share()
        return out


def nbody_anchor(ctx):
    """anchor(op, result, state, message) of SM.check_session: the observations that have an exact host reference, against
    it, on the state the replay handle had (equality, as in each feature's own suite; mass_k of unequal masses is a sum in
    the walk's order and has no exact reference: r2_k alone)."""
    import deposit_ref as DR
    import fof_ref as FR
    import knn_ref as KR
    import pairs_ref as PAIRS
    m = ctx.base["m"]

    def anchor(op, result, state, message):
        p, v = state["positions"], state["velocities"]
        if op.name == "knn":
            assert SM.same_bits(result[0], KR.knn(p, m, op.args[0])[0]), message
        elif op.name == "find_groups":
            lab, ng = FR.fof(p, ctx.kind.link)
            assert np.array_equal(result[0], lab) and result[1] == ng, message
        elif op.name == "group_catalogue":
            want = FR.catalogue(p, v, m, FR.fof(p, ctx.kind.link)[0], op.args[0])
            rows = min(want["count"], SM.capacity_of(op.args[1], ctx.kind.n))
            assert result["count"] == want["count"] and np.array_equal(result["label"], want["label"][:rows]), message
            assert np.array_equal(result["members"], want["members"][:rows]), message
        elif op.name == "pair_counts":
            counts, below = PAIRS.pair_counts(p, SM.pair_edges(ctx, op.args[0]))
            assert np.array_equal(result[0], counts) and result[1] == below, message
        elif op.name == "deposit":
            lo, hi = SM.deposit_box(ctx)
            out, stats, ex = DR.deposit(p, v, m, lo, hi, op.args[0], DR.CIC if op.args[1] == "cic" else DR.NGP, DR.ALL)
            got = np.concatenate([result["number"][None], result["mass"][None], result["momentum"], result["kinetic"][None]])
            assert SM.same_bits(got, out) and np.array_equal(result["exponents"], ex), message
            assert result["stats"] == tuple(int(x) for x in stats), message
    return anchor


# ---- boids --------------------------------------------------------------------------------------------------------------------
BOIDS_KINDS = {  # label -> (periodic, mode, eta)
    f"{box}_{mode}{'_noise' if eta else ''}": (box == "periodic", mode, eta)
    for box in ("walled", "periodic") for mode in ("metric", "topological") for eta in (0.0, 0.5)
}
BOIDS_SIZES = (1, 2, 257, 2049, 4097)
WALLED_LINK = 2.5
_BD = {}


def _walled_case(n):
    """Half the boids in clumps (boids_cases._clumpy), half uniform, in a box of bounds 20 (10 cells per side), from 2 049
    on bounds 30 (14 cells): flocks of many sizes at link 2.5.  n = 2: two boids 2 apart (linked); n = 1: one boid."""
    rng = np.random.default_rng(300 + n)
    b = 20.0 if n <= 257 else 30.0
    prm = BC.params(bounds=b)
    if n <= 2:
        pos = np.array([[1.0, 2.0, 3.0], [1.0, 4.0, 3.0]])[:n]
    else:
        pos = np.concatenate([BC._clumpy(rng, n // 2, b, 2.0), rng.uniform(-b, b, (n - n // 2, 3))])
    c = BC._case(f"walled_{n}", np.clip(pos, -b, b), prm, rng)
    c["link"] = WALLED_LINK
    return c


def _periodic_case(n):
    """torus_cases.sizes (the box of 3 cells per side) up to 257, torus_cases.mixed (7 cells per side) above."""
    return dict(TC.sizes(n)) if n <= 257 else dict(TC.mixed(n))


def boids_base(periodic, n):
    if (periodic, n) not in _BD:
        _BD[periodic, n] = _periodic_case(n) if periodic else _walled_case(n)
    return _BD[periodic, n]


def boids_kind(label, n):
    periodic, mode, eta = BOIDS_KINDS[label]
    c = boids_base(periodic, n)
    P = dict(zip(BC.R._KEYS, (float(x) for x in c["params"])))
    if periodic:
        _, length, dim, cell = PR.box(c["params"])
    else:
        cell, dim, _ = BC.R.grid(c["params"])
        length = 2.0 * P["bounds"]
    return SM.Kind("boids", f"{label}/n{n}", n, periodic=periodic, mode=mode, eta=eta, link=float(c["link"]),
                   perception=P["perception_radius"], dim=int(dim), cell=float(cell), length=float(length),
                   max_speed=P["max_speed"])


def boids_ctx(label, n):
    periodic = BOIDS_KINDS[label][0]
    return SM.Ctx(boids_kind(label, n), boids_base(periodic, n))


class BoidsFactory:
    """A fresh boids.Flock with the case's constants (config.BOIDS is put back at once) on the case's state, in the kind's
    neighbour mode and noise."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __call__(self):
        from boids import Flock
        import config.boids as config
        k, c = self.ctx.kind, self.ctx.base
        saved = dict(config.BOIDS)
        config.BOIDS.update(dict(zip(config.PARAM_ORDER, (float(x) for x in c["params"]))))
        try:
            f = Flock(k.n, seed=1, periodic=k.periodic)
        finally:
            config.BOIDS.clear()
            config.BOIDS.update(saved)
        try:
            f.set_state(c["pos"], c["vel"], c["col"])
            if k.mode == "topological":
                f.set_neighbour_mode("topological", 7)
            if k.eta:
                f.set_noise(k.eta, seed=5)
        except Exception:
            f.close()
            raise
        return f

    def state(self, h):
        h._cache = None  # (the Python object keeps the last fetched state: fetch again)
        return dict(positions=h.positions.copy(), velocities=h.velocities.copy(), colors=h.colors.copy(), noise=h.noise)


def boids_anchor(ctx):
    """As nbody_anchor.  The catalogue's rows are sums in the handle's row order, which no host reference knows after a
    step: count, labels and members are compared."""
    import boids_ref as R
    import flockstats_ref as FS
    import noise_ref as NR
    import topo_ref as T
    import torus_ref as TR
    import vcorr_ref as VR
    k, prm = ctx.kind, ctx.base["params"]
    memo = {}

    def analysis(p, link):
        key = (p.tobytes(), link)
        if key not in memo:
            memo.clear()
            memo[key] = TR.analyse(p, prm, link) if k.periodic else FS.analyse(p, link)
        return memo[key]

    def anchor(op, result, state, message):
        p, v = state["positions"], state["velocities"]
        name = op.name[len("periodic_"):] if op.name.startswith("periodic_") else op.name
        if name == "cell_indices":
            assert np.array_equal(result, (PR if k.periodic else R).cell_index(p, prm)), message
        elif name == "flocks":
            a = analysis(p, SM._link_of(k, op.args[0]))
            assert np.array_equal(result["labels"], a["labels"]), message
            assert (result["n_flocks"], result["links"]) == (a["n_flocks"], a["links"]), message
        elif name == "neighbour_stats":
            a = analysis(p, SM._link_of(k, op.args[0]))
            assert np.array_equal(result["count"], a["count"]) and SM.same_bits(result["nn_d2"], a["nn_d2"]), message
        elif name == "flock_catalogue":
            lab = analysis(p, SM._link_of(k, op.args[0]))["labels"]
            want = TR.catalogue(p, v, lab, prm, op.args[1]) if k.periodic else FS.catalogue(p, v, lab, op.args[1])
            rows = min(want["count"], SM.capacity_of(op.args[2], k.n))
            assert result["count"] == want["count"] and np.array_equal(result["label"], want["label"][:rows]), message
            assert np.array_equal(result["members"], want["members"][:rows]), message
        elif name == "topological_neighbours":
            want = (PR if k.periodic else T).neighbours(p, prm, op.args[0])
            assert np.array_equal(result["ids"], want["ids"]) and SM.same_bits(result["d2"], want["d2"]), message
            assert np.array_equal(result["count"], want["count"]), message
        elif name == "velocity_correlation":
            want = VR.correlate(p, v, prm, SM.vcorr_edges(k, *op.args), result["mean"], k.periodic)
            assert [int(x) for x in result["pairs"]] == [int(x) for x in want["pairs"]] and result["dot"] == want["dot"], message
            assert (result["evals"], result["qsum"], result["qsq"]) == (want["evals"], want["qsum"], want["qsq"]), message
        elif name == "noise_vectors":
            seed, step = state["noise"][1], state["noise"][2] if op.args[0] is None else op.args[0]
            assert SM.same_bits(result, NR.vectors(seed, step, np.arange(k.n))[0]), message
    return anchor


# ---- which seeds a (kind, size) test runs ---------------------------------------------------------------------------------------
def seeds_of(index):
    """SEEDS_PER_TEST consecutive seeds of SEEDS for the index-th size of a kind: every seed is run by some size of it"""
    return tuple(SEEDS[(SEEDS_PER_TEST * index + j) % len(SEEDS)] for j in range(SEEDS_PER_TEST))
