"""The grid-free boids reference (tests/boids_ref.py) and the constructed edge cases
(tests/boids_cases.py), checked on the host: against the reference's goldens, against the CPU oracle
(oracle/bdref.c), and for reaching the kernel branch each case is named for.

Comparisons: on the lattice inputs the alignment, cohesion and colour sums are exact in any order,
so ali / coh / avg must be bit-identical; the separation force is held to boids_ref.sep_bound
(summation order is the only difference).  The goldens are not lattice inputs: 1e-12 relative to
the largest value there.
"""
import numpy as np
import pytest

import boids_cases as BC
import boids_ref as R
from conftest import golden


@pytest.mark.parametrize("tag", ["sparse", "dense", "walls"])
def test_reference_reproduces_goldens(oracle, tag):
    g = golden("boids_" + tag)
    params = oracle.boids_params(bounds=float(g["bounds"]))
    F = R.flocking(g["pos_0"], g["vel_0"], g["col_0"], params)
    for mine, key in ((F.sep, "sep_1"), (F.ali, "ali_1"), (F.coh, "coh_1"), (F.avg, "avg_1")):
        ref = g[key]
        assert np.abs(mine - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), key
    assert np.array_equal(R.cell_index(g["pos_0"], params), g["cell_indices_1"])
    # physics() on the golden forces gives the golden state (ulp tolerance: see test_oracle_boids)
    p, v, c = R.physics(g["pos_0"], g["vel_0"], g["col_0"], (g["sep_1"], g["ali_1"], g["coh_1"], g["avg_1"]), params,
                        float(g["dt"]))
    for mine, key in ((p, "pos_1"), (v, "vel_1"), (c, "col_1")):
        assert np.allclose(mine, g[key], rtol=4e-16, atol=1e-15), key


_BUILDERS = {
    **{f"run_length_{c}": (lambda c=c: BC.run_length(c)) for c in (4094, 4095, 4096, 4097)},
    "mixed_lanes": BC.mixed_lanes,
    "hit_list": BC.hit_list,
    "thresholds": BC.thresholds,
    **{f"grid_{d}": (lambda d=d: BC.grid_dims(d)) for d in (3, 4, 31, 32, 33, 34, 63, 64, 65)},
    **{c["name"]: (lambda name=c["name"]: next(x for x in BC.parameter_cases() if x["name"] == name))
       for c in BC.parameter_cases()},
}


def test_host_cases_cover_the_list():
    assert sorted(c["name"] for c in BC.host_cases()) == sorted(_BUILDERS)


@pytest.mark.parametrize("name", sorted(_BUILDERS))
def test_reference_matches_oracle(oracle, name):
    """Same inputs, same rules: bit-exact on ali / coh / avg, bounded on sep; physics() of the
    oracle's forces is the oracle's next state, bit for bit."""
    c = _BUILDERS[name]()
    st = oracle.FlockStepper(c["pos"], c["vel"], c["col"], c["params"], use_numpy_argsort=True)
    st.step(c["dt"])
    F = R.flocking(c["pos"], c["vel"], c["col"], c["params"])
    assert R.same_bits(F.ali, st.ali), name
    assert R.same_bits(F.coh, st.coh), name
    assert R.same_bits(F.avg, st.avg), name
    R.check_sep(st.sep, F, c["vel"], c["params"], name)
    p, v, col = R.physics(c["pos"], c["vel"], c["col"], (st.sep, st.ali, st.coh, st.avg), c["params"], c["dt"])
    assert R.same_bits(p, st.pos) and R.same_bits(v, st.vel) and R.same_bits(col, st.col), name


def _reaches(name, c, F, gf):
    """The NumPy statement of what the case is for."""
    n = len(c["pos"])
    if name.startswith("run_length_"):
        count = int(name.rsplit("_", 1)[1])
        assert gf["runs"].max() == count  # the crowded cell's row is exactly `count` boids long
        assert gf["big"].any() == (count > 4095)
        assert (F.nb > 2000).sum() >= count  # its boids see two thirds of it
    elif name == "mixed_lanes":
        assert (gf["runs"] >= 8200).any() and gf["big"].any() and not gf["big"].all()
        waves = gf["big"][gf["order"]][: n // 64 * 64].reshape(-1, 64)
        assert (waves.any(axis=1) & ~waves.all(axis=1)).any()  # a wavefront with both kinds of lane
    elif name == "hit_list":
        for k in (0, 1, 27, 28, 29, 31, 32, 33, 63, 64, 80):
            assert (F.nb == k).any(), k
        assert F.nb.max() == 80 and not gf["big"].any()
        assert {int(x) % 4 for x in gf["candidates"]} == {0, 1, 2, 3}
    elif name == "thresholds":
        d = c["pos"][:, None] - c["pos"][None]
        dsq = (d * d).sum(axis=2)
        for v in (25.0, 9.0, 0.0, 2.0 ** -13, 2.0 ** -14):
            assert (dsq == v).any(), v
        assert (F.nb == 0).any() and (F.nsep == 1).any() and ((F.nb == 1) & (F.nsep == 0)).any()
    elif name.startswith("grid_"):
        dim = int(name.split("_")[1])
        assert R.grid(c["params"])[1] == dim
        cc = R.cell_coords(c["pos"], c["params"])
        border = np.unique(gf["cells"][np.any((cc == 0) | (cc == dim - 1), axis=1)])
        assert len(border) == dim ** 3 - max(dim - 2, 0) ** 3  # every border cell holds a boid
        lim = c["params"][0] + c["params"][5]
        assert (np.abs(c["pos"]) > lim + 10).any(axis=1).sum() > 100  # clamped from far outside
        if dim in (31, 33, 34, 63, 65):
            assert gf["straddle"].any()  # a row of three cells across two occupancy words
    else:
        P = R.unpack(c["params"])
        assert F.nb.mean() > 20
        if name == "separation_above_perception":
            assert np.array_equal(F.nsep, F.nb)
        if name == "max_force_clamps":
            assert np.allclose(np.linalg.norm(F.ali[F.nb > 0], axis=1), P["max_force"] * P["alignment_weight"])
        if name == "zero_weights":
            assert not F.sep.any() and not F.ali.any() and not F.coh.any() and F.nsep.sum() > 0
        if name == "blend_saturates":
            assert P["color_blend_rate"] * c["dt"] >= 1.0


@pytest.mark.parametrize("name", sorted(_BUILDERS))
def test_case_reaches_its_branch(name):
    c = _BUILDERS[name]()
    F = R.flocking(c["pos"], c["vel"], c["col"], c["params"])
    _reaches(name, c, F, BC.grid_facts(c["pos"], c["params"]))


def test_cell_index_restatement(oracle):
    """R.cell_index (used to check the kernel's at the 1290 grid) equals the oracle's int32 cells."""
    c = BC.grid_dims(33)
    st = oracle.FlockStepper(c["pos"], c["vel"], c["col"], c["params"])
    st.L.bdref_assign_cells(st.pos, st.cell_indices, st.cell, st.dim, st.offset, st.n)
    assert np.array_equal(R.cell_index(c["pos"], c["params"]), st.cell_indices)
    big = BC.largest_grid()
    ids = R.cell_index(big["pos"], big["params"])
    assert R.grid(big["params"])[1] == 1290 and ids.max() == 1290 ** 3 - 1 and ids.max() < 2 ** 31
    assert R.grid(BC.params(bounds=644.5, perception_radius=1.0))[1] == 1291
