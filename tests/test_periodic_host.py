"""The restatement of the periodic box (tests/periodic_ref.py) against a plain triple-loop brute force written from
include/bdmi.h, against topo_ref away from the faces, and against values written out by hand; and the constructed cases of
tests/periodic_cases.py against what they claim.  No GPU.
"""
import math

import numpy as np
import pytest

import boids_cases as BC
import boids_ref as R
import periodic_cases as PC
import periodic_ref as PR
import topo_ref as T

H = 2.0 ** -BC.PB


# ---- brute force: scalar Python floats, one boid, one candidate, one axis at a time ------------------------------------
def _steer(x, v, ms, mf, w):
    mag = math.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
    if not mag > 0:
        return [0.0, 0.0, 0.0]
    y = [(x[c] / mag) * ms - v[c] for c in range(3)]
    m2 = math.sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2])
    if m2 > mf:
        y = [(y[c] / m2) * mf for c in range(3)]
    return [y[c] * w for c in range(3)]


def brute(pos, vel, col, prm, k):
    """k = None: the metric set in id order.  Returns ids, d2, forces (n, 4, 3) and the metric counts."""
    P = R.unpack(prm)
    B = P["bounds"]
    L = 2 * B
    ps, ss = P["perception_radius"] ** 2, P["separation_radius"] ** 2
    n = len(pos)
    out_ids, out_d2, metric = [], [], []
    forces = np.zeros((n, 4, 3))
    for i in range(n):
        found = []
        for j in range(n):
            if j == i:
                continue
            q = [0.0] * 3
            for c in range(3):
                d0 = pos[i][c] - pos[j][c]
                q[c] = pos[j][c] + L if d0 > B else (pos[j][c] - L if d0 < -B else pos[j][c])
            d = [pos[i][c] - q[c] for c in range(3)]
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            if 1e-4 < d2 < ps:
                found.append((d2, j, q, d))
        metric.append(len(found))
        if k is not None:
            found = sorted(found, key=lambda e: (e[0], e[1]))[:k]
        out_ids.append([e[1] for e in found])
        out_d2.append([e[0] for e in found])
        S, A, C, Cl = ([0.0] * 3 for _ in range(4))
        nsep = 0
        for d2, j, q, d in found:
            if d2 < ss:
                dist = math.sqrt(d2)
                inv = 1.0 / dist
                for c in range(3):
                    S[c] += d[c] * inv / dist
                nsep += 1
            for c in range(3):
                A[c] += vel[j][c]
                C[c] += q[c]
                Cl[c] += col[j][c]
        m = len(found)
        v = list(vel[i])
        forces[i, 3] = col[i]
        if nsep:
            forces[i, 0] = _steer([S[c] / nsep for c in range(3)], v, P["max_speed"], P["max_force"], P["separation_weight"])
        if m:
            forces[i, 1] = _steer([A[c] / m for c in range(3)], v, P["max_speed"], P["max_force"], P["alignment_weight"])
            forces[i, 2] = _steer([C[c] / m - pos[i][c] for c in range(3)], v, P["max_speed"], P["max_force"],
                                  P["cohesion_weight"])
            forces[i, 3] = [(Cl[c] + col[i][c]) / (m + 1) for c in range(3)]
    return out_ids, out_d2, forces, metric


def _state(pos, seed=0):
    rng = np.random.default_rng(seed)
    pos = R.lattice(np.asarray(pos, dtype=np.float64), BC.PB)
    return pos, R.lattice(rng.uniform(-12.5, 12.5, pos.shape), BC.VB), R.id_colours(len(pos))


PRM3 = PC.box_params(3)  # bounds 7.5, perception 5: dim 3


def _small_inputs():
    B = 7.5
    rng = np.random.default_rng(5)
    out = [("dim3_random", rng.uniform(-B, B, (60, 3)))]
    # pairs 2 apart through one face, an edge and a corner: shifts on one, two and three axes, both signs
    out.append(("face_edge_corner", [[B - 1, 0, 0], [-B + 1, 0.5, 0], [0, B - 1, -B + 1], [0.5, -B + 1, B - 1],
                                     [B - 1, B - 1, B - 1], [-B + 1, -B + 1, -B + 1.5], [0, -3, 0.25]]))
    out.append(("exactly_on_the_faces", [[B, 0, 0], [-B, 1, 0], [B, B, -B], [-B + 2, -B, B], [0, 0, B], [1, 1, -B]]))
    # 2^-7 apart through a face: d2 = 2^-14 < 1e-4, excluded; and 2^-7 on two axes: 2^-13 > 1e-4, a neighbour
    out.append(("floor_through_a_face", [[B, 2, 2], [-B + 2 ** -7, 2, 2], [3, B, 0], [3 + 2 ** -7, -B + 2 ** -7, 0]]))
    # d0 == +-B exactly: no shift; next to it d0 = B + h: shifted.  Either way the pair is half a box apart, three
    # perception radii at least, and out of sight: the rule only has to be the same on both sides
    out.append(("d0_equals_B", [[3.75, 0, 0], [-3.75, 0, 0], [3.75, 4, 4], [-3.75 - H, 4, 4]]))
    for n in (1, 2, 7, 8):  # n in 1, 2, k, k + 1 for k = 7
        out.append((f"n_{n}", rng.uniform(-B, B, (n, 3))))
    return out


@pytest.mark.parametrize("name,pos", _small_inputs(), ids=[x[0] for x in _small_inputs()])
def test_restatement_agrees_with_brute_force(name, pos):
    pos, vel, col = _state(pos)
    n = len(pos)
    for k in (1, 7, 16):
        ids, d2, forces, metric = brute(pos, vel, col, PRM3, k)
        rows = PR.neighbours(pos, PRM3, k)
        assert rows["metric"].tolist() == metric and rows["count"].tolist() == [min(m, k) for m in metric]
        for i in range(n):
            c = rows["count"][i]
            assert rows["ids"][i, :c].tolist() == ids[i] and np.all(rows["ids"][i, c:] == -1), (name, k, i)
            assert R.same_bits(rows["d2"][i, :c], np.array(d2[i], dtype=np.float64)) and np.all(np.isinf(rows["d2"][i, c:]))
        F = PR.flocking(pos, vel, col, PRM3, k)
        for f, want in zip((F.sep, F.ali, F.coh, F.avg), np.moveaxis(forces, 1, 0)):
            assert R.same_bits(f, want), (name, k)
    # the metric rule: counts, and the sums that are exact on the lattice; the separation sum inside its bound
    _, _, forces, metric = brute(pos, vel, col, PRM3, None)
    F = PR.metric(pos, vel, col, PRM3)
    assert F.nb.tolist() == metric
    assert R.same_bits(F.ali, forces[:, 1]) and R.same_bits(F.coh, forces[:, 2]) and R.same_bits(F.avg, forces[:, 3])
    assert np.all(np.abs(F.sep - forces[:, 0]).max(axis=1) <= R.sep_bound(F, vel, PRM3))
    if name == "face_edge_corner":
        assert metric[:6] == [1] * 6 and metric[6] == 0
    if name == "exactly_on_the_faces":
        assert metric[0] >= 1 and metric[1] >= 1  # +B and -B are the same plane: 1 apart
    if name == "floor_through_a_face":
        assert metric == [0, 0, 1, 1]
    if name == "d0_equals_B":
        assert metric == [0, 0, 0, 0]
        assert PR.image(pos[0, 0], pos[1, 0], 7.5, 15.0) == pos[1, 0] and PR.image(pos[1, 0], pos[0, 0], 7.5, 15.0) == pos[0, 0]
        assert PR.image(pos[2, 0], pos[3, 0], 7.5, 15.0) == pos[3, 0] + 15.0


def test_rows_written_out_by_hand():
    """Boid 0 at x = 7 (B = 7.5) with neighbours on both sides of the face."""
    pos = np.array([[7.0, 0, 0], [6.0, 0, 0], [-7.0, 0, 0], [-6.5, 0, 0], [7.0, 3.0, 0], [-7.5, 0, 2.0], [0, 0, 0]])
    rows = PR.neighbours(pos, PRM3, 7)
    # images of 2, 3, 5 for boid 0: x = 8, 8.5, 7.5 -> d2 = 1, 2.25, 0.25 + 4; boid 1: 1; boid 4: 9; boid 6: 49 (out)
    assert rows["ids"][0].tolist() == [1, 2, 3, 5, 4, -1, -1]
    assert rows["d2"][0, :5].tolist() == [1.0, 1.0, 2.25, 4.25, 9.0] and rows["count"][0] == 5
    # and seen from the other side: boid 2 at -7 has 0 at -8, 1 at -9, 4 at (-8, 3)
    assert rows["ids"][2].tolist() == [3, 0, 1, 5, 4, -1, -1]
    assert rows["d2"][2, :5].tolist() == [0.25, 1.0, 4.0, 4.25, 10.0]
    vel, col = np.zeros_like(pos), R.id_colours(len(pos))
    vel[:, 1] = 1.0
    F = PR.flocking(pos, vel, col, PRM3, 7)
    # cohesion of boid 0 adds the IMAGES: x sum 6 + 8 + 8.5 + 7.5 + 7 = 37, mean 7.4, minus 7 = 0.4 > 0: towards the face
    assert F.coh[0, 0] > 0 and F.nb[0] == 5
    # separation from dx = p - q': neighbours 2 and 3 push boid 0 back (negative x), boid 1 pushes forward, equally far as 2
    assert F.nsep[0] == 4


def test_wrap_values():
    B, L = 7.5, 15.0
    x = np.array([B, np.nextafter(B, np.inf), np.nextafter(-B, -np.inf), -B, B + 1.0, -B - 1.0, 0.0])
    w = PR.wrap(x, B, L)
    assert w[0] == B and w[3] == -B and w[6] == 0.0  # on the face: stays
    assert w[1] == np.nextafter(B, np.inf) - L and w[2] == np.nextafter(-B, -np.inf) + L
    assert w[1] == -7.499999999999999 and w[2] == 7.499999999999999
    assert w[4] == -6.5 and w[5] == 6.5
    assert np.all(np.abs(w) <= B)
    # in physics(): a boid 0.1 inside the face moving out at 12 per unit time
    prm = PRM3
    pos, vel, col = np.array([[7.4, 0, -7.4]]), np.array([[12.0, 0, -12.0]]), np.zeros((1, 3))
    zero = np.zeros((1, 3))
    p, v, _ = PR.physics(pos, vel, col, (zero, zero, zero, col), prm, 0.0625)
    assert p[0].tolist() == [7.4 + 0.75 - 15.0, 0.0, -7.4 - 0.75 + 15.0] and v[0].tolist() == [12.0, 0.0, -12.0]
    assert PR.crossings(pos, p, prm).tolist() == [True]


def test_cell_index_and_box():
    assert PR.box(PRM3) == (7.5, 15.0, 3, 5.0)
    B, L, dim, cell = PR.box(BC.params(bounds=18.75))
    assert (L, dim) == (37.5, 7) and cell == 37.5 / 7 and cell >= 5.0
    pos = np.array([[-7.5, -7.5, -7.5], [7.5, 7.5, 7.5], [-2.5, 2.5, 0], [-2.5 - H, 0, 7.4]])
    assert PR.cell_index(pos, PRM3).tolist() == [0, 26, 1 + 2 * 3 + 9, 0 + 3 + 18]  # x == +B: the last cell


def test_interior_cluster_equals_the_walled_restatement():
    """Nothing within one cell of a face: no image is shifted, and the bits are topo_ref's on the walled parameters."""
    c = PC.interior_cluster()
    B, _, _, cell = PR.box(c["params"])
    assert np.all(np.abs(c["pos"]) < B - cell)
    for k in (1, 7, 16):
        rows, want = PR.neighbours(c["pos"], c["params"], k), T.neighbours(c["pos"], c["params"], k)
        assert np.array_equal(rows["ids"], want["ids"]) and R.same_bits(rows["d2"], want["d2"])
        F, W = PR.flocking(c["pos"], c["vel"], c["col"], c["params"], k, nb=rows), \
            T.flocking(c["pos"], c["vel"], c["col"], c["params"], k, nb=want)
        assert all(R.same_bits(a, b) for a, b in zip((F.sep, F.ali, F.coh, F.avg), (W.sep, W.ali, W.coh, W.avg)))
        assert (F.nb == k).any()
    M, W = PR.metric(c["pos"], c["vel"], c["col"], c["params"]), R.flocking(c["pos"], c["vel"], c["col"], c["params"])
    assert np.array_equal(M.nb, W.nb) and R.same_bits(M.ali, W.ali) and R.same_bits(M.coh, W.coh) and R.same_bits(M.avg, W.avg)


# ---- the constructed cases reach what they are named for --------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in PC.gpu_cases()}


def test_cases_are_inside_their_box_on_the_lattice(cases):
    for c in list(cases.values()) + [PC.trajectory(), PC.interior_cluster()] + [PC.sizes(n) for n in (1, 2, 255, 256, 257)]:
        B, L, dim, cell = PR.box(c["params"])
        assert np.all(np.abs(c["pos"]) <= B) and len(c["pos"]) <= 5000, c["name"]
        assert R.same_bits(c["pos"], R.lattice(c["pos"], BC.PB)) and B / H == round(B / H)
        assert dim >= 3 and cell >= R.unpack(c["params"])["perception_radius"]
    assert [PR.box(cases[f"box_{d}"]["params"])[2] for d in (3, 4, 33)] == [3, 4, 33]
    assert 3 ** 3 % 32 and 33 ** 3 % 32  # 27 and 35 937 cells: the last occupancy word is partly used, rows straddle words
    assert 4 ** 3 == 2 * 32              # dim 4 fills exactly two words: a row of four cells never straddles


def test_box_cases_hold_boids_exactly_on_the_faces(cases):
    for d in (3, 4, 33):
        c = cases[f"box_{d}"]
        B = PR.box(c["params"])[0]
        assert (c["pos"] == B).any() and (c["pos"] == -B).any()
        assert ((np.abs(c["pos"]) == B).sum(axis=1) == 3).any()  # a corner
        rows = PR.neighbours(c["pos"], c["params"], 16)
        print(c["name"], len(c["pos"]), "metric neighbours: mean", rows["metric"].mean(), "max", rows["metric"].max())
        assert (rows["metric"] > 16).any() and (rows["metric"] >= 1).mean() > 0.5


def test_face_waves_and_mixed_waves(cases):
    w = PC.wave_facts(cases["face_waves"]["pos"], cases["face_waves"]["params"])
    full = w["lanes"] == 64
    assert (full & (w["face"] == 64)).sum() >= 4 and (full & (w["face"] == 0)).sum() >= 4
    w = PC.wave_facts(cases["box_33"]["pos"], cases["box_33"]["params"])
    assert ((w["face"] > 0) & (w["face"] < w["lanes"])).sum() >= 4  # both kinds of lane in one wave


def test_long_runs_pass_the_note_limit_and_4095(cases):
    """runs[:, 1::2] are the segments through the x face: above the 2 047 of the 16-bit notes in one case, above 4 095 in
    the other; and boids whose every run is short enough for the notes sit next to them."""
    a = PR.run_facts(cases["long_run_2100"]["pos"], cases["long_run_2100"]["params"])
    through = a["runs"][:, 1::2].max(axis=1)
    assert PC.NOTE_LIMIT < through.max() <= 4095 and (through > PC.NOTE_LIMIT).sum() >= 60  # the boids of cell dim-1 (and of the rows around)
    assert (a["face"] & (a["runs"][:, 0::2].max(axis=1) > PC.NOTE_LIMIT)).any()  # the boids of cell 0: their run {0, 1}
    assert ((a["longest"] <= PC.NOTE_LIMIT) & (a["longest"] > 0)).any()
    b = PR.run_facts(cases["long_run_4200"]["pos"], cases["long_run_4200"]["params"])
    assert b["runs"][:, 1::2].max() > 4095 and (~b["face"] & (b["longest"] > 4095)).any()  # ... and cell 1: {0, 1, 2}
    assert ((b["longest"] <= PC.NOTE_LIMIT) & (b["longest"] > 0)).any()


def test_metric_separation_bound_is_tight_on_the_chosen_inputs(cases):
    """boids_ref.check_sep's tightness condition holds for the restatement alone on every input the GPU test uses."""
    for c in list(cases.values()) + [PC.sizes(n) for n in (0, 1, 2, 255, 256, 257)]:
        F = PR.metric(c["pos"], c["vel"], c["col"], c["params"])
        diff, worst = R.check_sep(F.sep, F, c["vel"], c["params"], c["name"])
        assert diff == 0.0
        print(c["name"], "separation terms up to", F.nsep.max(initial=0), "worst bound", worst)


def test_trajectory_case_crosses_faces():
    c = PC.trajectory()
    rows = PR.neighbours(c["pos"], c["params"], 7)
    assert 15 < rows["metric"].mean() < 25
    pos, vel, col = c["pos"], c["vel"], c["col"]
    crossed = np.zeros(len(pos), dtype=bool)
    B = PR.box(c["params"])[0]
    for _ in range(10):
        new = PR.step(pos, vel, col, c["params"], 7, c["dt"])
        crossed |= PR.crossings(pos, new[0], c["params"])
        pos, vel, col = new
        assert np.all(np.abs(pos) <= B)
    print("boids that crossed a face in ten steps:", crossed.sum())
    assert crossed.sum() >= 50
