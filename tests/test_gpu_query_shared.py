"""What the three tree queries share: the rows and wave-leaf kernel, the wave prologue, the
half search, one scratch struct and query_sync.  Two things that sharing could break and the per-query suites would not
see:

  order independence   the queries of one handle write the same rows and wave-leaf table and keep their scratch side by
                       side: whatever ran before, each gives the bits of a fresh handle that runs nothing else.
  work counters        `evals` and `cell_pairs` are integer sums over a deterministic walk.  tests/golden/query_evals.json
                       holds them as the commit before the queries were consolidated computed them
                       (scripts/gen_query_evals_golden.py); they must be EQUAL here: a pair tested twice, a leaf skipped or
                       a walk started at another node changes them even where the results happen to survive.
"""
import itertools
import json
import os

import numpy as np
import pytest

import query_cases as qc
from conftest import GOLDEN
from test_gpu_fof import CASES as FOF_CASES
from test_gpu_pairs import LINEAR

pytestmark = pytest.mark.gpu

GOLDEN_PATH = os.path.join(GOLDEN, "query_evals.json")
EVAL_SYSTEMS = ("n1", "n2", "n65", "n2049", "n4097", "trap", "far", "galaxy")
EVAL_KS = (1, 32, 64)
LOG = 0.5 * 2.0 ** np.arange(13)  # 12 logarithmic bins, 0.5 .. 2 048
EDGES = {"linear": LINEAR, "log": LOG}


def links(name):
    """the linking lengths test_gpu_fof.CASES has for that system"""
    return [b for n, b, _shape in FOF_CASES if n == name]


def collect(name):
    """{"knn/<k>": {"evals"}, "fof/<b>": {"evals"}, "pairs/<edges>": {"evals", "cell_pairs"}} of one system, through the
    public methods only"""
    p, m = qc.system(name)
    sim = qc.bh(p, m=m)
    out = {}
    try:
        for k in EVAL_KS:
            if k <= len(p) - 1:
                out[f"knn/{k}"] = {"evals": sim.knn(k, evals=True)[2]}
        for b in links(name):
            out[f"fof/{b}"] = {"evals": sim.find_groups(b, evals=True)[1]}
        for tag, e in EDGES.items():
            got = sim.pair_counts(e, evals=True)
            out[f"pairs/{tag}"] = {"evals": got[2], "cell_pairs": got[3]}
    finally:
        sim.close()
    return out


@pytest.mark.parametrize("name", EVAL_SYSTEMS)
def test_work_counters_equal_the_golden(gpu, name):
    with open(GOLDEN_PATH) as f:
        want = json.load(f)["systems"][name]
    got = collect(name)
    for key in sorted(want):
        print(f"{name} {key}: {got.get(key)} (golden {want[key]})")
    assert links(name) and set(got) == set(want), (sorted(got), sorted(want))
    assert got == want
    if len(qc.system(name)[0]) > 64:
        assert all(v["evals"] > 0 for v in got.values()), "the case lost its point: nothing was evaluated"
    if name == "galaxy":
        assert got["pairs/log"]["cell_pairs"] > 0  # cells are counted whole


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(tag, got, want):
    assert len(got) == len(want), tag
    for g, w in zip(got, want):
        assert np.array_equal(_bits(g), _bits(w)), tag


ORDER_CASES = {"n2049": 8.0, "far": 5.0}  # system -> linking length (of test_gpu_fof.CASES)


@pytest.mark.parametrize("name", sorted(ORDER_CASES))
def test_every_order_gives_the_bits_of_a_fresh_handle(gpu, name):
    b = ORDER_CASES[name]
    assert b in links(name)
    p, m = qc.system(name)
    queries = {
        "knn": lambda s: s.knn(8),
        "fof": lambda s: (s.find_groups(b), np.int64(s.n_groups)),
        "pairs": lambda s: (lambda c: (c[0], np.int64(c[1])))(s.pair_counts(LOG)),
    }

    def fresh(pos, vel):
        out = {}
        for q, run in queries.items():
            sim = qc.bh(pos, vel, m)
            try:
                out[q] = run(sim)
            finally:
                sim.close()
        return out

    want = fresh(p, None)
    assert 1 < int(want["fof"][1]) < len(p) and want["pairs"][0].sum() > len(p), (name, "the case lost its point")
    sim = qc.bh(p, m=m)
    try:
        for order in itertools.permutations(queries):
            for q in order:
                _same(f"{name} {q} in {order}", queries[q](sim), want[q])
        sim.step_many(0.2, 2)
        x, v = sim.get_positions_f64(), sim.get_velocities()
        assert not np.array_equal(x, p)
        assert np.array_equal(sim.get_masses(), m)
        got = {q: queries[q](sim) for q in ("pairs", "knn", "fof")}
    finally:
        sim.close()
    moved = fresh(x, v)  # the same positions give the same tree
    for q in queries:
        _same(f"{name} {q} after steps", got[q], moved[q])
