"""tests/direct_ref.py against the oracle and against hand-worked cases (no GPU).

The GPU tests of softening 0 and of tiny softening take their direct-sum references from direct_ref, so it must be
the oracle's sum where the oracle is defined (eps > 0) and follow the reference's dist_sq > eps^2 rule where the
oracle's all-pairs loop is not (eps = 0 with coincident bodies: 0 * inf)."""
import numpy as np
import pytest

from direct_ref import direct_accelerations, pair_weights


@pytest.mark.parametrize("eps", [1.0, 0.3, 1e-14])
def test_equals_the_oracle_for_positive_softening(oracle, eps):
    rng = np.random.RandomState(3)
    n = 3000
    pos = rng.normal(0, 50, (n, 3))
    m = rng.uniform(0.5, 2.0, n)
    rows = np.concatenate([[0, 1, n - 1], rng.choice(n, 61, replace=False)])
    got = direct_accelerations(pos, m, rows, 0.07, eps, chunk=512)
    ref = oracle.direct_forces_subset(pos, m, rows, 0.07, eps)
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() <= 1e-14 * scale


def test_equals_the_oracle_with_a_coincident_pair_for_positive_softening(oracle):
    """eps > 0: a coincident pair has d = 0, the oracle adds 0 and the rule skips it - the same sum."""
    rng = np.random.RandomState(4)
    pos = rng.normal(0, 10, (500, 3))
    pos[7] = pos[3]
    m = rng.uniform(0.5, 2.0, 500)
    rows = np.array([3, 7, 100])
    got = direct_accelerations(pos, m, rows, 1.0, 0.5)
    ref = oracle.direct_forces_subset(pos, m, rows, 1.0, 0.5)
    assert np.abs(got - ref).max() <= 1e-14 * np.abs(ref).max()


def test_hand_worked_unsoftened_cases():
    # two bodies on the x axis 2 apart: a_0 = G m_1 / 4 towards body 1, a_1 = G m_0 / 4 towards body 0
    pos = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    m = np.array([3.0, 5.0])
    a = direct_accelerations(pos, m, [0, 1], 2.0, 0.0)
    assert np.array_equal(a, [[2.5, 0.0, 0.0], [-1.5, 0.0, 0.0]])
    # a body alone: no pair at all
    assert np.array_equal(direct_accelerations(pos[:1], m[:1], [0], 1.0, 0.0), [[0.0, 0.0, 0.0]])
    # a coincident pair is skipped (d = 0: dist_sq = eps^2 = 0 is not > 0); the third body still pulls both
    pos = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 5.0]])
    m = np.array([1.0, 2.0, 8.0])
    a = direct_accelerations(pos, m, [0, 1, 2], 1.0, 0.0)
    assert np.isfinite(a).all()
    assert np.array_equal(a[0], [0.0, 0.0, 0.5]) and np.array_equal(a[1], [0.0, 0.0, 0.5])
    assert np.array_equal(a[2], [0.0, 0.0, -3.0 / 16.0])
    # the same coincident pair at eps = 1e-14: still skipped (d = 0 gives dist_sq == eps^2), the rest softened
    a = direct_accelerations(pos, m, [0, 2], 1.0, 1e-14)
    assert np.allclose(a, [[0.0, 0.0, 0.5], [0.0, 0.0, -3.0 / 16.0]], rtol=1e-15, atol=0)


def test_hand_worked_softened_pair():
    # |d| = 3, eps = 4: dist_sq = 25, a = G m d / 125
    pos = np.array([[0.0, 0.0, 0.0], [0.0, 3.0, 0.0]])
    a = direct_accelerations(pos, np.array([1.0, 10.0]), [0], 0.5, 4.0)
    assert np.allclose(a, [[0.0, 0.5 * 10.0 * 3.0 / 125.0, 0.0]], rtol=1e-15, atol=0)


def test_unsoftened_rows_are_every_pair_but_the_skipped_ones():
    """Sampled rows at eps = 0 equal an explicit double loop over the pairs that survive the rule."""
    rng = np.random.RandomState(5)
    n = 400
    pos = rng.uniform(-20, 20, (n, 3))
    pos[10] = pos[20]
    pos[30] = pos[20]
    m = rng.uniform(0.1, 3.0, n)
    rows = np.array([10, 20, 30, 0, n - 1])
    got = direct_accelerations(pos, m, rows, 0.3, 0.0, chunk=64)
    for k, i in enumerate(rows):
        want = np.zeros(3)
        for j in range(n):
            d = pos[j] - pos[i]
            dist_sq = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            if j != i and dist_sq > 0.0:
                want += 0.3 * m[j] / (dist_sq * np.sqrt(dist_sq)) * d
        assert np.allclose(got[k], want, rtol=1e-13, atol=0), i
    w = pair_weights(pos, m, rows, 0.3, 0.0)
    assert np.isfinite(w).all() and (w > 0).all()
