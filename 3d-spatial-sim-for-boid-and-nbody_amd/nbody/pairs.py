"""Host side of the binned pair counts (include/nbmi.h nbmi_pair_counts): what is derived from
``below`` and ``counts``.  Pure NumPy, no device."""
import numpy as np

PAIRS_MAX_BINS = 64
# the "auto" edges: 0.5 d1 2^(k/2), k = 0 .. 12, d1 = the median nearest-neighbour distance - 12 bins over six octaves,
# from half to 32 nearest-neighbour distances.  A convention, not a measured optimum.
AUTO_EDGES = 13


def auto_pair_edges(r2_1):
    """The 13 "auto" edges of a state from its knn(1) squared distances."""
    d = np.sqrt(np.asarray(r2_1, dtype=np.float64))
    d1 = float(np.median(d)) if len(d) else 0.0
    if not (np.isfinite(d1) and d1 > 0.0):
        raise ValueError("--pair-edges auto: the state's median nearest-neighbour distance is not finite and > 0 "
                         "(give --pair-edges e0,e1,...)")
    return [0.5 * d1 * 2.0 ** (k / 2.0) for k in range(AUTO_EDGES)]


def check_edges(edges):
    """The edges as a float64 array if nbmi_pair_counts would take them (ValueError otherwise): 2 .. 65 finite values,
    the first >= 0, strictly increasing, and so are their squares."""
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    if not 2 <= len(e) <= PAIRS_MAX_BINS + 1:
        raise ValueError(f"pair edges: need 2 .. {PAIRS_MAX_BINS + 1} edges, not {len(e)}")
    with np.errstate(over="ignore"):
        e2 = e * e
    if not (np.isfinite(e).all() and e[0] >= 0.0 and (np.diff(e) > 0.0).all() and np.isfinite(e2).all()
            and (np.diff(e2) > 0.0).all()):
        raise ValueError("pair edges: the edges (and their squares) must be finite, >= 0 and strictly increasing")
    return e


def cumulative(below, counts):
    """C(edges[k]) for k = 0 .. nb: the number of pairs within each edge (Python integers: no overflow)."""
    out, c = [int(below)], int(below)
    for x in counts:
        c += int(x)
        out.append(c)
    return out


def correlation_dimension(edges, below, counts, lo=None, hi=None):
    """(slope, points_used): the least-squares slope of log C(edges[k]) against log edges[k] over k >= 1 with C > 0 and
    lo <= edges[k] <= hi (None: no limit) - the correlation dimension D2, about 1 along a filament, 2 in a disc, 3 in a
    ball.  ValueError with fewer than two usable points."""
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    c = cumulative(below, counts)
    if len(c) != len(e):
        raise ValueError(f"correlation_dimension: {len(e)} edges need {len(e) - 1} counts, not {len(c) - 1}")
    use = [k for k in range(1, len(e)) if c[k] > 0 and (lo is None or e[k] >= lo) and (hi is None or e[k] <= hi)]
    if len(use) < 2:
        raise ValueError(f"correlation_dimension: {len(use)} usable points (need at least two with C > 0 inside the range)")
    x = np.log(e[use])
    y = np.log(np.array([float(c[k]) for k in use]))
    xm, ym = x.mean(), y.mean()
    return float(np.sum((x - xm) * (y - ym)) / np.sum((x - xm) ** 2)), len(use)


def xi_natural(dd, rr, n, n_random):
    """The natural estimator of the two-point correlation function per bin: dd / rr x n_random (n_random - 1) /
    (n (n - 1)) - 1 from the pair counts of the data (n bodies) and of a random catalogue (n_random points) in the same
    bins; nan where rr == 0."""
    dd = np.asarray(dd, dtype=np.float64)
    rr = np.asarray(rr, dtype=np.float64)
    out = np.full(dd.shape, np.nan)
    ok = rr != 0.0
    norm = float(n_random) * (float(n_random) - 1.0) / (float(n) * (float(n) - 1.0))
    out[ok] = dd[ok] / rr[ok] * norm - 1.0
    return out
