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


def _per_pair(count, total_pairs):
    return np.asarray(count, dtype=np.float64) / total_pairs


def xi_landy_szalay(dd, dr, rr, n, m):
    """The Landy-Szalay estimator per bin, (DD' - 2 DR' + RR') / RR' with every count divided by its number of pairs:
    DD' = dd / (n (n - 1) / 2), DR' = dr / (n m), RR' = rr / (m (m - 1) / 2) - dd and rr the unordered pair counts of the
    n bodies and of the m random points, dr the cross counts of the bodies about the random points (pair_counts_at's
    totals, every (point, body) pair once); nan where rr == 0."""
    n, m = float(n), float(m)
    dd_n = _per_pair(dd, n * (n - 1.0) / 2.0)
    dr_n = _per_pair(dr, n * m)
    rr_n = _per_pair(rr, m * (m - 1.0) / 2.0)
    out = np.full(dd_n.shape, np.nan)
    ok = np.asarray(rr) != 0
    out[ok] = (dd_n[ok] - 2.0 * dr_n[ok] + rr_n[ok]) / rr_n[ok]
    return out


def xi_davis_peebles(dd, dr, n, m):
    """The Davis-Peebles estimator per bin, (2 m / (n - 1)) dd / dr - 1: the unordered pair counts of the n bodies over
    their cross counts about m random points; nan where dr == 0."""
    dd = np.asarray(dd, dtype=np.float64)
    dr = np.asarray(dr, dtype=np.float64)
    out = np.full(dd.shape, np.nan)
    ok = dr != 0.0
    out[ok] = 2.0 * float(m) / (float(n) - 1.0) * dd[ok] / dr[ok] - 1.0
    return out


def counts_within(per_point):
    """(m, nb + 1) int64 from pair_counts_at's per-point rows: column k = the number of bodies within edges[k] of the
    point (the cumulative sum along the columns)."""
    return np.cumsum(np.asarray(per_point, dtype=np.int64), axis=-1, dtype=np.int64)


def sphere_density(per_point, edges, mass=1.0):
    """(m, nb + 1) float64: ``mass`` x counts_within over the volume 4/3 pi edges[k]^3 of each sphere - the mean density
    of bodies of that mass inside edges[k] of each point.  A zero radius gives +inf where the sphere holds a body, as
    nbmi_get_densities_f64 does for r2_k == 0, and nan where it holds none."""
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    within = counts_within(per_point)
    if within.shape[-1] != len(e):
        raise ValueError(f"sphere_density: {len(e)} edges need rows of {len(e)} columns, not {within.shape[-1]}")
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(mass) * within / (4.1887902047863905 * (e * e * e))
