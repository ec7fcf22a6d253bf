"""Pure NumPy helpers around the flock-analysis calls of include/bdmi.h (Flock.flocks, flock_catalogue, diagnostics,
neighbour_stats): the named fields of a row of 16 doubles, the size histogram of a catalogue, and the builder of the
JSON line that tools.flock_video writes with --diagnostics; and the order-against-noise experiment over
Flock.set_noise / Flock.diagnostics (order_parameter_series, binder_cumulant, noise_sweep), with percolation_summary for
the catalogue of a periodic flock (Flock.periodic_flock_catalogue); and the velocity correlation by distance from
Flock.velocity_correlation (velocity_correlation_function, correlation_length, susceptibility, radial_distribution,
correlation_line).  Nothing here touches the
device itself: the helpers work on any object with the Flock methods they name.
"""
import json

import numpy as np

ROW_FIELDS = ("members", "center", "velocity", "polarisation", "mean_speed", "milling", "lo", "hi")


def row_dict(row16) -> dict:
    """{m, c[3], vbar[3], polarisation, mean_speed, milling, lo[3], hi[3]} of the header, as plain Python values."""
    r = np.asarray(row16, dtype=np.float64)
    if r.shape != (16,):
        raise ValueError(f"a row has 16 doubles, got shape {r.shape}")
    return {"members": int(r[0]), "center": r[1:4].tolist(), "velocity": r[4:7].tolist(), "polarisation": float(r[7]),
            "mean_speed": float(r[8]), "milling": float(r[9]), "lo": r[10:13].tolist(), "hi": r[13:16].tolist()}


def size_histogram(members) -> dict:
    """Flocks per power-of-two size class: key 2^k counts the flocks with 2^k <= members < 2^(k+1)."""
    m = np.asarray(members, dtype=np.int64)
    if m.size and m.min() < 1:
        raise ValueError("a flock has at least one member")
    out = {}
    for size, cnt in zip(*np.unique(m, return_counts=True)):
        cls = 1 << (int(size).bit_length() - 1)
        out[cls] = out.get(cls, 0) + int(cnt)
    return out


def _settings(rec, neighbours, periodic, noise):
    """The keys that name what is not the default: present only when used."""
    if neighbours is not None:
        rec["neighbours"] = {"mode": str(neighbours["mode"]), "k": int(neighbours["k"])}
    if periodic:
        rec["periodic"] = True
    if noise is not None:
        rec["noise"] = {"eta": float(noise["eta"]), "seed": int(noise["seed"])}
    return rec


def global_line(frame, steps, global_row, neighbours=None, periodic=False, noise=None) -> str:
    """The short analysis line of a periodic flock: the frame, the step count and the whole flock's row, without flocks or
    neighbour counts (jsonl_line with ``flock_spans`` is the full one, from the Flock.periodic_* calls)."""
    rec = {"frame": int(frame), "steps": int(steps), "global": row_dict(global_row)}
    return json.dumps(_settings(rec, neighbours, periodic, noise))


def jsonl_line(frame, steps, global_row, n_flocks, links, mean_neighbours, flock_rows, flock_labels=None,
               link=None, min_members=None, qualifying=None, neighbours=None, noise=None, flock_spans=None,
               periodic=False) -> str:
    """One flock-analysis line: the frame, the step count, the whole flock's row, the number of flocks and links, the
    mean neighbour count and the rows of the largest flocks (largest first), as one JSON object without a newline.
    ``neighbours`` ({"mode": "topological", "k": K}) names the interaction rule where it is not the metric default,
    ``noise`` ({"eta": E, "seed": S}) the noise where there is one, ``periodic`` the periodic box.  ``flock_spans`` (the
    ``spans`` of Flock.periodic_flock_catalogue, bool (rows, 3)) adds ``"spans"`` to every listed flock; without it the
    line has no such key."""
    rows = [row_dict(r) for r in np.asarray(flock_rows, dtype=np.float64).reshape(-1, 16)]
    if flock_spans is not None:
        spans = np.asarray(flock_spans, dtype=bool).reshape(-1, 3)
        if len(spans) != len(rows):
            raise ValueError(f"flock_spans has {len(spans)} rows for {len(rows)} flocks")
        for r, sp in zip(rows, spans.tolist()):
            r["spans"] = sp
    if flock_labels is not None:
        for r, l in zip(rows, np.asarray(flock_labels).tolist()):
            r["label"] = int(l)
    rec = {"frame": int(frame), "steps": int(steps), "global": row_dict(global_row), "n_flocks": int(n_flocks),
           "links": int(links), "mean_neighbours": float(mean_neighbours), "flocks": rows}
    if link is not None:
        rec["link"] = float(link)
    if min_members is not None:
        rec["min_members"] = int(min_members)
    if qualifying is not None:
        rec["qualifying_flocks"] = int(qualifying)
    return json.dumps(_settings(rec, neighbours, periodic, noise))


def neighbour_rank_profile(d2) -> np.ndarray:
    """The mean distance to the 1st .. k-th neighbour, from the ``d2`` of Flock.topological_neighbours ((N, k) squared
    distances, padded with +inf): float64 (k,).  Entry s averages sqrt(d2[:, s]) over the boids that have an (s + 1)-th
    neighbour (+inf ignored) and is NaN where none has one."""
    d2 = np.asarray(d2, dtype=np.float64)
    if d2.ndim != 2:
        raise ValueError(f"d2 must be (N, k), got shape {d2.shape}")
    have = np.isfinite(d2)
    total = np.where(have, np.sqrt(np.where(have, d2, 0.0)), 0.0).sum(axis=0)
    cnt = have.sum(axis=0)
    return np.where(cnt > 0, total / np.maximum(cnt, 1), np.nan)


def percolation_summary(catalogue, n) -> dict:
    """What the catalogue of a periodic flock of ``n`` boids (Flock.periodic_flock_catalogue, largest flock first) says
    about percolation: ``largest_fraction`` = members of the largest flock / n (0 without a flock), ``spanning_flocks`` =
    how many of the catalogued flocks occupy every slab of at least one axis, ``largest_spans`` = the three per-axis
    flags of the largest.  Spanning is the header's conservative test: a flock that reaches around the box spans, and so
    does a C-shaped one that does not close."""
    members = np.asarray(catalogue["members"], dtype=np.int64)
    spans = np.asarray(catalogue["spans"], dtype=bool).reshape(-1, 3)
    if len(spans) != len(members):
        raise ValueError(f"the catalogue has {len(members)} flocks and {len(spans)} rows of spans")
    if int(n) < 0 or (members.size and int(members[0]) > int(n)):
        raise ValueError(f"n = {n} is smaller than the largest flock")
    if members.size == 0:
        return {"largest_fraction": 0.0, "spanning_flocks": 0, "largest_spans": [False, False, False]}
    return {"largest_fraction": float(members[0]) / float(n), "spanning_flocks": int(spans.any(axis=1).sum()),
            "largest_spans": spans[0].tolist()}


# ---- order against noise (Vicsek et al. 1995): the polarisation of a flock as a function of the noise amplitude --------
def order_parameter_series(rows) -> dict:
    """The time series of the order parameters from the rows of Flock.diagnostics() ((T, 16) float64, one row per
    sample): dict of ``polarisation``, ``milling`` and ``mean_speed``, float64 (T,) each."""
    r = np.asarray(rows, dtype=np.float64)
    if r.ndim != 2 or r.shape[1] != 16:
        raise ValueError(f"rows must be (T, 16), got shape {r.shape}")
    return {"polarisation": r[:, 7].copy(), "milling": r[:, 9].copy(), "mean_speed": r[:, 8].copy()}


def binder_cumulant(phi) -> float:
    """1 - <phi^4> / (3 <phi^2>^2) of the samples ``phi``: 2/3 in the ordered phase, towards 1/3 for the polarisation of
    a disordered flock in three dimensions; NaN without samples or where <phi^2> is 0."""
    phi = np.asarray(phi, dtype=np.float64)
    if phi.size == 0:
        return float("nan")
    m2, m4 = float(np.mean(phi ** 2)), float(np.mean(phi ** 4))
    return 1.0 - m4 / (3.0 * m2 * m2) if m2 > 0 else float("nan")


def noise_sweep(make_flock, etas, steps, discard, every, dt) -> list:
    """Order against noise.  For every ``eta`` of ``etas``: a fresh flock from ``make_flock()`` (any object with
    ``set_noise``, ``update`` and ``diagnostics``, closed afterwards if it has ``close``), ``set_noise(eta)`` with
    whatever seed and step the flock has, ``steps`` updates of ``dt``; behind the first ``discard`` updates every
    ``every``-th one is sampled.  Returns one dict per eta: ``eta``, ``samples``, ``polarisation_mean``,
    ``polarisation_std`` (population standard deviation) and ``binder`` (binder_cumulant of the samples)."""
    steps, discard, every = int(steps), int(discard), int(every)
    if steps < 1 or every < 1 or not 0 <= discard < steps:
        raise ValueError("noise_sweep: steps and every must be at least 1 and 0 <= discard < steps")
    out = []
    for eta in etas:
        flock = make_flock()
        try:
            seed = flock.noise[1] if hasattr(flock, "noise") else 0
            flock.set_noise(float(eta), seed=seed)
            rows = []
            for s in range(steps):
                flock.update(dt)
                if s >= discard and (s - discard) % every == 0:
                    rows.append(np.array(flock.diagnostics(), dtype=np.float64))
            phi = order_parameter_series(np.array(rows).reshape(-1, 16))["polarisation"]
        finally:
            if hasattr(flock, "close"):
                flock.close()
        out.append({"eta": float(eta), "samples": int(phi.size), "polarisation_mean": float(phi.mean()),
                    "polarisation_std": float(phi.std()), "binder": binder_cumulant(phi)})
    return out


# ---- velocity correlation by distance (Cavagna et al. 2010; Attanasi et al. 2014), from Flock.velocity_correlation ------
# `res` is that method's dict: edges (nb + 1), pairs and dot per slot (slot 0 = below the first edge, slot k = the bin
# (edges[k-1], edges[k]]), qsq = the sum of |q_i|^2, n = the number of boids; q in units of res["quantum"] = 2^-24.
def _vc_arrays(res):
    edges = np.asarray(res["edges"], dtype=np.float64)
    pairs = [int(x) for x in res["pairs"]]
    dot = [int(x) for x in res["dot"]]
    if len(edges) < 2 or len(pairs) != len(edges) or len(dot) != len(edges):
        raise ValueError("a correlation result has nb + 1 edges, pairs and dot, nb >= 1")
    centres = np.concatenate([[0.5 * edges[0]], 0.5 * (edges[:-1] + edges[1:])])
    return edges, pairs, dot, centres


def velocity_correlation_function(res):
    """``(r, C)``: the slot centres (slot 0: half the first edge) and the connected correlation C_k = dot_k / (pairs_k
    2^48), normalised by C0 = qsq / (n 2^48) so that a boid correlates with itself at 1.  NaN where a slot holds no pair,
    and everywhere when C0 is 0."""
    _, pairs, dot, centres = _vc_arrays(res)
    n, qsq = int(res["n"]), int(res["qsq"])
    c = np.full(len(pairs), np.nan)
    for k, (p, d) in enumerate(zip(pairs, dot)):
        if p > 0 and qsq > 0:
            c[k] = (d * n) / (p * qsq)  # exact integers, one correctly rounded division
    return centres, c


def correlation_length(res):
    """The first zero crossing of C(r): between the first two successive non-empty slots with C > 0 and then C <= 0,
    interpolated linearly between their centres.  None without a crossing."""
    r, c = velocity_correlation_function(res)
    ok = np.flatnonzero(~np.isnan(c))
    for a, b in zip(ok[:-1], ok[1:]):
        if c[a] > 0 >= c[b]:
            return float(r[a] + (r[b] - r[a]) * c[a] / (c[a] - c[b]))
    return None


def susceptibility(res):
    """The finite-size susceptibility: ``chi`` = max over k of (2 / n) sum_{j <= k} dot_j / 2^48, the largest cumulated
    correlation, and ``r`` = the edge edges[k] at which it is reached (the first such k).  n == 0: chi 0, r None."""
    edges, _, dot, _ = _vc_arrays(res)
    n = int(res["n"])
    if n == 0:
        return {"chi": 0.0, "r": None}
    best, at, run = None, None, 0
    for k, d in enumerate(dot):
        run += d
        if best is None or run > best:
            best, at = run, k
    return {"chi": (2 * best) / (n << 48), "r": float(edges[at])}


def radial_distribution(res, box):
    """``(r, g)`` of a periodic flock: pairs_k over what an ideal gas of n boids in the box would hold, n (n - 1) / 2
    times the shell's volume over L^3.  ``box`` is Flock.box (or the box length).  Slot 0 is the ball below the first edge
    (NaN where that edge is 0)."""
    edges, pairs, _, centres = _vc_arrays(res)
    length = float(box["length"] if isinstance(box, dict) else box)
    n = int(res["n"])
    vol = 4.0 / 3.0 * np.pi * np.diff(np.concatenate([[0.0], edges ** 3]))
    ideal = 0.5 * n * (n - 1) * vol / length ** 3
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(ideal > 0, np.asarray(pairs, dtype=np.float64) / ideal, np.nan)
    return centres, g


def correlation_line(frame, steps, res) -> str:
    """One line of tools.flock_video's correlation file: {frame, steps, edges, pairs, dot, mean, C, xi, chi}; NaN is
    written as null, dot as decimal strings where it exceeds 2^53."""
    _, c = velocity_correlation_function(res)
    rec = {"frame": int(frame), "steps": int(steps), "edges": [float(e) for e in res["edges"]],
           "pairs": [int(p) for p in res["pairs"]], "dot": [d if abs(d) < (1 << 53) else str(d) for d in map(int, res["dot"])],
           "mean": [float(x) for x in res["mean"]], "C": [None if np.isnan(x) else float(x) for x in c],
           "xi": correlation_length(res), "chi": susceptibility(res)["chi"]}
    return json.dumps(rec)
