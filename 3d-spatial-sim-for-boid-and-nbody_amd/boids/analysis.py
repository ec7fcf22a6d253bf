"""Pure NumPy helpers around the flock-analysis calls of include/bdmi.h (Flock.flocks, flock_catalogue, diagnostics,
neighbour_stats): the named fields of a row of 16 doubles, the size histogram of a catalogue, and the builder of the
JSON line that tools.flock_video writes with --diagnostics.  Nothing here touches the device.
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


def jsonl_line(frame, steps, global_row, n_flocks, links, mean_neighbours, flock_rows, flock_labels=None,
               link=None, min_members=None, qualifying=None, neighbours=None) -> str:
    """One flock-analysis line: the frame, the step count, the whole flock's row, the number of flocks and links, the
    mean neighbour count and the rows of the largest flocks (largest first), as one JSON object without a newline.
    ``neighbours`` ({"mode": "topological", "k": K}) names the interaction rule where it is not the metric default."""
    rows = [row_dict(r) for r in np.asarray(flock_rows, dtype=np.float64).reshape(-1, 16)]
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
    if neighbours is not None:
        rec["neighbours"] = {"mode": str(neighbours["mode"]), "k": int(neighbours["k"])}
    return json.dumps(rec)


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
