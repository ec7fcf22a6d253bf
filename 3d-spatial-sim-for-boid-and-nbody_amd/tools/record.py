"""Offline recorder on the HIP backend: the reference's frame / state on-disk format
(tools/record.py) and its record() GPU loop (:702-935, GPU branch :821-832).

On-disk contract kept so the reference's playback can read the output:
  recordings/<session>/metadata.json                     (:50-58)
  frame_%04d.npz   = np.savez(positions=f32 (N,3), colors=f32 (N,3))          (:88-96)
  frame_%04d.zstd  = u8 format (1 absolute | 2 delta) + u32 len + zstd(positions) +
                     u32 len + zstd(colors); format 2 payload = int16((cur-prev)*1000)   (:231-326)
  state_%04d.npz   = positions, velocities every 50 frames, previous one deleted   (:867-876)
                     (+ `masses`, a superset key: the reference loses masses on resume [quirk];
                     + `tracer_positions`, `tracer_velocities` in a --tracers session, with tracers_%06d.npy beside the frames)
  map_%06d.npy     = float32 (pixels, pixels) surface density every K frames in a --density-map session (a superset file)
The interactive menus, progress bars and the background compressor thread are UX and are not
reproduced; ``compress_recording`` converts finished .npz frames to .zstd with the same delta
chaining, and ``record(config with "zstd": True)`` writes .zstd frames directly: the int16 delta
payload is quantised ON THE DEVICE against the previous decoded frame kept in HBM (12 instead of
24 bytes per body over PCIe), zstd runs on the host.  With the config key "pipeline" (``--pipeline``) the loop
overlaps host and device instead of the reference's compressor thread: frames are fetched asynchronously
(``frame_begin`` / ``frame_wait``) and frame k - 1 is written while the device computes frame k; the files are the
same bytes (``record_pipelined``).  ``extend_recording`` is the reference's
``--extend`` (:1156-1199); Ctrl-C leaves a state checkpoint like the reference (:916-935).  ``main`` is the
reference's command line (``python -m tools.record``, :1128-1283) without the interactive menu; its --help lists
the differences.  zstd comes from the system libzstd through ctypes (python-zstandard is
not installed in this image); without it the .zstd functions raise and raw .npz still works.
"""
import ctypes as C
import json
import os
import struct
import time
from dataclasses import dataclass
from datetime import datetime
from pathlib import Path
from typing import Callable

import numpy as np

from nbody.pairs import auto_pair_edges, check_edges, correlation_dimension, xi_natural  # noqa: F401 (re-exported)

PROJECT_ROOT = Path(__file__).resolve().parent.parent
COMPRESSION_BATCH_SIZE = 50  # reference :225
ZSTD_LEVEL = 19              # reference :252
STATE_EVERY = 50             # reference :867


# ---- zstd through ctypes ------------------------------------------------------------------
_zstd = None


def _load_zstd():
    global _zstd
    if _zstd is None:
        for name in ("libzstd.so.1", "libzstd.so"):
            try:
                z = C.CDLL(name)
                break
            except OSError:
                z = None
        if z is None:
            raise RuntimeError("libzstd not found: .zstd frames unavailable (raw .npz frames still work)")
        z.ZSTD_compressBound.restype = C.c_size_t
        z.ZSTD_compressBound.argtypes = [C.c_size_t]
        z.ZSTD_compress.restype = C.c_size_t
        z.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
        z.ZSTD_decompress.restype = C.c_size_t
        z.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        z.ZSTD_getFrameContentSize.restype = C.c_ulonglong
        z.ZSTD_getFrameContentSize.argtypes = [C.c_void_p, C.c_size_t]
        z.ZSTD_isError.restype = C.c_uint
        z.ZSTD_isError.argtypes = [C.c_size_t]
        _zstd = z
    return _zstd


def zstd_compress(data: bytes, level: int = ZSTD_LEVEL) -> bytes:
    z = _load_zstd()
    cap = z.ZSTD_compressBound(len(data))
    dst = C.create_string_buffer(cap)
    n = z.ZSTD_compress(dst, cap, data, len(data), level)
    if z.ZSTD_isError(n):
        raise RuntimeError("ZSTD_compress failed")
    return dst.raw[:n]


def zstd_decompress(data: bytes) -> bytes:
    z = _load_zstd()
    size = z.ZSTD_getFrameContentSize(data, len(data))
    if size >= (1 << 62):
        raise ValueError("zstd frame without content size")
    dst = C.create_string_buffer(max(1, size))
    n = z.ZSTD_decompress(dst, size, data, len(data))
    if z.ZSTD_isError(n) or n != size:
        raise ValueError("ZSTD_decompress failed")
    return dst.raw[:size]


# ---- session directory / metadata (reference :43-85) ----------------------------------------
def get_recording_dir(session_name: str, root: Path = None) -> Path:
    base = Path(root or PROJECT_ROOT) / "recordings" / session_name
    base.mkdir(parents=True, exist_ok=True)
    return base


def write_metadata(rec_dir: Path, meta: dict):
    """The one writer of metadata.json (atomic: a resume depends on this file)."""
    _atomically(Path(rec_dir) / "metadata.json", lambda f: f.write(json.dumps(meta, indent=2).encode()))


def save_metadata(rec_dir: Path, config: dict, start_time: float):
    write_metadata(rec_dir, {**config, "start_time": start_time,
                             "start_datetime": datetime.fromtimestamp(start_time).isoformat()})


def set_metadata_key(config: dict, rec_dir, key: str, value):
    """The config with `key` set to a value that was just taken from the handle's state (an "auto" parameter), written
    into the session's metadata.json too, from where --resume and --extend read it back."""
    config = dict(config, **{key: value})
    if rec_dir is not None:
        meta = load_metadata(rec_dir) if (Path(rec_dir) / "metadata.json").exists() else dict(config)
        meta[key] = value
        write_metadata(rec_dir, meta)
    return config


def load_metadata(rec_dir: Path) -> dict:
    with open(Path(rec_dir) / "metadata.json", "r") as f:
        return json.load(f)


def _frame_paths(rec_dir, idx):
    rec_dir = Path(rec_dir)
    return rec_dir / f"frame_{idx:04d}.zstd", rec_dir / f"frame_{idx:04d}.npz"


def _frame_on_disk(rec_dir, idx) -> bool:
    return any(p.exists() for p in _frame_paths(rec_dir, idx))


def get_completed_frames(rec_dir: Path) -> int:
    """Number of contiguous frames from 0 present as .npz or .zstd (reference :67-76)."""
    count = 0
    while _frame_on_disk(rec_dir, count):
        count += 1
    return count


def find_latest_state(rec_dir: Path, max_frame: int):
    for frame in range(max_frame, -1, -1):
        p = Path(rec_dir) / f"state_{frame:04d}.npz"
        if p.exists():
            return p, frame
    return None, -1


# ---- frames (reference :88-210, :231-326) -----------------------------------------------------
def _atomically(path: Path, write):
    """`write(file object)` into a temporary name beside `path`, then os.replace: a frame or state file either exists
    complete or not at all.  An interrupt in the middle of a 24 MB frame write (a large share of a frame interval at
    1 M bodies) must not leave a truncated file that get_completed_frames() counts and a resume builds on."""
    path = Path(path)
    tmp = path.with_name("." + path.name + ".part")
    try:
        with open(tmp, "wb") as f:
            write(f)
        os.replace(tmp, path)
    except BaseException:
        try:
            tmp.unlink()
        except OSError:
            pass
        raise


def write_bytes_atomic(path: Path, blob: bytes):
    _atomically(path, lambda f: f.write(blob))


def save_frame(rec_dir: Path, frame_idx: int, positions: np.ndarray, colors: np.ndarray):
    p32, c32 = positions.astype(np.float32), colors.astype(np.float32)
    _atomically(Path(rec_dir) / f"frame_{frame_idx:04d}.npz", lambda f: np.savez(f, positions=p32, colors=c32))


def delta_quantize(cur: np.ndarray, prev: np.ndarray) -> np.ndarray:
    """int16((cur - prev) * 1000) with the reference's C-cast wrap-around beyond +-32.767
    (reference :254-262 [quirk]: lossy, wraps)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return ((cur - prev) * 1000).astype(np.int16)


def pack_container(fmt: int, pos_data: bytes, col_data: bytes) -> bytes:
    """format byte + u32 length + zstd(positions payload) + u32 length + zstd(colours payload) (reference :264-279)."""
    pc, cc = zstd_compress(pos_data), zstd_compress(col_data)
    return struct.pack("B", fmt) + struct.pack("I", len(pc)) + pc + struct.pack("I", len(cc)) + cc


def compress_frame(positions, colors, prev_positions=None, prev_colors=None) -> bytes:
    use_delta = prev_positions is not None and prev_colors is not None
    if use_delta:
        return pack_container(2, delta_quantize(positions, prev_positions).tobytes(),
                              delta_quantize(colors, prev_colors).tobytes())
    return pack_container(1, positions.astype(np.float32).tobytes(), colors.astype(np.float32).tobytes())


def _split_container(data: bytes):
    if len(data) < 1:
        raise ValueError("Invalid compressed data")
    fmt = data[0]
    off = 1
    (psz,) = struct.unpack("I", data[off:off + 4])
    off += 4
    pbytes = data[off:off + psz]
    off += psz
    (csz,) = struct.unpack("I", data[off:off + 4])
    off += 4
    return fmt, pbytes, data[off:off + csz]


def decompress_frame(data: bytes, prev_positions=None, prev_colors=None):
    fmt, pbytes, cbytes = _split_container(data)
    pos_data, col_data = zstd_decompress(pbytes), zstd_decompress(cbytes)
    if fmt == 1:
        return (np.frombuffer(pos_data, dtype=np.float32).reshape(-1, 3),
                np.frombuffer(col_data, dtype=np.float32).reshape(-1, 3))
    if fmt == 2:
        if prev_positions is None or prev_colors is None:
            raise ValueError("Delta compression requires previous frame")
        dp = np.frombuffer(pos_data, dtype=np.int16).reshape(-1, 3).astype(np.float32) / 1000.0
        dc = np.frombuffer(col_data, dtype=np.int16).reshape(-1, 3).astype(np.float32) / 1000.0
        return prev_positions + dp, prev_colors + dc
    raise ValueError(f"Unknown compression format: {fmt}")


def load_frame(rec_dir: Path, frame_idx: int, prev_positions=None, prev_colors=None):
    """(positions f32 (N,3), colors f32 (N,3)); delta frames are resolved by walking back to the
    nearest absolute (.zstd format 1) or raw .npz frame, iteratively (reference :99-210)."""
    zf, nf = _frame_paths(rec_dir, frame_idx)
    if zf.exists():
        data = zf.read_bytes()
        if data and data[0] == 2 and (prev_positions is None or prev_colors is None):
            if frame_idx == 0:
                raise ValueError(f"Frame {frame_idx:04d} appears to be delta-compressed but is the first frame")
            chain = []
            k = frame_idx - 1
            base = None
            while k >= 0:
                zk, nk = _frame_paths(rec_dir, k)
                if zk.exists():
                    dk = zk.read_bytes()
                    chain.append(dk)
                    if dk[0] == 1:
                        break
                elif nk.exists():
                    with np.load(nk) as d:
                        base = (d["positions"].copy(), d["colors"].copy())
                    break
                else:
                    raise FileNotFoundError(f"Frame {k:04d} not found (needed for delta decompression)")
                k -= 1
            if base is None:
                if not chain or chain[-1][0] != 1:
                    raise ValueError(f"Frame {frame_idx:04d} is delta-compressed but no base frame found")
                base = decompress_frame(chain.pop(), None, None)
            for dk in reversed(chain):
                base = decompress_frame(dk, base[0], base[1])
            prev_positions, prev_colors = base
        return decompress_frame(data, prev_positions, prev_colors)
    if nf.exists():
        with np.load(nf) as d:
            return d["positions"].copy(), d["colors"].copy()
    raise FileNotFoundError(f"Frame {frame_idx:04d} not found")


def compress_recording(rec_dir: Path, upto: int = None, batch_size: int = COMPRESSION_BATCH_SIZE):
    """Convert raw frames to .zstd like the reference's BackgroundCompressor batches (:329-470):
    within the run every frame after the very first is a delta against its predecessor."""
    rec_dir = Path(rec_dir)
    total = get_completed_frames(rec_dir) if upto is None else upto
    prev = None
    done = 0
    for idx in range(total):
        zf, nf = _frame_paths(rec_dir, idx)
        if zf.exists():
            prev = load_frame(rec_dir, idx, *(prev or (None, None)))
            continue
        with np.load(nf) as d:
            cur = (d["positions"].copy(), d["colors"].copy())
        blob = compress_frame(cur[0], cur[1], *(prev or (None, None)))
        write_bytes_atomic(zf, blob)
        nf.unlink()
        # the decoder sees the quantised frame: chain on what it will reconstruct
        prev = decompress_frame(blob, *(prev or (None, None)))
        done += 1
    return done


# ---- conservation diagnostics (diagnostics_every: K) -------------------------------------------
DIAGNOSTICS_FILE = "diagnostics.jsonl"


def diagnostics_line(sim, frame: int, substeps: int, dt: float, extra=None, masses=None) -> str:
    """One JSON line (with its newline) for the state `sim` holds after `frame` (-1: the initial state; with `masses` it
    also carries abs_momentum, the scale that the momentum drift is measured against).  Floats are written with repr
    (json's float form), so every value reads back bit for bit."""
    d = sim.diagnostics(potential=True)
    steps = (frame + 1) * substeps
    rec = {"frame": frame, "steps": steps, "time": steps * dt, "mass": d.mass, "center_of_mass": list(d.center_of_mass),
           "momentum": list(d.momentum), "angular_momentum": list(d.angular_momentum), "kinetic": d.kinetic,
           "potential": d.potential, "total": d.total, "terms": d.terms}
    # (the share describes the last step: none before the first one)
    share, all64 = sim.force_precision_share() if frame >= 0 and hasattr(sim, "force_precision_share") else (None, None)
    rec["force_precision_share"] = share
    rec["all_float64"] = all64
    if masses is not None:
        v = sim.get_velocities()
        rec["abs_momentum"] = float(np.sum(masses * np.sqrt(np.sum(v * v, axis=1))))
    if extra:
        rec.update(extra)
    return json.dumps(rec) + "\n"


def read_diagnostics(path: Path):
    """The complete lines of a diagnostics.jsonl as dicts; a torn last line (no newline, or not JSON) is left out."""
    path = Path(path)
    if not path.exists():
        return []
    out = []
    with open(path, "r") as f:
        for line in f:
            if not line.endswith("\n"):
                break
            try:
                out.append(json.loads(line))
            except ValueError:
                break
    return out


def truncate_diagnostics(path: Path, last_frame: int):
    """Keep the lines up to frame `last_frame` (a resume after the checkpoint of that frame), by an atomic rewrite."""
    keep = [r for r in read_diagnostics(path) if r["frame"] <= last_frame]
    _atomically(path, lambda f: f.write("".join(json.dumps(r) + "\n" for r in keep).encode()))
    return keep


def append_line(path: Path, line: str):
    """One complete line per write call; readers skip a line that a killed process left without its newline."""
    with open(path, "a") as f:
        f.write(line)
        f.flush()


def diagnostics_drift(rows):
    """(|E - E0| / |E0|, |P - P0| / sum m|v|_0, |L - L0| / |L0|) of the last row against the first."""
    a, b = rows[0], rows[-1]
    de = abs(b["total"] - a["total"]) / abs(a["total"]) if a["total"] else float("nan")
    dp = float(np.linalg.norm(np.subtract(b["momentum"], a["momentum"])))
    mv = a.get("abs_momentum")
    dp = dp / mv if mv else float("nan")
    l0 = float(np.linalg.norm(a["angular_momentum"]))
    dl = float(np.linalg.norm(np.subtract(b["angular_momentum"], a["angular_momentum"]))) / l0 if l0 else float("nan")
    return de, dp, dl


# ---- density colours (extra config key "color") -------------------------------------------
DENSITY_K = 32


def default_density_range(rho):
    """log10 range of the density ramp taken from a state's k-NN densities: from the 1st percentile of the finite
    log10 rho to its 99.9th percentile plus 1.0 - a decade of headroom, because collapsing systems get denser."""
    rho = np.asarray(rho, dtype=np.float64)
    lg = np.log10(rho[np.isfinite(rho) & (rho > 0.0)])
    if len(lg) == 0:
        raise ValueError("--color density: the state has no finite density to take a range from (give --density-range)")
    return float(np.percentile(lg, 1.0)), float(np.percentile(lg, 99.9)) + 1.0


def color_config(config: dict):
    """The "color" key of a config as (mode, k, range or None); ValueError for a malformed one.  Absent = speed."""
    c = config.get("color")
    if not c:
        return "speed", DENSITY_K, None
    mode = c.get("mode", "speed")
    if mode not in ("speed", "density"):
        raise ValueError(f"color mode must be speed or density, not {mode!r}")
    rng = c.get("log10_range")
    if rng is not None:
        rng = (float(rng[0]), float(rng[1]))
        if not (np.isfinite(rng[0]) and np.isfinite(rng[1]) and rng[1] > rng[0]):
            raise ValueError(f"--density-range: need finite LO < HI, not {rng[0]} {rng[1]}")
    return mode, int(c.get("k", DENSITY_K)), rng


def apply_color_mode(gpu_sim, config: dict, rec_dir: Path = None):
    """Put the handle into the config's colour mode.  A density session without a range takes it once, here, from the
    handle's current state (the initial one for a new recording) on the host, and writes it into metadata.json, from
    where --resume and --extend re-apply it.  Returns the config (with the range filled in)."""
    mode, k, rng = color_config(config)
    if mode != "density":
        return config
    if rng is None:
        rng = default_density_range(gpu_sim.densities(k))
        config = set_metadata_key(config, rec_dir, "color", {"mode": "density", "k": k, "log10_range": [rng[0], rng[1]]})
    gpu_sim.set_color_mode("density", k=k, log10_range=rng)
    return config


# ---- friends-of-friends groups (extra config key "groups") ---------------------------------
GROUPS_FILE = "groups.jsonl"
GROUPS_MIN_MEMBERS = 20
GROUPS_ROWS = 64  # catalogue rows kept per line


def default_linking_length(r2_1):
    """The linking length "auto" stands for: twice the median nearest-neighbour distance of a state (its knn(1)
    squared distances).  The factor 2 is a convention, not a measured optimum."""
    d = np.sqrt(np.asarray(r2_1, dtype=np.float64))
    b = 2.0 * float(np.median(d)) if len(d) else 0.0
    if not (np.isfinite(b) and b > 0.0):
        raise ValueError("--linking-length auto: the state's median nearest-neighbour distance is not finite and > 0 "
                         "(give --linking-length B)")
    return b


def groups_config(config: dict):
    """The "groups" key of a config, {"every": K, "link": b, "min_members": M}, as (every, link or None for an "auto" not
    yet taken, min_members); None without the key; ValueError for a malformed one."""
    g = config.get("groups")
    if not g:
        return None
    every, mm, link = int(g.get("every", 0)), int(g.get("min_members", GROUPS_MIN_MEMBERS)), g.get("link", "auto")
    if every <= 0:
        raise ValueError(f"--groups: K must be positive, not {every}")
    if mm < 1:
        raise ValueError(f"--min-members: M must be at least 1, not {mm}")
    if link == "auto" or link is None:
        return every, None, mm
    link = float(link)
    if not (np.isfinite(link) and link > 0.0):
        raise ValueError(f"--linking-length: B must be finite and > 0 (or auto), not {link}")
    return every, link, mm


def groups_line(sim, frame: int, link: float, min_members: int) -> str:
    """One JSON line (with its newline) for the groups of the state `sim` holds after `frame`: their number, the number
    of those with at least min_members bodies and the first GROUPS_ROWS rows of the catalogue, largest first.  Two
    queries per line: the catalogue call runs the build and the pair search again (its C call has no output for the
    number of all groups)."""
    sim.find_groups(link)
    cat = sim.group_catalogue(link, min_members=min_members, capacity=GROUPS_ROWS)
    rows = [{"label": int(cat["label"][i]), "members": int(cat["members"][i]), "mass": float(cat["mass"][i]),
             "center": [float(x) for x in cat["center"][i]], "velocity": [float(x) for x in cat["velocity"][i]],
             "lo": [float(x) for x in cat["lo"][i]], "hi": [float(x) for x in cat["hi"][i]]}
            for i in range(len(cat["label"]))]
    return json.dumps({"frame": frame, "link": link, "min_members": min_members, "n_groups": int(sim.n_groups),
                       "count": int(cat["count"]), "groups": rows}) + "\n"


# ---- binned pair counts (extra config key "pairs") -----------------------------------------
PAIRS_FILE = "pairs.jsonl"


def pairs_config(config: dict):
    """The "pairs" key of a config, {"every": K, "edges": [e0, e1, ...]}, as (every, edges or None for an "auto" not yet
    taken); None without the key; ValueError for a malformed one."""
    g = config.get("pairs")
    if not g:
        return None
    every, edges = int(g.get("every", 0)), g.get("edges", "auto")
    if every <= 0:
        raise ValueError(f"--pairs: K must be positive, not {every}")
    if edges is None or (isinstance(edges, str) and edges == "auto"):
        return every, None
    try:
        return every, [float(x) for x in check_edges(edges)]
    except (TypeError, ValueError) as e:
        raise ValueError(f"--pair-edges: {e}") from None


def pairs_line(sim, frame: int, edges) -> str:
    """One JSON line (with its newline) for the pair counts of the state `sim` holds after `frame`: the edges, the pairs
    within the first edge, the pairs per bin, and the correlation dimension over all edges with the number of points it
    used (null and 0 where fewer than two edges have a pair within them)."""
    counts, below = sim.pair_counts(edges)
    counts = [int(c) for c in counts]
    try:
        d2, points = correlation_dimension(edges, below, counts)
    except ValueError:
        d2, points = None, 0
    return json.dumps({"frame": frame, "edges": [float(e) for e in edges], "below": int(below), "counts": counts,
                       "d2": d2, "d2_points": points}) + "\n"


# ---- rotation curve (extra config key "rotation_curve") -------------------------------------
ROTATION_FILE = "rotation.jsonl"
CURVE_AUTO_RADII = 16  # "auto": spawn_radius * k / 16, k = 1 .. 16
CURVE_MAX_RADII = 256
CURVE_AZIMUTHS = 16


def check_curve_radii(radii):
    """The radii as a list of floats if a rotation curve can take them (ValueError otherwise): 1 .. 256 finite, positive,
    strictly increasing values."""
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    if not 1 <= len(r) <= CURVE_MAX_RADII:
        raise ValueError(f"need 1 .. {CURVE_MAX_RADII} radii, got {len(r)}")
    if not np.all(np.isfinite(r)) or np.any(r <= 0.0) or np.any(np.diff(r) <= 0.0):
        raise ValueError("the radii must be finite, positive and strictly increasing")
    return [float(x) for x in r]


def rotation_config(config: dict):
    """The "rotation_curve" key of a config, {"every": K, "radii": [r0, r1, ...]}, as (every, radii); None without the
    key; ValueError for a malformed one."""
    g = config.get("rotation_curve")
    if not g:
        return None
    every = int(g.get("every", 0))
    if every <= 0:
        raise ValueError(f"--rotation-curve: K must be positive, not {every}")
    try:
        return every, check_curve_radii(g.get("radii"))
    except (TypeError, ValueError) as e:
        raise ValueError(f"--curve-radii: {e}") from None


def rotation_line(sim, frame: int, radii) -> str:
    """One JSON line (with its newline) for the rotation curve of the state `sim` holds after `frame`, about its centre
    of mass in the plane z = const: per radius the azimuthal means of the inward acceleration and of the potential over
    CURVE_AZIMUTHS points of the ring, and the circular speed in that mean field (nbody/field.py)."""
    from nbody.field import rotation_curve
    center = [float(x) for x in sim.diagnostics(potential=False).center_of_mass]
    c = rotation_curve(sim, radii, center, azimuths=CURVE_AZIMUTHS, normal=(0, 0, 1))
    return json.dumps({"frame": frame, "center": center, "radii": [float(r) for r in radii],
                       "a_radial": [float(x) for x in c["a_radial"]], "v_circ": [float(x) for x in c["v_circ"]],
                       "phi": [float(x) for x in c["phi"]]}) + "\n"


# ---- time-step check (extra config key "timestep_check") ------------------------------------
TIMESTEP_FILE = "timestep.jsonl"
# chi = Omega dt per step.  Display values, not tolerances: 2 is the stability limit of a harmonic mode for both
# integrators; 0.1 and 0.5 are 63 and 13 steps per orbit.
CHI_LEVELS = (0.1, 0.5, 2.0)
CHI_MAX_LEVELS = 16
CHI_QUANTILES = (0.5, 0.9, 0.99, 1.0)
CHI_UNSTABLE = 2.0


def check_chi_levels(levels):
    """The levels as a list of floats if the time-step check can take them (ValueError otherwise): 1 .. 16 finite,
    positive, strictly increasing values."""
    v = np.asarray(levels, dtype=np.float64).reshape(-1)
    if not 1 <= len(v) <= CHI_MAX_LEVELS:
        raise ValueError(f"need 1 .. {CHI_MAX_LEVELS} levels, got {len(v)}")
    if not np.all(np.isfinite(v)) or np.any(v <= 0.0) or np.any(np.diff(v) <= 0.0):
        raise ValueError("the levels must be finite, positive and strictly increasing")
    return [float(x) for x in v]


def timestep_config(config: dict):
    """The "timestep_check" key of a config, {"every": K, "levels": [c0, c1, ...]}, as (every, dt of a step, levels);
    None without the key; ValueError for a malformed one."""
    g = config.get("timestep_check")
    if not g:
        return None
    every = int(g.get("every", 0))
    if every <= 0:
        raise ValueError(f"--timestep-check: K must be positive, not {every}")
    try:
        levels = check_chi_levels(g.get("levels", CHI_LEVELS))
    except (TypeError, ValueError) as e:
        raise ValueError(f"--chi-levels: {e}") from None
    return every, config["dt_per_frame"] / config["substeps"], levels


def timestep_line(sim, frame: int, dt: float, levels) -> str:
    """One JSON line (with its newline) for the state `sim` holds after `frame`: chi = phase_per_step(tidal_norm, dt), the
    orbital phase a step of `dt` advances at every body (nbody/field.py) - its quantiles over the bodies and, per level,
    the number of bodies above it."""
    from nbody.field import phase_per_step
    chi = phase_per_step(sim.tidal_norm(), dt)
    q = np.quantile(chi, CHI_QUANTILES) if len(chi) else np.zeros(len(CHI_QUANTILES))
    return json.dumps({"frame": frame, "dt": float(dt), "chi_quantiles": {str(k): float(v) for k, v in zip(CHI_QUANTILES, q)},
                       "levels": [float(c) for c in levels], "above": [int((chi > c).sum()) for c in levels],
                       "bodies": int(len(chi))}) + "\n"


# ---- radial profile and Lagrangian radii (extra config key "profile") -----------------------
PROFILE_FILE = "profile.jsonl"
PROFILE_FRACTIONS = (0.1, 0.25, 0.5, 0.75, 0.9)


def check_profile_edges(edges):
    """The edges as a list of floats if nbmi_radial_profile can take them (ValueError otherwise): 2 .. 257 finite values,
    the first >= 0, strictly increasing."""
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    if not 2 <= len(e) <= 257:
        raise ValueError(f"need 2 .. 257 edges, got {len(e)}")
    if not np.all(np.isfinite(e)) or e[0] < 0.0 or np.any(np.diff(e) <= 0.0):
        raise ValueError("the edges must be finite, >= 0 and strictly increasing")
    return [float(x) for x in e]


def profile_config(config: dict):
    """The "profile" key of a config, {"every": K, "edges": [e0, e1, ...], "fractions": [f0, ...]}, as (every, edges,
    fractions); None without the key; ValueError for a malformed one."""
    g = config.get("profile")
    if not g:
        return None
    every = int(g.get("every", 0))
    if every <= 0:
        raise ValueError(f"--profile: K must be positive, not {every}")
    try:
        edges = check_profile_edges(g.get("edges"))
    except (TypeError, ValueError) as e:
        raise ValueError(f"--profile-edges: {e}") from None
    try:
        fr = [float(x) for x in np.asarray(g.get("fractions", PROFILE_FRACTIONS), dtype=np.float64).reshape(-1)]
    except (TypeError, ValueError):
        fr = []
    if not 1 <= len(fr) <= 64 or not all(np.isfinite(f) and 0.0 < f <= 1.0 for f in fr):
        raise ValueError(f"--profile-fractions: need 1 .. 64 numbers in (0, 1], not {g.get('fractions')!r}")
    return every, edges, fr


def profile_line(sim, frame: int, edges, fractions) -> str:
    """One JSON line (with its newline) for the radial structure of the state `sim` holds after `frame`, about its centre
    of mass and relative to its velocity: per slot (the ball inside edges[0], then the shells) the bodies, the mass, the
    density, the mean radial velocity, both dispersions and the anisotropy (null for an empty slot), and the Lagrangian
    radii of `fractions` (nbody/profile.py)."""
    from nbody import profile as prof
    got = sim.radial_profile(edges, quantities=("number", "mass", "radial_momentum", "radial_kinetic", "kinetic"))
    center = [float(x) for x in got["center"]]
    rho, _ = prof.density_profile(got, edges)
    vel = prof.velocity_profile(got)
    radii = np.sqrt(sim.mass_radii(fractions, center=center)["radius2"])

    def clean(a):
        return [float(x) if np.isfinite(x) else None for x in a]
    return json.dumps({"frame": frame, "center": center, "bulk_velocity": [float(x) for x in got["bulk_velocity"]],
                       "edges": [float(e) for e in edges], "count": [int(c) for c in got["number"]],
                       "mass": [float(x) for x in got["mass"]], "density": clean(rho), "mean_vr": clean(vel["mean_vr"]),
                       "sigma_r": clean(vel["sigma_r"]), "sigma_t": clean(vel["sigma_t"]), "beta": clean(vel["beta"]),
                       "fractions": [float(f) for f in fractions], "lagrangian_radii": clean(radii)}) + "\n"


# ---- periodic side files: one description each, one mechanism for all -----------------------
@dataclass(frozen=True)
class LineStream:
    """A side file that gets one JSON line every K-th frame."""
    file: str
    settings: Callable           # config -> None (absent) or (every, parameters ...); ValueError for a malformed config
    line: Callable               # (sim, frame, parameters ...) -> the line for the state after `frame`
    key: str = None              # where the first parameter may be "auto" (None in the settings until taken): the config key
    auto: Callable = None        # and (sim, settings) -> its value with "auto" taken from the handle's current state
    first_line: Callable = None  # (sim, masses, parameters ...) -> the line a file that starts at frame 0 begins with

    def apply(self, gpu_sim, config: dict, rec_dir: Path = None):
        """The config with an "auto" parameter resolved: taken once, here, from the handle's current state (the initial one
        for a new recording) and written into metadata.json, from where --resume and --extend re-apply it."""
        s = self.settings(config)
        if s is None or self.auto is None or s[1] is not None:
            return config
        return set_metadata_key(config, rec_dir, self.key, self.auto(gpu_sim, s))


def diagnostics_config(config: dict):
    """The bare "diagnostics_every" key as (every, substeps, dt, extra keys of every line); None without it."""
    every, substeps, integrator = int(config.get("diagnostics_every") or 0), config["substeps"], config.get("integrator")
    # (a leapfrog session's lines say so: their velocities, hence K and E, are synchronized with the positions)
    extra = {"integrator": integrator} if integrator not in (None, "kick_drift") else None
    return (every, substeps, config["dt_per_frame"] / substeps, extra) if every > 0 else None


DIAGNOSTICS = LineStream(DIAGNOSTICS_FILE, diagnostics_config, diagnostics_line,
                         first_line=lambda sim, masses, *p: diagnostics_line(sim, -1, *p, masses=masses))
GROUPS = LineStream(GROUPS_FILE, groups_config, groups_line, key="groups",
                    auto=lambda sim, s: {"every": s[0], "link": default_linking_length(sim.knn(1)[0]), "min_members": s[2]})
PAIRS = LineStream(PAIRS_FILE, pairs_config, pairs_line, key="pairs",
                   auto=lambda sim, s: {"every": s[0], "edges": auto_pair_edges(sim.knn(1)[0])})
ROTATION = LineStream(ROTATION_FILE, rotation_config, rotation_line)  # ("auto" radii need no state: build_config)
PROFILE = LineStream(PROFILE_FILE, profile_config, profile_line)  # ("auto" edges need no state either)
apply_groups, apply_pairs = GROUPS.apply, PAIRS.apply  # (gpu_sim, config, rec_dir=None) -> the config, "auto" resolved
TIMESTEP = LineStream(TIMESTEP_FILE, timestep_config, timestep_line)
LINE_STREAMS = (DIAGNOSTICS, TIMESTEP, GROUPS, PROFILE, PAIRS, ROTATION)  # in the order of their lines after a frame; a new side file is one more entry


def line_due(frame: int, every: int) -> bool:
    return every > 0 and (frame + 1) % every == 0


def open_lines(gpu_sim, config: dict, rec_dir: Path, start_frame: int, masses):
    """Start (at frame 0) or truncate (a resume) the side file of every stream the config has on.  Returns (due, write):
    due(frame) says whether any stream has a line after `frame`, write(frame) appends the lines that are due and not yet
    written - the synchronous per-frame lines of both loops."""
    on, last = [], {}  # per stream: (stream, settings, path), and by path the last frame it has a line for
    for stream in LINE_STREAMS:
        s = stream.settings(config)
        if s is None:
            continue
        path = Path(rec_dir) / stream.file
        if start_frame == 0:  # a run from frame 0 starts the file afresh
            first = stream.first_line(gpu_sim, masses, *s[1:]) if stream.first_line else ""
            _atomically(path, lambda f: f.write(first.encode()))
        else:
            truncate_diagnostics(path, start_frame - 1)
        on.append((stream, s, path))

    def due(frame):
        return any(line_due(frame, s[0]) for _, s, _ in on)

    def write(frame):
        for stream, s, path in on:
            if line_due(frame, s[0]) and frame > last.get(path, start_frame - 1):
                append_line(path, stream.line(gpu_sim, frame, *s[1:]))
                last[path] = frame
    return due, write


# ---- massless tracers (extra config key "tracers") ------------------------------------------
def tracers_config(config: dict):
    """The "tracers" key of a config, {"file": the .npy of the seeds, "every": K}, as (file, every); None without the
    key.  every == 0: the tracers are carried (and checkpointed) but no tracer file is written."""
    t = config.get("tracers")
    if not t:
        return None
    every = int(t.get("every") or 0)
    if every < 0 or not t.get("file"):
        raise ValueError(f"--tracers: need a file and a period K >= 0, not {t}")
    return str(t["file"]), every


def load_tracer_seeds(path):
    """(positions, velocities) float64 from an .npy array (m, 3) or (m, 6), rows x y z [vx vy vz]; velocities None for
    (m, 3): the tracers start at rest."""
    a = np.load(path, allow_pickle=False)
    if a.ndim != 2 or a.shape[1] not in (3, 6):
        raise ValueError(f"--tracers: {path} holds an array of shape {a.shape}, not (m, 3) or (m, 6)")
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.ascontiguousarray(a[:, :3]), (np.ascontiguousarray(a[:, 3:]) if a.shape[1] == 6 else None)


def tracer_file(rec_dir, frame: int) -> Path:
    return Path(rec_dir) / f"tracers_{frame:06d}.npy"


def write_tracer_file(gpu_sim, rec_dir, frame: int):
    """tracers_%06d.npy: the tracers' positions after `frame`, (m, 3) float32 in the order of the seed file."""
    p = np.ascontiguousarray(gpu_sim.tracer_positions_f32(), dtype=np.float32)
    _atomically(tracer_file(rec_dir, frame), lambda f: np.save(f, p))


def last_tracer_file(rec_dir, upto: int):
    """The newest tracer file of a frame below `upto` (files beyond the completed frames are a cut-short run's), or None."""
    frames = sorted(int(p.stem.split("_")[1]) for p in Path(rec_dir).glob("tracers_[0-9][0-9][0-9][0-9][0-9][0-9].npy"))
    frames = [f for f in frames if f < upto]
    return tracer_file(rec_dir, frames[-1]) if frames else None


# ---- surface-density maps (extra config key "density_map") ----------------------------------
MAP_PIXELS = 512
MAP_HALF_WIDTH_FACTOR = 1.5  # x the preset's spawn radius


def density_map_config(config: dict):
    """The "density_map" key of a config, {"every": K, "pixels": n, "half_width": w, "axis": "x" | "y" | "z"}, as
    (every, pixels, half_width, axis); None without the key."""
    d = config.get("density_map")
    if not d:
        return None
    every, pixels, axis = int(d.get("every") or 0), int(d.get("pixels", MAP_PIXELS)), d.get("axis", "z")
    hw = float(d.get("half_width", MAP_HALF_WIDTH_FACTOR * config["spawn_radius"]))
    if every <= 0:
        raise ValueError(f"--density-map: K must be positive, not {d.get('every')}")
    if not 1 <= pixels <= 16384:
        raise ValueError(f"--map-pixels: need 1 .. 16384, not {pixels}")
    if not (np.isfinite(hw) and hw > 0.0):
        raise ValueError(f"--map-half-width: need a finite width > 0, not {hw}")
    if axis not in ("x", "y", "z"):
        raise ValueError(f"--map-axis: need x, y or z, not {axis!r}")
    return every, pixels, hw, axis


def map_file(rec_dir, frame: int) -> Path:
    return Path(rec_dir) / f"map_{frame:06d}.npy"


def write_map_file(gpu_sim, rec_dir, frame: int, pixels: int, half_width: float, axis: str):
    """map_%06d.npy: the surface density (mass per area, CIC) about the origin after `frame`, (pixels, pixels) float32."""
    from nbody.grid import surface_density
    m = np.ascontiguousarray(surface_density(gpu_sim, axis=axis, half_width=half_width, pixels=pixels), dtype=np.float32)
    _atomically(map_file(rec_dir, frame), lambda f: np.save(f, m))


def _with_maps(gpu_sim, rec_dir, dmap, lines_due, write_lines):
    """(due, write) of both loops with the maps added: a map is due like a line, and written after the lines."""
    every, pixels, half_width, axis = dmap

    def due(frame):
        return lines_due(frame) or line_due(frame, every)

    def write(frame):
        write_lines(frame)
        if line_due(frame, every):
            write_map_file(gpu_sim, rec_dir, frame, pixels, half_width, axis)
    return due, write


def map_frames(rec_dir, upto: int):
    """The frames below `upto` that have a map file, ascending (files beyond the completed frames are a cut-short run's)."""
    frames = sorted(int(p.stem.split("_")[1]) for p in Path(rec_dir).glob("map_[0-9][0-9][0-9][0-9][0-9][0-9].npy"))
    return [f for f in frames if f < upto]


# ---- initial conditions + the recording loops -----------------------------------------------------------------------
def _generate_initial_conditions(config: dict):
    from tools.presets import generate_distribution
    p, v, m = generate_distribution(config.get("distribution", "galaxy"), config["num_bodies"],
                                    config["spawn_radius"], config["G"])
    return p.astype(np.float64), v.astype(np.float64), m.astype(np.float64)


def frame_kind(frame: int, direct_zstd: bool, absolute: bool = False) -> str:
    """"f32" (raw .npz), or in a .zstd session "key" (format 1: frame 0, or a frame that must not depend on the delta
    chain - format 1 is legal anywhere) or "delta" (format 2)."""
    return ("key" if frame == 0 or absolute else "delta") if direct_zstd else "f32"


def write_frame_file(rec_dir: Path, frame: int, kind: str, a, b):
    """The file of one frame from the two arrays of its kind: positions and colours, or their int16 deltas."""
    if kind == "f32":
        save_frame(rec_dir, frame, a, b)
    else:
        zf, _ = _frame_paths(rec_dir, frame)
        write_bytes_atomic(zf, pack_container(1 if kind == "key" else 2, a.tobytes(), b.tobytes()))


def _after_frame(rec_dir: Path, frame: int, write_lines, write_state):
    """What follows a frame's file: its lines, and every STATE_EVERY frames the checkpoint that replaces the older one."""
    write_lines(frame)  # before the state checkpoint: a resume from it finds every line up to its frame
    if (frame + 1) % STATE_EVERY == 0:
        write_state(frame)
        old = Path(rec_dir) / f"state_{frame - STATE_EVERY:04d}.npz"
        if old.exists():
            old.unlink()


def device_frame(gpu_sim, start_frame: int, substeps: int) -> int:
    """The frame the DEVICE stands at, asked of the library: an interrupt is delivered when the step call returns,
    before a loop could note anything."""
    return start_frame - 1 + gpu_sim.step_count() // max(substeps, 1)


def _pause(at: int, write_lines, write_state):
    """Ctrl-C in either loop (reference :916-935), once every frame up to `at`, where the device stands, is on disk: its
    lines and a compressed state file so that --resume continues from there.  The checkpoint must be the state of
    exactly the last frame on disk, or a resume would skip or repeat one frame interval."""
    if at >= 0:
        write_lines(at)
        write_state(at, compressed=True)


def record_pipelined(gpu_sim, rec_dir: Path, start_frame: int, total_frames: int, substeps: int, dt: float,
                     direct_zstd: bool, lines_due, write_lines, write_state):
    """The recording loop of ``record(config with "pipeline": True)``: the files of the sequential loop, but
    the host compresses and writes frame k - 1 while the device computes frame k.  Per frame: step_many (enqueue),
    frame_begin (enqueue: one snapshot kernel, then the copy on a stream of its own), then the PREVIOUS frame is finished:
    frame_wait, its file through the sequential loop's writer, frame_release.  Where a line is due - `lines_due(frame)`
    says so, once for all side files; one period K given in its place stands for line_due(frame, K) - or a state
    checkpoint is, the frame itself is finished first: write_lines(frame) / write_state(frame, compressed=False) are the
    caller's synchronous writers, and the checkpoint stays the state of exactly the last frame on disk.

    `gpu_sim` needs step_many, frame_begin, frame_wait, frame_release, frames_pending and step_count (the backend object,
    or a stand-in: nothing here touches a device).  On Ctrl-C the library is asked which frames are in flight and where
    the device stands; every pending frame is written from its slot (a delta frame as a delta: the slot still holds the
    payload), a stepped frame that has no slot yet is taken, then the lines and the compressed checkpoint of the frame
    the device is at, and the interrupt is re-raised.  Returns the last frame written."""
    if not callable(lines_due):
        every, lines_due = int(lines_due), lambda frame: line_due(frame, every)

    def finish(slot, frame, kind):
        write_frame_file(rec_dir, frame, kind, *gpu_sim.frame_wait(slot))
        gpu_sim.frame_release(slot)

    frame = start_frame - 1
    held = None  # the frame begun and not yet written: (slot, frame, kind)
    try:
        for frame in range(start_frame, total_frames):
            gpu_sim.step_many(dt, substeps)
            kind = frame_kind(frame, direct_zstd)
            slot = gpu_sim.frame_begin(kind, 15.0)
            if held is not None:
                finish(*held)
            held = (slot, frame, kind)
            if (frame + 1) % STATE_EVERY == 0 or lines_due(frame):
                finish(*held)
                held = None
                _after_frame(rec_dir, frame, write_lines, write_state)
        if held is not None:
            finish(*held)
    except KeyboardInterrupt:
        # asked of the library, not of `held`: the interrupt may have come between a C call and the assignment
        pending = gpu_sim.frames_pending()
        at = device_frame(gpu_sim, start_frame, substeps)
        for slot, kind, steps in pending:
            f = start_frame - 1 + steps // max(substeps, 1)
            if _frame_on_disk(rec_dir, f):  # written, not yet released
                gpu_sim.frame_release(slot)
            else:                           # not written - or its write was cut short, which left nothing (_atomically)
                finish(slot, f, kind)
        if at >= start_frame and not _frame_on_disk(rec_dir, at):
            # stepped, no slot yet: the chain stands at frame at - 1, so the normal kind
            kind = frame_kind(at, direct_zstd)
            finish(gpu_sim.frame_begin(kind, 15.0), at, kind)
        _pause(at, write_lines, write_state)
        raise
    return frame


def record(config: dict, resume: bool = False, root: Path = None, quiet: bool = False, seed=None):
    """The reference's record() on the GPU branch (:760-775, :821-876): per frame `substeps` x
    step(dt_per_frame/substeps), compute_colors(15.0), get_positions, get_colors, raw frame;
    velocities only every 50th frame for the state checkpoint.  Returns the session directory."""
    from nbody.gpu_backend import Backend, create_gpu_simulation, get_backend

    def say(*a):
        if not quiet:
            print(*a)

    rec_dir = get_recording_dir(config["session_name"], root)
    start_frame = 0
    positions = velocities = masses = None
    tracer_state = None  # (positions, velocities) of the tracers in the checkpoint a resume starts from
    if resume:
        completed = get_completed_frames(rec_dir)
        if completed > 0:
            state_file, state_frame = find_latest_state(rec_dir, completed)
            if state_file is not None:
                with np.load(state_file) as st:
                    positions = st["positions"].astype(np.float64)
                    velocities = st["velocities"].astype(np.float64)
                    masses = st["masses"].astype(np.float64) if "masses" in st.files else None
                    if "tracer_positions" in st.files:
                        tracer_state = (st["tracer_positions"].astype(np.float64), st["tracer_velocities"].astype(np.float64))
                start_frame = state_frame + 1
                say(f"[Record] Resuming from frame {start_frame}")
    device_ic = bool(config.get("device_ic")) and positions is None
    if positions is None:
        # `seed` is a superset key of metadata.json: a resume / extend that finds no state checkpoint starts
        # over from frame 0 (as the reference does) and must then draw the SAME bodies (the reference, unseeded,
        # silently continues a recording with a different system)
        if seed is None:
            seed = config.get("seed")
        else:
            config = dict(config, seed=int(seed))
        if not device_ic:
            if seed is not None:
                np.random.seed(seed)
            positions, velocities, masses = _generate_initial_conditions(config)
        save_metadata(rec_dir, config, time.time())
    n = config["num_bodies"]
    total_frames = config["total_frames"]
    substeps = config["substeps"]
    dt = config["dt_per_frame"] / substeps
    if masses is None:
        masses = np.ones(n, dtype=np.float64)  # reference :752-753 [quirk]
    # extra config key (metadata.json, only when not the default): "leapfrog" = synchronized kick-drift-kick
    integrator = config.get("integrator", "kick_drift")
    # likewise "multipole": "quadrupole" = cell terms with second moments
    multipole = config.get("multipole", "monopole")

    backend, info = get_backend()
    if backend != Backend.HIP:
        raise RuntimeError(f"[Record] no HIP backend ({info}); this build has no CPU fallback")
    if device_ic:  # extra config key: bodies drawn on the GPU (statistical parity with the presets' generator)
        from tools.presets import generate_distribution_device
        gpu_sim = generate_distribution_device(config.get("distribution", "galaxy"), n, config["spawn_radius"],
                                               config["G"], config["softening"], config["damping"],
                                               theta=config.get("theta", 0.5), seed=42 if seed is None else seed,
                                               integrator=integrator, multipole=multipole)
    else:
        gpu_sim = create_gpu_simulation(positions, velocities, masses, config["G"], config["softening"],
                                        config["damping"], theta=config.get("theta", 0.5), force_gpu=True,
                                        integrator=integrator, multipole=multipole)
    if gpu_sim is None:
        raise RuntimeError("[Record] create_gpu_simulation returned None")
    if device_ic:  # the state checkpoints carry the generated masses (0.1 for "filament"), not the unit default
        masses = gpu_sim.get_masses()
    say(f"[Record] GPU acceleration: {backend.value} - {info}")
    # extra config key "color": {"mode": "density", "k": K, "log10_range": [lo, hi]} = frames coloured by the k-NN
    # density through the unchanged colour and frame calls of both loops
    # extra config keys "diagnostics_every", "timestep_check", "groups", "profile", "pairs", "rotation_curve": every K-th frame a line in a side file (LINE_STREAMS)
    try:
        config = apply_color_mode(gpu_sim, config, rec_dir)
        for stream in LINE_STREAMS:
            config = stream.apply(gpu_sim, config, rec_dir)
        direct_zstd = bool(config.get("zstd"))  # extra config key: write .zstd frames, delta payload quantised on the device
        if direct_zstd and start_frame > 0:
            # the delta chain continues from what a reader reconstructs for the last frame on disk
            gpu_sim.frame_set_previous(*load_frame(rec_dir, start_frame - 1))
        t0 = time.time()
        lines_due, write_lines = open_lines(gpu_sim, config, rec_dir, start_frame, masses)
        # extra config key "tracers": massless tracers carried by the steps, from the checkpoint on a
        # resume, from the seed file otherwise; every K-th frame their positions in a file of their own, which both
        # loops write where they write the lines
        tracers = tracers_config(config)
        if tracers is not None:
            gpu_sim.set_tracers(*(tracer_state if tracer_state is not None else load_tracer_seeds(tracers[0])))
            say(f"[Record] {gpu_sim.tracer_count:,} tracers" + (f", a file every {tracers[1]} frames" if tracers[1] else ""))
            side_due, side_lines = lines_due, write_lines

            def lines_due(frame):
                return side_due(frame) or line_due(frame, tracers[1])

            def write_lines(frame):
                side_lines(frame)
                if line_due(frame, tracers[1]):
                    write_tracer_file(gpu_sim, rec_dir, frame)
        # extra config key "density_map": every K-th frame a surface-density map, written like the tracer files
        dmap = density_map_config(config)
        if dmap is not None:
            say(f"[Record] a {dmap[1]} x {dmap[1]} surface-density map along {dmap[3]} every {dmap[0]} frames")
            lines_due, write_lines = _with_maps(gpu_sim, rec_dir, dmap, lines_due, write_lines)

        def write_frame(frame, absolute=False):
            gpu_sim.compute_colors(15.0)
            kind = frame_kind(frame, direct_zstd, absolute)
            a, b = (gpu_sim.frame_keyframe() if kind == "key" else gpu_sim.frame_delta() if kind == "delta"
                    else (gpu_sim.get_positions(), gpu_sim.get_colors()))
            write_frame_file(rec_dir, frame, kind, a, b)

        def write_state(frame, compressed=False):
            x, v = gpu_sim.get_positions_f64(), gpu_sim.get_velocities()
            more = dict(zip(("tracer_positions", "tracer_velocities"), gpu_sim.get_tracers())) if tracers is not None else {}
            _atomically(rec_dir / f"state_{frame:04d}.npz", lambda f: (np.savez_compressed if compressed else np.savez)(
                f, positions=x, velocities=v, masses=masses, **more))

        pipeline = bool(config.get("pipeline"))  # extra config key (metadata.json, only when set): the loop of DESIGN 4.11
        frame = start_frame - 1
        try:
            if pipeline:
                record_pipelined(gpu_sim, rec_dir, start_frame, total_frames, substeps, dt, direct_zstd, lines_due,
                                 write_lines, write_state)
            else:
                for frame in range(start_frame, total_frames):
                    gpu_sim.step_many(dt, substeps)
                    write_frame(frame)
                    _after_frame(rec_dir, frame, write_lines, write_state)
        except KeyboardInterrupt:
            at = device_frame(gpu_sim, start_frame, substeps)
            if not pipeline:  # (record_pipelined has done the same for its frames in flight)
                if at >= 0 and at == frame and not _frame_on_disk(rec_dir, at):
                    # stepped, frame not written - or its write was cut short: frames reach their name only complete
                    # (_atomically), so a cut-short write left nothing; the device-side delta chain may already have
                    # moved on, so this frame is written absolute
                    write_frame(at, absolute=True)
                _pause(at, write_lines, write_state)
            say(f"\n[Record] Paused at frame {at}; resume with record(config, resume=True)")
            raise
        say(f"[Record] {total_frames - start_frame} frames in {time.time() - t0:.2f}s -> {rec_dir}"
            + (" (pipelined)" if pipeline else ""))
    finally:
        gpu_sim.close()
    return rec_dir


def extend_recording(session_name: str, extra_frames: int, root: Path = None, quiet: bool = True):
    """The reference's ``--extend N session`` (:1156-1199): total_frames += N in metadata.json, then resume."""
    rec_dir = get_recording_dir(session_name, root)
    if not (rec_dir / "metadata.json").exists():
        raise FileNotFoundError(f"[Record] No recording found: {session_name}")
    config = load_metadata(rec_dir)
    config["total_frames"] = int(config["total_frames"]) + int(extra_frames)
    write_metadata(rec_dir, config)
    config["session_name"] = session_name
    return record(config, resume=True, root=root, quiet=quiet)


# ---- command line (reference :938-992, :1116-1283) ---------------------------------------------
def _session_dir(session_name: str, root: Path = None) -> Path:
    """get_recording_dir without creating it (a status query leaves no empty directory behind)."""
    return Path(root or PROJECT_ROOT) / "recordings" / session_name


def parse_number(value: str) -> int:
    """100000, 100k, 1.5m (case-insensitive) -> int (reference :1116-1125)."""
    value = value.strip().lower()
    for suffix, mult in (("k", 1_000), ("m", 1_000_000)):
        if value.endswith(suffix):
            return int(float(value[:-1]) * mult)
    return int(value)


def show_status(session_name: str, root: Path = None) -> bool:
    """Progress of one session (reference :938-961); False when it has no metadata.json."""
    rec_dir = _session_dir(session_name, root)
    if not (rec_dir / "metadata.json").exists():
        print(f"[Status] No recording found: {session_name}")
        return False
    meta = load_metadata(rec_dir)
    completed, total = get_completed_frames(rec_dir), meta["total_frames"]
    print(f"\n[Status] Recording: {session_name}")
    print(f"  Bodies: {meta['num_bodies']:,}")
    print(f"  Theta: {meta['theta']}")
    print(f"  Distribution: {meta.get('distribution', 'unknown')}")
    print(f"  Integrator: {meta.get('integrator', 'kick_drift')}")
    print(f"  Multipole: {meta.get('multipole', 'monopole')}")
    print(f"  Pipeline: {'on' if meta.get('pipeline') else 'off'}")
    color = meta.get("color") or {}
    if color.get("mode") == "density":
        rng = color.get("log10_range")
        print(f"  Color: density (k = {color.get('k', DENSITY_K)}, log10 rho range "
              + (f"{rng[0]:.3f} .. {rng[1]:.3f})" if rng else "not taken yet)"))
    else:
        print("  Color: speed")
    print(f"  Progress: {completed}/{total} frames ({completed / total * 100:.1f}%)")
    print(f"  Started: {meta.get('start_datetime', 'unknown')}")
    rows = read_diagnostics(rec_dir / DIAGNOSTICS_FILE)
    if rows:
        de, dp, dl = diagnostics_drift(rows)
        print(f"  Diagnostics: frame {rows[0]['frame']} -> {rows[-1]['frame']} ({len(rows)} lines)")
        print(f"    |E - E0| / |E0|:        {de:.3e}")
        print(f"    |P - P0| / sum m|v|_0:  {dp:.3e}")
        print(f"    |L - L0| / |L0|:        {dl:.3e}")
    g = meta.get("groups")
    if g:
        link = g.get("link", "auto")
        print(f"  Groups: every {g.get('every')} frames, linking length "
              + (f"{link:.6g}" if isinstance(link, (int, float)) else "auto (not taken yet)")
              + f", min members {g.get('min_members', GROUPS_MIN_MEMBERS)}")
        grows = read_diagnostics(rec_dir / GROUPS_FILE)
        if grows:
            last = grows[-1]
            largest = last["groups"][0]["members"] if last["groups"] else 0
            print(f"    frame {last['frame']}: {last['count']} groups of at least {last['min_members']} "
                  f"(of {last['n_groups']}), largest {largest} bodies")
    pk = meta.get("pairs")
    if pk:
        edges = pk.get("edges", "auto")
        print(f"  Pairs: every {pk.get('every')} frames, "
              + (f"{len(edges) - 1} bins from {edges[0]:.6g} to {edges[-1]:.6g}" if isinstance(edges, list)
                 else "edges auto (not taken yet)"))
        prows = read_diagnostics(rec_dir / PAIRS_FILE)
        if prows:
            last = prows[-1]
            within = int(last["below"]) + sum(int(c) for c in last["counts"])
            print(f"    frame {last['frame']}: D2 = "
                  + (f"{last['d2']:.3f} over {last['d2_points']} edges" if last.get("d2") is not None else "n/a")
                  + f", {within:,} pairs within {last['edges'][-1]:.6g}")
    rc = meta.get("rotation_curve")
    if rc:
        radii = rc.get("radii") or [0.0]
        print(f"  Rotation curve: every {rc.get('every')} frames, {len(radii)} radii from {radii[0]:.6g} to {radii[-1]:.6g}")
        rrows = read_diagnostics(rec_dir / ROTATION_FILE)
        if rrows:
            last = rrows[-1]
            k = int(np.argmax(last["v_circ"]))
            print(f"    frame {last['frame']}: peak v_circ = {last['v_circ'][k]:.6g} at R = {last['radii'][k]:.6g}")
    tk = meta.get("timestep_check")
    if tk:
        print(f"  Time-step check: every {tk.get('every')} frames, levels "
              + ", ".join(f"{c:.6g}" for c in tk.get("levels", CHI_LEVELS)))
        trows = read_diagnostics(rec_dir / TIMESTEP_FILE)
        if trows:
            last = trows[-1]
            q = last["chi_quantiles"]
            print(f"    frame {last['frame']}: dt = {last['dt']:.6g}, phase per step median {q['0.5']:.3g}, "
                  f"99 % {q['0.99']:.3g}, max {q['1.0']:.3g}")
            for c, k in zip(last["levels"], last["above"]):
                if c >= CHI_UNSTABLE and k > 0:
                    print(f"    WARNING: {k:,} of {last['bodies']:,} bodies advance more than {c:.6g} rad per step: "
                          f"their orbits are beyond the integrator's stability limit ({CHI_UNSTABLE:g}); reduce dt or raise substeps")
    pf = meta.get("profile")
    if pf:
        edges = pf.get("edges") or [0.0]
        print(f"  Profile: every {pf.get('every')} frames, {len(edges) - 1} shells from {edges[0]:.6g} to {edges[-1]:.6g}, "
              f"{len(pf.get('fractions', PROFILE_FRACTIONS))} Lagrangian radii")
        frows = read_diagnostics(rec_dir / PROFILE_FILE)
        if frows:
            last = frows[-1]
            fr = [abs(f - 0.5) for f in last["fractions"]]
            k = fr.index(min(fr))
            central = next((x for x in last["density"] if x is not None), None)
            half = last["lagrangian_radii"][k]
            print(f"    frame {last['frame']}: r({last['fractions'][k]:.3g} M) = "
                  + (f"{half:.6g}" if half is not None else "n/a") + ", central density = "
                  + (f"{central:.6g}" if central is not None else "n/a"))
    tc = meta.get("tracers")
    if tc:
        try:
            count = f"{len(np.load(tc.get('file'), mmap_mode='r', allow_pickle=False)):,}"
        except (OSError, ValueError, TypeError):
            count = "?"
        every = int(tc.get("every") or 0)
        print(f"  Tracers: {count} from {tc.get('file')}, " + (f"a file every {every} frames" if every else "no files"))
        last = last_tracer_file(rec_dir, completed)
        if last is not None:
            print(f"    last file: {last.name} ({len(np.load(last, mmap_mode='r')):,} rows)")
    dm = meta.get("density_map")
    if dm:
        print(f"  Density maps: every {dm.get('every')} frames, {dm.get('pixels')} x {dm.get('pixels')} pixels along "
              f"{dm.get('axis')}, half width {dm.get('half_width'):.6g}")
        frames = map_frames(rec_dir, completed)
        print(f"    {len(frames)} maps" + (f", the last after frame {frames[-1]}" if frames else ""))
    if completed < total:
        print(f"\n  To resume: python -m tools.record --resume {session_name}")
    else:
        print(f"\n  Complete! Export: python -m tools.export {session_name}")
    return True


def _sessions(root: Path = None):
    base = Path(root or PROJECT_ROOT) / "recordings"
    if not base.is_dir():
        return []
    return [d for d in base.iterdir() if d.is_dir() and (d / "metadata.json").exists()]


def list_recordings(root: Path = None):
    """One line per session with a metadata.json (reference :964-990)."""
    sessions = sorted(_sessions(root), key=lambda d: d.name)
    if not sessions:
        print("[List] No recordings found")
        return
    print(f"\n[List] Found {len(sessions)} recording(s):\n")
    for rec_dir in sessions:
        meta = load_metadata(rec_dir)
        completed, total = get_completed_frames(rec_dir), meta["total_frames"]
        status = "done" if completed >= total else f"{completed / total * 100:.0f}%"
        print(f"  {rec_dir.name:30s} | {meta['num_bodies']:>10,} bodies | {completed:>4}/{total:<4} frames | {status}")
    print()


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(
        prog="python -m tools.record",
        description="Record an N-body preset to recordings/<session>/ on the GPU.",
        epilog="Differences from the reference's recorder: there is no interactive menu (give --preset or "
               "--preset-id); --preset-id indexes this build's preset list (python -m tools.record --presets shows "
               "it); --dt sets dt_per_frame (the reference writes an unused 'dt' key); --presets, --seed, "
               "--device-ic, --diagnostics, --integrator, --multipole, --pipeline, --color, --density-k, --density-range, "
               "--groups, --linking-length, --min-members, --pairs, --pair-edges, --rotation-curve, --curve-radii, --timestep-check, --chi-levels, --profile, --profile-edges, --profile-fractions, --tracers, --tracers-every, "
               "--density-map, --map-pixels, --map-half-width, --map-axis and --root are "
               "additions.")
    ap.add_argument("session", nargs="?", help="session name (for --resume, --status or --extend)")
    ap.add_argument("--resume", action="store_true", help="resume an interrupted recording (default: the most recent)")
    ap.add_argument("--extend", type=int, metavar="FRAMES", help="extend an existing recording by N frames")
    ap.add_argument("--status", action="store_true", help="show a session's progress (all sessions without one)")
    ap.add_argument("--list", action="store_true", help="list all recordings")
    ap.add_argument("--presets", action="store_true", help="list the presets with their --preset-id")
    ap.add_argument("--preset", type=str, help="preset by name (e.g. quick_galaxy)")
    ap.add_argument("--preset-id", type=int, help="preset by index in this build's preset list")
    ap.add_argument("--bodies", "-n", type=str, help="override the number of bodies (100000, 100k, 1.5m)")
    ap.add_argument("--frames", "-f", type=int, help="override the number of frames")
    ap.add_argument("--theta", "-t", type=float, help="override the Barnes-Hut opening angle (0.3-1.5)")
    ap.add_argument("--dt", type=float, help="override dt_per_frame (the time advanced per recorded frame)")
    ap.add_argument("--seed", type=int, help="seed of the initial conditions (stored in metadata.json)")
    ap.add_argument("--device-ic", action="store_true",
                    help="draw the bodies on the GPU (statistically, not bitwise, like the host generator; "
                         "galaxy, collision, cluster, spiral and filament)")
    ap.add_argument("--diagnostics", type=int, metavar="K",
                    help="every K frames append energy, momentum and angular momentum to diagnostics.jsonl "
                         "(stored in metadata.json as diagnostics_every)")
    ap.add_argument("--integrator", choices=("kick_drift", "leapfrog"), default=None,
                    help="kick_drift (default, the reference's scheme) or leapfrog (synchronized kick-drift-kick: second "
                         "order, time-reversible; stored in metadata.json as integrator)")
    ap.add_argument("--multipole", choices=("monopole", "quadrupole"), default=None,
                    help="monopole (default, the reference's cell term) or quadrupole (cells also carry their second "
                         "moments: ~16 x smaller force error at the same theta; stored in metadata.json as multipole)")
    ap.add_argument("--pipeline", action="store_true",
                    help="write frame k - 1 while the device computes frame k (asynchronous frame fetch; the same files; "
                         "stored in metadata.json as pipeline)")
    ap.add_argument("--color", choices=("speed", "density"), default=None,
                    help="speed (default, the reference's ramp over |v| / 15) or density (the same ramp over log10 of the "
                         "k-nearest-neighbour density; stored in metadata.json as color)")
    ap.add_argument("--density-k", type=int, default=None, metavar="K",
                    help=f"neighbours of the density estimate, 1 .. 64 (default {DENSITY_K})")
    ap.add_argument("--density-range", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="log10(rho) at the ends of the ramp (default: taken once from the initial state: its 1st "
                         "percentile .. its 99.9th percentile + 1)")
    ap.add_argument("--groups", type=int, default=None, metavar="K",
                    help="every K frames append the friends-of-friends groups (their number and the 64 largest with "
                         "members, mass, centre, velocity and box) to groups.jsonl (stored in metadata.json as groups)")
    ap.add_argument("--linking-length", type=str, default=None, metavar="B|auto",
                    help="two bodies no further apart than B belong to one group (default auto: taken once from the "
                         "initial state, twice its median nearest-neighbour distance)")
    ap.add_argument("--min-members", type=int, default=None, metavar="M",
                    help=f"smallest group listed (default {GROUPS_MIN_MEMBERS})")
    ap.add_argument("--pairs", type=int, default=None, metavar="K",
                    help="every K frames append the binned pair counts (pairs within the first edge, pairs per bin, the "
                         "correlation dimension) to pairs.jsonl (stored in metadata.json as pairs)")
    ap.add_argument("--pair-edges", type=str, default=None, metavar="auto|e0,e1,...",
                    help="bin edges, 2 .. 65 increasing distances (default auto: taken once from the initial state, 12 "
                         "bins from half to 32 median nearest-neighbour distances, a factor sqrt 2 apart)")
    ap.add_argument("--rotation-curve", type=int, default=None, metavar="K",
                    help="every K frames append the rotation curve about the centre of mass (inward acceleration, circular "
                         "speed and potential per radius, means over 16 azimuths in the plane z = const) to rotation.jsonl "
                         "(stored in metadata.json as rotation_curve)")
    ap.add_argument("--curve-radii", type=str, default=None, metavar="auto|r0,r1,...",
                    help="1 .. 256 increasing radii (default auto: 16 radii, spawn_radius k / 16 for k = 1 .. 16)")
    ap.add_argument("--timestep-check", type=int, default=None, metavar="K",
                    help="every K frames append the orbital phase per step at the bodies (dt sqrt(|T| / sqrt 6) from the "
                         "tidal tensor T: quantiles, and the bodies above each level) to timestep.jsonl (stored in "
                         "metadata.json as timestep_check); --status warns when bodies exceed the stability limit 2")
    ap.add_argument("--chi-levels", type=str, default=None, metavar="c0,c1,...",
                    help="1 .. 16 increasing phase-per-step levels to count bodies above (default 0.1,0.5,2)")
    ap.add_argument("--profile", type=int, default=None, metavar="K",
                    help="every K frames append the radial profile about the centre of mass (bodies, mass, density, mean "
                         "radial velocity, dispersions and anisotropy per shell) and the Lagrangian radii to profile.jsonl "
                         "(stored in metadata.json as profile)")
    ap.add_argument("--profile-edges", type=str, default=None, metavar="auto|e0,e1,...",
                    help="2 .. 257 increasing radii (default auto: 48 log-spaced shells from spawn_radius / 256 to "
                         "4 spawn_radius)")
    ap.add_argument("--profile-fractions", type=str, default=None, metavar="f0,f1,...",
                    help="1 .. 64 mass fractions in (0, 1] for the Lagrangian radii (default 0.1,0.25,0.5,0.75,0.9)")
    ap.add_argument("--tracers", type=Path, default=None, metavar="FILE.npy",
                    help="massless tracers carried by the integrator: an array (m, 3) or (m, 6), rows x y z [vx vy vz] "
                         "(stored in metadata.json as tracers; state checkpoints carry them)")
    ap.add_argument("--tracers-every", type=int, default=None, metavar="K",
                    help="every K frames write the tracers' positions, (m, 3) float32, to tracers_%%06d.npy")
    ap.add_argument("--density-map", type=int, default=None, metavar="K",
                    help="every K frames write the surface density about the origin (mass per area, cloud-in-cell), "
                         "(pixels, pixels) float32, to map_%%06d.npy (stored in metadata.json as density_map)")
    ap.add_argument("--map-pixels", type=int, default=None, metavar="N", help=f"pixels per side (default {MAP_PIXELS})")
    ap.add_argument("--map-half-width", type=float, default=None, metavar="W",
                    help=f"half the side of the map (default {MAP_HALF_WIDTH_FACTOR} x the preset's spawn radius)")
    ap.add_argument("--map-axis", choices=("x", "y", "z"), default=None, help="the axis projected along (default z)")
    ap.add_argument("--root", type=Path, default=None, help="directory holding recordings/ (default: the package's)")
    return ap


def build_config(args) -> dict:
    """Preset + overrides -> the config record() takes; no I/O, no GPU.  ValueError with a printable message."""
    from nbody.gpu_backend import GENERATED_DISTRIBUTIONS
    from tools.presets import get_preset_by_index, get_preset_config
    if args.preset_id is not None:
        key, _ = get_preset_by_index(args.preset_id)
        if key is None:
            raise ValueError(f"Invalid preset index: {args.preset_id}")
        config = get_preset_config(key)
    elif args.preset:
        config = get_preset_config(args.preset)
        if config is None:
            raise ValueError(f"Unknown preset: {args.preset} (python -m tools.record --presets lists them)")
    else:
        raise ValueError("give --preset NAME or --preset-id N (this build has no interactive menu)")
    if args.session:
        config["session_name"] = args.session
    if args.bodies:
        try:
            config["num_bodies"] = parse_number(args.bodies)
        except ValueError:
            raise ValueError(f"Invalid bodies value: {args.bodies}") from None
        if config["num_bodies"] <= 0:
            raise ValueError(f"Invalid bodies value: {args.bodies}")
    if args.frames:
        config["total_frames"] = args.frames
    if args.theta:
        config["theta"] = args.theta
    if args.dt:
        config["dt_per_frame"] = args.dt
    if args.device_ic:
        if config["distribution"] not in GENERATED_DISTRIBUTIONS:
            raise ValueError(f"--device-ic: no device generator for {config['distribution']!r} "
                             f"(have {', '.join(GENERATED_DISTRIBUTIONS)})")
        config["device_ic"] = True
    if args.diagnostics is not None:
        if args.diagnostics <= 0:
            raise ValueError(f"--diagnostics: K must be positive, not {args.diagnostics}")
        config["diagnostics_every"] = int(args.diagnostics)
    if args.integrator is not None and args.integrator != "kick_drift":  # the default writes no key
        config["integrator"] = args.integrator
    if getattr(args, "multipole", None) is not None:  # written only when given
        config["multipole"] = args.multipole
    if getattr(args, "pipeline", False):  # the default writes no key
        config["pipeline"] = True
    color = getattr(args, "color", None)
    dk, dr = getattr(args, "density_k", None), getattr(args, "density_range", None)
    if color != "density" and (dk is not None or dr is not None):
        raise ValueError("--density-k and --density-range need --color density")
    if color == "density":  # the default writes no key
        k = DENSITY_K if dk is None else int(dk)
        if not 1 <= k <= 64 or k > config["num_bodies"] - 1:
            raise ValueError(f"--density-k: K must be in 1 .. min(64, bodies - 1), not {k}")
        config["color"] = {"mode": "density", "k": k}
        if dr is not None:
            config["color"]["log10_range"] = [float(dr[0]), float(dr[1])]
        color_config(config)  # (a bad range raises here)
    gk, gl, gm = (getattr(args, a, None) for a in ("groups", "linking_length", "min_members"))
    if gk is None and (gl is not None or gm is not None):
        raise ValueError("--linking-length and --min-members need --groups K")
    if gk is not None:  # the default writes no key
        link = "auto"
        if gl is not None and gl.strip().lower() != "auto":
            try:
                link = float(gl)
            except ValueError:
                raise ValueError(f"--linking-length: B must be a number or auto, not {gl!r}") from None
        config["groups"] = {"every": int(gk), "link": link, "min_members": GROUPS_MIN_MEMBERS if gm is None else int(gm)}
        groups_config(config)  # (a bad K, B or M raises here)
    pk, pe = (getattr(args, a, None) for a in ("pairs", "pair_edges"))
    if pk is None and pe is not None:
        raise ValueError("--pair-edges needs --pairs K")
    if pk is not None:  # the default writes no key
        edges = "auto"
        if pe is not None and pe.strip().lower() != "auto":
            try:
                edges = [float(x) for x in pe.split(",")]
            except ValueError:
                raise ValueError(f"--pair-edges: need auto or comma-separated numbers, not {pe!r}") from None
        config["pairs"] = {"every": int(pk), "edges": edges}
        pairs_config(config)  # (a bad K or bad edges raise here)
    ck, cr = (getattr(args, a, None) for a in ("rotation_curve", "curve_radii"))
    if ck is None and cr is not None:
        raise ValueError("--curve-radii needs --rotation-curve K")
    if ck is not None:  # the default writes no key
        if cr is None or cr.strip().lower() == "auto":
            radii = [config["spawn_radius"] * k / CURVE_AUTO_RADII for k in range(1, CURVE_AUTO_RADII + 1)]
        else:
            try:
                radii = [float(x) for x in cr.split(",")]
            except ValueError:
                raise ValueError(f"--curve-radii: need auto or comma-separated numbers, not {cr!r}") from None
        config["rotation_curve"] = {"every": int(ck), "radii": radii}
        rotation_config(config)  # (a bad K or bad radii raise here)
    tk, tl = (getattr(args, a, None) for a in ("timestep_check", "chi_levels"))
    if tk is None and tl is not None:
        raise ValueError("--chi-levels needs --timestep-check K")
    if tk is not None:  # the default writes no key
        levels = list(CHI_LEVELS)
        if tl is not None:
            try:
                levels = [float(x) for x in tl.split(",")]
            except ValueError:
                raise ValueError(f"--chi-levels: need comma-separated numbers, not {tl!r}") from None
        config["timestep_check"] = {"every": int(tk), "levels": levels}
        timestep_config(config)  # (a bad K or bad levels raise here)
    fk, fe, ff = (getattr(args, a, None) for a in ("profile", "profile_edges", "profile_fractions"))
    if fk is None and (fe is not None or ff is not None):
        raise ValueError("--profile-edges and --profile-fractions need --profile K")
    if fk is not None:  # the default writes no key
        if fe is None or fe.strip().lower() == "auto":
            from nbody.profile import auto_edges
            edges = [float(x) for x in auto_edges(config["spawn_radius"])]
        else:
            try:
                edges = [float(x) for x in fe.split(",")]
            except ValueError:
                raise ValueError(f"--profile-edges: need auto or comma-separated numbers, not {fe!r}") from None
        fractions = list(PROFILE_FRACTIONS)
        if ff is not None:
            try:
                fractions = [float(x) for x in ff.split(",")]
            except ValueError:
                raise ValueError(f"--profile-fractions: need comma-separated numbers, not {ff!r}") from None
        config["profile"] = {"every": int(fk), "edges": edges, "fractions": fractions}
        profile_config(config)  # (a bad K, bad edges or bad fractions raise here)
    tf, tk = (getattr(args, a, None) for a in ("tracers", "tracers_every"))
    if tf is None and tk is not None:
        raise ValueError("--tracers-every needs --tracers FILE.npy")
    if tf is not None:  # the default writes no key
        if tk is not None and tk <= 0:
            raise ValueError(f"--tracers-every: K must be positive, not {tk}")
        config["tracers"] = {"file": str(Path(tf).resolve()), "every": 0 if tk is None else int(tk)}
        tracers_config(config)
    mk, mp, mw, ma = (getattr(args, a, None) for a in ("density_map", "map_pixels", "map_half_width", "map_axis"))
    if mk is None and (mp is not None or mw is not None or ma is not None):
        raise ValueError("--map-pixels, --map-half-width and --map-axis need --density-map K")
    if mk is not None:  # the default writes no key
        config["density_map"] = {"every": int(mk), "pixels": MAP_PIXELS if mp is None else int(mp),
                                 "half_width": MAP_HALF_WIDTH_FACTOR * config["spawn_radius"] if mw is None else float(mw),
                                 "axis": "z" if ma is None else ma}
        density_map_config(config)  # (a bad K, N, W or axis raises here)
    return config


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    root = args.root
    if args.list:
        list_recordings(root)
        return 0
    if args.presets:
        from tools.presets import get_preset_list
        for idx, (key, p) in enumerate(get_preset_list()):
            print(f"  [{idx:2d}] {key:<24} {p['category']:<13} {p['distribution']:<10} {p['num_bodies']:>11,} bodies "
                  f"| {p['total_frames']:>5} frames")
        return 0
    if args.status:
        if args.session:
            return 0 if show_status(args.session, root) else 1
        list_recordings(root)
        return 0
    if args.extend:
        if not args.session:
            print("[Record] Error: --extend requires a session name")
            return 2
        if not (_session_dir(args.session, root) / "metadata.json").exists():
            print(f"[Record] No recording found: {args.session}")
            return 1
        print(f"[Record] Extending '{args.session}' by {args.extend} frames")
        extend_recording(args.session, args.extend, root=root, quiet=False)
        return 0
    if args.resume:
        session = args.session
        if session is None:
            sessions = sorted(_sessions(root), key=lambda d: d.stat().st_mtime, reverse=True)
            if not sessions:
                print("[Record] No recordings found to resume")
                return 1
            session = sessions[0].name
            print(f"[Record] Resuming most recent: {session}")
        rec_dir = _session_dir(session, root)
        if not (rec_dir / "metadata.json").exists():
            print(f"[Record] No metadata found for session: {session}")
            return 1
        config = load_metadata(rec_dir)
        config["session_name"] = session
        record(config, resume=True, root=root)
        return 0
    try:
        config = build_config(args)
    except ValueError as e:
        print(f"[Record] {e}")
        return 2
    print(f"[Record] Preset {config['name']!r}: {config['num_bodies']:,} bodies ({config['distribution']}), "
          f"{config['total_frames']} frames, theta {config['theta']}, dt_per_frame {config['dt_per_frame']}"
          + (", generated on the device" if config.get("device_ic") else ""))
    record(config, resume=False, root=root, seed=args.seed)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
