"""Flock - the reference's boids object (boids/flock.py:454-782) on the HIP backend.

Same constructor and ``update(dt)``; ``positions`` / ``velocities`` / ``colors`` are (N,3)
float64 arrays like the reference's, fetched from the device lazily (state lives in HBM
between updates).  One ``update`` = assign_cells -> sort -> cell table -> 27-cell sweep ->
physics (reference :627-678) in bdmi_step.  ``draw`` (OpenGL, :730) is out of scope; ``render`` gives the
same frame without GL, rasterised on the device (boids/render.py).
"""
import ctypes as C

import math

import numpy as np

import nbmi_native as _nat
from config import boids as config


NEIGHBOUR_MODES = ("metric", "topological")  # BDMI_NEIGHBOURS_METRIC = 0, BDMI_NEIGHBOURS_TOPOLOGICAL = 1


def rainbow_colors(count: int) -> np.ndarray:
    """Shuffled HSV rainbow, s=0.9 v=1.0, float32 maths (reference _generate_colors :587-608).
    Consumes the global NumPy RNG exactly once (np.random.shuffle)."""
    hues = np.linspace(0, 1, count, endpoint=False, dtype=np.float32)
    np.random.shuffle(hues)
    s, v = 0.9, 1.0
    h6 = hues * 6.0
    sector = h6.astype(np.int32) % 6
    f = h6 - np.floor(h6)
    p = v * (1.0 - s)
    q = v * (1.0 - s * f)
    t = v * (1.0 - s * (1.0 - f))
    vv = np.full_like(q, v)
    pp = np.full_like(q, p)
    table = ((vv, t, pp), (q, vv, pp), (pp, vv, t), (pp, q, vv), (t, pp, vv), (vv, pp, q))
    out = np.zeros((count, 3), dtype=np.float32)
    for k, chans in enumerate(table):
        mask = sector == k
        for c in range(3):
            out[mask, c] = chans[c][mask]
    return out


def generate_initial_state(num_boids: int, bounds: float, max_speed: float):
    """positions U(-b,b)^3, velocities U(-max_speed/2, max_speed/2)^3, rainbow colours - global
    NumPy RNG, call order of reference Flock.__init__ :488-490."""
    pos = ((np.random.rand(num_boids, 3) - 0.5) * 2 * bounds).astype(np.float64)
    vel = ((np.random.rand(num_boids, 3) - 0.5) * max_speed).astype(np.float64)
    col = rainbow_colors(num_boids).astype(np.float64)
    return pos, vel, col


class Flock:
    """Drop-in for reference boids.Flock (:454): ``Flock(num_boids)``, ``update(dt)``.

    ``periodic=True`` (not in the reference) makes the domain the periodic box [-bounds, bounds]^3 of include/bdmi.h:
    no walls, neighbours through the faces by their minimum image, positions wrapped by ``update``."""

    def __init__(self, num_boids: int = 1000, seed=None, device: int = 0, periodic: bool = False):
        self.num_boids = num_boids
        self._periodic = bool(periodic)
        B = config.BOIDS
        self.bounds = np.float64(B["bounds"])
        self.wall_margin = np.float64(B["wall_margin"])
        self.wall_weight = np.float64(B["wall_weight"])
        self.max_speed = np.float64(B["max_speed"])
        self.max_force = np.float64(B["max_force"])
        self.perception_radius = np.float64(B["perception_radius"])
        self.separation_radius = np.float64(B["separation_radius"])
        self.separation_weight = np.float64(B["separation_weight"])
        self.alignment_weight = np.float64(B["alignment_weight"])
        self.cohesion_weight = np.float64(B["cohesion_weight"])
        self.color_blend_rate = np.float64(B["color_blend_rate"])
        # spatial grid exactly as reference :478-481
        self.cell_size = float(self.perception_radius)
        self.grid_dim = int(np.ceil(self.bounds * 2 / self.cell_size)) + 2
        self.num_cells = self.grid_dim ** 3
        self.grid_offset = float(self.bounds + self.cell_size)
        self.fog_end = float(config.CAMERA["far_clip"])
        self.fov_margin = 1.15
        self.cone_length = np.float32(B["size"])          # reference :466-467
        self.cone_radius = np.float32(B["size"] * 0.35)
        self.verts_per_boid = 6
        if seed is not None:  # the reference is unseeded; extra kwarg
            np.random.seed(seed)
        pos, vel, col = generate_initial_state(num_boids, self.bounds, self.max_speed)
        self._visible_count = num_boids
        self._lib = _nat.load()
        params = np.array([float(B[k]) for k in config.PARAM_ORDER], dtype=np.float64)
        create = self._lib.bdmi_create_periodic if self._periodic else self._lib.bdmi_create
        self._h = create(num_boids, _nat.ptr(pos), _nat.ptr(vel), _nat.ptr(col), _nat.ptr(params), int(device))
        if not self._h:
            if _nat.last_error().startswith("bdmi_create_periodic: "):  # the library refused the box, not the device
                raise ValueError(_nat.last_error())
            raise RuntimeError(f"bdmi_create failed: {_nat.last_error()} (this build has no CPU fallback)")
        if self._periodic:  # the periodic grid in the place of the reference's (include/bdmi.h)
            self.grid_dim = self.grid_info()["grid_dim"]
            self.cell_size = self.box["cell_size"]
            self.num_cells = self.grid_dim ** 3
            self.grid_offset = float(self.bounds)
        self._cache = {"positions": pos, "velocities": vel, "colors": col}

    # ---- periodic box and noise (include/bdmi.h) -----------------------------------------------
    @property
    def periodic(self):
        return self._periodic

    @property
    def box(self):
        """dict of ``periodic``, ``length`` (2 * bounds) and ``cell_size`` of the handle's grid."""
        per, length, cell = C.c_int(0), C.c_double(0), C.c_double(0)
        _nat.check_arg(self._lib.bdmi_get_box(self._h, C.addressof(per), C.addressof(length), C.addressof(cell)),
                       "bdmi_get_box")
        return dict(periodic=bool(per.value), length=float(length.value), cell_size=float(cell.value))

    def set_noise(self, eta, seed=0, step=None):
        """Vectorial noise of amplitude ``eta * max_force``: every ``update`` adds ``eta * max_force * xi_i(step)`` to boid
        i's acceleration, xi a unit vector drawn from (seed, step, i) alone.  ``step=None`` keeps the handle's noise step,
        which counts the updates since the flock was made; ``eta=0`` is the step without noise."""
        _nat.check_arg(self._lib.bdmi_set_noise(self._h, float(eta), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                -1 if step is None else int(step)), "bdmi_set_noise")

    @property
    def noise(self):
        """``(eta, seed, step)``."""
        eta, seed, step = C.c_double(0), C.c_uint64(0), C.c_int64(0)
        _nat.check_arg(self._lib.bdmi_get_noise(self._h, C.addressof(eta), C.addressof(seed), C.addressof(step)),
                       "bdmi_get_noise")
        return float(eta.value), int(seed.value), int(step.value)

    def noise_vectors(self, step=None):
        """The unit vectors xi_i(step), float64 (N, 3) (default: the handle's current noise step)."""
        out = np.empty((self.num_boids, 3), dtype=np.float64)
        _nat.check_arg(self._lib.bdmi_noise_vectors(self._h, -1 if step is None else int(step), _nat.ptr(out)),
                       "bdmi_noise_vectors")
        return out

    # ---- state access (reference attributes) ----------------------------------------------
    def _fetch(self):
        if self._cache is None:
            n = self.num_boids
            pos, vel, col = (np.empty((n, 3)) for _ in range(3))
            _nat.check(self._lib.bdmi_get_state(self._h, _nat.ptr(pos), _nat.ptr(vel), _nat.ptr(col)),
                       "bdmi_get_state")
            self._cache = {"positions": pos, "velocities": vel, "colors": col}
        return self._cache

    @property
    def positions(self):
        return self._fetch()["positions"]

    @property
    def velocities(self):
        return self._fetch()["velocities"]

    @property
    def colors(self):
        return self._fetch()["colors"]

    def set_state(self, positions=None, velocities=None, colors=None):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in
                (positions, velocities, colors)]
        for a in arrs:
            if a is not None and a.shape != (self.num_boids, 3):
                raise ValueError("state arrays must be (N,3)")
        check = _nat.check_arg if self._periodic else _nat.check  # a periodic handle refuses positions outside its box
        check(self._lib.bdmi_set_state(self._h, *[_nat.ptr(a) for a in arrs]), "bdmi_set_state")
        self._cache = None

    # ---- the hot path -----------------------------------------------------------------------
    def update(self, dt: float, substeps: int = 1):
        """Flock.update(dt) (reference :627); no dt cap here - callers cap at 0.05."""
        check = _nat.check_arg if self._periodic else _nat.check  # a periodic handle refuses max_speed * |dt| >= its box
        check(self._lib.bdmi_step(self._h, float(np.float64(dt)), int(substeps)), "bdmi_step")
        self._cache = None

    def sync(self):
        _nat.check(self._lib.bdmi_sync(self._h), "bdmi_sync")

    # ---- parity hooks -------------------------------------------------------------------------
    def cell_indices(self) -> np.ndarray:
        out = np.empty(self.num_boids, dtype=np.int32)
        _nat.check(self._lib.bdmi_get_cell_indices(self._h, _nat.ptr(out)), "bdmi_get_cell_indices")
        return out

    def forces(self):
        """(separation, alignment, cohesion, avg_colors) for the current state, no integration."""
        n = self.num_boids
        outs = [np.empty((n, 3)) for _ in range(4)]
        _nat.check(self._lib.bdmi_get_forces(self._h, *[_nat.ptr(a) for a in outs]), "bdmi_get_forces")
        return tuple(outs)

    def grid_info(self):
        dim, cells, occ = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        _nat.check(self._lib.bdmi_grid_info(self._h, C.addressof(dim), C.addressof(cells), C.addressof(occ)),
                   "bdmi_grid_info")
        return dict(grid_dim=int(dim.value), num_cells=int(cells.value), occupied=int(occ.value))

    def enable_timers(self, on=True):
        _nat.check(self._lib.bdmi_enable_timers(self._h, 1 if on else 0), "bdmi_enable_timers")

    def timers(self, reset=False):
        ms = np.zeros(3)
        cnt = C.c_int64(0)
        _nat.check(self._lib.bdmi_get_timers(self._h, _nat.ptr(ms), C.addressof(cnt), 1 if reset else 0),
                   "bdmi_get_timers")
        return dict(sort_ms=ms[0], table_ms=ms[1], sweep_ms=ms[2], steps=int(cnt.value))

    # ---- flock analysis (include/bdmi.h: flock finder, catalogue, order parameters, neighbour statistics) ----
    def _link(self, link):
        return float(self.perception_radius if link is None else link)

    def flocks(self, link=None):
        """The flocks of the current state: boids no further apart than ``link`` (default: the perception radius) are
        linked, a flock is a connected component.  dict of ``labels`` (int32 (N,), the smallest boid index of each
        boid's flock), ``n_flocks``, ``links`` (linked pairs) and ``evals`` (distances evaluated)."""
        labels = np.empty(self.num_boids, dtype=np.int32)
        nf, links, evals = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _nat.check_arg(self._lib.bdmi_flocks(self._h, self._link(link), _nat.ptr(labels), C.addressof(nf),
                                             C.addressof(links), C.addressof(evals)), "bdmi_flocks")
        return dict(labels=labels, n_flocks=int(nf.value), links=int(links.value), evals=int(evals.value))

    def flock_catalogue(self, link=None, min_members=1, capacity=64):
        """The flocks with at least ``min_members`` members, largest first (ties by label): dict of ``count`` (all
        qualifying flocks), ``label``, ``members`` and ``rows`` ((rows, 16) float64, see boids.analysis.row_dict) of
        the first ``capacity`` of them."""
        cap = int(capacity)
        label = np.empty(max(cap, 0), dtype=np.int32)
        members = np.empty(max(cap, 0), dtype=np.int64)
        rows = np.empty((max(cap, 0), 16), dtype=np.float64)
        cnt = C.c_int64(0)
        _nat.check_arg(self._lib.bdmi_flock_catalogue(self._h, self._link(link), int(min_members), cap, _nat.ptr(label),
                                                      _nat.ptr(members), _nat.ptr(rows), C.addressof(cnt)),
                       "bdmi_flock_catalogue")
        k = min(int(cnt.value), cap)
        return dict(count=int(cnt.value), label=label[:k], members=members[:k], rows=rows[:k])

    def diagnostics(self):
        """The row of the whole flock (float64 (16,)): centre, mean velocity, polarisation, mean speed, milling, box."""
        row = np.empty(16, dtype=np.float64)
        _nat.check_arg(self._lib.bdmi_diagnostics(self._h, _nat.ptr(row)), "bdmi_diagnostics")
        return row

    def neighbour_stats(self, radius=None):
        """Per boid: ``count`` of the others within ``radius`` (default: the perception radius) and ``nn_d2``, the
        squared distance of the nearest of them (inf without one); plus ``evals``."""
        count = np.empty(self.num_boids, dtype=np.int32)
        nn = np.empty(self.num_boids, dtype=np.float64)
        evals = C.c_int64(0)
        _nat.check_arg(self._lib.bdmi_neighbour_stats(self._h, self._link(radius), _nat.ptr(count), _nat.ptr(nn),
                                                      C.addressof(evals)), "bdmi_neighbour_stats")
        return dict(count=count, nn_d2=nn, evals=int(evals.value))

    # ---- flock analysis on a periodic flock (include/bdmi.h: links through the faces, a flock's row on the torus) ----
    def periodic_flocks(self, link=None):
        """``flocks`` on a periodic flock: links are followed through the faces of the box.  The same dict."""
        labels = np.empty(self.num_boids, dtype=np.int32)
        nf, links, evals = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _nat.check_arg(self._lib.bdmi_periodic_flocks(self._h, self._link(link), _nat.ptr(labels), C.addressof(nf),
                                                      C.addressof(links), C.addressof(evals)), "bdmi_periodic_flocks")
        return dict(labels=labels, n_flocks=int(nf.value), links=int(links.value), evals=int(evals.value))

    def periodic_flock_catalogue(self, link=None, min_members=1, capacity=64):
        """``flock_catalogue`` on a periodic flock.  A flock that straddles a face is unwrapped before its row is taken:
        its centre lies inside the flock (brought back into the box), ``hi`` may exceed the bounds and ``hi - lo`` is its
        extent.  The dict of ``flock_catalogue`` plus ``wrap`` (int32 (rows, 3): per axis the cell coordinate the flock
        was cut at, -1 where it occupies every slab of the axis) and ``spans`` (bool (rows, 3): ``wrap == -1``; a flock
        that reaches around the box spans, and so does one that merely has a member in every slab)."""
        cap = int(capacity)
        label = np.empty(max(cap, 0), dtype=np.int32)
        members = np.empty(max(cap, 0), dtype=np.int64)
        rows = np.empty((max(cap, 0), 16), dtype=np.float64)
        wrap = np.empty((max(cap, 0), 3), dtype=np.int32)
        cnt = C.c_int64(0)
        _nat.check_arg(self._lib.bdmi_periodic_flock_catalogue(self._h, self._link(link), int(min_members), cap,
                                                               _nat.ptr(label), _nat.ptr(members), _nat.ptr(rows),
                                                               _nat.ptr(wrap), C.addressof(cnt)),
                       "bdmi_periodic_flock_catalogue")
        k = min(int(cnt.value), cap)
        return dict(count=int(cnt.value), label=label[:k], members=members[:k], rows=rows[:k], wrap=wrap[:k],
                    spans=wrap[:k] == -1)

    def periodic_neighbour_stats(self, radius=None):
        """``neighbour_stats`` on a periodic flock: the others within ``radius`` through the faces.  The same dict."""
        count = np.empty(self.num_boids, dtype=np.int32)
        nn = np.empty(self.num_boids, dtype=np.float64)
        evals = C.c_int64(0)
        _nat.check_arg(self._lib.bdmi_periodic_neighbour_stats(self._h, self._link(radius), _nat.ptr(count), _nat.ptr(nn),
                                                               C.addressof(evals)), "bdmi_periodic_neighbour_stats")
        return dict(count=count, nn_d2=nn, evals=int(evals.value))

    # ---- velocity correlation beyond sight (include/bdmi.h: bdmi_velocity_correlation), walled or periodic ----
    def heading_moments(self, mean=(0.0, 0.0, 0.0)):
        """The exact integer moments of the quantised heading fluctuations q_i = rint((u_i - mean) 2^24): dict of
        ``qsum`` (3 ints) and ``qsq`` (int, the sum of |q_i|^2).  No grid is built."""
        mean = np.ascontiguousarray(mean, dtype=np.float64).reshape(3)
        self5 = np.zeros(5, dtype=np.int64)
        _nat.check_arg(self._lib.bdmi_velocity_correlation(self._h, 0, None, _nat.ptr(mean), None, None, _nat.ptr(self5),
                                                           None), "bdmi_velocity_correlation")
        return dict(qsum=[int(x) for x in self5[:3]], qsq=(int(self5[3]) << 32) + int(self5[4]))

    def velocity_correlation(self, edges, mean=None):
        """The connected correlation of the headings by distance: for the bins ``edges`` (increasing, at most 65 of them,
        the last one at most 16 cells, and on a periodic flock below half the box) the exact number of pairs per bin and
        the exact sum of q_i . q_j over them, q the heading fluctuation about ``mean`` in units of 2^-24 (default: the
        mean heading).  Slot 0 is "below the first edge".  dict of ``edges``, ``pairs`` (int64 (nb+1,)), ``dot`` (Python
        ints), ``mean``, ``quantum``, ``reach`` (cells), ``evals``, ``qsum``, ``qsq`` and ``n``; boids.analysis turns it into
        C(r), the correlation length and the susceptibility."""
        edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        nb = len(edges) - 1
        if nb < 1:
            raise ValueError("velocity_correlation: at least two edges (one bin)")
        n = self.num_boids
        if mean is None:
            s = self.heading_moments()["qsum"]
            mean = [x / (n * 2.0 ** 24) if n else 0.0 for x in s]
        mean = np.ascontiguousarray(mean, dtype=np.float64).reshape(3)
        pairs = np.zeros(nb + 1, dtype=np.int64)
        dot = np.zeros((nb + 1, 2), dtype=np.int64)
        self5 = np.zeros(5, dtype=np.int64)
        evals = C.c_int64(0)
        _nat.check_arg(self._lib.bdmi_velocity_correlation(self._h, nb, _nat.ptr(edges), _nat.ptr(mean), _nat.ptr(pairs),
                                                           _nat.ptr(dot), _nat.ptr(self5), C.addressof(evals)),
                       "bdmi_velocity_correlation")
        return dict(edges=edges, pairs=pairs, dot=[(int(h) << 32) + int(l) for h, l in dot], mean=mean.tolist(),
                    quantum=2.0 ** -24, reach=int(math.ceil(float(edges[-1]) / self.box["cell_size"])), evals=int(evals.value),
                    qsum=[int(x) for x in self5[:3]], qsq=(int(self5[3]) << 32) + int(self5[4]), n=n)

    # ---- topological interaction (include/bdmi.h: the k nearest neighbours within sight) ---------------------
    def set_neighbour_mode(self, mode, k=7):
        """``"metric"`` (the default: every boid within the perception radius counts, the reference's rule) or
        ``"topological"``: each boid interacts with its ``k`` nearest neighbours within the perception radius
        (1 <= k <= 16).  ``update`` and ``forces`` follow the mode; ``k`` is ignored for ``"metric"``."""
        if mode not in NEIGHBOUR_MODES:
            raise ValueError(f"set_neighbour_mode: mode must be one of {NEIGHBOUR_MODES}, got {mode!r}")
        _nat.check_arg(self._lib.bdmi_set_neighbour_mode(self._h, NEIGHBOUR_MODES.index(mode), int(k)),
                       "bdmi_set_neighbour_mode")

    @property
    def neighbour_mode(self):
        """``(name, k)`` of the handle's interaction rule."""
        mode, k = C.c_int(0), C.c_int(0)
        _nat.check_arg(self._lib.bdmi_get_neighbour_mode(self._h, C.addressof(mode), C.addressof(k)),
                       "bdmi_get_neighbour_mode")
        return NEIGHBOUR_MODES[int(mode.value)], int(k.value)

    def topological_neighbours(self, k=None):
        """Per boid its ``k`` nearest neighbours within the perception radius (default: the handle's k), nearest
        first, ties by boid index: dict of ``ids`` (int32 (N, k), padded with -1), ``d2`` (float64 (N, k), squared
        distances, padded with inf) and ``count`` (int32 (N,)).  Works in either mode."""
        k = self.neighbour_mode[1] if k is None else int(k)
        rows = max(k, 0)
        ids = np.empty((self.num_boids, rows), dtype=np.int32)
        d2 = np.empty((self.num_boids, rows), dtype=np.float64)
        count = np.zeros(self.num_boids, dtype=np.int32)
        _nat.check_arg(self._lib.bdmi_topological_neighbours(self._h, k, _nat.ptr(ids), _nat.ptr(d2), _nat.ptr(count)),
                       "bdmi_topological_neighbours")
        return dict(ids=ids, d2=d2, count=count)

    # ---- render-side reduction (reference :680-728) on the device -----------------------------
    def frustum_tangents(self, fov=None, aspect=None):
        """(tan_h, tan_v) of the visibility test for a vertical field of view in degrees (reference :737-739 and
        _compute_visibility: the half angles widened by fov_margin)."""
        fov_rad = math.radians(fov) if fov else math.radians(75)
        aspect = aspect if aspect else (16 / 9)
        half_fov_v = (fov_rad / 2) * self.fov_margin
        half_fov_h = math.atan(math.tan(half_fov_v) * aspect)
        return math.tan(half_fov_h), math.tan(half_fov_v)

    def visible_vertices(self, cam_pos=None, cam_forward=None, cam_right=None, cam_up=None, fov=None, aspect=None):
        """What draw() (reference :730-756) hands to its VBOs: (vertices, vert_colors) float32,
        6 rows per visible boid in ascending boid order; sets _visible_count.  Frustum test
        (compute_visibility_numba), compaction and cone building (build_vertices_numba) run on
        the GPU, only the visible part is copied back."""
        n = self.num_boids
        if cam_pos is None:  # reference: everything visible
            cam = np.array([0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0], dtype=np.float64)
            cam[0:3] = (0.0, 0.0, -1e300)
            tan_h = tan_v = float("inf")
            fog = float("inf")
        else:
            tan_h, tan_v = self.frustum_tangents(fov, aspect)
            fog = self.fog_end
            cam = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).reshape(3) for a in
                                                       (cam_pos, cam_forward, cam_right, cam_up)]))
        if getattr(self, "_vertices", None) is None:
            self._vertices = np.zeros((n * 6, 3), dtype=np.float32)
            self._vert_colors = np.zeros((n * 6, 3), dtype=np.float32)
        cnt = C.c_int64(0)
        _nat.check(self._lib.bdmi_visible_vertices(self._h, _nat.ptr(cam), tan_h, tan_v, fog, float(self.cone_length),
                                                   float(self.cone_radius), _nat.ptr(self._vertices),
                                                   _nat.ptr(self._vert_colors), n, C.addressof(cnt)),
                   "bdmi_visible_vertices")
        self._visible_count = int(cnt.value)
        k = self._visible_count * self.verts_per_boid
        return self._vertices[:k], self._vert_colors[:k]

    def render(self, renderer, camera, out=None, **shading):
        """The frame draw() would put on the screen, rasterised on the device by a boids.render.HIPFlockRenderer
        through a boids.render.OrbitCamera; sets _visible_count.  Returns uint8 (H, W, 3)."""
        return renderer.render_flock(self, camera, out=out, **shading)

    def draw(self, *args, **kwargs):
        raise NotImplementedError("OpenGL rendering (reference boids/flock.py:730) is out of scope of this build; "
                                  "visible_vertices() returns what draw() would upload")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bdmi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
