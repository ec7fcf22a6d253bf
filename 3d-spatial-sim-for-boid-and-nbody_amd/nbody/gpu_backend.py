"""Backend seam of the N-body simulation - MI355X / HIP edition.

Mirrors the reference's nbody/gpu_backend.py: the ``Backend`` enum (:29-33) gains a ``HIP``
member that ``detect_backend`` (:36-55) tries first; ``get_backend`` / ``force_backend``
(:119-132) keep their cached-global behaviour; ``create_gpu_simulation`` (:623-679) returns an
object speaking the reference's backend protocol

    step(dt) / compute_colors(max_speed) / get_positions() -> (N,3) f32 /
    get_velocities() -> (N,3) f64 / get_colors() -> (N,3) f32 / sync()

(reference class CUDASimulation, :336-409) or ``None`` when no HIP device exists - the
reference's own "fall back" convention.  This package has no CPU path to fall back to, so its
callers (NBodySimulation, record) raise on ``None``.
"""
import ctypes as C
import os
from dataclasses import dataclass
from enum import Enum
from typing import Optional, Tuple

import numpy as np

import nbmi_native as _nat

METHOD_BARNES_HUT = 0
METHOD_DIRECT = 1

# distributions nbmi_create_generated draws on the device (NBMI_IC_* of include/nbmi.h)
GENERATED_DISTRIBUTIONS = {"galaxy": 0, "collision": 1, "cluster": 2, "spiral": 3, "filament": 4}
# integrators of nbmi_set_integrator (NBMI_INTEGRATOR_* of include/nbmi.h)
INTEGRATORS = {"kick_drift": 0, "leapfrog": 1}
# multipole orders of nbmi_set_multipole (NBMI_MULTIPOLE_* of include/nbmi.h)
MULTIPOLES = {"monopole": 0, "quadrupole": 1}
# colour modes of nbmi_set_color_mode (NBMI_COLOR_* of include/nbmi.h)
COLOR_MODES = {"speed": 0, "density": 1}
DEPOSIT_SCHEMES = {"ngp": 0, "cic": 1}  # NBMI_DEPOSIT_*
DEPOSIT_QUANTITIES = {"number": 1, "mass": 2, "momentum": 4, "kinetic": 8}  # in the order of the planes
# planes of nbmi_radial_profile (NBMI_PROFILE_*), in the order of the planes; "angular_momentum" has three
PROFILE_QUANTITIES = {"number": 1, "mass": 2, "radial_momentum": 4, "radial_kinetic": 8, "kinetic": 16,
                      "angular_momentum": 32}
KNN_MAX_K = 64


def _multipole_code(name):
    if name not in MULTIPOLES:
        raise ValueError(f"multipole must be one of {sorted(MULTIPOLES)}, not {name!r}")
    return MULTIPOLES[name]


def _integrator_code(name):
    if name not in INTEGRATORS:
        raise ValueError(f"integrator must be one of {sorted(INTEGRATORS)}, not {name!r}")
    return INTEGRATORS[name]


class Backend(Enum):
    HIP = "hip"                    # MI355X: Barnes-Hut (default) or direct N^2 in hand-written HIP
    CUDA = "cuda"                  # reference members kept so `Backend.X` comparisons still work
    METAL_BH = "metal_barnes_hut"
    METAL = "metal"
    CPU = "cpu"


def _check_hip() -> Tuple[bool, str]:
    try:
        n = _nat.device_count()
    except (ImportError, OSError, AttributeError) as e:  # library missing / stale
        return False, f"libnbmi.so unavailable: {e}"
    if n > 0:
        return True, f"{n} HIP device(s), gfx950 kernels (libnbmi.so)"
    return False, "no HIP device"


def detect_backend() -> Tuple[Backend, str]:
    ok, info = _check_hip()
    if ok:
        return Backend.HIP, info
    return Backend.CPU, info


_BACKEND: Optional[Backend] = None
_BACKEND_INFO: str = ""


def get_backend() -> Tuple[Backend, str]:
    """Current backend, detected once and cached (reference :119-125)."""
    global _BACKEND, _BACKEND_INFO
    if _BACKEND is None:
        _BACKEND, _BACKEND_INFO = detect_backend()
        print(f"[GPU] Using backend: {_BACKEND.value} - {_BACKEND_INFO}")
    return _BACKEND, _BACKEND_INFO


def force_backend(backend: Backend):
    """Pin the backend (reference :128-132)."""
    global _BACKEND, _BACKEND_INFO
    _BACKEND = backend
    _BACKEND_INFO = f"Forced: {backend.value}"


def _default_device():
    """the device of this process's local rank (torchrun's LOCAL_RANK), modulo the devices present"""
    return int(os.environ.get("LOCAL_RANK", "0")) % max(1, _nat.device_count())


def _as_f64(a, shape_tail):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape[1:] != shape_tail:
        raise ValueError(f"expected array of shape (N,{','.join(map(str, shape_tail))}), got {a.shape}")
    return a


# What deposit() and radial_profile() share: the named quantities of a fixed-point sum over the state
def _sum_names(what, quantities, table):
    """The chosen names of ``table`` (name -> bit) in the library's plane order; ValueError for none or an unknown one."""
    if isinstance(quantities, str):
        quantities = (quantities,)
    unknown = [q for q in quantities if q not in table]
    if unknown or not quantities:
        raise ValueError(f"{what}: quantities must be some of {list(table)}, not {list(quantities)}")
    return [q for q in table if q in quantities]


def _sum_planes(names, table, vector, shape, stats, extra, call):
    """Allocates one float64 plane of ``shape`` per name (three for ``vector``), runs ``call(bits, out, st, ex)`` on their
    pointers and returns the result dict: a plane per name, ``extra``, "exponents" and, with ``stats``, "stats"."""
    width = {q: 3 if q == vector else 1 for q in names}
    planes = sum(width.values())
    out = np.zeros((planes,) + tuple(shape), dtype=np.float64)
    st = np.zeros(3, dtype=np.int64)
    ex = np.zeros(planes, dtype=np.int32)
    call(sum(table[q] for q in names), _nat.ptr(out), _nat.ptr(st), _nat.ptr(ex))
    res, p = {}, 0
    for q in names:
        res[q] = out[p:p + 3] if q == vector else out[p]
        p += width[q]
    res.update(extra, exponents=ex)
    if stats:
        res["stats"] = tuple(int(x) for x in st)
    return res


@dataclass(frozen=True)
class Diagnostics:
    """Conserved quantities of a handle's current float64 state (include/nbmi.h, nbmi_diagnostics).
    ``potential`` (W) and ``total`` (E = K + W) are None when the potential was not asked for; ``terms`` is the number
    of (body, node) terms applied to it (0 then)."""
    mass: float
    center_of_mass: Tuple[float, float, float]
    momentum: Tuple[float, float, float]
    angular_momentum: Tuple[float, float, float]
    kinetic: float
    potential: Optional[float]
    total: Optional[float]
    terms: int


class _HIPSimulation:
    """Shared implementation of the backend protocol on top of the nbmi_* C ABI."""

    _method = METHOD_BARNES_HUT

    def __init__(self, positions, velocities, masses, G, softening, damping, theta=0.5, device=None,
                 integrator="kick_drift", multipole="monopole"):
        _integrator_code(integrator)
        _multipole_code(multipole)
        lib = _nat.load()
        pos = _as_f64(positions, (3,))
        vel = _as_f64(velocities, (3,))
        m = _as_f64(masses, ())
        if not (len(pos) == len(vel) == len(m)):
            raise ValueError("positions, velocities and masses must have the same length")
        if device is None:
            device = _default_device()
        self.n = len(pos)
        self.G, self.softening, self.damping, self.theta = float(G), float(softening), float(damping), float(theta)
        self.device = int(device)
        self._lib = lib
        self._h = lib.nbmi_create(self.n, _nat.ptr(pos), _nat.ptr(vel), _nat.ptr(m), self.G, self.softening,
                                  self.damping, self.theta, self._method, self.device)
        if not self._h:
            raise RuntimeError(f"nbmi_create failed: {_nat.last_error()}")
        kind = "Barnes-Hut" if self._method == METHOD_BARNES_HUT else "direct N^2"
        print(f"[HIP] Initialized with {self.n:,} bodies ({kind}) on device {self.device}")
        self._apply_options(integrator, multipole)

    @classmethod
    def generated(cls, distribution, n, spawn_radius, G, softening, damping, theta=0.5, seed=42, device=None,
                  integrator="kick_drift", multipole="monopole"):
        """Same backend object, but the bodies are drawn ON THE DEVICE from the reference's
        generate_distribution formulas (tools/presets.py:104-295, :350-397, :609-684; `distribution`
        one of GENERATED_DISTRIBUTIONS) with a Philox stream keyed by `seed`: statistical parity
        with the NumPy generator, per-body parity (to the bound recorded in DESIGN.md) with the host replay
        in tests/icgen_ref.py; no host arrays, no upload."""
        kinds = GENERATED_DISTRIBUTIONS
        _integrator_code(integrator)
        _multipole_code(multipole)
        if distribution not in kinds:
            raise ValueError(f"device-side generator has {sorted(kinds)}, not {distribution!r}")
        self = cls.__new__(cls)
        lib = _nat.load()
        if device is None:
            device = _default_device()
        self.n = int(n)
        self.G, self.softening, self.damping, self.theta = float(G), float(softening), float(damping), float(theta)
        self.device = int(device)
        self._lib = lib
        self._h = lib.nbmi_create_generated(kinds[distribution], self.n, float(spawn_radius), int(seed) & (2 ** 64 - 1),
                                            self.G, self.softening, self.damping, self.theta, cls._method, self.device)
        if not self._h:
            raise RuntimeError(f"nbmi_create_generated failed: {_nat.last_error()}")
        print(f"[HIP] Generated {self.n:,} bodies ({distribution}, seed {seed}) on device {self.device}")
        self._apply_options(integrator, multipole)
        return self

    def _apply_options(self, integrator, multipole):
        """Constructor options that the library may refuse for this handle: a refusal closes the handle before it raises."""
        try:
            if integrator != "kick_drift":
                self.set_integrator(integrator)
            if multipole != "monopole":
                self.set_multipole(multipole)
        except Exception:
            self.close()
            raise

    def get_masses(self) -> np.ndarray:
        out = np.empty(self.n, dtype=np.float64)
        _nat.check(self._lib.nbmi_get_masses_f64(self._h, _nat.ptr(out)), "nbmi_get_masses_f64")
        return out

    # ---- reference protocol -------------------------------------------------------------
    def step(self, dt: float):
        _nat.check(self._lib.nbmi_step(self._h, float(dt), 1), "nbmi_step")

    def compute_colors(self, max_speed: float):
        _nat.check(self._lib.nbmi_compute_colors(self._h, float(max_speed)), "nbmi_compute_colors")

    def get_positions(self) -> np.ndarray:
        out = np.empty((self.n, 3), dtype=np.float32)
        _nat.check(self._lib.nbmi_get_positions_f32(self._h, _nat.ptr(out)), "nbmi_get_positions_f32")
        return out

    def get_velocities(self) -> np.ndarray:
        out = np.empty((self.n, 3), dtype=np.float64)
        _nat.check(self._lib.nbmi_get_velocities_f64(self._h, _nat.ptr(out)), "nbmi_get_velocities_f64")
        return out

    def get_colors(self) -> np.ndarray:
        out = np.empty((self.n, 3), dtype=np.float32)
        _nat.check(self._lib.nbmi_get_colors_f32(self._h, _nat.ptr(out)), "nbmi_get_colors_f32")
        return out

    def sync(self):
        _nat.check(self._lib.nbmi_sync(self._h), "nbmi_sync")

    # ---- supersets ----------------------------------------------------------------------
    def step_many(self, dt: float, substeps: int):
        """`substeps` steps enqueued back to back without host round trips."""
        _nat.check(self._lib.nbmi_step(self._h, float(dt), int(substeps)), "nbmi_step")

    def set_integrator(self, integrator: str):
        """"kick_drift" (default, the reference's scheme) or "leapfrog" (synchronized kick-drift-kick: second order,
        time-reversible, positions and velocities at the same instant; include/nbmi.h nbmi_set_integrator).  Owner-mode
        and sharded handles refuse leapfrog with ValueError."""
        code = _integrator_code(integrator)
        _nat.check_arg(self._lib.nbmi_set_integrator(self._h, code), f"set_integrator({integrator!r})", "nbmi_set_integrator")

    @property
    def integrator(self) -> str:
        out = C.c_int(0)
        _nat.check(self._lib.nbmi_get_integrator(self._h, C.addressof(out)), "nbmi_get_integrator")
        return {v: k for k, v in INTEGRATORS.items()}[out.value]

    def set_multipole(self, multipole: str):
        """"monopole" (default, the reference's term) or "quadrupole": an applied cell term also carries the cell's
        second moments; the accepted (body, node) sets do not change (include/nbmi.h nbmi_set_multipole).  Direct,
        owner-mode and sharded handles refuse quadrupole with ValueError."""
        code = _multipole_code(multipole)
        _nat.check_arg(self._lib.nbmi_set_multipole(self._h, code), f"set_multipole({multipole!r})", "nbmi_set_multipole")

    @property
    def multipole(self) -> str:
        out = C.c_int(0)
        _nat.check(self._lib.nbmi_get_multipole(self._h, C.addressof(out)), "nbmi_get_multipole")
        return {v: k for k, v in MULTIPOLES.items()}[out.value]

    def step_count(self) -> int:
        """Steps the device has been asked to take since the handle was created (counted by the library)."""
        return int(self._lib.nbmi_step_count(self._h))

    def get_positions_f64(self) -> np.ndarray:
        out = np.empty((self.n, 3), dtype=np.float64)
        _nat.check(self._lib.nbmi_get_positions_f64(self._h, _nat.ptr(out)), "nbmi_get_positions_f64")
        return out

    def set_state(self, positions, velocities):
        pos = _as_f64(positions, (3,))
        vel = _as_f64(velocities, (3,))
        if len(pos) != self.n or len(vel) != self.n:
            raise ValueError("state arrays must have N rows")
        _nat.check(self._lib.nbmi_set_state(self._h, _nat.ptr(pos), _nat.ptr(vel)), "nbmi_set_state")

    def accelerations(self) -> np.ndarray:
        """Accelerations of the current positions (force pass only, no integration)."""
        out = np.empty((self.n, 3), dtype=np.float64)
        _nat.check(self._lib.nbmi_get_accelerations_f64(self._h, _nat.ptr(out)), "nbmi_get_accelerations_f64")
        return out

    def diagnostics(self, potential=True) -> Diagnostics:
        """Mass, centre of mass, momentum, angular momentum (about the origin), kinetic and - with ``potential`` -
        potential and total energy of the current state, computed on the device in float64 (deterministic: the same
        state gives the same bits).  Barnes-Hut handles: the tree potential over the force walk's own accepted terms;
        direct handles: the exact pair sum.  The call does not change what the next step computes."""
        out = np.empty(12, dtype=np.float64)
        terms = C.c_int64(0)
        _nat.check(self._lib.nbmi_diagnostics(self._h, 1 if potential else 0, _nat.ptr(out), C.addressof(terms)),
                   "nbmi_diagnostics")
        w = float(out[11]) if potential else None
        k = float(out[10])
        return Diagnostics(mass=float(out[0]), center_of_mass=tuple(float(x) for x in out[1:4]),
                           momentum=tuple(float(x) for x in out[4:7]), angular_momentum=tuple(float(x) for x in out[7:10]),
                           kinetic=k, potential=w, total=(k + w) if potential else None, terms=int(terms.value))

    def potentials(self) -> np.ndarray:
        """phi (N,) float64 per unit mass, G included, in the caller's body order (see diagnostics())."""
        out = np.empty(self.n, dtype=np.float64)
        _nat.check(self._lib.nbmi_get_potentials_f64(self._h, _nat.ptr(out)), "nbmi_get_potentials_f64")
        return out

    # ---- the field at arbitrary points (include/nbmi.h nbmi_field_at) ----
    _field_refusal = None  # as _query_refusal below: the owner-mode class refuses before calling the library

    def field_at(self, points, potential=True, terms=False):
        """The gravitational field of the current float64 state at the (m, 3) ``points`` (any array-like): acc (m, 3)
        float64, or (acc, phi) with ``potential``, or (acc, phi, terms) with ``terms`` (phi None without ``potential``)
        - phi (m,) per unit mass, G included, terms (m,) int32 the nodes (direct handles: bodies) applied per point.
        Barnes-Hut handles walk the tree of the current positions as a body at the point would, direct handles sum
        over all bodies; a point's row does not depend on the other points.  ValueError for a wrong shape (before the
        library is called), for a coordinate that is not finite or beyond 1e18, and for owner-mode and sharded handles.
        The call does not change what the next step computes."""
        what = "field_at"
        if self._field_refusal:
            raise ValueError(f"{what}: {self._field_refusal}")
        p = np.ascontiguousarray(points, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError(f"{what}: expected points of shape (m, 3), got {p.shape}")
        m = len(p)
        acc = np.zeros((m, 3), dtype=np.float64)
        phi = np.zeros(m, dtype=np.float64) if potential else None
        cnt = np.zeros(m, dtype=np.int32) if terms else None
        _nat.check_arg(self._lib.nbmi_field_at(self._h, m, _nat.ptr(p), _nat.ptr(acc), _nat.ptr(phi), _nat.ptr(cnt)),
                       what, "nbmi_field_at")
        if terms:
            return acc, phi, cnt
        return (acc, phi) if potential else acc

    # ---- the tidal tensor at points and at the bodies (include/nbmi.h nbmi_tidal_at) ----
    def tidal_at(self, points, terms=False):
        """The tidal tensor T_ab = da_a/dx_b of the current float64 state at the (m, 3) ``points``: (m, 6) float64 rows
        {Txx, Tyy, Tzz, Txy, Txz, Tyz}, or (rows, terms) with ``terms`` - (m,) int32, the number ``field_at`` gives for
        the same point.  nbody/field.py turns the rows into matrices, eigenvalues, norms and time-step measures.
        Refusals as ``field_at``'s; the call does not change what the next step computes."""
        what = "tidal_at"
        if self._field_refusal:
            raise ValueError(f"{what}: {self._field_refusal}")
        p = np.ascontiguousarray(points, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError(f"{what}: expected points of shape (m, 3), got {p.shape}")
        m = len(p)
        t6 = np.zeros((m, 6), dtype=np.float64)
        cnt = np.zeros(m, dtype=np.int32) if terms else None
        _nat.check_arg(self._lib.nbmi_tidal_at(self._h, m, _nat.ptr(p), _nat.ptr(t6), _nat.ptr(cnt)), what, "nbmi_tidal_at")
        return (t6, cnt) if terms else t6

    def _tidal_bodies(self, what, rows, norm):
        if self._field_refusal:
            raise ValueError(f"{what}: {self._field_refusal}")
        t6 = np.zeros((self.n, 6), dtype=np.float64) if rows else None
        nrm = np.zeros(self.n, dtype=np.float64) if norm else None
        _nat.check_arg(self._lib.nbmi_get_tidal_f64(self._h, _nat.ptr(t6), _nat.ptr(nrm)), what, "nbmi_get_tidal_f64")
        return t6, nrm

    def tidal(self, norm=False):
        """The tidal tensor at every body's own position, (N, 6) float64 in the caller's body order - ``tidal_at`` of
        ``get_positions_f64()`` bit for bit, without the upload - or (rows, norm) with ``norm``: (N,) Frobenius norms."""
        t6, nrm = self._tidal_bodies("tidal", True, norm)
        return (t6, nrm) if norm else t6

    def tidal_norm(self) -> np.ndarray:
        """(N,) float64: the Frobenius norm of every body's tidal tensor (``tidal(norm=True)[1]``, the rows not copied)."""
        return self._tidal_bodies("tidal_norm", False, True)[1]

    # ---- massless tracers carried by the integrator (include/nbmi.h nbmi_set_tracers) ----
    def set_tracers(self, positions, velocities=None):
        """Replace the handle's tracers by the (m, 3) ``positions`` with ``velocities`` (None: at rest): test particles
        that every later step moves in the bodies' field - nbmi_field_at's acceleration, the handle's integrator, all
        float64 - and that pull on nothing.  m == 0 removes them.  ValueError for a wrong shape (before the library is
        called), for a value that is not finite or a coordinate beyond 1e18, and for owner-mode and sharded handles."""
        what = "set_tracers"
        if self._field_refusal:
            raise ValueError(f"{what}: {self._field_refusal}")
        p = np.ascontiguousarray(positions, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError(f"{what}: expected positions of shape (m, 3), got {p.shape}")
        v = None
        if velocities is not None:
            v = np.ascontiguousarray(velocities, dtype=np.float64)
            if v.shape != p.shape:
                raise ValueError(f"{what}: expected velocities of shape {p.shape}, got {v.shape}")
        _nat.check_arg(self._lib.nbmi_set_tracers(self._h, len(p), _nat.ptr(p), _nat.ptr(v)), what, "nbmi_set_tracers")

    @property
    def tracer_count(self) -> int:
        return int(self._lib.nbmi_tracer_count(self._h))

    def get_tracers(self):
        """(positions, velocities), (m, 3) float64 each, rows in the order of set_tracers."""
        m = self.tracer_count
        p, v = np.empty((m, 3), dtype=np.float64), np.empty((m, 3), dtype=np.float64)
        _nat.check(self._lib.nbmi_get_tracers_f64(self._h, _nat.ptr(p), _nat.ptr(v)), "nbmi_get_tracers_f64")
        return p, v

    def tracer_positions_f32(self) -> np.ndarray:
        out = np.empty((self.tracer_count, 3), dtype=np.float32)
        _nat.check(self._lib.nbmi_get_tracer_positions_f32(self._h, _nat.ptr(out)), "nbmi_get_tracer_positions_f32")
        return out

    # ---- k-nearest neighbours, densities, density colours (include/nbmi.h nbmi_knn) ----
    _query_refusal = None # classes whose handles the library refuses say so here, and refuse before calling it

    def _query_call(self, what, rc):
        _nat.check_arg(rc, what)  # ValueError: refused for this handle, or a bad argument

    def _query_refuse(self, what, tree=True):
        """``tree=False``: a call that needs the whole state but no tree (direct handles pass; owner mode does not)."""
        why = self._query_refusal if tree else self._field_refusal
        if why:
            raise ValueError(f"{what}: {why}")

    # ---- fields on a regular grid (include/nbmi.h nbmi_deposit; helpers in nbody/grid.py) ----
    def deposit(self, lo, hi, dims, scheme="cic", quantities=("mass",), stats=False):
        """Deposit the current float64 state on a grid of ``dims`` = (nx, ny, nz) cells covering [lo, hi) per axis
        (a dims of 1 projects along that axis).  ``scheme``: "ngp" or "cic"; ``quantities``: any of "number", "mass",
        "momentum", "kinetic" (q = 1, m, m v, m |v|^2).  Returns a dict with one float64 array of shape (nz, ny, nx) per
        quantity - "momentum": (3, nz, ny, nx) -, "exponents" (int32, one per plane in the library's order: every value
        of a plane is an integer multiple of 2 ** exponent) and, with ``stats``, "stats" = (bodies deposited,
        contributions, bodies skipped as not finite).  The sums are exact integer sums of fixed-point contributions:
        the result is independent of the order of the bodies and the same bits on every call.  Velocities are read as
        stored (kick-drift: half a step from the positions).  Barnes-Hut and direct handles; ValueError for bad
        arguments, a quantity whose maximum is not finite, and owner-mode and sharded handles.  The call does not change
        what the next step computes."""
        what = "deposit"
        self._query_refuse(what, tree=False)
        names = _sum_names(what, quantities, DEPOSIT_QUANTITIES)
        if scheme not in DEPOSIT_SCHEMES:
            raise ValueError(f"{what}: scheme must be one of {list(DEPOSIT_SCHEMES)}, not {scheme!r}")
        lo_, hi_ = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (lo, hi))
        d = np.ascontiguousarray(dims, dtype=np.int64).reshape(-1)
        if len(lo_) != 3 or len(hi_) != 3 or len(d) != 3:
            raise ValueError(f"{what}: lo, hi and dims must have three entries each")
        if (d < 1).any() or int(d.max()) > 1 << 28 or int(d[0]) * int(d[1]) * int(d[2]) > 1 << 28:
            raise ValueError(f"{what}: dims {d.tolist()} must be >= 1 with at most 2^28 values in all planes")
        d32 = d.astype(np.int32)
        return _sum_planes(names, DEPOSIT_QUANTITIES, "momentum", (int(d[2]), int(d[1]), int(d[0])), stats, {},
                           lambda bits, out, st, ex: self._query_call(what, self._lib.nbmi_deposit(
                               self._h, _nat.ptr(lo_), _nat.ptr(hi_), _nat.ptr(d32), DEPOSIT_SCHEMES[scheme], bits, out, st, ex)))

    # ---- radial profiles and mass radii (include/nbmi.h nbmi_radial_profile; nbody/profile.py) ----
    def _profile_center(self, what, center, bulk_velocity):
        """(centre, bulk velocity) as float64 3-vectors: "com" = the centre of mass and P / M of diagnostics(), None or
        "origin" = zeros, a 3-sequence as given."""
        d = None
        out = []
        for name, val in (("center", center), ("bulk_velocity", bulk_velocity)):
            if val is None or (isinstance(val, str) and val == "origin"):
                out.append(np.zeros(3, dtype=np.float64))
            elif isinstance(val, str) and val == "com":
                if d is None:  # diagnostics(potential=False), a handle it refuses (a shard) being a ValueError here
                    d = np.empty(12, dtype=np.float64)
                    terms = C.c_int64(0)
                    _nat.check_arg(self._lib.nbmi_diagnostics(self._h, 0, _nat.ptr(d), C.addressof(terms)), what,
                                   "nbmi_diagnostics")
                if name == "center":
                    out.append(np.array([float(x) for x in d[1:4]], dtype=np.float64))
                else:
                    out.append(np.array([float(x) for x in d[4:7]], dtype=np.float64) / np.float64(float(d[0])))
            else:
                a = None if isinstance(val, str) else np.ascontiguousarray(val, dtype=np.float64).reshape(-1)
                if a is None or len(a) != 3:
                    raise ValueError(f'{what}: {name} must be "com", "origin", None or three numbers, not {val!r}')
                out.append(a)
        return out

    def radial_profile(self, edges, center="com", bulk_velocity="com", quantities=("number", "mass"), stats=False):
        """Sums of per-body quantities over the shells between the nb + 1 radii ``edges`` about ``center``, velocities
        taken relative to ``bulk_velocity`` ("com": the centre of mass and its velocity from ``diagnostics``; None or
        "origin": zeros; or three numbers).  ``quantities``: any of "number", "mass", "radial_momentum" (m v_r),
        "radial_kinetic" (m v_r^2), "kinetic" (m w^2), "angular_momentum" (m r x w).  Returns a dict with one float64
        array of nb + 1 values per quantity - entry 0 the ball inside edges[0], entry s the shell (edges[s-1], edges[s]];
        "angular_momentum": (3, nb + 1) -, "center", "bulk_velocity", "exponents" (int32 per plane in the library's order)
        and, with ``stats``, "stats" = (bodies in a slot, bodies beyond the last edge, bodies skipped as not finite).
        Exact integer sums of fixed-point contributions: independent of the order of the bodies, the same bits on every
        call.  Barnes-Hut and direct handles; ValueError for bad arguments, a quantity whose maximum is not finite, and
        owner-mode and sharded handles.  The call does not change what the next step computes."""
        what = "radial_profile"
        self._query_refuse(what, tree=False)
        names = _sum_names(what, quantities, PROFILE_QUANTITIES)
        e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        if len(e) < 2 or len(e) > 257:
            raise ValueError(f"{what}: expected 2 .. 257 edges, got {len(e)}")
        c, b = self._profile_center(what, center, bulk_velocity)
        return _sum_planes(names, PROFILE_QUANTITIES, "angular_momentum", (len(e),), stats, {"center": c, "bulk_velocity": b},
                           lambda bits, out, st, ex: self._query_call(what, self._lib.nbmi_radial_profile(
                               self._h, _nat.ptr(c), _nat.ptr(b), len(e) - 1, _nat.ptr(e), bits, out, st, ex)))

    def mass_radii(self, fractions, center="com"):
        """The squared radii about ``center`` (as in ``radial_profile``) that hold the given ``fractions`` (each in
        (0, 1], any order) of the mass of the bodies with finite coordinates: a dict with "radius2" (the smallest r^2 of
        a body within which at least that fraction lies, NaN if there is no mass), "inside" (bodies within it, int64),
        "mass_inside", "total_mass", "center", "stats" = (bodies taking part, bodies skipped) and "exponent" (the masses
        are counted in units of 2 ** exponent).  Exact and unique: a rank selection over integer masses in which bodies
        of equal r^2 enter together.  Barnes-Hut and direct handles; ValueError as for ``radial_profile``."""
        what = "mass_radii"
        self._query_refuse(what, tree=False)
        f = np.ascontiguousarray(fractions, dtype=np.float64).reshape(-1)
        if len(f) < 1 or len(f) > 64:
            raise ValueError(f"{what}: expected 1 .. 64 fractions, got {len(f)}")
        c, = self._profile_center(what, center, None)[:1]
        r2 = np.zeros(len(f), dtype=np.float64)
        inside = np.zeros(len(f), dtype=np.int64)
        mass = np.zeros(len(f), dtype=np.float64)
        total, ex = C.c_double(0.0), C.c_int32(0)
        st = np.zeros(2, dtype=np.int64)
        self._query_call(what, self._lib.nbmi_mass_radii(self._h, _nat.ptr(c), len(f), _nat.ptr(f), _nat.ptr(r2), _nat.ptr(inside),
                                                       _nat.ptr(mass), C.addressof(total), _nat.ptr(st), C.addressof(ex)))
        return {"radius2": r2, "inside": inside, "mass_inside": mass, "total_mass": float(total.value), "center": c,
                "stats": tuple(int(x) for x in st), "exponent": int(ex.value)}

    def knn(self, k: int, evals=False):
        """(r2_k, mass_k), (N,) float64 each in the caller's body order: the squared distance to the k-th nearest other
        body - exact, equal to a brute force bit for bit - and the mass within it, own mass and ties included.
        ``evals=True`` also returns the number of distances the call evaluated.  1 <= k <= min(64, N - 1).  Barnes-Hut
        handles only; the call does not change what the next step computes."""
        self._query_refuse(f"knn({k})")
        r2 = np.empty(self.n, dtype=np.float64)
        mk = np.empty(self.n, dtype=np.float64)
        ev = C.c_int64(0)
        self._query_call(f"knn({k})", self._lib.nbmi_knn(self._h, int(k), _nat.ptr(r2), _nat.ptr(mk),
                                                      C.addressof(ev) if evals else None))
        return (r2, mk, int(ev.value)) if evals else (r2, mk)

    def densities(self, k: int = 32) -> np.ndarray:
        """rho (N,) float64: mass_k over the volume of the k-th neighbour sphere; +inf where that radius is 0."""
        self._query_refuse(f"densities({k})")
        out = np.empty(self.n, dtype=np.float64)
        self._query_call(f"densities({k})", self._lib.nbmi_get_densities_f64(self._h, int(k), _nat.ptr(out)))
        return out

    def set_color_mode(self, mode: str, k: int = 32, log10_range=(0.0, 1.0)):
        """What compute_colors / frame_begin colour by: "speed" (default; the reference's ramp over speed / max_speed) or
        "density" (the same ramp over where log10 of the k-NN density lies in ``log10_range``; max_speed is then
        ignored).  Density mode is refused with ValueError where knn() is, and for a bad k or range."""
        if mode not in COLOR_MODES:
            raise ValueError(f"color mode must be one of {sorted(COLOR_MODES)}, not {mode!r}")
        lo, hi = (float(x) for x in log10_range)
        if mode == "density":
            self._query_refuse("set_color_mode('density')")
        self._query_call(f"set_color_mode({mode!r})", self._lib.nbmi_set_color_mode(self._h, COLOR_MODES[mode], int(k), lo, hi))

    def _color_mode(self):
        mode, k = C.c_int(0), C.c_int(0)
        lo, hi = C.c_double(0.0), C.c_double(0.0)
        _nat.check(self._lib.nbmi_get_color_mode(self._h, C.addressof(mode), C.addressof(k), C.addressof(lo), C.addressof(hi)),
                   "nbmi_get_color_mode")
        return {v: n for n, v in COLOR_MODES.items()}[mode.value], k.value, (lo.value, hi.value)

    @property
    def color_mode(self) -> str:
        return self._color_mode()[0]

    @property
    def color_settings(self):
        """{"mode", "k", "log10_range"} as the library holds them (k and the range are the last density mode's)."""
        mode, k, rng = self._color_mode()
        return {"mode": mode, "k": k, "log10_range": [rng[0], rng[1]]}

    # ---- friends-of-friends groups (include/nbmi.h nbmi_fof) ----
    n_groups = None  # of the last find_groups(), singletons included

    def find_groups(self, link: float, evals=False):
        """labels (N,) int32 in the caller's body order: the smallest body index of the connected component that body i
        belongs to when two bodies are linked iff d2 <= link * link - exact, equal to a brute force.  The number of
        groups (singletons included) is left in ``n_groups``; ``evals=True`` also returns the number of distances the
        call evaluated.  Refused with ValueError where knn() is and for a link that is not finite and > 0; the call
        does not change what the next step computes."""
        what = f"find_groups({link})"
        self._query_refuse(what)
        labels = np.empty(self.n, dtype=np.int32)
        ng, ev = C.c_int64(0), C.c_int64(0)
        self._query_call(what, self._lib.nbmi_fof(self._h, float(link), _nat.ptr(labels), C.addressof(ng),
                                                C.addressof(ev) if evals else None))
        self.n_groups = int(ng.value)
        return (labels, int(ev.value)) if evals else labels

    def group_catalogue(self, link: float, min_members: int = 20, capacity=None):
        """The groups of find_groups(link) with at least ``min_members`` bodies, largest first (ties by label): a dict of
        ``count`` (the number of such groups, which may exceed the rows returned), ``label`` int32, ``members`` int64,
        ``mass``, ``center`` (rows, 3), ``velocity`` (rows, 3), ``lo`` / ``hi`` (rows, 3: the bounding box).
        ``capacity`` limits the rows returned (default: all).  The same state gives the same bits."""
        what = f"group_catalogue({link}, min_members={min_members})"
        self._query_refuse(what)
        cap = self.n // max(1, int(min_members)) if capacity is None else int(capacity)
        rows = max(cap, 0)
        label = np.empty(rows, dtype=np.int32)
        members = np.empty(rows, dtype=np.int64)
        out = np.empty((rows, 13), dtype=np.float64)
        cnt = C.c_int64(0)
        self._query_call(what, self._lib.nbmi_fof_catalogue(self._h, float(link), int(min_members), cap, _nat.ptr(label),
                                                          _nat.ptr(members), _nat.ptr(out), C.addressof(cnt)))
        k = min(int(cnt.value), rows)
        return {"count": int(cnt.value), "label": label[:k], "members": members[:k], "mass": out[:k, 0].copy(),
                "center": out[:k, 1:4].copy(), "velocity": out[:k, 4:7].copy(), "lo": out[:k, 7:10].copy(),
                "hi": out[:k, 10:13].copy()}

    def color_by_groups(self, link: float, min_members: int = 20):
        """One shot: the colours compute_colors leaves (get_colors, visible_points, render) become group colours - every
        group of at least ``min_members`` bodies in a colour of its own (the speed ramp at a hash of its label), every
        other body grey.  The colour mode is not touched: the next compute_colors colours as before."""
        what = f"color_by_groups({link}, min_members={min_members})"
        self._query_refuse(what)
        self._query_call(what, self._lib.nbmi_compute_group_colors(self._h, float(link), int(min_members)))

    # ---- the minimum spanning tree (include/nbmi.h nbmi_mst; consumers in nbody/mst.py) ----
    def minimum_spanning_tree(self, evals=False):
        """(edges int32 (N - 1, 2), d2 float64 (N - 1,)): the Euclidean minimum spanning tree of the bodies under the
        strict order (d2, i, j) on pairs - unique, exact, equal to a brute force - sorted ascending by that key, with
        edges[k, 0] < edges[k, 1] in the caller's body order.  Cutting it at any link gives find_groups(link)
        (``nbody.mst.cut``); ``evals=True`` returns (edges, d2, rounds, evals): also the Boruvka rounds run and the distances
        the call evaluated.  Refused with ValueError where knn() is; the call does not change what the next step computes."""
        what = "minimum_spanning_tree"
        self._query_refuse(what)
        m = max(self.n - 1, 0)
        ei, ej = np.empty(m, dtype=np.int32), np.empty(m, dtype=np.int32)
        d2 = np.empty(m, dtype=np.float64)
        rounds, ev = C.c_int64(0), C.c_int64(0)
        self._query_call(what, self._lib.nbmi_mst(self._h, _nat.ptr(ei), _nat.ptr(ej), _nat.ptr(d2), C.addressof(rounds),
                                                C.addressof(ev) if evals else None))
        edges = np.stack([ei, ej], axis=1)
        return (edges, d2, int(rounds.value), int(ev.value)) if evals else (edges, d2)

    def mst_rounds(self):
        """The rounds of the last minimum_spanning_tree(), a measurement hook: a list of {"evals", "edges", "ms"} - the
        distances the round evaluated (0 unless that call had ``evals=True``), the edges it appended and the host's wall
        time for it."""
        ev, ed, ms = np.zeros(64, dtype=np.int64), np.zeros(64, dtype=np.int64), np.zeros(64, dtype=np.float64)
        k = self._lib.nbmi_mst_rounds(self._h, 64, _nat.ptr(ev), _nat.ptr(ed), _nat.ptr(ms))
        _nat.check(min(k, 0), "nbmi_mst_rounds")
        return [{"evals": int(ev[i]), "edges": int(ed[i]), "ms": float(ms[i])} for i in range(min(k, 64))]

    # ---- binned pair counts (include/nbmi.h nbmi_pair_counts) ----
    def pair_counts(self, edges, evals=False):
        """(counts int64 (nb,), below int) for the nb + 1 ``edges`` (1 <= nb <= 64, finite, >= 0, strictly increasing):
        counts[k] = the number of unordered pairs of bodies with edges[k]^2 < d2 <= edges[k + 1]^2, below = those with
        d2 <= edges[0]^2 - exact, equal to a brute force.  ``evals=True`` returns (counts, below, evals, cell_pairs): the
        distances the call evaluated and the pairs it counted through whole cells.  Refused with ValueError where knn()
        is and for bad edges; the call does not change what the next step computes."""
        e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        what = f"pair_counts({len(e)} edges)"
        self._query_refuse(what)
        nb = len(e) - 1
        counts = np.zeros(max(nb, 0), dtype=np.int64)
        below, ev, cells = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._query_call(what, self._lib.nbmi_pair_counts(self._h, nb, _nat.ptr(e) if len(e) else None, _nat.ptr(counts),
                                                        C.addressof(below), C.addressof(ev) if evals else None,
                                                        C.addressof(cells) if evals else None))
        return (counts, int(below.value), int(ev.value), int(cells.value)) if evals else (counts, int(below.value))

    # ---- counts about arbitrary points (include/nbmi.h nbmi_pair_counts_at) ----
    def pair_counts_at(self, points, edges, per_point=False, evals=False):
        """(counts int64 (nb,), below int) of the bodies about the (m, 3) ``points`` for the nb + 1 ``edges`` (as
        pair_counts'): counts[k] = the number of (point, body) pairs with edges[k]^2 < d2 <= edges[k + 1]^2, below = those
        with d2 <= edges[0]^2 - DR, exact, equal to a brute force; nothing is excluded, a point on a body counts that
        body in ``below``.  ``per_point=True`` appends the (m, nb + 1) int32 rows whose column sums these are (column 0:
        below; nbody/pairs.py has counts_within and sphere_density for them), ``evals=True`` appends evals, cell_pairs:
        the distances the call evaluated and the pairs it counted through whole cells.  ValueError for a wrong shape or
        bad edges (before the library is called), for a coordinate that is not finite or beyond 1e18, and where knn() is
        refused; the call does not change what the next step computes."""
        from nbody.pairs import check_edges
        what = "pair_counts_at"
        self._query_refuse(what)
        p = np.ascontiguousarray(points, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError(f"{what}: expected points of shape (m, 3), got {p.shape}")
        e = np.ascontiguousarray(check_edges(edges))
        m, nb = len(p), len(e) - 1
        counts = np.zeros(nb, dtype=np.int64)
        rows = np.zeros((m, nb + 1), dtype=np.int32) if per_point else None
        below, ev, cells = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._query_call(what, self._lib.nbmi_pair_counts_at(self._h, m, _nat.ptr(p), nb, _nat.ptr(e), _nat.ptr(counts),
                                                           C.addressof(below), _nat.ptr(rows),
                                                           C.addressof(ev) if evals else None,
                                                           C.addressof(cells) if evals else None))
        out = (counts, int(below.value))
        if per_point:
            out += (rows,)
        return out + (int(ev.value), int(cells.value)) if evals else out

    def neighbour_counts(self, edges):
        """(N, nb + 1) int32, in the caller's body order: pair_counts_at's per-point rows at the bodies' own positions
        with 1 subtracted from column 0, the body itself.  Column 0 is then the number of OTHER bodies within edges[0] of
        body i - its coincident twins among them -, column k + 1 the number in (edges[k], edges[k + 1]]."""
        self._query_refuse("neighbour_counts")
        rows = self.pair_counts_at(self.get_positions_f64(), edges, per_point=True)[2]
        rows[:, 0] -= 1
        return rows

    def correlation_function(self, edges, randoms, estimator="natural"):
        """xi (nb,) float64, the two-point correlation function from DD = this handle's pair_counts(edges) and RR = those
        of the (M, 3) random catalogue ``randoms`` (a temporary Barnes-Hut handle with unit masses at rest).
        ``estimator``: "natural", DD / RR x M (M - 1) / (N (N - 1)) - 1, nan where RR == 0; "landy-szalay" and
        "davis-peebles" (nbody/pairs.py xi_landy_szalay, xi_davis_peebles) also take DR = pair_counts_at(randoms, edges),
        the bodies counted about the random points.  ValueError for any other name."""
        from nbody.pairs import xi_davis_peebles, xi_landy_szalay, xi_natural
        what = "correlation_function"
        if estimator not in ("natural", "landy-szalay", "davis-peebles"):
            raise ValueError(f'{what}: estimator = {estimator!r} is none of "natural", "landy-szalay", "davis-peebles"')
        self._query_refuse(what)
        r = _as_f64(randoms, (3,))
        dd = self.pair_counts(edges)[0]
        if estimator != "natural":
            dr = self.pair_counts_at(r, edges)[0]
            if estimator == "davis-peebles":
                return xi_davis_peebles(dd, dr, self.n, len(r))
        tmp = HIPBarnesHutSimulation(r, np.zeros_like(r), np.ones(len(r)), 1.0, 0.1, 1.0)
        try:
            rr = tmp.pair_counts(edges)[0]
        finally:
            tmp.close()
        if estimator == "landy-szalay":
            return xi_landy_szalay(dd, dr, rr, self.n, len(r))
        return xi_natural(dd, rr, self.n, len(r))

    def visible_points(self, cam_pos, cam_forward, cam_right, cam_up, tan_h, tan_v, far_dist):
        """Frustum culling + compaction on the device (reference compute_visibility_points,
        nbody/simulation.py:403-434, and the gather of draw(), :927-928): returns
        (positions[mask] float32, colors[mask] float32) in body order - only these rows leave the GPU.
        The two arrays are views into buffers this object re-uses: valid until the next call."""
        cam = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).reshape(3) for a in
                                                   (cam_pos, cam_forward, cam_right, cam_up)]))
        cnt = C.c_int64(0)
        if not hasattr(self, "_vis_buf") or self._vis_buf[0].shape[0] != self.n:
            self._vis_buf = (np.empty((self.n, 3), dtype=np.float32), np.empty((self.n, 3), dtype=np.float32))
        p, c = self._vis_buf
        _nat.check(self._lib.nbmi_visible_points(self._h, _nat.ptr(cam), float(tan_h), float(tan_v), float(far_dist),
                                                 _nat.ptr(p), _nat.ptr(c), self.n, C.addressof(cnt)),
                   "nbmi_visible_points")
        k = int(cnt.value)
        return p[:k], c[:k]

    def render(self, renderer, params=None, out=None, **camera):
        """This handle's bodies drawn by a nbody.render.HIPPointRenderer on the device (current positions, colours of
        the last compute_colors): uint8 (H, W, 3)."""
        return renderer.render_sim(self, params=params, out=out, **camera)

    # frame codec on the device (tools/record.py: format-1 / format-2 payloads of a .zstd frame)
    def frame_keyframe(self):
        """(positions f32 (N,3), colours f32 (N,3)); they become the device's previous decoded frame."""
        p, c = np.empty((self.n, 3), dtype=np.float32), np.empty((self.n, 3), dtype=np.float32)
        _nat.check(self._lib.nbmi_frame_keyframe(self._h, _nat.ptr(p), _nat.ptr(c)), "nbmi_frame_keyframe")
        return p, c

    def frame_delta(self):
        """(int16 (N,3) position deltas, int16 (N,3) colour deltas) = int16((cur - prev) * 1000) against the
        previous DECODED frame kept on the device (reference tools/record.py:254-262), 12 B/body over PCIe."""
        dp, dc = np.empty((self.n, 3), dtype=np.int16), np.empty((self.n, 3), dtype=np.int16)
        _nat.check(self._lib.nbmi_frame_delta_i16(self._h, _nat.ptr(dp), _nat.ptr(dc)), "nbmi_frame_delta_i16")
        return dp, dc

    def frame_set_previous(self, positions, colors):
        p = np.ascontiguousarray(positions, dtype=np.float32)
        c = np.ascontiguousarray(colors, dtype=np.float32)
        _nat.check(self._lib.nbmi_frame_set_previous(self._h, _nat.ptr(p), _nat.ptr(c)), "nbmi_frame_set_previous")

    # asynchronous frames (include/nbmi.h nbmi_frame_begin)
    FRAME_KINDS = {"f32": 0, "key": 1, "delta": 2}

    def frame_begin(self, kind="f32", max_speed=15.0) -> int:
        """Enqueue a frame of the current state and return its slot without waiting: "f32" = what compute_colors(max_speed)
        + get_positions() + get_colors() return, "key" / "delta" = frame_keyframe() / frame_delta() with the colour pass
        included.  Steps enqueued afterwards do not change the frame.  Two slots: a third begin without a frame_release
        raises ValueError, as does "delta" without a previous frame."""
        if kind not in self.FRAME_KINDS:
            raise ValueError(f"frame kind must be one of {sorted(self.FRAME_KINDS)}, not {kind!r}")
        slot = C.c_int(-1)
        rc = self._lib.nbmi_frame_begin(self._h, self.FRAME_KINDS[kind], float(max_speed), C.addressof(slot))
        _nat.check_arg(rc, f"frame_begin({kind!r})", "nbmi_frame_begin")  # refused: no free slot / no previous frame / owner mode
        return int(slot.value)

    def frame_wait(self, slot: int):
        """Wait for that slot's copy (not for the steps enqueued since) and return its two (N,3) arrays: float32 positions
        and colours, or int16 position and colour deltas.  They are read-only views of the slot's pinned memory, not
        copies: they die with frame_release(slot) - copy what has to live longer.  Deferred device errors raise as in
        sync(), as they stood at the begin."""
        first, second = C.c_void_p(0), C.c_void_p(0)
        kind, steps = C.c_int(0), C.c_int64(0)
        rc = self._lib.nbmi_frame_wait(self._h, int(slot), C.addressof(first), C.addressof(second), C.addressof(kind),
                                       C.addressof(steps))
        _nat.check_arg(rc, f"frame_wait({slot})", "nbmi_frame_wait")
        dtype = np.dtype(np.int16 if kind.value == self.FRAME_KINDS["delta"] else np.float32)

        def view(p):
            if self.n == 0:
                a = np.empty((0, 3), dtype=dtype)
            else:
                a = np.frombuffer((C.c_char * (self.n * 3 * dtype.itemsize)).from_address(p.value), dtype=dtype).reshape(self.n, 3)
            a.flags.writeable = False
            return a
        return view(first), view(second)

    def frame_release(self, slot: int):
        """Free the slot for the next frame_begin; the arrays frame_wait returned for it must no longer be used."""
        _nat.check_arg(self._lib.nbmi_frame_release(self._h, int(slot)), f"frame_release({slot})", "nbmi_frame_release")

    def frames_pending(self):
        """[(slot, kind, steps), ...] of the frames begun and not released, oldest first; steps = step_count() at the
        begin.  Kept by the library, so it is right even when an interrupt cut the call that began a frame."""
        slots, kinds, steps = (C.c_int * 2)(), (C.c_int * 2)(), (C.c_int64 * 2)()
        k = self._lib.nbmi_frame_pending(self._h, slots, kinds, steps)
        if k < 0:
            _nat.check(k, "nbmi_frame_pending")
        names = {v: n for n, v in self.FRAME_KINDS.items()}
        return [(int(slots[i]), names[kinds[i]], int(steps[i])) for i in range(k)]

    # multi-GPU row exchange (device pointers; see nbody/sharded.py)
    def set_shard(self, begin, end):
        rc = self._lib.nbmi_set_shard(self._h, int(begin), int(end))
        if rc == -1 and (self.integrator == "leapfrog" or self.multipole == "quadrupole" or self.tracer_count):
            raise ValueError(f"set_shard: {_nat.last_error()}")
        _nat.check(rc, "nbmi_set_shard")

    def set_exchange_sync(self, sync: bool):
        _nat.check(self._lib.nbmi_set_exchange_sync(self._h, 1 if sync else 0), "nbmi_set_exchange_sync")

    def export_shard(self, dev_ptr):
        _nat.check(self._lib.nbmi_export_shard(self._h, int(dev_ptr)), "nbmi_export_shard")

    def import_ranks(self, dev_ptr, begin, end):
        _nat.check(self._lib.nbmi_import_ranks(self._h, int(dev_ptr), int(begin), int(end)), "nbmi_import_ranks")

    def enable_timers(self, on=True):
        _nat.check(self._lib.nbmi_enable_timers(self._h, 1 if on else 0), "nbmi_enable_timers")

    def timers(self, reset=False):
        ms = np.zeros(5)
        cnt = C.c_int64(0)
        _nat.check(self._lib.nbmi_get_timers(self._h, _nat.ptr(ms), C.addressof(cnt), 1 if reset else 0),
                   "nbmi_get_timers")
        names = ("keys_ms", "sort_ms", "tree_ms", "walk_ms", "other_ms")
        d = dict(zip(names, ms.tolist()))
        d["steps"] = int(cnt.value)
        return d

    def stream_handle(self) -> int:
        return int(self._lib.nbmi_stream(self._h) or 0)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.nbmi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HIPBarnesHutSimulation(_HIPSimulation):
    """Octree build + tree walk + kick-drift on the GPU (reference CPU path
    nbody/simulation.py:63-305 behind the protocol of MetalBarnesHutSimulation,
    nbody/metal/metal_backend.py:246)."""

    _method = METHOD_BARNES_HUT

    def build_tree(self):
        _nat.check(self._lib.nbmi_build_tree(self._h), "nbmi_build_tree")

    def force_precision_share(self):
        """(share of the waves whose own density asked for float64 forces in the last step, every wave float64?)"""
        share, all64 = C.c_double(0.0), C.c_int(0)
        _nat.check(self._lib.nbmi_force_precision_share(self._h, C.addressof(share), C.addressof(all64)),
                   "nbmi_force_precision_share")
        return float(share.value), bool(all64.value)

    FORCE_PRECISION = {"auto": 0, "f32": 1, "f64": 2}

    def set_force_precision(self, mode="auto", tau=0.0):
        """Arithmetic of the pair forces: "auto" (default: float64 for the waves whose bodies sit densely enough that
        G rho dt^2 > tau, fp32 elsewhere), "f32", "f64" (the reference's own arithmetic, nbody/simulation.py:246-268).
        The accepted (body, node) sets are the reference's in every mode."""
        _nat.check(self._lib.nbmi_set_force_precision(self._h, self.FORCE_PRECISION[mode], float(tau)),
                   "nbmi_set_force_precision")

    def tree_stats(self, depth=True):
        """num_nodes as build_octree returns it, max depth, root half size (compute_bounds).
        depth=False skips the reduction kernel behind max_depth (one small D2H copy only)."""
        nn, md, b = C.c_int64(0), C.c_int32(0), C.c_double(0)
        _nat.check(self._lib.nbmi_tree_stats(self._h, C.addressof(nn), C.addressof(md) if depth else None,
                                             C.addressof(b)), "nbmi_tree_stats")
        out = dict(num_nodes=int(nn.value), bounds=float(b.value))
        if depth:
            out["max_depth"] = int(md.value)
        return out

    def morton_keys(self):
        """(key_hi, key_lo) uint64 per body, caller's order, for the last built tree."""
        hi = np.empty(self.n, dtype=np.uint64)
        lo = np.empty(self.n, dtype=np.uint64)
        _nat.check(self._lib.nbmi_get_keys(self._h, _nat.ptr(hi), _nat.ptr(lo)), "nbmi_get_keys")
        return hi, lo

    def sort_keys(self):
        """The keys the device sorts by (octant digits relabelled along the Hilbert curve), caller's order."""
        hi = np.empty(self.n, dtype=np.uint64)
        lo = np.empty(self.n, dtype=np.uint64)
        _nat.check(self._lib.nbmi_get_sort_keys(self._h, _nat.ptr(hi), _nat.ptr(lo)), "nbmi_get_sort_keys")
        return hi, lo

    def cells(self):
        """(level, key) of every node of the last built tree."""
        nn = self.tree_stats()["num_nodes"]
        level = np.empty(nn, dtype=np.int32)
        key = np.empty(nn, dtype=np.uint64)
        _nat.check(self._lib.nbmi_get_cells(self._h, _nat.ptr(level), _nat.ptr(key), nn), "nbmi_get_cells")
        return level, key

    def cell_moments(self):
        """(level, key, P) of every node of the last built tree in quadrupole mode: P (num_nodes, 6) float64 =
        {Pxx, Pyy, Pzz, Pxy, Pxz, Pyz} of the walk's fp32 records (leaves: zeros)."""
        nn = self.tree_stats()["num_nodes"]
        level = np.empty(nn, dtype=np.int32)
        key = np.empty(nn, dtype=np.uint64)
        mom = np.empty((nn, 6), dtype=np.float64)
        rc = self._lib.nbmi_get_cell_moments(self._h, _nat.ptr(level), _nat.ptr(key), _nat.ptr(mom), nn)
        _nat.check_arg(rc, "cell_moments", "nbmi_get_cell_moments")
        return level, key, mom

    def walk_counters(self):
        out = np.zeros(17, dtype=np.int64)
        _nat.check(self._lib.nbmi_walk_counters(self._h, _nat.ptr(out)), "nbmi_walk_counters")
        return dict(wave_visits=int(out[0]), lane_visits=int(out[1]), lane_accepts=int(out[2]),
                    window_misses={8 << w: int(out[3 + w]) for w in range(4)}, jumps=int(out[7]),
                    xcd_visits=[int(v) for v in out[8:16]], band_visits=int(out[16]))

    def key_order(self):
        """Body indices along the sort-key order of the last built tree (octree DFS, the eight children of a cell
        in Hilbert-curve order; see sort_keys)."""
        out = np.empty(self.n, dtype=np.int32)
        _nat.check(self._lib.nbmi_get_order(self._h, _nat.ptr(out)), "nbmi_get_order")
        return out


class HIPOwnerSimulation(HIPBarnesHutSimulation):
    """Owner-mode handle of the multi-GPU stage 2 (include/nbmi.h, nbmi_create_owner): the bodies of one
    octant-key range, their own octree inside the global root cube, plus received locally essential trees.
    Driven by nbody/sharded.py::LetBarnesHut; buffers are device pointers."""

    def __init__(self, positions, velocities, masses, global_ids, capacity, let_capacity, world, rank, G, softening,
                 damping, theta=0.5, device=None):
        lib = _nat.load()
        pos = _as_f64(positions, (3,))
        vel = _as_f64(velocities, (3,))
        m = _as_f64(masses, ())
        ids = np.ascontiguousarray(global_ids, dtype=np.int32)
        if not (len(pos) == len(vel) == len(m) == len(ids)):
            raise ValueError("positions, velocities, masses and ids must have the same length")
        if device is None:
            device = _default_device()
        self.G, self.softening, self.damping, self.theta = float(G), float(softening), float(damping), float(theta)
        self.device = int(device)
        self.world, self.rank = int(world), int(rank)
        self.capacity, self.let_capacity = int(capacity), int(let_capacity)
        self._lib = lib
        self._h = lib.nbmi_create_owner(len(pos), _nat.ptr(pos), _nat.ptr(vel), _nat.ptr(m), _nat.ptr(ids), self.capacity,
                                        self.let_capacity, self.world, self.rank, self.G, self.softening, self.damping,
                                        self.theta, self.device)
        if not self._h:
            raise RuntimeError(f"nbmi_create_owner failed: {_nat.last_error()}")
        print(f"[HIP] rank {rank}/{world}: owner of {len(pos):,} bodies (capacity {capacity:,}) on device {self.device}")

    @property
    def n(self):
        return int(self._lib.nbmi_owner_count(self._h)) if self._h else 0

    _query_refusal = "owner-mode handles are not supported (the neighbours may live on other ranks)"
    _field_refusal = "owner-mode handles are not supported (the field needs the other ranks' trees)"

    def set_multipole(self, multipole: str):
        if _multipole_code(multipole) != MULTIPOLES["monopole"]:
            raise ValueError("owner-mode handles support only monopole terms (the exchanged tree rows carry no second "
                             "moments)")
        super().set_multipole(multipole)

    def set_integrator(self, integrator: str):
        if _integrator_code(integrator) != INTEGRATORS["kick_drift"]:
            raise ValueError("owner-mode handles support only the kick_drift integrator (the exchanged rows carry no "
                             "acceleration columns)")
        super().set_integrator(integrator)

    def ids(self):
        out = np.empty(self.n, dtype=np.int32)
        _nat.check(self._lib.nbmi_owner_get_ids(self._h, _nat.ptr(out)), "nbmi_owner_get_ids")
        return out

    def owner_maxabs(self, dev_maxabs):
        _nat.check(self._lib.nbmi_owner_maxabs(self._h, int(dev_maxabs)), "nbmi_owner_maxabs")

    def owner_sample(self, dev_maxabs, dev_samples, nsamples, nvalid=0):
        """`nvalid` of the `nsamples` slots get a key sample (0: all of them)."""
        _nat.check(self._lib.nbmi_owner_sample(self._h, int(dev_maxabs), int(dev_samples), int(nsamples), int(nvalid)),
                   "nbmi_owner_sample")

    def owner_partition(self, dev_all_samples, total, dev_send_rows):
        counts = np.zeros(self.world, dtype=np.int64)
        _nat.check(self._lib.nbmi_owner_partition(self._h, int(dev_all_samples), int(total), int(dev_send_rows),
                                                  _nat.ptr(counts)), "nbmi_owner_partition")
        return counts

    def owner_adopt(self, dev_recv_rows, n_new, dev_maxabs, dev_bbox, dev_chain=0):
        _nat.check(self._lib.nbmi_owner_adopt(self._h, int(dev_recv_rows), int(n_new), int(dev_maxabs), int(dev_bbox), int(dev_chain)),
                   "nbmi_owner_adopt")

    def chain_doubles(self):
        """float64 words of a rank's boundary table (nbmi_owner_adopt writes it, all ranks' tables go to owner_export_let)."""
        return int(self._lib.nbmi_owner_chain_doubles())

    def owner_export_let(self, dev_boxes, dev_chains, dev_let):
        """Rows for every destination rank (packed in rank order in `dev_let`); returns the counts."""
        counts = np.zeros(self.world, dtype=np.int64)
        _nat.check(self._lib.nbmi_owner_export_let(self._h, int(dev_boxes), int(dev_chains), int(dev_let), _nat.ptr(counts)),
                   "nbmi_owner_export_let")
        return counts

    def owner_set_dt(self, dt):
        """dt of the step about to be exchanged: force precision "auto" is decided while owner_adopt builds the tree."""
        _nat.check(self._lib.nbmi_owner_set_dt(self._h, float(dt)), "nbmi_owner_set_dt")

    def let_row_bytes(self):
        return int(self._lib.nbmi_owner_let_row_bytes())

    def owner_step_facts(self):
        """After owner_export_let: int64[4] = (waves asking for float64 forces, waves, tree rows that fit in front of /
        behind the own piece of the walk array)."""
        out = np.zeros(4, dtype=np.int64)
        _nat.check(self._lib.nbmi_owner_step_facts(self._h, _nat.ptr(out)), "nbmi_owner_step_facts")
        return out

    def owner_set_all64(self, verdict):
        """The ranks' common decision for the next owner_step: True / False = every wave float64 / the waves decide;
        None = this rank's own rule."""
        _nat.check(self._lib.nbmi_owner_set_all64(self._h, -1 if verdict is None else int(bool(verdict))), "nbmi_owner_set_all64")

    def owner_step(self, dev_lets, counts, dt):
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        _nat.check(self._lib.nbmi_owner_step(self._h, int(dev_lets), _nat.ptr(counts), float(dt)), "nbmi_owner_step")


class HIPDirectSimulation(_HIPSimulation):
    """All-pairs O(N^2) forces, LDS tiled (reference CUDASimulation, nbody/gpu_backend.py:336-409;
    no theta)."""

    _method = METHOD_DIRECT
    _query_refusal = "direct N^2 handles have no tree"

    def __init__(self, positions, velocities, masses, G, softening, damping, device=None, integrator="kick_drift",
                 multipole="monopole"):
        super().__init__(positions, velocities, masses, G, softening, damping, theta=0.0, device=device,
                         integrator=integrator, multipole=multipole)


# Reference thresholds (:618-620) exist because its GPU paths are O(N^2); the HIP Barnes-Hut
# backend is O(N log N) like the reference's Metal one, so it takes every size.
HIP_BH_THRESHOLD = 100_000_000  # = kMaxBodies of libnbmi.so (node links are 32-bit byte offsets): beyond it the factory returns None


def create_gpu_simulation(positions: np.ndarray, velocities: np.ndarray, masses: np.ndarray, G: float,
                          softening: float, damping: float, theta: float = 0.5, force_gpu: bool = False,
                          method: Optional[str] = None, integrator: str = "kick_drift", multipole: str = "monopole"):
    """Reference signature (:623-625) plus ``method`` ("barnes_hut" default, or "direct"), ``integrator``
    ("kick_drift" default, or "leapfrog"; see _HIPSimulation.set_integrator) and ``multipole`` ("monopole" default, or
    "quadrupole"; see _HIPSimulation.set_multipole).

    Returns a backend object, or None if the HIP backend is not available / not selected."""
    backend, _info = get_backend()
    n = len(positions)
    if backend != Backend.HIP:
        return None
    method = method or os.environ.get("NBMI_METHOD", "barnes_hut")
    if method == "direct":
        return HIPDirectSimulation(positions, velocities, masses, G, softening, damping, integrator=integrator,
                                   multipole=multipole)
    if n <= HIP_BH_THRESHOLD or force_gpu:
        return HIPBarnesHutSimulation(positions, velocities, masses, G, softening, damping, theta, integrator=integrator,
                                      multipole=multipole)
    print(f"[GPU] {n:,} bodies exceeds the HIP Barnes-Hut limit ({HIP_BH_THRESHOLD:,})")
    return None
