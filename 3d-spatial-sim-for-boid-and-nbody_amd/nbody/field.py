"""Host side of the field evaluation (include/nbmi.h nbmi_field_at): what is derived from the
field at chosen points.  Pure NumPy over any object with ``field_at(points, potential=True)`` -> (acc (m, 3), phi (m,))
(and, for the tracers of section 4.19, ``get_tracers()`` -> (positions, velocities)); no device.  At the end, what is
derived from the tidal tensor's rows (``tidal_at`` / ``tidal``, section 4.27): plain functions of arrays."""
import numpy as np


def _unit(v, what):
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if v.shape != (3,) or not np.all(np.isfinite(v)) or not np.linalg.norm(v) > 0.0:
        raise ValueError(f"{what} must be a finite, non-zero 3-vector, got {v}")
    return v / np.linalg.norm(v)


def _ring_frame(normal):
    """Two unit vectors (e1, e2) that span the plane with the given normal, e1 x e2 = normal / |normal|."""
    n = _unit(normal, "normal")
    helper = np.zeros(3)
    helper[int(np.argmin(np.abs(n)))] = 1.0  # the axis least aligned with the normal
    if abs(n[2]) == 1.0:
        helper = np.array([1.0, 0.0, 0.0])  # z normal: e1 = x, e2 = +-y
    e1 = helper - np.dot(helper, n) * n
    e1 /= np.linalg.norm(e1)
    return e1, np.cross(n, e1)


def _ring_dirs(azimuths, normal):
    k = int(azimuths)
    if k < 1:
        raise ValueError(f"azimuths must be at least 1, got {azimuths}")
    e1, e2 = _ring_frame(normal)
    a = 2.0 * np.pi * np.arange(k) / k
    return np.cos(a)[:, None] * e1 + np.sin(a)[:, None] * e2  # (k, 3) unit radial directions


def _radii(radii):
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(r)) or np.any(r <= 0.0):
        raise ValueError("radii must be finite and positive")
    return r


def ring_points(center, radii, azimuths=16, normal=(0, 0, 1)):
    """(len(radii) * azimuths, 3) points: for every radius, ``azimuths`` equally spaced points of the circle of that
    radius about ``center`` in the plane with the given normal; row r * azimuths + k is radius r, azimuth k."""
    c = np.asarray(center, dtype=np.float64).reshape(3)
    r = _radii(radii)
    d = _ring_dirs(azimuths, normal)
    return (c + r[:, None, None] * d[None, :, :]).reshape(-1, 3)


def rotation_curve(sim, radii, center, azimuths=16, normal=(0, 0, 1)):
    """dict of (len(radii),) float64 arrays: ``radii``; ``a_radial``, the azimuthal mean of the inward acceleration
    -a . r_hat on the ring; ``v_circ`` = sqrt(R max(a_radial, 0)), the speed of a circular orbit in that mean field;
    ``phi``, the azimuthal mean of the potential."""
    r = _radii(radii)
    d = _ring_dirs(azimuths, normal)
    acc, phi = sim.field_at(ring_points(center, r, azimuths, normal), potential=True)
    acc = np.asarray(acc, dtype=np.float64).reshape(len(r), len(d), 3)
    a_radial = -(acc * d[None, :, :]).sum(axis=2).mean(axis=1)
    return {"radii": r, "a_radial": a_radial, "v_circ": np.sqrt(r * np.maximum(a_radial, 0.0)),
            "phi": np.asarray(phi, dtype=np.float64).reshape(len(r), len(d)).mean(axis=1)}


def potential_slice(sim, center, half_extent, resolution, axes=(0, 1)):
    """(resolution, resolution) float64 image of phi on the square of half width ``half_extent`` through ``center``
    spanned by the two coordinate ``axes``: pixel [i, j] is at center + u_j along axes[0] and + u_i along axes[1], u the
    ``resolution`` pixel centres of [-half_extent, half_extent]."""
    c = np.asarray(center, dtype=np.float64).reshape(3)
    res = int(resolution)
    a0, a1 = (int(a) for a in axes)
    if res < 1 or not float(half_extent) > 0.0 or not np.isfinite(half_extent):
        raise ValueError("potential_slice needs resolution >= 1 and a finite half_extent > 0")
    if a0 == a1 or not {a0, a1} <= {0, 1, 2}:
        raise ValueError(f"axes must be two different coordinates of 0, 1, 2, got {axes}")
    u = (np.arange(res) + 0.5) * (2.0 * float(half_extent) / res) - float(half_extent)
    pts = np.empty((res, res, 3), dtype=np.float64)
    pts[:] = c
    pts[:, :, a0] += u[None, :]
    pts[:, :, a1] += u[:, None]
    _, phi = sim.field_at(pts.reshape(-1, 3), potential=True)
    return np.asarray(phi, dtype=np.float64).reshape(res, res)


def circular_tracers(sim, radii, center, per_ring=16, normal=(0, 0, 1)):
    """(positions, velocities), (len(radii) * per_ring, 3) float64 each: seeds for ``sim.set_tracers`` on ring_points'
    rings (row r * per_ring + k is radius r, azimuth k), every one moving at rotation_curve's ``v_circ`` of its ring along
    the ring, counter-clockwise about ``normal``.  The bodies' bulk motion is not added."""
    r = _radii(radii)
    d = _ring_dirs(per_ring, normal)
    v_circ = rotation_curve(sim, r, center, per_ring, normal)["v_circ"]
    tangent = np.cross(_unit(normal, "normal"), d)  # (per_ring, 3) unit vectors along the ring
    vel = (v_circ[:, None, None] * tangent[None, :, :]).reshape(-1, 3)
    return ring_points(center, r, per_ring, normal), vel


def tracer_energies(sim):
    """(m,) float64: the specific energy 0.5 |v|^2 + phi of every tracer of ``sim`` (``get_tracers``) in the bodies'
    current potential (``field_at``).  In a static potential it is conserved along a tracer's orbit."""
    p, v = sim.get_tracers()
    p, v = np.asarray(p, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if len(p) == 0:
        return np.zeros(0, dtype=np.float64)
    _, phi = sim.field_at(p, potential=True)
    return 0.5 * (v * v).sum(axis=1) + np.asarray(phi, dtype=np.float64)


def escape_speed(phi):
    """sqrt(max(-2 phi, 0)): the speed at which a test particle at potential phi is unbound (phi -> 0 at infinity)."""
    return np.sqrt(np.maximum(-2.0 * np.asarray(phi, dtype=np.float64), 0.0))


# ---- the tidal tensor (include/nbmi.h nbmi_tidal_at): what is derived from rows
# {Txx, Tyy, Tzz, Txy, Txz, Tyz} of ``tidal_at`` / ``tidal`` ----
def _t6(t6):
    t = np.asarray(t6, dtype=np.float64)
    if t.ndim != 2 or t.shape[1] != 6:
        raise ValueError(f"expected tidal rows of shape (m, 6), got {t.shape}")
    return t


def tidal_matrix(t6):
    """(m, 3, 3) float64: the symmetric matrices T_ab = da_a/dx_b of the (m, 6) rows."""
    t = _t6(t6)
    return t[:, [0, 3, 4, 3, 1, 5, 4, 5, 2]].reshape(-1, 3, 3)


def tidal_eigenvalues(t6):
    """(m, 3) float64: the eigenvalues of T per row, descending (``numpy.linalg.eigvalsh``).  Positive: stretching along
    that axis; negative: compression.  A point mass G M at distance r gives (2, -1, -1) G M / r^3."""
    return np.linalg.eigvalsh(tidal_matrix(t6))[:, ::-1]


def tidal_norm(t6):
    """(m,) float64: the Frobenius norm of T per row, in the association of the device's ``norm``."""
    t = _t6(t6)
    return np.sqrt(((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
                   + 2.0 * ((t[:, 3] * t[:, 3] + t[:, 4] * t[:, 4]) + t[:, 5] * t[:, 5]))


def phase_per_step(norm, dt):
    """dt sqrt(norm / sqrt(6)): the orbital phase a step of ``dt`` advances where the tidal tensor has Frobenius norm
    ``norm``.  On a Kepler orbit T has eigenvalues (2, -1, -1) G M / r^3, norm sqrt(6) G M / r^3, so this is Omega dt;
    the kick-drift and leapfrog steps are unstable on a harmonic mode once it reaches 2."""
    return float(dt) * np.sqrt(np.asarray(norm, dtype=np.float64) / np.sqrt(6.0))


def web_type(t6, threshold=0.0):
    """(m,) int: the number of eigenvalues of -T (the Hessian of phi) above ``threshold``, the T-web class of the point:
    0 void, 1 sheet, 2 filament, 3 knot."""
    return (-tidal_eigenvalues(t6) > float(threshold)).sum(axis=1)


def tidal_radius(gm, t6):
    """(m,) float64: cbrt(gm / lambda_max), the distance from a satellite of mass parameter ``gm`` = G m at which the
    largest stretching eigenvalue lambda_max of the host's T balances the satellite's own pull; inf where lambda_max <= 0
    (nothing stretches).  This is the static tidal limit: it carries no centrifugal term, so for a satellite on a
    circular orbit the Jacobi radius is smaller (cbrt(gm / (lambda_max + Omega^2)))."""
    lam = tidal_eigenvalues(t6)[:, 0]
    gm = np.broadcast_to(np.asarray(gm, dtype=np.float64), lam.shape)
    pos = lam > 0.0
    return np.where(pos, np.cbrt(gm / np.where(pos, lam, 1.0)), np.inf)
