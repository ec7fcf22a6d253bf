"""Radial structure from ``sim.radial_profile`` and ``sim.mass_radii`` (include/nbmi.h nbmi_radial_profile,
nbmi_mass_radii): density and enclosed mass, radial dispersion and anisotropy, rotation,
Lagrangian radii and the density centre.  Pure NumPy except where a function takes a ``sim``.

A profile's arrays have nb + 1 entries: entry 0 is the ball inside edges[0], entry s the shell (edges[s-1], edges[s]]."""
import numpy as np

DEFAULT_FRACTIONS = (0.1, 0.25, 0.5, 0.75, 0.9)


def auto_edges(spawn_radius, shells=48):
    """``shells`` + 1 log-spaced radii from spawn_radius * 2^-8 to 4 * spawn_radius."""
    r, shells = float(spawn_radius), int(shells)
    if not (np.isfinite(r) and r > 0.0) or not 1 <= shells <= 256:
        raise ValueError(f"auto_edges: spawn_radius {spawn_radius!r} must be > 0 and shells {shells!r} in 1 .. 256")
    e = r * np.exp2(np.linspace(-8.0, 2.0, shells + 1))
    e[0], e[-1] = r / 256.0, 4.0 * r
    return e


def shell_volumes(edges):
    """Volumes of the nb + 1 slots: the ball of edges[0], then the shells."""
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    ball = 4.0 / 3.0 * np.pi * e ** 3
    return np.concatenate([ball[:1], np.diff(ball)])


def _ratio(num, den):
    """num / den, NaN where den is 0"""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(den != 0.0, num / np.where(den != 0.0, den, 1.0), np.nan)


def density_profile(planes, edges):
    """(rho, enclosed): the "mass" plane over the slot volumes (NaN for a ball of radius 0) and the cumulative mass
    M(<= edges[s]) per slot."""
    mass = np.asarray(planes["mass"], dtype=np.float64)
    return _ratio(mass, shell_volumes(edges)), np.cumsum(mass)


def velocity_profile(planes):
    """Mass-weighted, from the "mass", "radial_momentum", "radial_kinetic" and "kinetic" planes: a dict with "mean_vr",
    "sigma_r2" = <v_r^2> - <v_r>^2, "sigma_t2" = <w^2> - <v_r^2> (both clamped at 0), "sigma_r", "sigma_t" and
    "beta" = 1 - sigma_t2 / (2 sigma_r2).  Empty shells give NaN (and so does beta where sigma_r2 is 0)."""
    mass = np.asarray(planes["mass"], dtype=np.float64)
    mean_vr = _ratio(planes["radial_momentum"], mass)
    vr2 = _ratio(planes["radial_kinetic"], mass)
    w2 = _ratio(planes["kinetic"], mass)
    with np.errstate(all="ignore"):
        sr2 = np.where(np.isnan(vr2), np.nan, np.maximum(vr2 - mean_vr * mean_vr, 0.0))
        st2 = np.where(np.isnan(w2), np.nan, np.maximum(w2 - vr2, 0.0))
        beta = 1.0 - _ratio(st2, 2.0 * sr2)
    return {"mean_vr": mean_vr, "sigma_r2": sr2, "sigma_t2": st2, "sigma_r": np.sqrt(sr2), "sigma_t": np.sqrt(st2),
            "beta": beta}


def rotation_profile(planes):
    """(j (3, nb + 1), |j|): the specific angular momentum vector per slot from the "angular_momentum" and "mass" planes,
    and its magnitude; NaN for empty slots."""
    j = _ratio(planes["angular_momentum"], np.asarray(planes["mass"], dtype=np.float64)[None, :])
    return j, np.sqrt((j * j).sum(axis=0))


def lagrangian_radii(sim, fractions=DEFAULT_FRACTIONS, center="com"):
    """The radii about ``center`` that hold the ``fractions`` of the mass: sqrt of ``sim.mass_radii``'s radius2."""
    return np.sqrt(sim.mass_radii(fractions, center=center)["radius2"])


def density_center(sim, k=32):
    """The Casertano-Hut density centre sum(rho_i x_i) / sum(rho_i) over the k-NN densities ``sim.densities(k)``, summed
    on the host; a valid ``center`` argument.  Barnes-Hut handles only (k-NN needs the tree).  Bodies whose density is
    not finite (coincident bodies) or whose position is not finite are left out."""
    rho = np.asarray(sim.densities(int(k)), dtype=np.float64)
    x = np.asarray(sim.get_positions_f64(), dtype=np.float64)
    ok = np.isfinite(rho) & np.isfinite(x).all(axis=1)
    total = rho[ok].sum()
    if not total > 0.0:
        raise ValueError("density_center: no body with a finite, positive density")
    return (rho[ok, None] * x[ok]).sum(axis=0) / total
