"""Fields on a regular grid from ``sim.deposit`` (include/nbmi.h nbmi_deposit): surface-density
maps, mean-velocity and dispersion maps, the density contrast and its power spectrum.  Pure NumPy except where
``surface_density`` calls ``deposit``."""
import numpy as np

AXES = {"x": 0, "y": 1, "z": 2}
# The largest depth a projection uses: far beyond any coordinate a simulation holds, and small enough that the width
# of the slab and its reciprocal stay finite.
ALL_DEPTH = 1.0e300


def map_box(axis="z", center=(0.0, 0.0, 0.0), half_width=1.0, pixels=512, depth=None):
    """(lo, hi, dims) of the deposit behind ``surface_density``: ``pixels`` x ``pixels`` cells of the square of
    ``half_width`` about ``center`` in the plane normal to ``axis``, one cell along it - ``depth`` on either side of
    the centre, or (None) everything."""
    if axis not in AXES:
        raise ValueError(f"axis must be one of {sorted(AXES)}, not {axis!r}")
    a = AXES[axis]
    hw, px = float(half_width), int(pixels)
    if not (np.isfinite(hw) and hw > 0.0) or px < 1:
        raise ValueError(f"need a finite half_width > 0 and pixels >= 1, not {half_width} and {pixels}")
    c = np.asarray(center, dtype=np.float64).reshape(3)
    lo, hi, dims = c - hw, c + hw, [px, px, px]
    if depth is None:
        lo[a], hi[a] = -ALL_DEPTH, ALL_DEPTH
    else:
        lo[a], hi[a] = c[a] - float(depth), c[a] + float(depth)
    dims[a] = 1
    return lo, hi, dims


def surface_density(sim, axis="z", center=(0.0, 0.0, 0.0), half_width=1.0, pixels=512, scheme="cic", depth=None):
    """Mass per area, (pixels, pixels) float64, of the bodies projected along ``axis``: rows run along the higher of the
    two remaining axes, columns along the lower (axis "z": [iy, ix]).  ``depth=None`` takes every body with finite
    coordinates along the axis, else those within ``depth`` of the centre."""
    lo, hi, dims = map_box(axis, center, half_width, pixels, depth)
    mass = sim.deposit(lo, hi, dims, scheme=scheme, quantities=("mass",))["mass"]
    h = 2.0 * float(half_width) / int(pixels)
    return mass.reshape(int(pixels), int(pixels)) / (h * h)


def velocity_maps(planes):
    """(mean velocity (3, ...), dispersion (...)) from a deposit's "mass", "momentum" and "kinetic" planes:
    momentum / mass and sqrt(max(kinetic / mass - |mean v|^2, 0)); both NaN where the mass is 0."""
    mass = np.asarray(planes["mass"], dtype=np.float64)
    mom = np.asarray(planes["momentum"], dtype=np.float64)
    kin = np.asarray(planes["kinetic"], dtype=np.float64)
    m = np.where(mass != 0.0, mass, np.nan)
    mean = mom / m
    sigma = np.sqrt(np.maximum(kin / m - (mean * mean).sum(axis=0), 0.0))  # (maximum keeps the NaN)
    return mean, sigma


def density_contrast(mass_grid):
    """delta = rho / mean(rho) - 1 of a mass (or density) grid."""
    g = np.asarray(mass_grid, dtype=np.float64)
    mean = g.mean()
    if not mean > 0.0:
        raise ValueError("density_contrast: the grid's mean is not positive")
    return g / mean - 1.0


def power_spectrum(mass_grid, box_length, scheme="cic", nbins=None):
    """(k, P(k), modes) of a cubic (n, n, n) mass grid over a box of side ``box_length``: rfftn of the contrast,
    divided by the scheme's window prod_a sinc(k_a h / 2)^p (p = 1 for "ngp", 2 for "cic"; h = box_length / n),
    P = |delta_k|^2 V / n^6, averaged over ``nbins`` (default n // 2) shells of width 2 pi / box_length starting half
    a width below the fundamental - bin j is centred on j + 1 fundamentals.  k is the mean |k| of a shell's modes
    (NaN, with P, where it has none); the k = 0 mode is left out, and every mode counts once with its conjugate."""
    g = np.asarray(mass_grid, dtype=np.float64)
    if g.ndim != 3 or len(set(g.shape)) != 1:
        raise ValueError(f"power_spectrum: need a cubic grid, not {g.shape}")
    if scheme not in ("ngp", "cic"):
        raise ValueError(f"power_spectrum: scheme must be 'ngp' or 'cic', not {scheme!r}")
    n, L = g.shape[0], float(box_length)
    nbins = n // 2 if nbins is None else int(nbins)
    dk = np.fft.rfftn(density_contrast(g))
    kf = 2.0 * np.pi / L
    full, half = np.fft.fftfreq(n, 1.0 / n), np.fft.rfftfreq(n, 1.0 / n)  # integer mode numbers
    p = 1 if scheme == "ngp" else 2
    wf, wh = np.sinc(full / n) ** p, np.sinc(half / n) ** p  # np.sinc(x) = sin(pi x) / (pi x); k h / 2 = pi j / n
    window = wf[:, None, None] * wf[None, :, None] * wh[None, None, :]
    power = (np.abs(dk / window) ** 2) * (L ** 3 / float(n) ** 6)
    kk = np.sqrt(full[:, None, None] ** 2 + full[None, :, None] ** 2 + half[None, None, :] ** 2)
    # a real field: the modes with 0 < kz < Nyquist stand for their conjugates too
    weight = np.where((half > 0) & ((n % 2 == 1) | (half < n // 2)), 2.0, 1.0)[None, None, :] * np.ones_like(kk)
    b = np.floor(kk - 0.5).astype(np.int64)  # shell j: j + 0.5 <= |k| / kf < j + 1.5
    ok = (kk > 0.0) & (b >= 0) & (b < nbins)
    modes = np.bincount(b[ok], weights=weight[ok], minlength=nbins)
    with np.errstate(invalid="ignore", divide="ignore"):
        pk = np.bincount(b[ok], weights=(weight * power)[ok], minlength=nbins) / modes
        km = np.bincount(b[ok], weights=(weight * kk)[ok], minlength=nbins) / modes * kf
    return km, pk, modes.astype(np.int64)
