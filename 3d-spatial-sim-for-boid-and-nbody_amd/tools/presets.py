"""Initial-condition generators and presets needed by the hot path's harness.

Restates five distributions of the reference's generate_distribution - ``galaxy``, ``collision``,
``cluster`` (tools/presets.py:91-232, :350-397) and the large-scale ``spiral`` (:234-295) and
``filament`` (:609-684, the "cosmic web") - and its rotation curve helper (:52-88), drawing from
the GLOBAL NumPy RNG in the same order with the same float64 expressions, so ``np.random.seed(s)``
before the call reproduces the reference's arrays bit for bit (pinned by tests/golden/ic_pins.npz
and ic_pins_more.npz).  The code is written in this module's own structure, not copied.  PRESETS
holds the 35 reference presets built on these five distributions, with the reference's constants
(tests/golden/presets_ref.json).  The other 20 distributions and their 31 presets are content
below 1 M bodies and are not provided.
"""
from typing import List, Tuple

import numpy as np

DISTRIBUTIONS = {
    "galaxy": "Classic spiral disk galaxy",
    "collision": "Two galaxies colliding",
    "spiral": "Multi-arm spiral galaxy",
    "cluster": "Dense star cluster (globular)",
    "filament": "Cosmic web filament",
}


def compute_rotation_curve(r: np.ndarray, masses: np.ndarray, G: float, softening: float) -> np.ndarray:
    """Circular speed of a softened disk from the enclosed (radius-sorted) mass; reference :52-88."""
    order = np.argsort(r)
    rs = r[order]
    enclosed = np.cumsum(masses[order])
    eps = softening * 2
    eps_sq = eps ** 2
    r_sq = rs ** 2
    v = np.sqrt(G * enclosed * r_sq / (r_sq + eps_sq) ** 1.5)
    inner_scale = softening * 2
    v *= np.maximum((rs ** 2) / (rs ** 2 + inner_scale ** 2), 0.3)
    return v[np.argsort(order)]


def _soft_truncated_radii(count, scale_length, max_r, floor):
    """Exp(scale) radii, softly capped near max_r, floored (reference :110-116, :161-165)."""
    r = np.random.exponential(scale_length, count)
    r = r * (1 - np.exp(-max_r / (r + 0.01)))
    return np.maximum(r, floor)


def _disk_galaxy(pos, vel, masses, R, G, count, scale_length, softening, max_r, height, disp, spin,
                 x0=0.0, y0=0.0):
    """One rotating exponential disk written into the (count,3) views pos/vel."""
    r = _soft_truncated_radii(count, scale_length, max_r, R * 0.001)
    theta = np.random.uniform(0, 2 * np.pi, count)
    if x0 == 0.0 and y0 == 0.0:
        disk_height = R * height * (1 + (r / R) ** 0.5 * 0.3)
        z = np.random.normal(0, 1, count) * disk_height
        pos[:, 0] = r * np.cos(theta)
        pos[:, 1] = z
        pos[:, 2] = r * np.sin(theta)
    else:
        pos[:, 0] = r * np.cos(theta) + x0
        disk_height = R * height * (1 + (r / R) ** 0.5 * 0.3)
        if y0 == 0.0:
            pos[:, 1] = np.random.normal(0, 1, count) * disk_height
        else:
            pos[:, 1] = np.random.normal(0, 1, count) * disk_height + y0
        pos[:, 2] = r * np.sin(theta)
    speed = compute_rotation_curve(r, masses, G, softening)
    if spin > 0:  # counter-clockwise in the XZ plane
        vel[:, 0] = -speed * np.sin(theta)
        vel[:, 2] = speed * np.cos(theta)
    else:  # clockwise (second galaxy of "collision")
        vel[:, 0] = speed * np.sin(theta)
        vel[:, 2] = -speed * np.cos(theta)
    radial_factor = r / (r + softening * 2)
    sigma = speed * disp * radial_factor + np.sqrt(G * count * 0.00005)
    vel[:, 0] += np.random.normal(0, sigma, count)
    vel[:, 2] += np.random.normal(0, sigma, count)
    vel[:, 1] = np.random.normal(0, sigma * 0.25, count)


def _spiral_galaxy(pos, vel, masses, R, G, n):
    """Exponential disk whose bodies sit on 4 trailing log-spiral arms with a radius-dependent angular scatter;
    rotation curve floored at 0.7 of a point-mass speed.  Draw order: radii, arm index, arm scatter, height,
    then the three velocity dispersions."""
    softening = R * 0.03
    r = _soft_truncated_radii(n, R * 0.3, R * 1.0, R * 0.001)
    num_arms = 4
    base_theta = -np.log(r / (R * 0.02) + 1) / 0.35
    arm_offset = np.random.randint(0, num_arms, n) * (2 * np.pi / num_arms)
    theta = base_theta + arm_offset + np.random.normal(0, 0.12 + 0.15 * (r / R) ** 0.5, n)
    pos[:, 0] = r * np.cos(theta)
    pos[:, 2] = r * np.sin(theta)
    pos[:, 1] = np.random.normal(0, 1, n) * (R * 0.012 * (1 + (r / R) ** 0.5 * 0.3))
    speed = compute_rotation_curve(r, masses, G, softening)
    speed = np.maximum(speed, np.sqrt(G * (n * 0.001) / (r + softening)) * 0.7)
    phi = np.arctan2(pos[:, 2], pos[:, 0])  # tangential to the final position angle
    vel[:, 0] = -speed * np.sin(phi)
    vel[:, 2] = speed * np.cos(phi)
    sigma = speed * 0.10 * (r / (r + softening * 2)) + np.sqrt(G * n * 0.00005)
    vel[:, 0] += np.random.normal(0, sigma, n)
    vel[:, 2] += np.random.normal(0, sigma, n)
    vel[:, 1] = np.random.normal(0, sigma * 0.25, n)


FILAMENT_GRID = 8  # 8^3 candidate nodes over [-1.25 R, 1.25 R]^3


def _unit(v):
    return v / (np.linalg.norm(v) + 1e-10)


def _cosmic_web(pos, R, n):
    """Bodies in elongated clouds around a random 35 % of the 8^3 grid nodes; fills `pos`, returns the
    velocities (Hubble flow 0.05 x + N(0, 0.3), no centre-of-mass correction).  Draw order: node activity,
    node weights (power law a=2), one choice() over the active nodes, then per active node that received
    bodies: axis randn(3), axial offsets, perp randn(3), two perpendicular offset arrays."""
    g = FILAMENT_GRID
    spacing = R * 2.5 / g
    coords = np.linspace(-R * 1.25, R * 1.25, g)
    centers = np.stack(np.meshgrid(coords, coords, coords, indexing="ij"), axis=-1).reshape(-1, 3)
    active = centers[np.random.random(len(centers)) < 0.35]
    weights = np.random.power(2.0, len(active))
    weights /= weights.sum()
    node_of = np.random.choice(len(active), size=n, p=weights)
    for k in range(len(active)):
        members = np.flatnonzero(node_of == k)
        if members.size == 0:
            continue  # the reference skips this node's draws
        axis = _unit(np.random.randn(3))
        along = np.random.normal(0, spacing * 0.8, members.size)
        perp1 = np.random.randn(3)
        perp1 = _unit(perp1 - perp1.dot(axis) * axis)
        perp2 = _unit(np.cross(axis, perp1))
        across1 = np.random.normal(0, spacing * 0.12, members.size)
        across2 = np.random.normal(0, spacing * 0.12, members.size)
        pos[members] = (active[k] + along[:, None] * axis + across1[:, None] * perp1
                        + across2[:, None] * perp2)
    return pos * 0.05 + np.random.normal(0, 0.3, (n, 3))


def generate_distribution(distribution: str, n: int, R: float, G: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(positions (n,3), velocities (n,3), masses (n,)) float64; reference signature :91."""
    positions = np.zeros((n, 3), dtype=np.float64)
    velocities = np.zeros((n, 3), dtype=np.float64)
    masses = np.ones(n, dtype=np.float64)

    if distribution == "galaxy":  # reference :104-146
        _disk_galaxy(positions, velocities, masses, R, G, n, R * 0.3, R * 0.03, R * 1.0, 0.012, 0.12, +1)
        com_vel = np.sum(velocities * masses[:, np.newaxis], axis=0) / np.sum(masses)
        velocities -= com_vel

    elif distribution == "collision":  # reference :148-232
        half = n // 2
        n2 = n - half
        scale_length = R * 0.25
        softening = R * 0.025
        separation = (R * 0.5) * 3.5
        _disk_galaxy(positions[:half], velocities[:half], masses[:half], R, G, half, scale_length, softening,
                     R * 0.5, 0.01, 0.10, +1, x0=-separation / 2)
        _disk_galaxy(positions[half:], velocities[half:], masses[half:], R, G, n2, scale_length, softening,
                     R * 0.5, 0.01, 0.10, -1, x0=separation / 2, y0=R * 0.15)
        total_mass = n * 0.001
        collision_speed = np.sqrt(2 * G * total_mass / separation) * 0.6
        velocities[:half, 0] += collision_speed
        velocities[half:, 0] -= collision_speed

    elif distribution == "cluster":  # Plummer sphere, reference :350-397
        a = R * 0.3
        u = np.random.uniform(0, 1, n)
        r = a / np.sqrt(u ** (-2 / 3) - 1)
        r = np.clip(r, 0, R * 1.5)
        phi = np.random.uniform(0, 2 * np.pi, n)
        cos_theta = np.random.uniform(-1, 1, n)
        sin_theta = np.sqrt(1 - cos_theta ** 2)
        positions[:, 0] = r * sin_theta * np.cos(phi)
        positions[:, 1] = r * cos_theta
        positions[:, 2] = r * sin_theta * np.sin(phi)
        total_mass = n * 0.001
        r_a_sq = (r / a) ** 2
        sigma_sq = G * total_mass / (6 * a) * (1 + r_a_sq) ** (-0.5)
        sigma = np.sqrt(np.maximum(sigma_sq, G * total_mass / (6 * a) * 0.01))
        # The reference draws (|normal|, uniform, uniform) per body in a Python loop; the scalar
        # draws interleave, so the stream must be consumed body by body to match it.
        scale = sigma * np.sqrt(3)
        for i in range(n):
            v_mag = np.abs(np.random.normal(0, scale[i]))
            v_phi = np.random.uniform(0, 2 * np.pi)
            v_cos = np.random.uniform(-1, 1)
            v_sin = np.sqrt(1 - v_cos ** 2)
            velocities[i, 0] = v_mag * v_sin * np.cos(v_phi)
            velocities[i, 1] = v_mag * v_cos
            velocities[i, 2] = v_mag * v_sin * np.sin(v_phi)
        com_vel = np.sum(velocities * masses[:, np.newaxis], axis=0) / np.sum(masses)
        velocities -= com_vel

    elif distribution == "spiral":  # four trailing logarithmic arms, reference :234-295
        _spiral_galaxy(positions, velocities, masses, R, G, n)
        com_vel = np.sum(velocities * masses[:, np.newaxis], axis=0) / np.sum(masses)
        velocities -= com_vel

    elif distribution == "filament":  # cosmic web, reference :609-684
        velocities = _cosmic_web(positions, R, n)
        masses[:] = 0.1

    else:
        raise ValueError(f"distribution {distribution!r} is not part of this build "
                         f"(available: {sorted(DISTRIBUTIONS)})")
    return positions, velocities, masses


def generate_distribution_device(distribution: str, n: int, R: float, G: float, softening: float, damping: float = 1.0,
                                 theta: float = 0.5, seed: int = 42, device=None, integrator: str = "kick_drift",
                                 multipole: str = "monopole"):
    """generate_distribution + backend construction in one step, on the GPU: returns a
    HIPBarnesHutSimulation whose bodies were drawn on the device (nbmi_create_generated; Philox
    stream: statistical parity with generate_distribution, per-body parity with the host replay of that
    stream in tests/icgen_ref.py).  At 10 M bodies this replaces seconds of
    NumPy and a 640 MB upload by a few milliseconds."""
    from nbody.gpu_backend import HIPBarnesHutSimulation
    return HIPBarnesHutSimulation.generated(distribution, n, R, G, softening, damping, theta=theta, seed=seed,
                                            device=device, integrator=integrator, multipole=multipole)


def _preset(name, desc, cat, n, theta, G, eps, R, dist, frames, dtf, sub, fps, est):
    return {"name": name, "description": desc, "category": cat, "num_bodies": n, "theta": theta, "G": G,
            "softening": eps, "damping": 1.0, "spawn_radius": R, "distribution": dist, "total_frames": frames,
            "dt_per_frame": dtf, "substeps": sub, "target_fps": fps, "estimated_time": est}


# The presets BASELINE.json / SURVEY 8(d) name; constants as reference tools/presets.py
# :1774-1790, :1516-1532, :1552-1568, :1868-1884, :2424-2440.
PRESETS = {
    "quick_galaxy": _preset("Quick Galaxy", "Fast galaxy simulation for testing", "FAST", 100_000, 0.95, 0.15,
                            3.0, 500.0, "galaxy", 500, 0.2, 1, 30, "~25 seconds"),
    "4k_galaxy_1m": _preset("4K Galaxy 1M", "1 million body galaxy, ultra cinematic", "CINEMATIC_4K", 1_000_000,
                            0.5, 0.07, 1.5, 800.0, "galaxy", 3600, 0.05, 5, 60, "~11 hours"),
    "accurate_cluster": _preset("Globular Cluster", "Physically accurate globular cluster (Plummer model)",
                                "SCIENTIFIC", 200_000, 0.5, 0.05, 1.0, 300.0, "cluster", 2000, 0.08, 4, 24,
                                "~50 minutes"),
    "extreme_10m_collision": _preset("10 Million Collision", "Massive collision with 10M bodies", "EXTREME",
                                     10_000_000, 1.3, 0.08, 6.0, 2000.0, "collision", 500, 0.25, 1, 20,
                                     "~30 minutes"),
}


# The other 31 reference presets whose distribution this module generates, grouped as get_preset_list() orders
# them; constants as the reference's (where it defines a key twice, its later definition).
PRESETS.update({
    # TINY
    "demo_cluster": _preset("Demo Cluster", "Quick demo of cluster dynamics", "TINY",
            20_000, 0.95, 0.15, 3.0, 150.0, "cluster", 300, 0.2, 1, 30, "~5 seconds"),
    "tiny_collision": _preset("Tiny Collision", "Very small collision for testing", "TINY",
            15_000, 0.95, 0.25, 5.0, 250.0, "collision", 250, 0.3, 1, 30, "~5 seconds"),
    "tiny_galaxy": _preset("Tiny Galaxy", "Very small galaxy for testing", "TINY",
            10_000, 0.95, 0.2, 5.0, 200.0, "galaxy", 200, 0.3, 1, 30, "~3 seconds"),
    # FAST
    "mini_cluster": _preset("Mini Cluster", "Small dense star cluster", "FAST",
            50_000, 0.95, 0.2, 2.0, 200.0, "cluster", 400, 0.15, 1, 30, "~10 seconds"),
    "quick_collision": _preset("Quick Collision", "Fast collision simulation", "FAST",
            80_000, 0.95, 0.2, 3.5, 400.0, "collision", 600, 0.25, 1, 30, "~25 seconds"),
    # CINEMATIC
    "collision_majesty": _preset("Galactic Collision", "Two massive galaxies colliding, Andromeda-style", "CINEMATIC",
            400_000, 0.75, 0.12, 2.0, 700.0, "collision", 4000, 0.15, 3, 24, "~1 hour"),
    "galaxy_epic": _preset("Epic Galaxy", "Massive spiral galaxy, cinematic quality", "CINEMATIC",
            500_000, 0.7, 0.1, 2.5, 600.0, "galaxy", 3000, 0.12, 3, 24, "~1 hour"),
    "spiral_milkyway": _preset("Milky Way Spiral", "Four-arm spiral galaxy like our Milky Way", "CINEMATIC",
            300_000, 0.8, 0.08, 2.0, 600.0, "spiral", 2500, 0.1, 3, 24, "~30 minutes"),
    # CINEMATIC_4K
    "4k_cluster_300k": _preset("4K Globular Cluster", "Dense star cluster, ultra accurate physics", "CINEMATIC_4K",
            300_000, 0.4, 0.05, 1.0, 300.0, "cluster", 3600, 0.04, 6, 60, "~6 hours"),
    "4k_collision_1m": _preset("4K Collision 1M", "Epic 1M body collision, production quality", "CINEMATIC_4K",
            1_000_000, 0.5, 0.08, 1.5, 900.0, "collision", 6000, 0.06, 5, 60, "~18 hours"),
    "4k_collision_500k": _preset("4K Collision 500K",
                   "Two galaxies colliding, 4K 60fps, high accuracy", "CINEMATIC_4K",
            500_000, 0.5, 0.1, 1.5, 700.0, "collision", 6000, 0.06, 5, 60, "~9 hours"),
    "4k_collision_epic": _preset("4K Collision Epic", "3-minute collision drama at 60fps", "CINEMATIC_4K",
            600_000, 0.55, 0.09, 1.5, 800.0, "collision", 10_800, 0.06, 4, 60, "~12 hours"),
    "4k_galaxy_500k": _preset("4K Galaxy 500K", "500K body galaxy, 4K 60fps quality, high accuracy", "CINEMATIC_4K",
            500_000, 0.5, 0.08, 1.5, 600.0, "galaxy", 3600, 0.05, 5, 60, "~5 hours"),
    "4k_galaxy_long": _preset("4K Galaxy Long", "Extended 2-minute galaxy evolution at 60fps", "CINEMATIC_4K",
            500_000, 0.55, 0.07, 1.5, 650.0, "galaxy", 7200, 0.05, 4, 60, "~7 hours"),
    "4k_spiral_1m": _preset("4K Spiral 1M", "Stunning 1M body spiral, ultra smooth", "CINEMATIC_4K",
            1_000_000, 0.5, 0.05, 1.5, 850.0, "spiral", 3600, 0.05, 5, 60, "~11 hours"),
    "4k_spiral_500k": _preset("4K Spiral 500K", "Multi-arm spiral galaxy, 4K 60fps", "CINEMATIC_4K",
            500_000, 0.5, 0.06, 1.5, 650.0, "spiral", 3600, 0.05, 5, 60, "~5 hours"),
    # ARTISTIC
    "cosmic_web": _preset("Cosmic Web", "Large-scale structure of the universe (needs millions)", "ARTISTIC",
            500_000, 0.95, 0.02, 5.0, 1200.0, "filament", 800, 0.3, 1, 24, "~5 minutes"),
    # MEGA
    "mega_collision": _preset("Mega Collision", "Two 500K body galaxies colliding", "MEGA",
            1_000_000, 0.95, 0.12, 3.5, 1000.0, "collision", 3000, 0.15, 2, 24, "~1 hour"),
    "million_stars": _preset("Million Star Galaxy", "Massive 1M body galaxy (very long render)", "MEGA",
            1_000_000, 0.95, 0.1, 3.0, 800.0, "galaxy", 2000, 0.15, 2, 24, "~40 minutes"),
    # EXTREME
    "extreme_10m_galaxy": _preset("10 Million Star Galaxy", "Ultra-massive galaxy with 10M bodies", "EXTREME",
            10_000_000, 1.3, 0.06, 6.0, 1600.0, "galaxy", 500, 0.25, 1, 20, "~30 minutes"),
    "extreme_10m_web": _preset("10 Million Cosmic Web", "Large cosmic web with filaments and voids", "EXTREME",
            10_000_000, 1.3, 0.02, 10.0, 3000.0, "filament", 500, 0.35, 1, 20, "~30 minutes"),
    "extreme_20m_galaxy": _preset("20 Million Star Galaxy", "Hyper-massive galaxy with 20M bodies", "EXTREME",
            20_000_000, 1.4, 0.05, 8.0, 2000.0, "galaxy", 500, 0.3, 1, 20, "~1 hour"),
    "extreme_20m_spiral": _preset("20 Million Spiral", "Mega spiral galaxy with 20M stars", "EXTREME",
            20_000_000, 1.4, 0.04, 8.0, 2200.0, "spiral", 500, 0.3, 1, 20, "~1 hour"),
    "extreme_20m_web": _preset("20 Million Cosmic Web", "Massive cosmic web structure", "EXTREME",
            20_000_000, 1.4, 0.015, 12.0, 4000.0, "filament", 500, 0.4, 1, 20, "~1 hour"),
    "extreme_50m_collision": _preset("50 Million Collision", "Ultimate collision with 50M bodies", "EXTREME",
            50_000_000, 1.5, 0.05, 10.0, 3500.0, "collision", 500, 0.35, 1, 20, "~2 hours"),
    "extreme_50m_galaxy": _preset("50 Million Star Galaxy", "Insane 50M body galaxy - multi-day render", "EXTREME",
            50_000_000, 1.5, 0.04, 10.0, 3000.0, "galaxy", 500, 0.35, 1, 20, "~2 hours"),
    "extreme_50m_web": _preset("50 Million Cosmic Web",
                   "Ultimate cosmic web - CMB-like large scale structure", "EXTREME",
            50_000_000, 1.5, 0.01, 15.0, 5000.0, "filament", 500, 0.4, 1, 20, "~2 hours"),
    "extreme_5m_collision": _preset("5 Million Collision", "Epic collision with 5M bodies", "EXTREME",
            5_000_000, 1.2, 0.1, 5.0, 1500.0, "collision", 500, 0.2, 1, 20, "~17 minutes"),
    "extreme_5m_galaxy": _preset("5 Million Star Galaxy",
                   "Massive galaxy with 5M bodies, approximate physics", "EXTREME",
            5_000_000, 1.2, 0.08, 5.0, 1200.0, "galaxy", 500, 0.2, 1, 20, "~17 minutes"),
    "extreme_5m_spiral": _preset("5 Million Spiral", "Gigantic spiral galaxy with 5M stars", "EXTREME",
            5_000_000, 1.2, 0.06, 5.0, 1400.0, "spiral", 500, 0.2, 1, 20, "~17 minutes"),
    "extreme_5m_web": _preset("5 Million Cosmic Web", "Cosmic web with clear filamentary structure", "EXTREME",
            5_000_000, 1.2, 0.025, 8.0, 2500.0, "filament", 500, 0.35, 1, 20, "~17 minutes"),
})

# get_preset_list()'s category order (reference :2649-2657); unknown categories sort last
CATEGORY_ORDER = ["TINY", "FAST", "CINEMATIC", "CINEMATIC_4K", "ARTISTIC", "SCIENTIFIC", "CHAOS", "MEGA", "EXTREME"]


def get_preset_list() -> List[Tuple[str, dict]]:
    """(key, preset) pairs by category (CATEGORY_ORDER), then key: the reference's menu order."""
    def rank(item):
        cat = item[1]["category"]
        return (CATEGORY_ORDER.index(cat) if cat in CATEGORY_ORDER else 99, item[0])
    return sorted(PRESETS.items(), key=rank)


def get_preset_by_index(index: int) -> Tuple[str, dict]:
    """Entry `index` of get_preset_list(); (None, None) out of range."""
    presets = get_preset_list()
    if 0 <= index < len(presets):
        return presets[index]
    return None, None


def list_distributions():
    """Print the distributions this build generates."""
    print("\nAvailable spawn distributions:")
    print("-" * 40)
    for name, desc in DISTRIBUTIONS.items():
        print(f"  {name:<15} - {desc}")


def get_preset_config(key: str) -> dict:
    """Preset dict + ``session_name`` (reference :2701-2709); None for unknown keys."""
    if key not in PRESETS:
        return None
    preset = PRESETS[key].copy()
    preset["session_name"] = key
    return preset
