"""Boids constants, values as reference config/boids.py:30-46."""

WINDOW = {"width": 1280, "height": 720}

CAMERA = {
    "fov": 90.0,
    "near_clip": 0.1,
    "far_clip": 1000.0,
    "initial_radius": 120.0,
    "initial_theta": 45.0,
    "initial_phi": 25.0,
    "min_phi": -89.0,
    "max_phi": 89.0,
}

COLORS = {"background": (0.01, 0.01, 0.02, 1.0)}

BOIDS = {
    "count": 500000,
    "bounds": 500.0,
    "max_speed": 25.0,
    "max_force": 60.0,
    "size": 1.2,
    "wall_margin": 3.0,
    "wall_weight": 10.0,
    "perception_radius": 5.0,
    "separation_radius": 3.0,
    "separation_weight": 2.5,
    "alignment_weight": 1.0,
    "cohesion_weight": 1.0,
    "color_blend_rate": 1.0,
}

# order in which the C ABI takes them (include/bdmi.h)
PARAM_ORDER = ("bounds", "wall_margin", "wall_weight", "max_speed", "max_force", "perception_radius",
               "separation_radius", "separation_weight", "alignment_weight", "cohesion_weight",
               "color_blend_rate")
