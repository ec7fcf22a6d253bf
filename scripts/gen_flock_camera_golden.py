"""Writes tests/golden/flock_camera.npz: position, axes and look-at point of the reference's orbital Camera
(core/camera.py) for a dozen (theta, phi, radius), negative radius and |phi| = 89 included, plus the state after a
few rotate() calls.  tests/test_raster_host.py checks boids.render.OrbitCamera against it.

    python scripts/gen_flock_camera_golden.py --reference <checkout of the reference project>

The reference's camera module is loaded from that checkout at run time under stand-in `OpenGL.GL` / `OpenGL.GLU`
modules (its GL calls sit in apply(), which is not called; the look-at rule of apply() is restated here from its two
branches); nothing of it is copied.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

STATES = [  # (theta, phi, radius)
    (45.0, 25.0, 120.0), (45.0, 25.0, 20.0), (45.0, 25.0, 5.0), (0.0, 0.0, 100.0), (90.0, 0.0, 250.0),
    (180.0, -35.0, 60.0), (300.0, 60.0, 1500.0), (10.0, 89.0, 80.0), (200.0, -89.0, 80.0), (45.0, 25.0, -50.0),
    (135.0, -10.0, -300.0), (359.5, 12.5, 0.0),
]
ROTATIONS = [(10.0, 5.0), (350.0, 80.0), (-30.0, -200.0), (0.3, 0.0)]  # applied in turn from the reference's initial state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("-o", "--output", default=os.path.join(os.path.dirname(__file__), "..", "tests", "golden",
                                                           "flock_camera.npz"))
    a = ap.parse_args()
    ref = os.path.abspath(a.reference)
    for name in ("OpenGL", "OpenGL.GL", "OpenGL.GLU"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, ref)
    spec = importlib.util.spec_from_file_location("reference_camera", os.path.join(ref, "core", "camera.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    rows = []
    for theta, phi, radius in STATES:
        cam = mod.Camera()
        cam.theta, cam.phi, cam.radius = theta, phi, radius
        pos, direction = cam.get_position(), cam.get_direction()
        forward, right, up = cam.get_camera_axes()
        look = cam.target if cam.radius >= 0 else pos - direction * 10
        rows.append(np.concatenate([pos, direction, forward, right, up, look]))
    cam = mod.Camera()
    initial = (cam.theta, cam.phi, cam.radius)
    rotated = []
    for d_theta, d_phi in ROTATIONS:
        cam.rotate(d_theta, d_phi)
        rotated.append((cam.theta, cam.phi))
    arr = np.array(rows, dtype=np.float64)
    np.savez(a.output, states=np.array(STATES, dtype=np.float64), position=arr[:, 0:3], direction=arr[:, 3:6],
             forward=arr[:, 6:9], right=arr[:, 9:12], up=arr[:, 12:15], look_at=arr[:, 15:18],
             initial=np.array(initial, dtype=np.float64), rotations=np.array(ROTATIONS, dtype=np.float64),
             rotated=np.array(rotated, dtype=np.float64))
    print(f"{a.output}: {len(rows)} camera states, {len(rotated)} rotations")


if __name__ == "__main__":
    main()
