"""Writes tests/golden/export_camera.npz: eye position and up vector of the reference exporter's ExportCamera for
every camera mode, over several configurations, frame counts and frame indices.  tests/test_render_host.py checks
tools.export.ExportCamera against it.

    python scripts/gen_export_camera_golden.py --reference <checkout of the reference project>

The reference's camera module is imported from that checkout at run time; nothing of it is copied.  Its exporter
imports the reference's tools.record, which needs the `zstandard` package at import time: an empty stand-in module
is enough, the camera never compresses anything (its GL imports sit inside methods that are not called).
"""
import argparse
import os
import sys
import types

import numpy as np

MODES = ("fixed", "orbit", "spiral", "zoom", "zoomout", "zoomin", "cinematic", "flyby", "topdown")
CONFIGS = [  # (speed, radius, phi, theta)
    (0.3, 800.0, 25.0, 45.0),
    (1.7, 350.0, -40.0, 10.0),
    (0.05, 2500.0, 95.0, 300.0),
]
TOTALS = (1, 2, 7, 120)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("-o", "--output", default=os.path.join(os.path.dirname(__file__), "..", "tests", "golden",
                                                           "export_camera.npz"))
    a = ap.parse_args()
    sys.modules.setdefault("zstandard", types.ModuleType("zstandard"))
    sys.path.insert(0, os.path.abspath(a.reference))
    from tools.export import ExportCamera, ExportConfig  # the reference's

    rows = []
    for m, mode in enumerate(MODES):
        for k, (speed, radius, phi, theta) in enumerate(CONFIGS):
            for total in TOTALS:
                idxs = sorted({0, 1, total // 2, total - 1, total + 3} & set(range(total + 4)))
                for i in idxs:
                    cfg = ExportConfig()
                    cfg.camera_mode = mode
                    cfg.camera_rotation_speed = speed
                    cfg.camera_radius = radius
                    cfg.camera_initial_phi = phi
                    cfg.camera_initial_theta = theta
                    cam = ExportCamera(cfg)
                    cam.update(i, total)
                    eye = np.asarray(cam.get_position(), dtype=np.float64)
                    up = np.asarray(cam.get_up_vector(), dtype=np.float64)
                    rows.append((m, k, total, i, *eye, *up))
    arr = np.array(rows, dtype=np.float64)
    np.savez(a.output, modes=np.array(MODES), configs=np.array(CONFIGS, dtype=np.float64),
             mode=arr[:, 0].astype(np.int32), config=arr[:, 1].astype(np.int32), total=arr[:, 2].astype(np.int32),
             index=arr[:, 3].astype(np.int32), eye=arr[:, 4:7], up=arr[:, 7:10])
    print(f"{a.output}: {len(rows)} camera states")


if __name__ == "__main__":
    main()
