"""Headless flock renderer on the device (csrc/raster.hip behind bdmi_render_triangles / bdmi_render_flock).

The image is the one the reference's fixed-function GL pass draws for a flock (opaque flat-coloured triangles, depth
test, linear fog towards the clear colour), with every implementation-defined detail fixed in include/bdmi.h so that
a frame is the same bytes on every run.  No GL context, display or window system is needed; the reference's
wireframe cube and HUD text are not drawn.

    flock = Flock(500_000, seed=1)
    cam = OrbitCamera()
    with HIPFlockRenderer(1280, 720) as r:
        flock.update(1 / 60)
        img = r.render_flock(flock, cam)                       # uint8 (H, W, 3), row 0 at the top
        img = r.render_triangles(vertices, colors, eye=(80, 50, 80))
"""
import ctypes as C
import math

import numpy as np

import nbmi_native as _nat
from config import boids as config
from nbody.render import PARAM_COUNT, HIPPointRenderer

_CAM = config.CAMERA
DEFAULTS = dict(target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovy=_CAM["fov"], near=_CAM["near_clip"],
                far=_CAM["far_clip"], fog_start=50.0, fog_end=_CAM["far_clip"] * 0.8,
                bg=tuple(config.COLORS["background"][:3]))


def flock_render_params(eye, target=DEFAULTS["target"], up=DEFAULTS["up"], fovy=DEFAULTS["fovy"], near=DEFAULTS["near"],
                        far=DEFAULTS["far"], fog_start=DEFAULTS["fog_start"], fog_end=DEFAULTS["fog_end"],
                        bg=DEFAULTS["bg"]):
    """The 17 doubles of bdmi_render_triangles: eye, target, up, fovy, near, far, fog_start, fog_end, bg.  Defaults
    are the reference application's (gluPerspective(90, W/H, 0.1, 1000), linear fog 50 .. 800 towards the clear colour
    (0.01, 0.01, 0.02))."""
    p = np.empty(PARAM_COUNT, dtype=np.float64)
    p[0:3] = np.asarray(eye, dtype=np.float64).reshape(3)
    p[3:6] = np.asarray(target, dtype=np.float64).reshape(3)
    p[6:9] = np.asarray(up, dtype=np.float64).reshape(3)
    p[9:14] = (fovy, near, far, fog_start, fog_end)
    p[14:17] = np.asarray(bg, dtype=np.float64).reshape(3)
    return p


class OrbitCamera:
    """The reference's orbital camera (core/camera.py): a point on a sphere of `radius` around `target`, at azimuth
    `theta` and elevation `phi` in degrees, looking at the target.  A negative radius puts the camera on the far side
    looking outwards, as the reference's apply() does."""

    def __init__(self, theta=None, phi=None, radius=None, target=(0.0, 0.0, 0.0)):
        self.theta = float(_CAM["initial_theta"] if theta is None else theta)
        self.phi = float(_CAM["initial_phi"] if phi is None else phi)
        self.radius = float(_CAM["initial_radius"] if radius is None else radius)
        self.target = np.asarray(target, dtype=np.float64).reshape(3)

    def get_direction(self):
        """Unit vector from the target towards the camera."""
        th, ph = math.radians(self.theta), math.radians(self.phi)
        return np.array([math.cos(ph) * math.cos(th), math.sin(ph), math.cos(ph) * math.sin(th)])

    def get_position(self):
        return self.radius * self.get_direction()

    def get_camera_axes(self):
        """(forward, right, up): forward points from the camera along -direction; right falls back to +x when forward
        is within 0.001 of the world's up axis."""
        forward = -self.get_direction()
        right = np.cross(forward, np.array([0.0, 1.0, 0.0]))
        length = np.linalg.norm(right)
        right = np.array([1.0, 0.0, 0.0]) if length < 0.001 else right / length
        up = np.cross(right, forward)
        return forward, right, up / np.linalg.norm(up)

    def rotate(self, d_theta, d_phi=0.0):
        self.theta = (self.theta + d_theta) % 360
        self.phi = max(_CAM["min_phi"], min(_CAM["max_phi"], self.phi + d_phi))

    def look_at(self):
        """The point gluLookAt is aimed at: the target, or 10 units beyond the camera when the radius is negative."""
        if self.radius >= 0:
            return self.target
        return self.get_position() - self.get_direction() * 10

    def view(self):
        """eye / target / up of the frame (the reference passes (0, 1, 0) as up)."""
        return dict(eye=self.get_position(), target=self.look_at(), up=(0.0, 1.0, 0.0))

    def frustum(self, flock, fov, aspect):
        """What the visibility test takes: cam12 = {position, forward, right, up} and (tan_h, tan_v) derived as
        Flock.visible_vertices derives them."""
        cam12 = np.ascontiguousarray(np.concatenate([self.get_position(), *self.get_camera_axes()]), dtype=np.float64)
        tan_h, tan_v = flock.frustum_tangents(fov, aspect)
        return cam12, tan_h, tan_v


def _params(params, kw):
    if params is not None:
        if kw:
            raise TypeError("pass either params or keyword camera settings, not both")
        p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1)
        if p.size != PARAM_COUNT:
            raise ValueError(f"params must hold {PARAM_COUNT} values, got {p.size}")
        return p
    if "eye" not in kw:
        raise TypeError("render needs params or eye=...")
    return flock_render_params(**kw)


class HIPFlockRenderer(HIPPointRenderer):
    """One renderer per output size (the nbmi_render handle of the point renderer; its z-buffer is allocated at the
    first triangle frame).  stats() after a triangle frame: triangles drawn, fragments, winning fragments, pixels
    with a fragment; timers(): project + rasterise in project_ms, 0 in sort_ms, resolve_ms, copy in pack_ms."""

    def render_triangles(self, vertices, colors, params=None, out=None, **camera):
        """vertices, colors: (3T, 3) float32, triangle t = rows 3t .. 3t+2, flat-coloured by its first colour row.
        Camera / shading either as `params` (flock_render_params()) or as its keywords (eye=... required)."""
        p = _params(params, camera)
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        c = np.ascontiguousarray(colors, dtype=np.float32)
        if v.ndim != 2 or v.shape[1:] != (3,) or c.shape != v.shape or len(v) % 3:
            raise ValueError(f"vertices and colors must both be (3T, 3), got {v.shape} and {c.shape}")
        img = self._out(out)
        _nat.check(self._lib.bdmi_render_triangles(self._h, _nat.ptr(v), _nat.ptr(c), len(v) // 3, _nat.ptr(p),
                                                   _nat.ptr(img)), "bdmi_render_triangles")
        return img

    def render_flock(self, flock, camera, out=None, **shading):
        """The frame Flock.draw would put on the screen for an OrbitCamera: frustum test, cone building and
        rasterisation on the device, only the image crosses PCIe.  `shading` overrides flock_render_params keywords
        (fovy, near, far, fog_start, fog_end, bg).  Sets flock._visible_count."""
        kw = dict(camera.view())
        kw.update(shading)
        p = flock_render_params(**kw)
        cam12, tan_h, tan_v = camera.frustum(flock, float(p[9]), self.width / self.height)
        img = self._out(out)
        cnt = C.c_int64(0)
        _nat.check(self._lib.bdmi_render_flock(self._h, flock._h, _nat.ptr(cam12), tan_h, tan_v, float(flock.fog_end),
                                               float(flock.cone_length), float(flock.cone_radius), _nat.ptr(p),
                                               _nat.ptr(img), C.addressof(cnt)), "bdmi_render_flock")
        flock._visible_count = int(cnt.value)
        return img


__all__ = ["HIPFlockRenderer", "OrbitCamera", "flock_render_params", "DEFAULTS"]
