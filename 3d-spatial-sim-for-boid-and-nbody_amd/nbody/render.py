"""Headless point renderer on the device (csrc/render.hip behind the nbmi_render_* C ABI).

The image is the one the reference exporter's fixed-function GL pass draws (smooth points, additive blending, depth
test, EXP2 fog), with every implementation-defined detail fixed in include/nbmi.h so that a frame is the same bytes
on every run.  No GL context, display or window system is needed.

    r = HIPPointRenderer(1920, 1080)
    img = r.render(positions, colors, eye=(800, 300, 0))     # uint8 (H, W, 3), row 0 at the top
    img = r.render_sim(sim, eye=(800, 300, 0))               # a live handle's bodies, read on the device
"""
import os

import numpy as np

import nbmi_native as _nat

PARAM_COUNT = 17
DEFAULTS = dict(target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovy=75.0, near=0.1, far=10000.0, point_size=1.5,
                fog_density=0.0003, bg=(0.0, 0.0, 0.02))


def render_params(eye, target=DEFAULTS["target"], up=DEFAULTS["up"], fovy=DEFAULTS["fovy"], near=DEFAULTS["near"],
                  far=DEFAULTS["far"], point_size=DEFAULTS["point_size"], fog_density=DEFAULTS["fog_density"],
                  bg=DEFAULTS["bg"]):
    """The 17 doubles of nbmi_render_points: eye, target, up, fovy, near, far, point_size, fog_density, bg.
    Defaults are the reference exporter's (gluPerspective(75, W/H, 0.1, 10000), point size 1.5, fog 0.0003,
    background (0, 0, 0.02))."""
    p = np.empty(PARAM_COUNT, dtype=np.float64)
    p[0:3] = np.asarray(eye, dtype=np.float64).reshape(3)
    p[3:6] = np.asarray(target, dtype=np.float64).reshape(3)
    p[6:9] = np.asarray(up, dtype=np.float64).reshape(3)
    p[9:14] = (fovy, near, far, point_size, fog_density)
    p[14:17] = np.asarray(bg, dtype=np.float64).reshape(3)
    return p


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
    return render_params(**kw)


class HIPPointRenderer:
    """One renderer per output size.  Owns a HIP stream, its device buffers and a pinned image buffer."""

    def __init__(self, width, height, device=None):
        lib = _nat.load()
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0")) % max(1, _nat.device_count())
        self.width, self.height, self.device = int(width), int(height), int(device)
        self._lib = lib
        self._h = lib.nbmi_render_create(self.width, self.height, self.device)
        if not self._h:
            raise RuntimeError(f"nbmi_render_create failed: {_nat.last_error()}")

    def _out(self, out):
        shape = (self.height, self.width, 3)
        if out is None:
            return np.empty(shape, dtype=np.uint8)
        if out.shape != shape or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous uint8 array of shape {shape}")
        return out

    def render(self, positions, colors, params=None, out=None, **camera):
        """positions, colors: (N, 3) float32 in draw order.  Camera / shading either as `params` (render_params())
        or as keywords of render_params (eye=... required).  Returns uint8 (H, W, 3) RGB, row 0 at the top."""
        p = _params(params, camera)
        pos = np.ascontiguousarray(positions, dtype=np.float32)
        col = np.ascontiguousarray(colors, dtype=np.float32)
        if pos.ndim != 2 or pos.shape[1:] != (3,) or col.shape != pos.shape:
            raise ValueError(f"positions and colors must both be (N, 3), got {pos.shape} and {col.shape}")
        img = self._out(out)
        _nat.check(self._lib.nbmi_render_points(self._h, _nat.ptr(pos), _nat.ptr(col), len(pos), _nat.ptr(p),
                                                _nat.ptr(img)), "nbmi_render_points")
        return img

    def render_sim(self, sim, params=None, out=None, **camera):
        """The bodies of a live simulation handle (current positions, colours of its last compute_colors), read on
        the device: nothing but the image crosses PCIe."""
        p = _params(params, camera)
        img = self._out(out)
        _nat.check(self._lib.nbmi_render_sim(self._h, sim._h, _nat.ptr(p), _nat.ptr(img)), "nbmi_render_sim")
        return img

    def stats(self):
        """Of the last frame: points drawn (inside the clip volume), fragments, passing fragments, pixels touched."""
        s = np.zeros(4, dtype=np.int64)
        _nat.check(self._lib.nbmi_render_stats(self._h, _nat.ptr(s)), "nbmi_render_stats")
        return dict(zip(("drawn", "fragments", "passing", "pixels"), (int(x) for x in s)))

    def timers(self):
        """Device milliseconds of the last frame per phase."""
        t = np.zeros(4, dtype=np.float64)
        _nat.check(self._lib.nbmi_render_timers(self._h, _nat.ptr(t)), "nbmi_render_timers")
        return dict(zip(("project_ms", "sort_ms", "resolve_ms", "pack_ms"), t.tolist()))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.nbmi_render_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


__all__ = ["HIPPointRenderer", "render_params", "DEFAULTS", "PARAM_COUNT"]
