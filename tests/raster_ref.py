"""NumPy restatement of the flock frame defined in include/bdmi.h ("Image semantics of a flock frame").

Float64 in the order the header writes it, exact int64 edge functions.  The triangle set-up is vectorised over all
triangles; fragments are generated for batches of triangles that share a box size class (small boxes: thousands of
triangles at once; large boxes: one triangle over its whole box); the resolve pass is vectorised over the winning pixels.
"""
import math

import numpy as np

SUB = 16
GUARD = float(1 << 20)
DMAX = (1 << 24) - 1
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
_BATCH_ELEMS = 1 << 21


def make_params(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovy=90.0, near=0.1, far=1000.0, fog_start=50.0,
                fog_end=800.0, bg=(0.01, 0.01, 0.02)):
    return np.array([*eye, *target, *up, fovy, near, far, fog_start, fog_end, *bg], dtype=np.float64)


NO_FOG = dict(fog_start=1e9, fog_end=2e9)


def view_constants(params, W, H):
    eye, target, up = params[0:3], params[3:6], params[6:9]
    fovy, near, far = (float(x) for x in params[9:12])

    def norm(a):
        return a / math.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])

    f = norm(target - eye)
    s = norm(cross(f, up))
    u = cross(s, f)
    cot = 1.0 / math.tan(fovy * math.pi / 360.0)
    aspect = W / H
    za = (far + near) / (near - far)
    zb = 2.0 * far * near / (near - far)
    return f, s, u, cot, aspect, za, zb


def _dot(a, e):
    return (a[0] * e[..., 0] + a[1] * e[..., 1]) + a[2] * e[..., 2]


class Setup:
    """Per-triangle quantities of every triangle that is not discarded (index arrays into the input rows)."""

    def __init__(self, verts, W, H, params):
        near = params[10]
        f, s, u, cot, aspect, za, zb = view_constants(params, W, H)
        v32 = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3, 3)
        p = v32.astype(np.float64)
        with np.errstate(all="ignore"):
            e = p - params[0:3]
            xe, ye, ze = _dot(s, e), _dot(u, e), -_dot(f, e)
            xc, yc, zc, wc = (cot / aspect) * xe, cot * ye, za * ze + zb, -ze
            ok = np.isfinite(p).all(axis=(1, 2)) & (wc >= near).all(axis=1) & (zc <= wc).all(axis=1)
            xw = (xc / wc) * (W / 2) + W / 2
            yw = (yc / wc) * (H / 2) + H / 2
            ok &= (np.abs(xw) <= GUARD).all(axis=1) & (np.abs(yw) <= GUARD).all(axis=1)
            zn = zc / wc
        t = np.nonzero(ok)[0]
        xw, yw, zn, wc = xw[t], yw[t], zn[t], wc[t]
        X = np.floor(xw * SUB + 0.5).astype(np.int64)
        Y = np.floor(yw * SUB + 0.5).astype(np.int64)
        area2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
        keep = area2 != 0
        t, X, Y, zn, wc, area2 = t[keep], X[keep], Y[keep], zn[keep], wc[keep], area2[keep]
        flip = area2 < 0
        order = np.where(flip[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))
        rows = np.arange(len(t))[:, None]
        self.t = t
        self.X, self.Y, self.zn, self.w = X[rows, order], Y[rows, order], zn[rows, order], wc[rows, order]
        self.area2 = np.abs(area2)
        half = SUB // 2
        self.i0 = np.maximum(0, -((-(self.X.min(axis=1) - half)) // SUB))     # ceil((Xmin - 8) / 16)
        self.i1 = np.minimum(W - 1, (self.X.max(axis=1) - half) // SUB)        # floor((Xmax - 8) / 16)
        self.j0 = np.maximum(0, -((-(self.Y.min(axis=1) - half)) // SUB))
        self.j1 = np.minimum(H - 1, (self.Y.max(axis=1) - half) // SUB)

    def edges(self, k, PX, PY):
        """E_0, E_1, E_2 and coverage of the set-up rows k at the sample points (PX, PY) (broadcast against k)."""
        E, inside = [], True
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            dx, dy = self.X[k, c] - self.X[k, b], self.Y[k, c] - self.Y[k, b]
            shape = (-1,) + (1,) * (np.ndim(PX) - 1)
            dx, dy = dx.reshape(shape), dy.reshape(shape)
            Ea = dx * (PY - self.Y[k, b].reshape(shape)) - dy * (PX - self.X[k, b].reshape(shape))
            owns = (dy < 0) | ((dy == 0) & (dx > 0))
            inside = inside & ((Ea > 0) | ((Ea == 0) & owns))
            E.append(Ea)
        return E, inside

    def lambdas(self, k, E):
        a2 = self.area2[k].astype(np.float64).reshape((-1,) + (1,) * (E[0].ndim - 1))
        return [Ea.astype(np.float64) / a2 for Ea in E]


def _fragments(S, k, side_x, side_y, W):
    """Fragments of the set-up rows k on a side_y x side_x grid of pixels from each box's corner:
    (pixel index, z-buffer word) arrays."""
    oi = np.arange(side_x, dtype=np.int64)[None, None, :]
    oj = np.arange(side_y, dtype=np.int64)[None, :, None]
    i = S.i0[k][:, None, None] + oi
    j = S.j0[k][:, None, None] + oj
    inbox = (i <= S.i1[k][:, None, None]) & (j <= S.j1[k][:, None, None])
    E, inside = S.edges(k, i * SUB + SUB // 2, j * SUB + SUB // 2)
    inside = inside & inbox
    lam = S.lambdas(k, E)
    zn = S.zn[k]
    zf = (lam[0] * zn[:, 0, None, None] + lam[1] * zn[:, 1, None, None]) + lam[2] * zn[:, 2, None, None]
    d = np.floor((zf * 0.5 + 0.5) * DMAX + 0.5)
    ok = inside & (d >= 0) & (d < DMAX)
    tt = np.broadcast_to(S.t[k][:, None, None], ok.shape)[ok].astype(np.uint64)
    word = (d[ok].astype(np.uint64) << np.uint64(32)) | tt
    pix = (j * W + i)[ok]
    return pix, word


def raster_ref(verts, cols, W, H, params, buffers=False):
    """verts, cols: (3T, 3) float32.  Returns (image uint8 (H, W, 3), [drawn, fragments, pixels], per-pixel fragment
    count int64 (H, W) in WINDOW rows: row j of the count is image row H - 1 - j).  buffers=True appends the depth
    buffer and the winning triangle per pixel (int64 (H, W), window rows; 2^24 - 1 and -1 where nothing was drawn)."""
    params = np.asarray(params, dtype=np.float64)
    fog_start, fog_end = params[12], params[13]
    bg = params[14:17]
    cols = np.ascontiguousarray(cols, dtype=np.float32).reshape(-1, 3)
    S = Setup(verts, W, H, params)
    zbuf = np.full(W * H, EMPTY, dtype=np.uint64)
    cover = np.zeros(W * H, dtype=np.int64)
    bw, bh = S.i1 - S.i0 + 1, S.j1 - S.j0 + 1
    live = np.nonzero((bw > 0) & (bh > 0))[0]
    frags = 0
    if len(live):
        side = np.maximum(bw[live], bh[live])
        cls = np.ceil(np.log2(side)).astype(np.int64)  # box fits a 2^cls square
        for c in np.unique(cls):
            ks = live[cls == c]
            n = 1 << int(c)
            if n * n * 4 <= _BATCH_ELEMS:  # many triangles per batch, square grid
                per = max(1, _BATCH_ELEMS // (n * n))
                groups = [(ks[a:a + per], n, n) for a in range(0, len(ks), per)]
            else:  # one triangle at a time over its own box, in bands of rows
                groups = []
                for k in ks:
                    rows = max(1, _BATCH_ELEMS // int(bw[k]))
                    groups.append((np.array([k]), int(bw[k]), int(bh[k]), rows))
            for g in groups:
                if len(g) == 3:
                    pix, word = _fragments(S, g[0], g[1], g[2], W)
                    np.minimum.at(zbuf, pix, word)
                else:
                    k, sx, sy, rows = g
                    j0 = S.j0[k].copy()
                    parts = []
                    for r0 in range(0, sy, rows):  # bands: shift the box corner, keep j1
                        S.j0[k] = j0 + r0
                        parts.append(_fragments(S, k, sx, min(rows, sy - r0), W))
                    S.j0[k] = j0
                    pix = np.concatenate([p[0] for p in parts])
                    word = np.concatenate([p[1] for p in parts])
                    zbuf[pix] = np.minimum(zbuf[pix], word)  # one triangle: every pixel at most once
                frags += len(pix)
                cover += np.bincount(pix, minlength=W * H)
    img = np.empty((H, W, 3), dtype=np.uint8)
    img[:] = np.floor(bg * 255 + 0.5).astype(np.uint8)
    pix = np.nonzero(zbuf != EMPTY)[0]
    if len(pix):
        t = (zbuf[pix] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        k = np.searchsorted(S.t, t)
        i, j = pix % W, pix // W
        E, _ = S.edges(k, i * SUB + SUB // 2, j * SUB + SUB // 2)
        lam = S.lambdas(k, E)
        w = S.w[k]
        wf = 1.0 / ((lam[0] / w[:, 0] + lam[1] / w[:, 1]) + lam[2] / w[:, 2])
        fog = np.minimum(1.0, np.maximum(0.0, (fog_end - wf) / (fog_end - fog_start)))
        C = cols[3 * t].astype(np.float64)
        with np.errstate(invalid="ignore"):
            C = np.where(C > 0.0, np.where(C > 1.0, 1.0, C), 0.0)  # NaN -> 0
        Cf = fog[:, None] * C + (1.0 - fog[:, None]) * bg
        img[H - 1 - j, i] = np.floor(Cf * 255 + 0.5).astype(np.uint8)
    out = (img, [int(len(S.t)), int(frags), int(len(pix))], cover.reshape(H, W))
    if buffers:
        hit = zbuf != EMPTY
        depth = np.where(hit, zbuf >> np.uint64(32), np.uint64(DMAX)).astype(np.int64).reshape(H, W)
        winner = np.where(hit, zbuf & np.uint64(0xFFFFFFFF), EMPTY).astype(np.int64).reshape(H, W)
        out += (depth, winner)
    return out
