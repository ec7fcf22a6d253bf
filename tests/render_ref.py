"""NumPy restatement of the point renderer's image (include/nbmi.h, "headless point renderer"), written from that
text and used only by the tests.  Vectorised: fragments are generated per window offset, ordered by (pixel, row),
and the depth rule becomes one running minimum of (P - pixel) * 2^24 + d, which cannot cross a pixel boundary
because pixels ascend.

render_ref(positions, colors, W, H, params) -> (uint8 (H, W, 3), [drawn, fragments, passing, pixels])
"""
import math

import numpy as np

DEPTH_CLEAR = (1 << 24) - 1


def make_params(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovy=75.0, near=0.1, far=10000.0, point_size=1.5,
                fog_density=0.0003, bg=(0.0, 0.0, 0.02)):
    return np.array([*eye, *target, *up, fovy, near, far, point_size, fog_density, *bg], dtype=np.float64)


def _normalize(a):
    n = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    return [a[0] / n, a[1] / n, a[2] / n]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def view_constants(W, H, params):
    p = [float(x) for x in params]
    eye, target, up = p[0:3], p[3:6], p[6:9]
    fovy, near, far, ps, dens, bg = p[9], p[10], p[11], p[12], p[13], p[14:17]
    f = _normalize([target[0] - eye[0], target[1] - eye[1], target[2] - eye[2]])
    s = _normalize(_cross(f, up))
    u = _cross(s, f)
    cot = 1.0 / math.tan(fovy * math.pi / 360.0)
    aspect = W / H
    return dict(eye=eye, f=f, s=s, u=u, xs=cot / aspect, ys=cot, za=(far + near) / (near - far),
                zb=2.0 * far * near / (near - far), R=ps / 2.0, dens=dens, bg=bg)


def _dot(a, x, y, z):
    return a[0] * x + a[1] * y + a[2] * z


def render_ref(positions, colors, W, H, params):
    v = view_constants(W, H, params)
    pos = np.asarray(positions, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    col = np.asarray(colors, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    bg = v["bg"]
    bg8 = np.array([math.floor(b * 255.0 + 0.5) for b in bg], dtype=np.int64)
    P = W * H
    ex, ey, ez = pos[:, 0] - v["eye"][0], pos[:, 1] - v["eye"][1], pos[:, 2] - v["eye"][2]
    xe = _dot(v["s"], ex, ey, ez)
    ye = _dot(v["u"], ex, ey, ez)
    ze = -_dot(v["f"], ex, ey, ez)
    xc, yc = v["xs"] * xe, v["ys"] * ye
    zc, wc = v["za"] * ze + v["zb"], -ze
    with np.errstate(invalid="ignore"):
        keep = (np.abs(xc) <= wc) & (np.abs(yc) <= wc) & (np.abs(zc) <= wc)
    idx = np.nonzero(keep)[0]
    drawn = int(idx.size)
    xc, yc, zc, wc, ze = xc[idx], yc[idx], zc[idx], wc[idx], ze[idx]
    xw = (xc / wc) * (W / 2.0) + (W / 2.0)
    yw = (yc / wc) * (H / 2.0) + (H / 2.0)
    d = np.floor(((zc / wc) * 0.5 + 0.5) * 16777215.0 + 0.5).astype(np.int64)
    t = v["dens"] * (-ze)
    fog = np.exp(-(t * t))
    c0 = col[idx]
    with np.errstate(invalid="ignore"):
        cc = np.where(c0 > 0.0, np.where(c0 > 1.0, 1.0, c0), 0.0)
    cf = fog[:, None] * cc + (1.0 - fog)[:, None] * np.array(bg)[None, :]
    vv = np.floor(cf * 4080.0 + 0.5).astype(np.int64)

    R = v["R"]
    R2 = R * R
    i0 = np.floor(xw - R).astype(np.int64)
    i1 = np.floor(xw + R).astype(np.int64)
    j0 = np.floor(yw - R).astype(np.int64)
    j1 = np.floor(yw + R).astype(np.int64)
    offs = [(a + 0.5) / 4.0 for a in range(4)]
    K = int(math.ceil(2 * R)) + 1
    frag_pix, frag_pt, frag_c = [], [], []
    for dj in range(K):
        jj = j0 + dj
        okj = (jj <= j1) & (jj >= 0) & (jj < H)
        dy = [(jj.astype(np.float64) + o) - yw for o in offs]
        dy2 = [y * y for y in dy]
        for di in range(K):
            ii = i0 + di
            ok = okj & (ii <= i1) & (ii >= 0) & (ii < W)
            if not ok.any():
                continue
            dx = [(ii.astype(np.float64) + o) - xw for o in offs]
            dx2 = [x * x for x in dx]
            c = np.zeros(ii.shape, dtype=np.int64)
            for b in range(4):
                for a in range(4):
                    c += (dx2[a] + dy2[b] <= R2)
            ok &= c >= 1
            sel = np.nonzero(ok)[0]
            frag_pix.append(jj[sel] * W + ii[sel])
            frag_pt.append(sel)
            frag_c.append(c[sel])
    if frag_pix:
        pix = np.concatenate(frag_pix)
        pt = np.concatenate(frag_pt)
        cov = np.concatenate(frag_c)
    else:
        pix = pt = cov = np.zeros(0, dtype=np.int64)
    nfr = int(pix.size)
    acc = np.zeros((P, 3), dtype=np.int64)
    passing = 0
    pixels = 0
    if nfr:
        order = np.argsort(pix * max(1, drawn) + pt, kind="stable")  # by pixel, then draw order (unique keys)
        pix, pt, cov = pix[order], pt[order], cov[order]
        dd = d[pt]
        comp = (P - pix) * (1 << 24) + dd
        run = np.minimum.accumulate(comp)
        excl = np.empty_like(run)
        excl[0] = np.iinfo(np.int64).max
        excl[1:] = run[:-1]
        ok = (comp < excl) & (dd < DEPTH_CLEAR)
        passing = int(ok.sum())
        pixels = int(np.unique(pix).size)
        contrib = cov[ok, None] * vv[pt[ok]]
        for ch in range(3):
            acc[:, ch] = np.bincount(pix[ok], weights=contrib[:, ch].astype(np.float64), minlength=P).astype(np.int64)
    out = np.minimum(255, bg8[None, :] + ((acc + 128) >> 8)).astype(np.uint8)
    img = out.reshape(H, W, 3)[::-1].copy()
    return img, [drawn, nfr, passing, pixels]


def compare(a, b, max_frac=1e-5):
    """(ok, n_channels that differ by 1, n_channels that differ by more): fogged images may differ by one in a
    few channels (device exp against the C library's)."""
    diff = np.abs(a.astype(np.int16) - b.astype(np.int16))
    n1 = int((diff == 1).sum())
    nbig = int((diff > 1).sum())
    return nbig == 0 and n1 <= max_frac * diff.size, n1, nbig
