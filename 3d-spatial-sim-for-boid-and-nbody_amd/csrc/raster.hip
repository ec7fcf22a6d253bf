// Headless triangle rasteriser: the image fixed-function GL draws for the reference's flock (opaque flat-coloured
// GL_TRIANGLES, GL_LESS depth test, linear fog), defined exactly in include/bdmi.h "Image semantics of a flock frame".
//
// One frame, all on the renderer's stream:
//   rasterise  k_raster        one thread per triangle: transform, discards, snap, area, pixel box.  A box of at most
//                              kSmallBox pixel centres is walked by the thread itself; a larger one goes to the large
//                              list as (triangle, first chunk), one 64-bit atomic add that hands out the list slot and
//                              the chunk range together, so the chunk ranges ascend with the slots
//              k_raster_large  a fixed grid of workgroups strides over all chunks (32 x 8 pixel centres, one per
//                              thread) of all listed triangles; a chunk finds its triangle by bisection of the list
//              Every fragment: plain load of the pixel's word, then one 64-bit atomicMin of (d << 32 | t) if smaller.
//              The minimum is the fragment GL_LESS keeps when the triangles are drawn in row order, whatever order
//              the hardware runs them in.
//   resolve    k_resolve       one thread per pixel: the winning triangle's set-up again, its barycentrics at this
//                              pixel, eye depth, fog, colour; RGB8 with the vertical flip
//   copy       the image into the renderer's pinned buffer
// The triangle set-up is one device function used by all three kernels, so no per-triangle record is stored: the resolve
// pass re-derives from 36 bytes of vertices what a record would hold in 96.
// Integer edge functions and correctly rounded float64 only (no FMA: -ffp-contract=off), no transcendental function.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/bdmi.h"
#include "../../include/nbmi.h"
#include "common.h"
#include "render_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kSmallBox = 64;        // pixel centres one thread walks alone
constexpr int kChunkW = 32, kChunkH = 8;  // one large-path work item: kBlock pixel centres, one per thread
constexpr int kLargeGrid = 4096;     // workgroups of k_raster_large (16 per CU)
constexpr int kChunkBits = 36;       // packed counter: large triangles << 36 | chunks
constexpr unsigned long long kChunkMask = (1ull << kChunkBits) - 1ull;
constexpr double kDepthMax = 16777215.0;  // 2^24 - 1
constexpr double kGuard = 1048576.0;      // 2^20 pixels
constexpr int64_t kMaxTriangles = 2147483647LL;
enum { kDrawn = 0, kFrags = 1, kPixels = 2, kCounter = 4, kError = 5, kCtlWords = 6 };

struct TView {
    double eye[3], s[3], u[3], f[3];
    double xs, ys, za, zb, w2, h2;
    double near, fog_start, fog_end;
    double bg[3];
    int W, H;
};

struct Large {
    unsigned long long first;  // first chunk of this triangle in the frame's chunk numbering
    uint32_t t, pad;
};

struct Tri {
    int64_t X[3], Y[3], area2;
    double w[3], zn[3];
    int i0, i1, j0, j1;  // pixel box clamped to the viewport; empty if i1 < i0 or j1 < j0
};

// Everything of triangle t that does not depend on the pixel (include/bdmi.h).  false: discarded.
__device__ __forceinline__ bool setup(const TView &v, const float *__restrict__ verts, int64_t t, Tri &T) {
    const float *p = verts + 9 * t;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float px = p[3 * k], py = p[3 * k + 1], pz = p[3 * k + 2];
        if (!(isfinite(px) && isfinite(py) && isfinite(pz))) return false;
        const double ex = (double)px - v.eye[0], ey = (double)py - v.eye[1], ez = (double)pz - v.eye[2];
        const double xe = v.s[0] * ex + v.s[1] * ey + v.s[2] * ez;
        const double ye = v.u[0] * ex + v.u[1] * ey + v.u[2] * ez;
        const double ze = -(v.f[0] * ex + v.f[1] * ey + v.f[2] * ez);
        const double xc = v.xs * xe, yc = v.ys * ye;
        const double zc = v.za * ze + v.zb, wc = -ze;
        if (!(wc >= v.near) || !(zc <= wc)) return false;
        const double xw = (xc / wc) * v.w2 + v.w2;
        const double yw = (yc / wc) * v.h2 + v.h2;
        if (!(fabs(xw) <= kGuard) || !(fabs(yw) <= kGuard)) return false;
        T.X[k] = (int64_t)floor(xw * 16.0 + 0.5);
        T.Y[k] = (int64_t)floor(yw * 16.0 + 0.5);
        T.w[k] = wc;
        T.zn[k] = zc / wc;
    }
    int64_t a2 = (T.X[1] - T.X[0]) * (T.Y[2] - T.Y[0]) - (T.Y[1] - T.Y[0]) * (T.X[2] - T.X[0]);
    if (a2 == 0) return false;
    if (a2 < 0) {
        a2 = -a2;
        const int64_t x = T.X[1], y = T.Y[1];
        const double w = T.w[1], z = T.zn[1];
        T.X[1] = T.X[2]; T.Y[1] = T.Y[2]; T.w[1] = T.w[2]; T.zn[1] = T.zn[2];
        T.X[2] = x; T.Y[2] = y; T.w[2] = w; T.zn[2] = z;
    }
    T.area2 = a2;
    const int64_t xmin = min(T.X[0], min(T.X[1], T.X[2])), xmax = max(T.X[0], max(T.X[1], T.X[2]));
    const int64_t ymin = min(T.Y[0], min(T.Y[1], T.Y[2])), ymax = max(T.Y[0], max(T.Y[1], T.Y[2]));
    // pixel centres 16 i + 8 inside [min, max]: ceil((min - 8) / 16) <= i <= floor((max - 8) / 16)
    T.i0 = (int)max((int64_t)0, (xmin + 7) >> 4);
    T.i1 = (int)min((int64_t)v.W - 1, (xmax - 8) >> 4);
    T.j0 = (int)max((int64_t)0, (ymin + 7) >> 4);
    T.j1 = (int)min((int64_t)v.H - 1, (ymax - 8) >> 4);
    return true;
}

// The three edge functions at the centre of pixel (i, j); E[a] belongs to the edge opposite vertex a.
__device__ __forceinline__ bool edges(const Tri &T, int i, int j, int64_t E[3]) {
    const int64_t px = 16 * (int64_t)i + 8, py = 16 * (int64_t)j + 8;
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        const int64_t dx = T.X[c] - T.X[b], dy = T.Y[c] - T.Y[b];
        E[a] = dx * (py - T.Y[b]) - dy * (px - T.X[b]);
        const bool owns = dy < 0 || (dy == 0 && dx > 0);
        in = in && (E[a] > 0 || (E[a] == 0 && owns));
    }
    return in;
}

// One pixel of one triangle: coverage, depth, z-buffer.  Returns 1 for a fragment.
__device__ __forceinline__ unsigned fragment(const Tri &T, uint32_t t, int i, int j, int W,
                                             unsigned long long *__restrict__ zbuf) {
    int64_t E[3];
    if (!edges(T, i, j, E)) return 0;
    const double a2 = (double)T.area2;
    const double l0 = (double)E[0] / a2, l1 = (double)E[1] / a2, l2 = (double)E[2] / a2;
    const double zf = (l0 * T.zn[0] + l1 * T.zn[1]) + l2 * T.zn[2];
    const double d = floor((zf * 0.5 + 0.5) * kDepthMax + 0.5);
    if (!(d >= 0.0 && d < kDepthMax)) return 0;
    const unsigned long long word = ((unsigned long long)d << 32) | t;
    unsigned long long *z = zbuf + (size_t)j * W + i;
    if (word < *z) atomicMin(z, word);  // the word only ever falls: a stale read costs an atomic, never a fragment
    return 1;
}

__device__ __forceinline__ void block_add(unsigned v, unsigned *sh, unsigned long long *dst) {
    if (threadIdx.x == 0) *sh = 0;
    __syncthreads();
    if (v) atomicAdd(sh, v);
    __syncthreads();
    if (threadIdx.x == 0 && *sh) atomicAdd(dst, (unsigned long long)*sh);
    __syncthreads();
}

__global__ __launch_bounds__(kBlock) void k_raster(TView v, const float *__restrict__ verts, int64_t n,
                                                  unsigned long long *__restrict__ zbuf, Large *__restrict__ large,
                                                  int64_t cap_large, unsigned long long *__restrict__ ctl) {
    __shared__ unsigned sh;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned drawn = 0, frags = 0;
    Tri T;
    if (t < n && setup(v, verts, t, T)) {
        drawn = 1;
        const int bw = T.i1 - T.i0 + 1, bh = T.j1 - T.j0 + 1;
        if (bw > 0 && bh > 0) {
            if ((int64_t)bw * bh <= kSmallBox) {
                for (int j = T.j0; j <= T.j1; j++)
                    for (int i = T.i0; i <= T.i1; i++) frags += fragment(T, (uint32_t)t, i, j, v.W, zbuf);
            } else {
                const unsigned long long chunks =
                    (unsigned long long)((bw + kChunkW - 1) / kChunkW) * (unsigned long long)((bh + kChunkH - 1) / kChunkH);
                const unsigned long long old = atomicAdd(&ctl[kCounter], (1ull << kChunkBits) | chunks);
                const unsigned long long slot = old >> kChunkBits, first = old & kChunkMask;
                if (slot >= (unsigned long long)cap_large || slot >= (1ull << (64 - kChunkBits)) - 1ull ||
                    first + chunks > kChunkMask)
                    ctl[kError] = 1ull;  // the frame is refused; nothing is written outside the list
                else
                    large[slot] = Large{first, (uint32_t)t, 0u};
            }
        }
    }
    block_add(drawn, &sh, &ctl[kDrawn]);
    block_add(frags, &sh, &ctl[kFrags]);
}

__global__ __launch_bounds__(kBlock) void k_raster_large(TView v, const float *__restrict__ verts,
                                                        unsigned long long *__restrict__ zbuf,
                                                        const Large *__restrict__ large, int64_t cap_large,
                                                        unsigned long long *__restrict__ ctl) {
    __shared__ unsigned sh;
    if (ctl[kError]) return;
    const unsigned long long packed = ctl[kCounter];
    const int64_t count = (int64_t)(packed >> kChunkBits);  // <= cap_large, or the error word is set
    const unsigned long long total = packed & kChunkMask;
    unsigned frags = 0;
    for (unsigned long long w = blockIdx.x; w < total; w += gridDim.x) {
        int64_t lo = 0, hi = count - 1;  // the last entry with first <= w
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (large[mid].first <= w) lo = mid; else hi = mid - 1;
        }
        const Large e = large[lo];
        Tri T;
        if (!setup(v, verts, (int64_t)e.t, T)) continue;  // never: it was listed because it set up
        const int cw = (T.i1 - T.i0 + kChunkW) / kChunkW;
        const unsigned long long c = w - e.first;
        const int cy = (int)(c / (unsigned long long)cw), cx = (int)(c - (unsigned long long)cy * cw);
        const int i = T.i0 + cx * kChunkW + ((int)threadIdx.x & (kChunkW - 1));
        const int j = T.j0 + cy * kChunkH + ((int)threadIdx.x / kChunkW);
        if (i <= T.i1 && j <= T.j1) frags += fragment(T, e.t, i, j, v.W, zbuf);
    }
    block_add(frags, &sh, &ctl[kFrags]);
}

__device__ __forceinline__ uint8_t shade(double c0, double fog, double bg) {
    const double c = !(c0 > 0.0) ? 0.0 : (c0 > 1.0 ? 1.0 : c0);
    const double cf = fog * c + (1.0 - fog) * bg;
    return (uint8_t)floor(cf * 255.0 + 0.5);
}

__global__ __launch_bounds__(kBlock) void k_resolve(TView v, const float *__restrict__ verts,
                                                   const float *__restrict__ cols,
                                                   const unsigned long long *__restrict__ zbuf, uint8_t bg0, uint8_t bg1,
                                                   uint8_t bg2, uint8_t *__restrict__ out,
                                                   unsigned long long *__restrict__ ctl) {
    __shared__ unsigned sh;
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned hit = 0;
    if (q < (int64_t)v.W * v.H) {
        const int row = (int)(q / v.W), i = (int)(q - (int64_t)row * v.W);
        const int j = v.H - 1 - row;  // row 0 of the image is the top: GL's last row
        const unsigned long long word = zbuf[(size_t)j * v.W + i];
        uint8_t rgb[3] = {bg0, bg1, bg2};
        Tri T;
        const int64_t t = (int64_t)(word & 0xffffffffull);
        if (word != ~0ull && setup(v, verts, t, T)) {
            hit = 1;
            int64_t E[3];
            (void)edges(T, i, j, E);
            const double a2 = (double)T.area2;
            const double l0 = (double)E[0] / a2, l1 = (double)E[1] / a2, l2 = (double)E[2] / a2;
            const double wf = 1.0 / ((l0 / T.w[0] + l1 / T.w[1]) + l2 / T.w[2]);
            double fog = (v.fog_end - wf) / (v.fog_end - v.fog_start);
            fog = fog < 0.0 ? 0.0 : (fog > 1.0 ? 1.0 : fog);
#pragma unroll
            for (int ch = 0; ch < 3; ch++) rgb[ch] = shade((double)cols[9 * t + ch], fog, v.bg[ch]);
        }
        out[3 * q] = rgb[0]; out[3 * q + 1] = rgb[1]; out[3 * q + 2] = rgb[2];
    }
    block_add(hit, &sh, &ctl[kPixels]);
}

inline int grid_for(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }

int check_render(nbmi_render *r, const char *what) {
    if (!r) { nbmi::set_error("%s: null renderer", what); return NBMI_ERR_ARG; }
    if (hipSetDevice(r->device) != hipSuccess) { nbmi::set_error("hipSetDevice(%d) failed", r->device); return NBMI_ERR_HIP; }
    return 0;
}

// The per-frame constants of the view (include/bdmi.h), computed once on the host as the point renderer's are.
int make_view(const nbmi_render *r, const double *p, TView *v) {
    if (!p) { nbmi::set_error("bdmi_render: null params"); return NBMI_ERR_ARG; }
    for (int k = 0; k < 17; k++)
        if (!isfinite(p[k])) { nbmi::set_error("bdmi_render: params[%d] is not finite", k); return NBMI_ERR_ARG; }
    const double fovy = p[9], zn = p[10], zf = p[11], fs = p[12], fe = p[13];
    if (!(fovy > 0.0 && fovy < 180.0) || !(zn > 0.0 && zf > zn)) {
        nbmi::set_error("bdmi_render: need 0 < fovy < 180 and 0 < near < far");
        return NBMI_ERR_ARG;
    }
    if (!(fe > fs)) { nbmi::set_error("bdmi_render: need fog_end > fog_start"); return NBMI_ERR_ARG; }
    for (int k = 0; k < 3; k++)
        if (!(p[14 + k] >= 0.0 && p[14 + k] <= 1.0)) { nbmi::set_error("bdmi_render: bg outside [0, 1]"); return NBMI_ERR_ARG; }
    double f[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]};
    const double fl = sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]);
    if (!(fl > 0.0)) { nbmi::set_error("bdmi_render: eye == target"); return NBMI_ERR_ARG; }
    for (int k = 0; k < 3; k++) f[k] = f[k] / fl;
    const double *up = p + 6;
    double s[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
    const double sl = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
    if (!(sl > 0.0)) { nbmi::set_error("bdmi_render: up is parallel to the view direction"); return NBMI_ERR_ARG; }
    for (int k = 0; k < 3; k++) s[k] = s[k] / sl;
    const double u[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};
    const double cot = 1.0 / tan(fovy * M_PI / 360.0);
    const double aspect = (double)r->W / (double)r->H;
    for (int k = 0; k < 3; k++) { v->eye[k] = p[k]; v->s[k] = s[k]; v->u[k] = u[k]; v->f[k] = f[k]; v->bg[k] = p[14 + k]; }
    v->xs = cot / aspect;
    v->ys = cot;
    v->za = (zf + zn) / (zn - zf);
    v->zb = 2.0 * zf * zn / (zn - zf);
    v->w2 = (double)r->W / 2.0;
    v->h2 = (double)r->H / 2.0;
    v->near = zn;
    v->fog_start = fs;
    v->fog_end = fe;
    v->W = r->W;
    v->H = r->H;
    return 0;
}

int ensure_frame(nbmi_render *r, int64_t n) {
    const size_t P = (size_t)r->W * r->H;
    if (!r->zbuf) {
        NBMI_HIP_CHECK(hipMalloc((void **)&r->zbuf, P * sizeof(unsigned long long)));
        NBMI_HIP_CHECK(hipMalloc((void **)&r->tri_ctl, kCtlWords * sizeof(unsigned long long)));
    }
    if (n > r->cap_large) {
        const int64_t c = std::min(kMaxTriangles, std::max(n, r->cap_large + r->cap_large / 2));
        NBMI_HIP_CHECK(hipStreamSynchronize(r->stream));
        (void)hipFree(r->tri_large);
        r->tri_large = nullptr;
        r->cap_large = 0;
        NBMI_HIP_CHECK(hipMalloc(&r->tri_large, (size_t)c * sizeof(Large)));
        r->cap_large = c;
    }
    return 0;
}

int ensure_upload(nbmi_render *r, int64_t n) {
    if (n <= r->cap_tri) return 0;
    const int64_t c = std::min(kMaxTriangles, std::max(n, r->cap_tri + r->cap_tri / 2));
    NBMI_HIP_CHECK(hipStreamSynchronize(r->stream));
    (void)hipFree(r->d_tri); (void)hipHostFree(r->h_tri);
    r->d_tri = r->h_tri = nullptr;
    r->cap_tri = 0;
    NBMI_HIP_CHECK(hipMalloc((void **)&r->d_tri, (size_t)c * 18 * sizeof(float)));
    NBMI_HIP_CHECK(hipHostMalloc((void **)&r->h_tri, (size_t)c * 18 * sizeof(float), hipHostMallocDefault));
    r->cap_tri = c;
    return 0;
}

// One frame of n triangles already on the device (enqueued behind whatever the renderer's stream holds).
int raster_frame(nbmi_render *r, const float *d_verts, const float *d_cols, int64_t n, const TView &v, uint8_t *out) {
    if (ensure_frame(r, n)) return NBMI_ERR_HIP;
    hipStream_t st = r->stream;
    const int64_t P = (int64_t)r->W * r->H;
    uint8_t bg8[3];
    for (int k = 0; k < 3; k++) bg8[k] = (uint8_t)floor(v.bg[k] * 255.0 + 0.5);
    NBMI_HIP_CHECK(hipEventRecord(r->ev[0], st));
    NBMI_HIP_CHECK(hipMemsetAsync(r->zbuf, 0xff, (size_t)P * sizeof(unsigned long long), st));
    NBMI_HIP_CHECK(hipMemsetAsync(r->tri_ctl, 0, kCtlWords * sizeof(unsigned long long), st));
    if (n > 0) {
        k_raster<<<grid_for(n), kBlock, 0, st>>>(v, d_verts, n, r->zbuf, (Large *)r->tri_large, r->cap_large, r->tri_ctl);
        k_raster_large<<<kLargeGrid, kBlock, 0, st>>>(v, d_verts, r->zbuf, (const Large *)r->tri_large, r->cap_large,
                                                     r->tri_ctl);
        NBMI_HIP_CHECK(hipGetLastError());
    }
    NBMI_HIP_CHECK(hipEventRecord(r->ev[1], st));
    k_resolve<<<grid_for(P), kBlock, 0, st>>>(v, d_verts, d_cols, r->zbuf, bg8[0], bg8[1], bg8[2], r->d_img, r->tri_ctl);
    NBMI_HIP_CHECK(hipGetLastError());
    NBMI_HIP_CHECK(hipEventRecord(r->ev[2], st));
    NBMI_HIP_CHECK(hipMemcpyAsync(r->h_img, r->d_img, (size_t)P * 3, hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipMemcpyAsync(r->h_small, r->tri_ctl, kCtlWords * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipEventRecord(r->ev[3], st));
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    r->timed = true;
    r->tri_frame = true;
    if (r->h_small[kError]) {
        nbmi::set_error("bdmi_render: the large triangles of this frame exceed 2^28 - 2 triangles or 2^36 - 1 chunks of "
                        "32 x 8 pixels");
        return NBMI_ERR_CAPACITY;
    }
    r->last_stats[0] = (int64_t)r->h_small[kDrawn];
    r->last_stats[1] = (int64_t)r->h_small[kFrags];
    r->last_stats[2] = r->last_stats[3] = (int64_t)r->h_small[kPixels];
    memcpy(out, r->h_img, (size_t)P * 3);
    return 0;
}

}  // namespace

void nbmi::raster_free(nbmi_render *r) {
    (void)hipFree(r->zbuf); (void)hipFree(r->tri_ctl); (void)hipFree(r->tri_large);
    (void)hipFree(r->d_tri); (void)hipHostFree(r->h_tri);
    r->zbuf = r->tri_ctl = nullptr;
    r->tri_large = nullptr;
    r->d_tri = r->h_tri = nullptr;
    r->cap_large = r->cap_tri = 0;
}

extern "C" {

int bdmi_render_triangles(nbmi_render *r, const float *vertices, const float *colors, int64_t n, const double *params,
                          uint8_t *out) {
    if (int rc = check_render(r, "bdmi_render_triangles")) return rc;
    if (n < 0 || n > kMaxTriangles || !out || (n > 0 && (!vertices || !colors))) {
        nbmi::set_error("bdmi_render_triangles: bad arguments (triangles = %lld, at most %lld; null pointer?)", (long long)n,
                        (long long)kMaxTriangles);
        return NBMI_ERR_ARG;
    }
    TView v;
    if (int rc = make_view(r, params, &v)) return rc;
    if (n > 0) {
        if (ensure_upload(r, n)) return NBMI_ERR_HIP;
        memcpy(r->h_tri, vertices, (size_t)n * 36);
        memcpy(r->h_tri + 9 * n, colors, (size_t)n * 36);
        NBMI_HIP_CHECK(hipMemcpyAsync(r->d_tri, r->h_tri, (size_t)n * 72, hipMemcpyHostToDevice, r->stream));
    }
    return raster_frame(r, r->d_tri, r->d_tri + 9 * n, n, v, out);
}

int bdmi_render_flock(nbmi_render *r, bdmi_flock *f, const double *cam12, double tan_h, double tan_v, double fog_end_vis,
                      double cone_length, double cone_radius, const double *params, uint8_t *out, int64_t *visible_boids) {
    if (int rc = check_render(r, "bdmi_render_flock")) return rc;
    if (!f || !cam12 || !out) { nbmi::set_error("bdmi_render_flock: null argument"); return NBMI_ERR_ARG; }
    TView v;
    if (int rc = make_view(r, params, &v)) return rc;
    int64_t n = 0, count = 0;
    int dev = 0, slab = 0;
    if (int rc = nbmi::flock_source(f, &n, &dev, &slab)) return rc;
    if (slab) { nbmi::set_error("bdmi_render_flock: slab handles hold ghosts and a part of the flock"); return NBMI_ERR_ARG; }
    if (dev != r->device) {
        nbmi::set_error("bdmi_render_flock: the flock lives on device %d, the renderer on %d", dev, r->device);
        return NBMI_ERR_ARG;
    }
    const float *d_verts = nullptr, *d_cols = nullptr;
    if (int rc = nbmi::flock_visible_device(f, cam12, tan_h, tan_v, fog_end_vis, cone_length, cone_radius, &d_verts,
                                            &d_cols, &count, r->ev_src))
        return rc;
    if (visible_boids) *visible_boids = count;
    NBMI_HIP_CHECK(hipSetDevice(r->device));
    if (count > 0) NBMI_HIP_CHECK(hipStreamWaitEvent(r->stream, r->ev_src, 0));
    return raster_frame(r, d_verts, d_cols, 2 * count, v, out);
}

}  // extern "C"
