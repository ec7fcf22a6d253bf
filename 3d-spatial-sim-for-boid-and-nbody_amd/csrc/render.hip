// Headless point renderer: the image fixed-function GL draws for the exporter's GL_POINTS pass (smooth points,
// additive GL_SRC_ALPHA/GL_ONE blending, GL_LESS depth test, EXP2 fog), defined exactly in include/nbmi.h.
//
// One frame, all on the renderer's stream:
//   project   k_count   one thread per point: view, projection, clip, depth, fog'd colour -> 8-byte point record;
//                       fragments (pixels with coverage >= 1) per 256-point tile
//             scan::k_scan_values  exclusive scan of the tile counts (one workgroup); the total goes to the host
//   emit      k_emit    the same per-point work again, fragments written as (pixel, point << 5 | coverage) in row order
//   sort      the hand-written stable radix sort (radix.hip) by pixel, ceil(log2(W H)) key bits: draw order inside a pixel
//   resolve   k_resolve_min  per 2 048-fragment tile: min of (P - pixel) << 24 | depth.  Pixels ascend, so the composite
//                            of any earlier pixel is larger than every composite of a later one and a plain running
//                            minimum over the whole array never crosses a pixel boundary
//             scan::k_scan_values  exclusive min-scan of the tile minima (one workgroup)
//             k_resolve fragment passes iff composite < running minimum of everything before it (and depth < 2^24-1);
//                       coverage x colour of the passing ones summed per pixel run inside the tile, one 64-bit integer
//                       atomic per (pixel, tile, channel) - a pixel's run may span any number of tiles
//   pack      k_pack    RGB8 with the vertical flip, then one copy into the renderer's pinned buffer
// Integer sums only: the image does not depend on the order the hardware runs anything in.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/nbmi.h"
#include "common.h"
#include "render_internal.h"
#include "scan.h"

namespace {

constexpr int kBlock = 256;                    // points per workgroup (project / emit)
constexpr int kResItems = 8;                   // fragments per thread (resolve)
constexpr int kResTile = kBlock * kResItems;   // fragments per resolve workgroup
constexpr int kMaxWin = 5;                     // pixels per axis a point can reach: ceil(2R) + 1 with R <= 2
constexpr uint32_t kDepthClear = (1u << 24) - 1u;
constexpr int64_t kMaxPoints = (int64_t)1 << 27;      // point index << 5 | coverage in 32 bits
constexpr int64_t kMaxFragments = ((int64_t)1 << 30) - 1;  // what the radix sort takes in one call
constexpr int kMaxSide = 16384;

struct View {
    double eye[3], s[3], u[3], f[3];
    double xs, ys;   // cot / aspect, cot
    double za, zb;   // z_c = za z_e + zb
    double w2, h2;   // W / 2, H / 2
    double R, R2;
    double dens;
    double bg[3];
    int W, H;
};

// Everything of one point that does not depend on the pixel.  false: clipped.
__device__ __forceinline__ bool project(const View &v, const float *__restrict__ pos, int64_t i, double &xw, double &yw,
                                        uint32_t &d, double &ze) {
    const double ex = (double)pos[3 * i] - v.eye[0];
    const double ey = (double)pos[3 * i + 1] - v.eye[1];
    const double ez = (double)pos[3 * i + 2] - v.eye[2];
    const double xe = v.s[0] * ex + v.s[1] * ey + v.s[2] * ez;
    const double ye = v.u[0] * ex + v.u[1] * ey + v.u[2] * ez;
    ze = -(v.f[0] * ex + v.f[1] * ey + v.f[2] * ez);
    const double xc = v.xs * xe, yc = v.ys * ye;
    const double zc = v.za * ze + v.zb, wc = -ze;
    if (!(fabs(xc) <= wc && fabs(yc) <= wc && fabs(zc) <= wc)) return false;  // NaN fails too
    xw = (xc / wc) * v.w2 + v.w2;
    yw = (yc / wc) * v.h2 + v.h2;
    d = (uint32_t)floor(((zc / wc) * 0.5 + 0.5) * 16777215.0 + 0.5);
    return true;
}

// First pixel of the window on one axis and how many pixels of it lie inside [0, size)
__device__ __forceinline__ void window(double c, double R, int size, int &lo, int &cnt) {
    int a = (int)floor(c - R), b = (int)floor(c + R);
    if (b > a + kMaxWin - 1) b = a + kMaxWin - 1;  // never: ceil(2R) + 1 <= 5
    if (a < 0) a = 0;
    if (b > size - 1) b = size - 1;
    lo = a;
    cnt = b >= a ? b - a + 1 : 0;
}

// squared distances of the 4 sample columns (rows) of pixel p from the centre
__device__ __forceinline__ void sample_d2(int p, double c, double out[4]) {
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const double dx = ((double)p + ((double)a + 0.5) / 4.0) - c;
        out[a] = dx * dx;
    }
}

__device__ __forceinline__ int coverage(const double dx2[4], const double dy2[4], double R2) {
    int c = 0;
#pragma unroll
    for (int b = 0; b < 4; b++)
#pragma unroll
        for (int a = 0; a < 4; a++) c += (dx2[a] + dy2[b] <= R2) ? 1 : 0;
    return c;
}

// Fragments of a point: bit (row * kMaxWin + col) of the returned mask for each pixel of the window with coverage >= 1
__device__ __forceinline__ uint32_t frag_mask(const View &v, double xw, double yw, int i0, int ni, int j0, int nj) {
    uint32_t m = 0;
    for (int jj = 0; jj < nj; jj++) {
        double dy2[4];
        sample_d2(j0 + jj, yw, dy2);
        for (int ii = 0; ii < ni; ii++) {
            double dx2[4];
            sample_d2(i0 + ii, xw, dx2);
            if (coverage(dx2, dy2, v.R2) > 0) m |= 1u << (jj * kMaxWin + ii);
        }
    }
    return m;
}

__device__ __forceinline__ uint32_t shade(const View &v, const float *__restrict__ col, int64_t i, int ch, double fog) {
    const double c0 = (double)col[3 * i + ch];
    const double c = !(c0 > 0.0) ? 0.0 : (c0 > 1.0 ? 1.0 : c0);
    const double cf = fog * c + (1.0 - fog) * v.bg[ch];
    return (uint32_t)floor(cf * 4080.0 + 0.5);
}

__global__ __launch_bounds__(kBlock) void k_count(View v, const float *__restrict__ pos, const float *__restrict__ col,
                                                 int64_t n, uint64_t *__restrict__ rec, uint32_t *__restrict__ tile_cnt,
                                                 unsigned long long *__restrict__ stats) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t nf = 0, drawn = 0;
    double xw, yw, ze;
    uint32_t d;
    if (i < n && project(v, pos, i, xw, yw, d, ze)) {
        drawn = 1;
        int i0, ni, j0, nj;
        window(xw, v.R, v.W, i0, ni);
        window(yw, v.R, v.H, j0, nj);
        nf = (uint32_t)__popc(frag_mask(v, xw, yw, i0, ni, j0, nj));
        const double t = v.dens * (-ze);
        const double fog = exp(-(t * t));
        rec[i] = ((uint64_t)d << 36) | ((uint64_t)shade(v, col, i, 0, fog) << 24) |
                 ((uint64_t)shade(v, col, i, 1, fog) << 12) | (uint64_t)shade(v, col, i, 2, fog);
    }
    const uint32_t tot_f = scan::block_scan<kBlock>(nf, 0u, scan::Sum()).total;
    const uint32_t tot_d = scan::block_scan<kBlock>(drawn, 0u, scan::Sum()).total;
    if (threadIdx.x == 0) {
        tile_cnt[blockIdx.x] = tot_f;
        if (tot_d) atomicAdd(&stats[0], (unsigned long long)tot_d);
    }
}

__global__ __launch_bounds__(kBlock) void k_emit(View v, const float *__restrict__ pos, int64_t n,
                                                const uint64_t *__restrict__ tile_off, uint32_t *__restrict__ keys,
                                                uint32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double xw = 0, yw = 0, ze;
    uint32_t d, m = 0;
    int i0 = 0, ni = 0, j0 = 0, nj = 0;
    if (i < n && project(v, pos, i, xw, yw, d, ze)) {
        window(xw, v.R, v.W, i0, ni);
        window(yw, v.R, v.H, j0, nj);
        m = frag_mask(v, xw, yw, i0, ni, j0, nj);
    }
    uint64_t o = (uint64_t)scan::tile_slot<kBlock>(tile_off, (unsigned)__popc(m));
    for (int jj = 0; jj < nj && m; jj++) {
        double dy2[4];
        sample_d2(j0 + jj, yw, dy2);
        for (int ii = 0; ii < ni; ii++) {
            if (!((m >> (jj * kMaxWin + ii)) & 1u)) continue;
            double dx2[4];
            sample_d2(i0 + ii, xw, dx2);
            const uint32_t c = (uint32_t)coverage(dx2, dy2, v.R2);
            keys[o] = (uint32_t)(j0 + jj) * (uint32_t)v.W + (uint32_t)(i0 + ii);
            vals[o] = ((uint32_t)i << 5) | c;
            o++;
        }
    }
}

__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return b < a ? b : a; }

__device__ __forceinline__ uint64_t composite(uint32_t key, uint64_t rec, uint64_t P) {
    return ((P - key) << 24) | (rec >> 36);
}

__global__ __launch_bounds__(kBlock) void k_resolve_min(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                       const uint64_t *__restrict__ rec, int64_t nf, uint64_t P,
                                                       uint64_t *__restrict__ tile_min) {
    const int64_t first = (int64_t)blockIdx.x * kResTile + (int64_t)threadIdx.x * kResItems;
    uint64_t mn = ~0ull;
    for (int k = 0; k < kResItems; k++) {
        const int64_t q = first + k;
        if (q < nf) mn = umin64(mn, composite(keys[q], rec[vals[q] >> 5], P));
    }
    const uint64_t tot = scan::block_scan<kBlock>(mn, ~(uint64_t)0, scan::Min()).total;
    if (threadIdx.x == 0) tile_min[blockIdx.x] = tot;
}

struct Seg {  // segmented sum element: a run head inside, and the sums since the last head
    uint32_t head;
    uint64_t s[3];
};
__device__ __forceinline__ Seg lane_up(const Seg &v, int d) {  // scan.h's lane shift for this type
    return Seg{__shfl_up(v.head, d), {__shfl_up(v.s[0], d), __shfl_up(v.s[1], d), __shfl_up(v.s[2], d)}};
}
struct OpSeg {
    __device__ Seg operator()(const Seg &a, const Seg &b) const {  // a before b
        Seg r;
        r.head = a.head | b.head;
        for (int ch = 0; ch < 3; ch++) r.s[ch] = b.head ? b.s[ch] : a.s[ch] + b.s[ch];
        return r;
    }
};

__global__ __launch_bounds__(kBlock) void k_resolve(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                   const uint64_t *__restrict__ rec, int64_t nf, uint64_t P,
                                                   const uint64_t *__restrict__ tile_pre,
                                                   unsigned long long *__restrict__ acc,
                                                   unsigned long long *__restrict__ stats) {
    const int64_t tile_first = (int64_t)blockIdx.x * kResTile;
    const int64_t tile_end = tile_first + kResTile < nf ? tile_first + kResTile : nf;
    const int64_t first = tile_first + (int64_t)threadIdx.x * kResItems;
    uint32_t key[kResItems];
    uint64_t cm[kResItems], r[kResItems];
    uint32_t cov[kResItems];
    uint64_t mn = ~0ull;
#pragma unroll
    for (int k = 0; k < kResItems; k++) {
        const int64_t q = first + k;
        key[k] = 0; cm[k] = ~0ull; r[k] = 0; cov[k] = 0;
        if (q < nf) {
            key[k] = keys[q];
            const uint32_t vq = vals[q];
            r[k] = rec[vq >> 5];
            cov[k] = vq & 31u;
            cm[k] = composite(key[k], r[k], P);
            mn = umin64(mn, cm[k]);
        }
    }
    uint64_t run = scan::block_scan<kBlock>(mn, ~(uint64_t)0, scan::Min()).excl;
    run = umin64(run, tile_pre[blockIdx.x]);
    // which fragments pass, their contributions, and the run heads
    uint32_t pass = 0, head = 0;
    uint64_t con[kResItems][3];
    uint32_t prev_key = first > 0 && first < nf ? keys[first - 1] : 0xffffffffu;
#pragma unroll
    for (int k = 0; k < kResItems; k++) {
        const int64_t q = first + k;
        con[k][0] = con[k][1] = con[k][2] = 0;
        if (q < nf) {
            if (q == 0 || key[k] != prev_key) head |= 1u << k;
            prev_key = key[k];
            const uint32_t d = (uint32_t)(r[k] >> 36);
            if (cm[k] < run && d < kDepthClear) {
                pass |= 1u << k;
                con[k][0] = (uint64_t)cov[k] * ((r[k] >> 24) & 0xfffu);
                con[k][1] = (uint64_t)cov[k] * ((r[k] >> 12) & 0xfffu);
                con[k][2] = (uint64_t)cov[k] * (r[k] & 0xfffu);
            }
            run = umin64(run, cm[k]);
        }
    }
    // carry of the run that enters this thread's first fragment from the threads before it in the tile
    Seg agg{0u, {0, 0, 0}};
#pragma unroll
    for (int k = 0; k < kResItems; k++) {
        if ((head >> k) & 1u) { agg.head = 1u; agg.s[0] = agg.s[1] = agg.s[2] = 0; }
        for (int ch = 0; ch < 3; ch++) agg.s[ch] += con[k][ch];
    }
    const Seg carry = scan::block_scan<kBlock>(agg, Seg{0u, {0, 0, 0}}, OpSeg()).excl;
    uint64_t s[3] = {carry.s[0], carry.s[1], carry.s[2]};
#pragma unroll
    for (int k = 0; k < kResItems; k++) {
        const int64_t q = first + k;
        if (q >= nf) break;
        if ((head >> k) & 1u) s[0] = s[1] = s[2] = 0;
        for (int ch = 0; ch < 3; ch++) s[ch] += con[k][ch];
        const bool last = (q + 1 == tile_end) || (k + 1 < kResItems ? key[k + 1] != key[k] : keys[q + 1] != key[k]);
        if (last) {
            for (int ch = 0; ch < 3; ch++)
                if (s[ch]) atomicAdd(&acc[3 * (uint64_t)key[k] + ch], (unsigned long long)s[ch]);
        }
    }
    const uint32_t t_pass = scan::block_scan<kBlock>((uint32_t)__popc(pass), 0u, scan::Sum()).total;
    const uint32_t t_head = scan::block_scan<kBlock>((uint32_t)__popc(head), 0u, scan::Sum()).total;
    if (threadIdx.x == 0) {
        if (t_pass) atomicAdd(&stats[2], (unsigned long long)t_pass);
        if (t_head) atomicAdd(&stats[3], (unsigned long long)t_head);
    }
}

__global__ __launch_bounds__(kBlock) void k_pack(const unsigned long long *__restrict__ acc, int W, int H, uint32_t bg0,
                                                uint32_t bg1, uint32_t bg2, uint8_t *__restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= (int64_t)W * H) return;
    const int64_t row = q / W, x = q - row * W;
    const int64_t p = (int64_t)(H - 1 - row) * W + x;  // row 0 of the image is the top: GL's last row
    const uint32_t bg[3] = {bg0, bg1, bg2};
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const unsigned long long v = bg[ch] + ((acc[3 * p + ch] + 128ull) >> 8);
        out[3 * q + ch] = (uint8_t)(v < 255ull ? v : 255ull);
    }
}

inline int grid_for(int64_t n, int64_t per) { return (int)((n + per - 1) / per); }

}  // namespace

namespace {

template <typename T>
int dmalloc(T **p, size_t count) {
    void *q = nullptr;
    NBMI_HIP_CHECK(hipMalloc(&q, (count ? count : 1) * sizeof(T)));
    *p = (T *)q;
    return 0;
}

void free_points(nbmi_render *r) {
    (void)hipFree(r->d_pos); (void)hipFree(r->d_col); (void)hipHostFree(r->h_stage);
    (void)hipFree(r->rec); (void)hipFree(r->tile_cnt); (void)hipFree(r->tile_off);
    r->d_pos = r->d_col = r->h_stage = nullptr;
    r->rec = nullptr; r->tile_cnt = nullptr; r->tile_off = nullptr;
    r->cap_pts = 0;
}

void free_frags(nbmi_render *r) {
    (void)hipFree(r->keys); (void)hipFree(r->vals); (void)hipFree(r->keys2); (void)hipFree(r->vals2);
    (void)hipFree(r->tile_min); (void)hipFree(r->tile_pre); (void)hipFree(r->sort_tmp);
    r->keys = r->vals = r->keys2 = r->vals2 = nullptr;
    r->tile_min = r->tile_pre = nullptr;
    r->sort_tmp = nullptr;
    r->sort_bytes = 0;
    r->cap_frags = 0;
}

int ensure_points(nbmi_render *r, int64_t n, bool staging) {
    if (n <= r->cap_pts && (!staging || r->h_stage)) return 0;
    const int64_t c = std::max(n, r->cap_pts + r->cap_pts / 2);
    NBMI_HIP_CHECK(hipStreamSynchronize(r->stream));
    free_points(r);
    const int64_t tiles = grid_for(c, kBlock);
    if (dmalloc(&r->d_pos, 3 * c) || dmalloc(&r->d_col, 3 * c) || dmalloc(&r->rec, c) || dmalloc(&r->tile_cnt, tiles) ||
        dmalloc(&r->tile_off, tiles + 1))
        return NBMI_ERR_HIP;
    NBMI_HIP_CHECK(hipHostMalloc((void **)&r->h_stage, (size_t)6 * c * sizeof(float), hipHostMallocDefault));
    r->cap_pts = c;
    return 0;
}

int ensure_frags(nbmi_render *r, int64_t nf, int bits) {
    const size_t need_sort = nbmi::radix_temp_bytes_u32((size_t)nf, bits);
    if (nf <= r->cap_frags && need_sort <= r->sort_bytes) return 0;
    const int64_t c = std::min(kMaxFragments, std::max(nf, r->cap_frags + r->cap_frags / 2));
    free_frags(r);
    const int64_t tiles = grid_for(c, kResTile);
    const size_t sb = nbmi::radix_temp_bytes_u32((size_t)c, bits > 24 ? bits : 24);
    if (dmalloc(&r->keys, c) || dmalloc(&r->vals, c) || dmalloc(&r->keys2, c) || dmalloc(&r->vals2, c) ||
        dmalloc(&r->tile_min, tiles) || dmalloc(&r->tile_pre, tiles + 1))
        return NBMI_ERR_HIP;
    NBMI_HIP_CHECK(hipMalloc(&r->sort_tmp, sb));
    NBMI_HIP_CHECK(nbmi::radix_init_temp(r->sort_tmp, r->stream));
    r->sort_bytes = sb;
    r->cap_frags = c;
    return 0;
}

// The per-frame constants of the view (include/nbmi.h "Image semantics"), computed once on the host.
int make_view(const nbmi_render *r, const double *p, View *v, uint32_t bg8[3]) {
    if (!p) { nbmi::set_error("nbmi_render: null params"); return NBMI_ERR_ARG; }
    for (int k = 0; k < 17; k++)
        if (!isfinite(p[k])) { nbmi::set_error("nbmi_render: params[%d] is not finite", k); return NBMI_ERR_ARG; }
    const double fovy = p[9], zn = p[10], zf = p[11], ps = p[12], dens = p[13];
    if (!(fovy > 0.0 && fovy < 180.0) || !(zn > 0.0 && zf > zn)) {
        nbmi::set_error("nbmi_render: need 0 < fovy < 180 and 0 < near < far");
        return NBMI_ERR_ARG;
    }
    if (!(ps > 0.0 && ps <= 4.0)) { nbmi::set_error("nbmi_render: point_size %g outside (0, 4]", ps); return NBMI_ERR_ARG; }
    if (!(dens >= 0.0)) { nbmi::set_error("nbmi_render: fog_density must be >= 0"); return NBMI_ERR_ARG; }
    for (int k = 0; k < 3; k++)
        if (!(p[14 + k] >= 0.0 && p[14 + k] <= 1.0)) { nbmi::set_error("nbmi_render: bg outside [0, 1]"); return NBMI_ERR_ARG; }
    double f[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]};
    const double fl = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    if (!(fl > 0.0)) { nbmi::set_error("nbmi_render: eye == target"); return NBMI_ERR_ARG; }
    for (int k = 0; k < 3; k++) f[k] = f[k] / fl;
    const double *up = p + 6;
    double s[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
    const double sl = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    if (!(sl > 0.0)) { nbmi::set_error("nbmi_render: up is parallel to the view direction"); return NBMI_ERR_ARG; }
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
    v->R = ps / 2.0;
    v->R2 = v->R * v->R;
    v->dens = dens;
    v->W = r->W;
    v->H = r->H;
    for (int k = 0; k < 3; k++) bg8[k] = (uint32_t)floor(p[14 + k] * 255.0 + 0.5);
    return 0;
}

int key_bits(const nbmi_render *r) {
    const uint64_t P = (uint64_t)r->W * (uint64_t)r->H;
    int b = 1;
    while (((uint64_t)1 << b) < P) b++;
    return b;
}

// One frame of n points already in r->d_pos / r->d_col (enqueued behind whatever the stream holds).
int render_frame(nbmi_render *r, int64_t n, const View &v, const uint32_t bg8[3], uint8_t *out) {
    hipStream_t st = r->stream;
    const int64_t P = (int64_t)r->W * r->H;
    NBMI_HIP_CHECK(hipEventRecord(r->ev[0], st));
    NBMI_HIP_CHECK(hipMemsetAsync(r->acc, 0, (size_t)P * 3 * sizeof(unsigned long long), st));
    NBMI_HIP_CHECK(hipMemsetAsync(r->stats, 0, 4 * sizeof(unsigned long long), st));
    int64_t nf = 0;
    const int64_t tiles = grid_for(n, kBlock);
    if (n > 0) {
        k_count<<<(int)tiles, kBlock, 0, st>>>(v, r->d_pos, r->d_col, n, r->rec, r->tile_cnt, r->stats);
        scan::k_scan_values<<<1, scan::kScanThreads, 0, st>>>(r->tile_cnt, r->tile_off, tiles, (int64_t)0, (uint64_t)0,
                                                              scan::Sum());
        NBMI_HIP_CHECK(hipGetLastError());
        NBMI_HIP_CHECK(hipMemcpyAsync(r->h_small, r->tile_off + tiles, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    }
    NBMI_HIP_CHECK(hipEventRecord(r->ev[1], st));
    if (n > 0) {
        NBMI_HIP_CHECK(hipStreamSynchronize(st));
        nf = (int64_t)r->h_small[0];
        if (nf > kMaxFragments) {
            nbmi::set_error("nbmi_render: %lld fragments, more than the %lld one frame can sort", (long long)nf,
                            (long long)kMaxFragments);
            return NBMI_ERR_CAPACITY;
        }
    }
    const int bits = key_bits(r);
    if (nf > 0 && ensure_frags(r, nf, bits)) return NBMI_ERR_HIP;
    NBMI_HIP_CHECK(hipEventRecord(r->ev[2], st));
    if (nf > 0) {
        k_emit<<<(int)tiles, kBlock, 0, st>>>(v, r->d_pos, n, r->tile_off, r->keys, r->vals);
        NBMI_HIP_CHECK(hipGetLastError());
    }
    NBMI_HIP_CHECK(hipEventRecord(r->ev[3], st));
    if (nf > 0)
        NBMI_HIP_CHECK(nbmi::radix_sort_pairs_u32(r->sort_tmp, r->sort_bytes, r->keys, r->keys2, r->vals, r->vals2,
                                                  (size_t)nf, 0, bits, st));
    NBMI_HIP_CHECK(hipEventRecord(r->ev[4], st));
    if (nf > 0) {
        const int64_t rt = grid_for(nf, kResTile);
        k_resolve_min<<<(int)rt, kBlock, 0, st>>>(r->keys2, r->vals2, r->rec, nf, (uint64_t)P, r->tile_min);
        scan::k_scan_values<<<1, scan::kScanThreads, 0, st>>>(r->tile_min, r->tile_pre, rt, (int64_t)0, ~(uint64_t)0,
                                                              scan::Min());
        k_resolve<<<(int)rt, kBlock, 0, st>>>(r->keys2, r->vals2, r->rec, nf, (uint64_t)P, r->tile_pre, r->acc, r->stats);
        NBMI_HIP_CHECK(hipGetLastError());
    }
    NBMI_HIP_CHECK(hipEventRecord(r->ev[5], st));
    k_pack<<<grid_for(P, kBlock), kBlock, 0, st>>>(r->acc, r->W, r->H, bg8[0], bg8[1], bg8[2], r->d_img);
    NBMI_HIP_CHECK(hipGetLastError());
    NBMI_HIP_CHECK(hipMemcpyAsync(r->h_img, r->d_img, (size_t)P * 3, hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipMemcpyAsync(r->h_small + 1, r->stats, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    r->h_small[5] = 0;
    if (r->sort_tmp) NBMI_HIP_CHECK(nbmi::radix_error_word(r->sort_tmp, (unsigned *)(r->h_small + 5), st));
    NBMI_HIP_CHECK(hipEventRecord(r->ev[6], st));
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    r->timed = true;
    r->tri_frame = false;
    if (r->h_small[5]) {
        NBMI_HIP_CHECK(nbmi::radix_init_temp(r->sort_tmp, st));
        NBMI_HIP_CHECK(hipStreamSynchronize(st));
        nbmi::set_error("nbmi_render: device radix sort: a look-back spin timed out; the frame is invalid");
        return NBMI_ERR_HIP;
    }
    r->last_stats[0] = (int64_t)r->h_small[1];
    r->last_stats[1] = nf;
    r->last_stats[2] = (int64_t)r->h_small[3];
    r->last_stats[3] = (int64_t)r->h_small[4];
    memcpy(out, r->h_img, (size_t)P * 3);
    return 0;
}

int check_render(nbmi_render *r, const char *what) {
    if (!r) { nbmi::set_error("%s: null renderer", what); return NBMI_ERR_ARG; }
    if (hipSetDevice(r->device) != hipSuccess) { nbmi::set_error("hipSetDevice(%d) failed", r->device); return NBMI_ERR_HIP; }
    return 0;
}

}  // namespace

extern "C" {

void nbmi_render_destroy(nbmi_render *r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    free_points(r);
    free_frags(r);
    nbmi::raster_free(r);
    (void)hipFree(r->acc); (void)hipFree(r->stats); (void)hipFree(r->d_img);
    (void)hipHostFree(r->h_img); (void)hipHostFree(r->h_small);
    for (hipEvent_t &e : r->ev)
        if (e) (void)hipEventDestroy(e);
    if (r->ev_src) (void)hipEventDestroy(r->ev_src);
    if (r->stream) (void)hipStreamDestroy(r->stream);
    delete r;
}

nbmi_render *nbmi_render_create(int width, int height, int device) {
    nbmi::clear_error();
    if (width <= 0 || height <= 0 || width > kMaxSide || height > kMaxSide) {
        nbmi::set_error("nbmi_render_create: size %d x %d outside [1, %d]", width, height, kMaxSide);
        return nullptr;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) {
        (void)hipGetLastError();
        nbmi::set_error("nbmi_render_create: no HIP device %d (have %d)", device, count);
        return nullptr;
    }
    nbmi_render *r = new nbmi_render;
    r->W = width; r->H = height; r->device = device;
    const size_t P = (size_t)width * height;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
    for (hipEvent_t &ev : r->ev)
        if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->ev_src, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void **)&r->acc, P * 3 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void **)&r->stats, 4 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void **)&r->d_img, P * 3);
    if (e == hipSuccess) e = hipHostMalloc((void **)&r->h_img, P * 3, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void **)&r->h_small, 8 * sizeof(uint64_t), hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        nbmi::set_error("nbmi_render_create: %s", hipGetErrorString(e));
        nbmi_render_destroy(r);
        return nullptr;
    }
    return r;
}

int nbmi_render_points(nbmi_render *r, const float *pos, const float *col, int64_t n, const double *params, uint8_t *out) {
    if (int rc = check_render(r, "nbmi_render_points")) return rc;
    if (n < 0 || n >= kMaxPoints || !out || (n > 0 && (!pos || !col))) {
        nbmi::set_error("nbmi_render_points: bad arguments (n = %lld, at most %lld; null pointer?)", (long long)n,
                        (long long)kMaxPoints - 1);
        return NBMI_ERR_ARG;
    }
    View v;
    uint32_t bg8[3];
    if (int rc = make_view(r, params, &v, bg8)) return rc;
    if (n > 0) {
        if (ensure_points(r, n, true)) return NBMI_ERR_HIP;
        memcpy(r->h_stage, pos, (size_t)n * 12);
        memcpy(r->h_stage + 3 * n, col, (size_t)n * 12);
        NBMI_HIP_CHECK(hipMemcpyAsync(r->d_pos, r->h_stage, (size_t)n * 12, hipMemcpyHostToDevice, r->stream));
        NBMI_HIP_CHECK(hipMemcpyAsync(r->d_col, r->h_stage + 3 * n, (size_t)n * 12, hipMemcpyHostToDevice, r->stream));
    }
    return render_frame(r, n, v, bg8, out);
}

int nbmi_render_sim(nbmi_render *r, nbmi_sim *sim, const double *params, uint8_t *out) {
    if (int rc = check_render(r, "nbmi_render_sim")) return rc;
    if (!sim || !out) { nbmi::set_error("nbmi_render_sim: null argument"); return NBMI_ERR_ARG; }
    View v;
    uint32_t bg8[3];
    if (int rc = make_view(r, params, &v, bg8)) return rc;
    int64_t n = 0;
    int dev = 0;
    if (int rc = nbmi::render_source(sim, &n, &dev)) return rc;
    if (dev != r->device) {
        nbmi::set_error("nbmi_render_sim: the handle lives on device %d, the renderer on %d", dev, r->device);
        return NBMI_ERR_ARG;
    }
    if (n >= kMaxPoints) { nbmi::set_error("nbmi_render_sim: %lld bodies, at most %lld", (long long)n, (long long)kMaxPoints - 1); return NBMI_ERR_ARG; }
    if (n > 0) {
        if (hipSetDevice(r->device) != hipSuccess || ensure_points(r, n, false)) return NBMI_ERR_HIP;
        if (int rc = nbmi::render_fetch(sim, r->d_pos, r->d_col, r->ev_src)) return rc;
        NBMI_HIP_CHECK(hipSetDevice(r->device));
        NBMI_HIP_CHECK(hipStreamWaitEvent(r->stream, r->ev_src, 0));
    }
    return render_frame(r, n, v, bg8, out);
}

int nbmi_render_stats(nbmi_render *r, int64_t *out4) {
    if (int rc = check_render(r, "nbmi_render_stats")) return rc;
    if (!out4) { nbmi::set_error("nbmi_render_stats: null output"); return NBMI_ERR_ARG; }
    for (int k = 0; k < 4; k++) out4[k] = r->last_stats[k];
    return 0;
}

int nbmi_render_timers(nbmi_render *r, double *out_ms4) {
    if (int rc = check_render(r, "nbmi_render_timers")) return rc;
    if (!out_ms4) { nbmi::set_error("nbmi_render_timers: null output"); return NBMI_ERR_ARG; }
    for (int k = 0; k < 4; k++) out_ms4[k] = 0.0;
    if (!r->timed) return 0;
    if (r->tri_frame) {  // rasterise, resolve, copy
        float t[3];
        for (int k = 0; k < 3; k++) NBMI_HIP_CHECK(hipEventElapsedTime(&t[k], r->ev[k], r->ev[k + 1]));
        out_ms4[0] = t[0];
        out_ms4[2] = t[1];
        out_ms4[3] = t[2];
        return 0;
    }
    float t[6];
    for (int k = 0; k < 6; k++) NBMI_HIP_CHECK(hipEventElapsedTime(&t[k], r->ev[k], r->ev[k + 1]));
    out_ms4[0] = (double)t[0] + (double)t[2];  // count + scan, emit (not the host's read of the total between them)
    out_ms4[1] = t[3];
    out_ms4[2] = t[4];
    out_ms4[3] = t[5];
    return 0;
}

}  // extern "C"
