// Boids fixed-radius neighbour sweep on MI355X (gfx950).  C ABI in include/bdmi.h.
//
// One bdmi_step == one Flock.update(dt) of the reference (boids/flock.py:627-678):
//   assign_cells (:30-44) -> argsort + build_cell_lists (:610-625, :47-65) ->
//   compute_flocking_spatial (:68-238) -> update_physics_numba (:241-308).
// float64 state and arithmetic like the reference (this path is bandwidth bound; MI355X
// float64 vector rate is far above what ~7 candidates per boid need).
//
// HBM layout: master state SoA float64 {p, v, c} x 3 + int32 id, kept in CELL-SORTED order
// between steps (buffer A).  Per step: cell keys from A -> radix sort (cell, rank) -> gather A into
// the read-side copy B (array of 32-byte {x,y,z,-} records per quantity: one cache line per
// neighbour position) -> 1-bit-per-cell occupancy map + {start,end} pair per non-empty cell ->
// sweep kernel tests the occupancy bit (L2 resident) before touching the pair table, reads
// neighbours from B and writes the updated boid back to A at the same rank, physics fused.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/bdmi.h"
#include "common.h"
#include "visible.h"
#include "unionfind.h"

namespace {

constexpr int kBlock = 256;

struct Boids {
    double *px, *py, *pz, *vx, *vy, *vz, *cr, *cg, *cb;
    int32_t *id;
};

// read-side copy of the boids for the sweep: array of structures, one 32-byte record per boid and
// quantity, so that a neighbour's position is ONE cache line (the SoA master touches three)
struct BoidsAoS {
    double4 *p, *v, *c;  // {x,y,z,-}, {vx,vy,vz,-}, {r,g,b,-}
    int32_t *id;
};

// Flock.__init__'s grid (flock.py:478-481): the cell is the perception radius, so a boid's neighbours lie in the 3 x 3 x 3
// cells around its own, whatever the parameters
struct GridP {
    static constexpr bool kPeriodic = false;
    double cell_size, offset;
    int dim;
};
// The grid of a periodic handle (include/bdmi.h, "Periodic handles"): the box [-B, B]^3 cut into dim^3 cells of
// L / dim >= the perception radius, offset = B; the 27 cells around a boid wrap modulo dim.  The same members first, so
// that cell_coord is one function; B and L serve the minimum image and the wrap of the integration.
struct GridPer {
    static constexpr bool kPeriodic = true;
    double cell_size, offset;
    int dim;
    double B, L;
};

struct FlockP {
    static constexpr bool kNoisy = false;
    double perception_sq, separation_sq, sep_w, ali_w, coh_w, max_speed, max_force;
    double bounds, margin, wall_force, blend, dt;
};
// A step with the noise term of include/bdmi.h ("Noise"): amp = eta * max_force, and the Philox key and counter words
struct FlockPN : FlockP {
    static constexpr bool kNoisy = true;
    double amp;
    uint32_t seed_lo, seed_hi, step_lo, step_hi;
};

// get_cell_index (flock.py:16-27): int() truncation toward zero, then clamp
template <class G>
__device__ __forceinline__ int cell_coord(double v, const G &g) {
    int c = (int)((v + g.offset) / g.cell_size);
    c = c < 0 ? 0 : c;
    c = c > g.dim - 1 ? g.dim - 1 : c;
    return c;
}

// (A periodic handle runs k_assign and k_cells_out as they are: its grid is the GridP part of its GridPer.)
__global__ __launch_bounds__(kBlock) void k_assign(Boids a, int64_t n, GridP g, uint32_t *__restrict__ keys,
                                                   uint32_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int cx = cell_coord(a.px[i], g), cy = cell_coord(a.py[i], g), cz = cell_coord(a.pz[i], g);
    keys[i] = (uint32_t)(cx + cy * g.dim + cz * g.dim * g.dim);
    idx[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kBlock) void k_reorder(Boids a, BoidsAoS b, const uint32_t *__restrict__ perm, int64_t n) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const uint32_t j = perm[r];
    b.p[r] = make_double4(a.px[j], a.py[j], a.pz[j], 0.0);
    b.v[r] = make_double4(a.vx[j], a.vy[j], a.vz[j], 0.0);
    b.c[r] = make_double4(a.cr[j], a.cg[j], a.cb[j], 0.0);
    b.id[r] = a.id[j];
}

// build_cell_lists (flock.py:47-65) from sorted keys, as a COMPACT table: the non-empty cells are
// numbered in cell order (rank k), cell_start[k] = first sorted boid of the k-th non-empty cell
// (its end is cell_start[k + 1]); occ[w] = {bits, prefix}: one bit per cell of the 32 cells of word w
// (non-empty or not) and the rank of the word's first non-empty cell, so that one 8-byte load gives
//     rank(cell) = occ[cell >> 5].prefix + popcount(occ[cell >> 5].bits & ((1 << (cell & 31)) - 1)).
// 2 MB + 4 B per non-empty cell, all cache resident; the table indexed by cell (66 MB at the
// reference grid, one random 128-byte line per lookup) was where the sweep's HBM traffic came from.
// The tile compaction of scan.h over the sorted keys, selecting the first boid of each cell.
struct FirstOfCell {
    const uint32_t *keys_s;
    __device__ unsigned operator()(int64_t first, int64_t n) const {
        return scan::item_mask(first, n, [&](int64_t r) { return r == 0 || keys_s[r - 1] != keys_s[r]; });
    }
};
struct EmitTable {
    const uint32_t *keys_s;
    int64_t n;
    const uint32_t *tile_cnt;
    int64_t ntiles;
    uint2 *occ;
    int32_t *cell_start;
    __device__ void operator()(unsigned m, int64_t first, int64_t slot) const {
        unsigned rank = (unsigned)slot;
        // a thread's 8 consecutive boids usually fall into one or two occupancy words: OR their bits
        // locally and issue one atomic per word
        uint32_t pend_word = 0xffffffffu, pend_bits = 0u;
#pragma unroll
        for (int k = 0; k < scan::kItems; k++) {
            if (!((m >> k) & 1u)) continue;
            const int64_t r = first + k;
            const uint32_t c = keys_s[r];
            cell_start[rank] = (int32_t)r;
            if ((c >> 5) != pend_word) {
                if (pend_bits) atomicOr(&occ[pend_word].x, pend_bits);
                pend_word = c >> 5;
                pend_bits = 0u;
            }
            pend_bits |= 1u << (c & 31);
            if (r == 0 || (keys_s[r - 1] >> 5) != (c >> 5)) occ[c >> 5].y = rank;
            rank++;
        }
        if (pend_bits) atomicOr(&occ[pend_word].x, pend_bits);
        if (blockIdx.x == 0 && threadIdx.x == 0) cell_start[tile_cnt[ntiles]] = (int32_t)n;  // end of the last cell
    }
};

// number of non-empty cells of the last grid; on demand only (bdmi_grid_info), one atomic per block
__global__ __launch_bounds__(kBlock) void k_count_cells(const uint32_t *__restrict__ keys_s, int64_t n,
                                                        unsigned long long *occupied) {
    __shared__ unsigned red[kBlock / 64];
    unsigned cnt = 0;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock)
        cnt += (r == 0 || keys_s[r - 1] != keys_s[r]) ? 1u : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; w++) cnt += red[w];
        atomicAdd(occupied, (unsigned long long)cnt);
    }
}

// steer(): mean -> normalise * max_speed - v -> clamp to max_force -> * weight
// (the repeated block of flock.py:174-234); returns false if the magnitude is 0.
__device__ __forceinline__ bool steer(double &x, double &y, double &z, double vx, double vy, double vz,
                                      double max_speed, double max_force, double w) {
    double mag = sqrt(x * x + y * y + z * z);
    if (!(mag > 0)) return false;
    x = (x / mag) * max_speed - vx;
    y = (y / mag) * max_speed - vy;
    z = (z / mag) * max_speed - vz;
    mag = sqrt(x * x + y * y + z * z);
    if (mag > max_force) {
        x = (x / mag) * max_force;
        y = (y / mag) * max_force;
        z = (z / mag) * max_force;
    }
    x *= w; y *= w; z *= w;
    return true;
}

// XCD-aware block remap (same idea as the tree walk's): hardware deals consecutive blocks round-robin
// over the 8 XCDs, each with its own L2.  A boid's candidates sit up to ~grid_dim^2 * density ranks
// away in the cell-sorted order (the cz +- 1 planes), so each XCD gets one CONTIGUOUS eighth of the
// blocks and finds them in its own L2 instead of re-fetching them from HBM.  xcd_contiguous = 0
// keeps the hardware order (measurement knob BDMI_XCD=0).
__device__ __forceinline__ int64_t logical_block(int b, int nb, int xcd_contiguous) {
    if (!xcd_contiguous) return b;
    const int xcd = b & 7, j = b >> 3;
    const int q = nb >> 3, rem = nb & 7;
    return (int64_t)xcd * q + (xcd < rem ? xcd : rem) + j;
}

// The image of a candidate q for the boid at p (include/bdmi.h): per axis q + L if p - q > B, q - L if p - q < -B, else q
// itself (equality does not shift).  Every formula of the sweep then takes the image for the neighbour's position.  On a
// walled grid this is the identity and costs nothing.
template <class G>
__device__ __forceinline__ double4 image_of(const double4 &p, const double4 &q, const G &g) {
    if constexpr (G::kPeriodic) {
        auto axis = [&](double pc, double qc) {
            const double d0 = pc - qc;
            return d0 > g.B ? qc + g.L : (d0 < -g.B ? qc - g.L : qc);
        };
        return make_double4(axis(p.x, q.x), axis(p.y, q.y), axis(p.z, q.z), q.w);
    } else {
        return q;
    }
}

// xi_i(step) of include/bdmi.h: Marsaglia's (1972) unit vector from the first pair of Philox words inside the unit disc.
// One Philox block in the common case (two pairs, each accepted with probability pi / 4); the rejection loop is per lane.
__device__ __forceinline__ void noise_xi(uint32_t id, uint32_t step_lo, uint32_t step_hi, uint32_t seed_lo, uint32_t seed_hi,
                                         double &x, double &y, double &z) {
    const uint32_t key[2] = {seed_lo, seed_hi};
    for (uint32_t a = 0;; a++) {
        const uint32_t ctr[4] = {id, step_lo, step_hi, a};
        uint32_t w[4];
        nbmi::philox4x32_10(ctr, key, w);
#pragma unroll
        for (int pr = 0; pr < 2; pr++) {
            const double x1 = ((double)w[2 * pr] + 0.5) * 0x1p-31 - 1.0, x2 = ((double)w[2 * pr + 1] + 0.5) * 0x1p-31 - 1.0;
            const double s = x1 * x1 + x2 * x2;
            if (s < 1.0) {
                const double t = sqrt(1.0 - s);
                x = (2.0 * x1) * t; y = (2.0 * x2) * t; z = 1.0 - 2.0 * s;
                return;
            }
        }
    }
}

// The neighbour sums of one boid, and one neighbour's contribution to them (flock.py:150-172): shared by the metric
// sweep (k_flock, both of its candidate loops) and the topological one (k_flock_topo).
struct FlockSums {
    double sx = 0, sy = 0, sz = 0, alx = 0, aly = 0, alz = 0, cox = 0, coy = 0, coz = 0, clr = 0, clg = 0, clb = 0;
    int sep_count = 0, nb_count = 0;
    __device__ __forceinline__ void add(const double4 &pi, const double4 &qp, const double4 &qv, const double4 &qc,
                                        double separation_sq) {
        const double dx = pi.x - qp.x, dy = pi.y - qp.y, dz = pi.z - qp.z;
        const double dist_sq = dx * dx + dy * dy + dz * dz;
        if (dist_sq < separation_sq) {
            const double dist = sqrt(dist_sq);
            const double inv_dist = 1.0 / dist;
            sx += dx * inv_dist / dist;
            sy += dy * inv_dist / dist;
            sz += dz * inv_dist / dist;
            sep_count++;
        }
        alx += qv.x; aly += qv.y; alz += qv.z;
        cox += qp.x; coy += qp.y; coz += qp.z;
        clr += qc.x; clg += qc.y; clb += qc.z;
        nb_count++;
    }
};

// The end of compute_flocking_spatial (means and steer(), flock.py:174-238) and update_physics_numba (flock.py:241-308)
// for the boid at rank r (records pi4, vi4, ci4), from its neighbour sums.  kPhysics=false: write the four force arrays
// (caller's boid order) instead of integrating.  A periodic grid drops the wall terms and wraps the new position once; a
// noisy PP adds amp * xi to the acceleration (not to the four force arrays).  Both are compile-time: the walled,
// noise-free instance is the code it was.
template <bool kPhysics, class G, class PP>
__device__ __forceinline__ void flock_finish(const BoidsAoS &b, const Boids &a, int64_t r, const G &g, const PP &P, const double4 &pi4,
                                             const double4 &vi4, const double4 &ci4, FlockSums S, double *__restrict__ o_sep,
                                             double *__restrict__ o_ali, double *__restrict__ o_coh, double *__restrict__ o_avg) {
    const double pix = pi4.x, piy = pi4.y, piz = pi4.z, vix = vi4.x, viy = vi4.y, viz = vi4.z, cir = ci4.x, cig = ci4.y, cib = ci4.z;
    const int nb_count = S.nb_count;
    double fsx = 0, fsy = 0, fsz = 0, fax = 0, fay = 0, faz = 0, fcx = 0, fcy = 0, fcz = 0;
    double avr = cir, avg = cig, avb = cib;  // caller pre-fill: avg_colors <- colors (flock.py:636)
    if (S.sep_count > 0) {
        S.sx /= S.sep_count; S.sy /= S.sep_count; S.sz /= S.sep_count;
        if (steer(S.sx, S.sy, S.sz, vix, viy, viz, P.max_speed, P.max_force, P.sep_w)) { fsx = S.sx; fsy = S.sy; fsz = S.sz; }
    }
    if (nb_count > 0) {
        S.alx /= nb_count; S.aly /= nb_count; S.alz /= nb_count;
        if (steer(S.alx, S.aly, S.alz, vix, viy, viz, P.max_speed, P.max_force, P.ali_w)) { fax = S.alx; fay = S.aly; faz = S.alz; }
        S.cox = S.cox / nb_count - pix; S.coy = S.coy / nb_count - piy; S.coz = S.coz / nb_count - piz;
        if (steer(S.cox, S.coy, S.coz, vix, viy, viz, P.max_speed, P.max_force, P.coh_w)) { fcx = S.cox; fcy = S.coy; fcz = S.coz; }
        avr = (S.clr + cir) / (nb_count + 1);
        avg = (S.clg + cig) / (nb_count + 1);
        avb = (S.clb + cib) / (nb_count + 1);
    }
    if (!kPhysics) {
        const int64_t o = 3 * (int64_t)b.id[r];
        o_sep[o] = fsx; o_sep[o + 1] = fsy; o_sep[o + 2] = fsz;
        o_ali[o] = fax; o_ali[o + 1] = fay; o_ali[o + 2] = faz;
        o_coh[o] = fcx; o_coh[o + 1] = fcy; o_coh[o + 2] = fcz;
        o_avg[o] = avr; o_avg[o + 1] = avg; o_avg[o + 2] = avb;
        return;
    }
    double acc[3] = {fsx + fax + fcx, fsy + fay + fcy, fsz + faz + fcz};
    if constexpr (PP::kNoisy) {
        double xi[3];
        noise_xi((uint32_t)b.id[r], P.step_lo, P.step_hi, P.seed_lo, P.seed_hi, xi[0], xi[1], xi[2]);
#pragma unroll
        for (int d = 0; d < 3; d++) acc[d] += P.amp * xi[d];
    }
    const double pos[3] = {pix, piy, piz};
    if constexpr (!G::kPeriodic) {
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const double dist_pos = pos[d] - (P.bounds - P.margin);
            if (dist_pos > 0) acc[d] -= fmin(dist_pos / P.margin * 2.0, 1.0) * P.wall_force;
            const double dist_neg = (-P.bounds + P.margin) - pos[d];
            if (dist_neg > 0) acc[d] += fmin(dist_neg / P.margin * 2.0, 1.0) * P.wall_force;
        }
    }
    double nvx = vix + acc[0] * P.dt, nvy = viy + acc[1] * P.dt, nvz = viz + acc[2] * P.dt;
    const double speed = sqrt(nvx * nvx + nvy * nvy + nvz * nvz);
    if (speed > P.max_speed) {
        const double scale = P.max_speed / speed;
        nvx *= scale; nvy *= scale; nvz *= scale;
    }
    a.vx[r] = nvx; a.vy[r] = nvy; a.vz[r] = nvz;
    if constexpr (G::kPeriodic) {
        // bdmi_step has checked max_speed * |dt| < L: one wrap brings the boid back into [-B, B]
        auto wrapped = [&](double x) { return x > g.B ? x - g.L : (x < -g.B ? x + g.L : x); };
        a.px[r] = wrapped(pix + nvx * P.dt); a.py[r] = wrapped(piy + nvy * P.dt); a.pz[r] = wrapped(piz + nvz * P.dt);
    } else {
        a.px[r] = pix + nvx * P.dt; a.py[r] = piy + nvy * P.dt; a.pz[r] = piz + nvz * P.dt;
    }
    a.cr[r] = cir + (avr - cir) * P.blend;
    a.cg[r] = cig + (avg - cig) * P.blend;
    a.cb[r] = cib + (avb - cib) * P.blend;
    a.id[r] = b.id[r];
}

// ---- the candidate runs of a boid ----------------------------------------------------------------------------------------
// The reference visits the 27 cells around a boid one by one (flock.py:117-132).  Cells that differ only in x have
// consecutive indices, and boids are sorted by cell index, so the candidates of one (y, z) row of cells are ONE contiguous
// run of sorted boids: nine runs instead of 27 cell visits, each found with two rank lookups in the compact table.  Same
// candidate set as the reference; the floating-point sums run in a different order (the reference's own order inside a
// cell is unspecified anyway: np.argsort, flock.py:618).
//
// emit(q_begin, q_end) for the non-empty rows around the boid at p, in row order (z outer, y inner): the one lookup of
// every kernel that sweeps the grid.  A row of cells is 3 cells = at most two words of the occupancy table, and what a row
// costs is a chain of dependent loads (table word -> run bounds -> candidates), not arithmetic: the three rows of a z plane
// go through each stage TOGETHER, so that their loads are in flight at the same time.
//
// On a periodic grid (GridPer) the rows wrap in y and z, and in x a boid in cell 0 or dim - 1 has its three cells in TWO
// runs of the sorted order ({dim-1} and {0, 1}, or {dim-2, dim-1} and {0}): up to 18 runs per boid, one row's two segments
// next to each other.  dim >= 3 keeps the 27 wrapped cells distinct, so every boid is a candidate once.  Same shape: the
// table words of a z plane's six segments are requested before any is used.
struct RunWords {
    uint2 wa, wb;
    int lo_bit, hi_bit;
    bool two, ok;
};
// the occupancy words of the cells [c_lo, c_hi] of one row (at most two words)
__device__ __forceinline__ RunWords run_words(const uint2 *__restrict__ occ, int64_t c_lo, int64_t c_hi, bool ok) {
    RunWords w;
    w.ok = ok;
    w.lo_bit = (int)(c_lo & 31);
    w.hi_bit = (int)(c_hi & 31);
    w.two = (c_lo >> 5) != (c_hi >> 5);
    w.wa = ok ? occ[c_lo >> 5] : make_uint2(0u, 0u);
    w.wb = (ok && w.two) ? occ[c_hi >> 5] : make_uint2(0u, 0u);
    return w;
}
// the run [qb, qe) of sorted boids in those cells; qb == qe == 0 when all are empty
__device__ __forceinline__ void run_bounds(const RunWords &w, const int32_t *__restrict__ cell_start, int32_t &qb, int32_t &qe) {
    uint32_t ba = w.wa.x & (~0u << w.lo_bit);
    uint32_t bb = w.wb.x & (~0u >> (31 - w.hi_bit));
    if (!w.two) { ba &= ~0u >> (31 - w.hi_bit); bb = 0u; }
    qb = 0; qe = 0;
    if (w.ok && (ba | bb)) {
        const uint2 fw = ba ? w.wa : w.wb;
        const int first = ba ? __ffs(ba) - 1 : __ffs(bb) - 1;
        const uint2 lw = bb ? w.wb : w.wa;
        const int last = bb ? 31 - __clz(bb) : 31 - __clz(ba);
        qb = cell_start[fw.y + __popc(fw.x & ((1u << first) - 1u))];
        qe = cell_start[lw.y + __popc(lw.x & ((1u << last) - 1u)) + 1u];
    }
}
template <class Emit>
__device__ __forceinline__ void for_each_run(const double4 &p, const GridPer &g, const uint2 *__restrict__ occ,
                                             const int32_t *__restrict__ cell_start, Emit emit) {
    const int dim = g.dim;
    const int cx = cell_coord(p.x, g), cy = cell_coord(p.y, g), cz = cell_coord(p.z, g);
    // segment 0 = the cells next to each other, segment 1 = the one cell through the x face (face cells only)
    int lo[2] = {cx - 1, 0}, hi[2] = {cx + 1, 0};
    const bool face = cx == 0 || cx == dim - 1;
    if (cx == 0) { lo[0] = 0; hi[0] = 1; lo[1] = hi[1] = dim - 1; }
    if (cx == dim - 1) { lo[0] = dim - 2; hi[0] = dim - 1; lo[1] = hi[1] = 0; }
    for (int dz = -1; dz <= 1; dz++) {
        int ncz = cz + dz;
        ncz = ncz < 0 ? dim - 1 : (ncz >= dim ? 0 : ncz);
        RunWords w[6];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            int ncy = cy + j - 1;
            ncy = ncy < 0 ? dim - 1 : (ncy >= dim ? 0 : ncy);
            const int64_t row = (int64_t)ncy * dim + (int64_t)ncz * dim * dim;
            w[2 * j] = run_words(occ, row + lo[0], row + hi[0], true);
            w[2 * j + 1] = run_words(occ, row + lo[1], row + hi[1], face);
        }
        int32_t qb[6], qe[6];
#pragma unroll
        for (int j = 0; j < 6; j++) run_bounds(w[j], cell_start, qb[j], qe[j]);
#pragma unroll
        for (int j = 0; j < 6; j++)
            if (qe[j] > qb[j]) emit(qb[j], qe[j]);
    }
}

// ... and the walled grid's nine runs (the periodic overload is above)
template <class Emit>
__device__ __forceinline__ void for_each_run(const double4 &p, const GridP &g, const uint2 *__restrict__ occ,
                                             const int32_t *__restrict__ cell_start, Emit emit) {
    const int cx = cell_coord(p.x, g), cy = cell_coord(p.y, g), cz = cell_coord(p.z, g);
    const int x_lo = cx - 1 < 0 ? 0 : cx - 1;
    const int x_hi = cx + 1 > g.dim - 1 ? g.dim - 1 : cx + 1;
    for (int ncz = cz - 1; ncz <= cz + 1; ncz++) {
        const bool zok = ncz >= 0 && ncz < g.dim;
        uint2 wa[3], wb[3];
        int lo_bit[3], hi_bit[3];
        bool two[3], rok[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int ncy = cy + j - 1;
            rok[j] = zok && ncy >= 0 && ncy < g.dim;
            const int64_t row = (int64_t)ncy * g.dim + (int64_t)ncz * g.dim * g.dim;
            const int64_t c_lo = row + x_lo, c_hi = row + x_hi;
            lo_bit[j] = (int)(c_lo & 31);
            hi_bit[j] = (int)(c_hi & 31);
            two[j] = (c_lo >> 5) != (c_hi >> 5);
            wa[j] = rok[j] ? occ[c_lo >> 5] : make_uint2(0u, 0u);
            wb[j] = (rok[j] && two[j]) ? occ[c_hi >> 5] : make_uint2(0u, 0u);
        }
        int32_t qb[3], qe[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            uint32_t ba = wa[j].x & (~0u << lo_bit[j]);
            uint32_t bb = wb[j].x & (~0u >> (31 - hi_bit[j]));
            if (!two[j]) { ba &= ~0u >> (31 - hi_bit[j]); bb = 0u; }
            qb[j] = 0; qe[j] = 0;
            if (rok[j] && (ba | bb)) {
                // first and last non-empty cell of the row
                const uint2 fw = ba ? wa[j] : wb[j];
                const int first = ba ? __ffs(ba) - 1 : __ffs(bb) - 1;
                const uint2 lw = bb ? wb[j] : wa[j];
                const int last = bb ? 31 - __clz(bb) : 31 - __clz(ba);
                const uint32_t k_lo = fw.y + __popc(fw.x & ((1u << first) - 1u));
                const uint32_t k_hi = lw.y + __popc(lw.x & ((1u << last) - 1u)) + 1u;
                qb[j] = cell_start[k_lo];
                qe[j] = cell_start[k_hi];
            }
        }
#pragma unroll
        for (int j = 0; j < 3; j++)
            if (qe[j] > qb[j]) emit(qb[j], qe[j]);
    }
}

// The sweeps (k_flock, topo_select) only NOTE the runs, in the lane's LDS column runs[2 row], runs[2 row + 1][thread], and
// walk all nine in ONE loop behind the lookups [r4]; only the non-empty runs are noted, so that loop never has to step over
// an empty one.  Returns their number; big = one of them is longer than the 16-bit notes of k_flock can address.
// A walled boid has up to 9 runs: 4 bits of row, 12 of offset.  A periodic one has up to 18: 5 bits of row, 11 of offset,
// and the one-by-one path above 2047.
template <class G>
struct RunNotes {
    static constexpr int kRuns = G::kPeriodic ? 18 : 9;
    static constexpr int kOffBits = G::kPeriodic ? 11 : 12;
    static constexpr int kMaxLen = (1 << kOffBits) - 1;
};
template <int kThreads, class G>
__device__ __forceinline__ int note_runs(const double4 &p, const G &g, const uint2 *__restrict__ occ,
                                         const int32_t *__restrict__ cell_start, int32_t (*runs)[kThreads], bool &big) {
    int nr = 0;
    big = false;
    for_each_run(p, g, occ, cell_start, [&](int32_t qb, int32_t qe) {
        runs[2 * nr][threadIdx.x] = qb;
        runs[2 * nr + 1][threadIdx.x] = qe;
        nr++;
        big = big || qe - qb > RunNotes<G>::kMaxLen;
    });
    return nr;
}

// A lane's nr > 0 noted runs back to back: next() is the next candidate rank, or -1 behind the last one, and `code` its
// (row << kOffBits) | offset in the row's run (k_flock's 16-bit note of a neighbour).
template <int kThreads, int kOffBits>
struct RunCursor {
    const int32_t (*runs)[kThreads];
    int nr, row = 0;
    int32_t q, e, q_first;
    __device__ __forceinline__ RunCursor(const int32_t (*runs_)[kThreads], int nr_) : runs(runs_), nr(nr_) {
        q = q_first = runs[0][threadIdx.x];
        e = runs[1][threadIdx.x];
    }
    __device__ __forceinline__ int32_t next(unsigned &code) {
        if (q >= e) {  // the run is used up: on to the next noted one (none of them is empty)
            if (row + 1 >= nr) { row = nr; return -1; }
            row++;
            q = q_first = runs[2 * row][threadIdx.x];
            e = runs[2 * row + 1][threadIdx.x];
        }
        code = ((unsigned)row << kOffBits) | (unsigned)(q - q_first);
        return q++;
    }
};
// The walk over a lane's noted runs: four candidates per trip with their position records requested together;
// before_trip() ahead of every trip, test(rank, code, position record) for every candidate in run order.  (A lane
// without runs leaves at once: with the cursor's first loads behind a condition of their own the compiler wrapped lookup
// and walk into one wave-level loop, 1.1 - 1.6 % on the topological sweep at k = 16: profiles/boids_runs_ab.txt.)
template <int kThreads, int kOffBits, class Before, class Test>
__device__ __forceinline__ void walk_runs(const double4 *__restrict__ pos, const int32_t (*runs)[kThreads], int nr,
                                          Before before_trip, Test test) {
    if (nr == 0) return;
    RunCursor<kThreads, kOffBits> cur(runs, nr);
    for (;;) {
        before_trip();
        unsigned k0 = 0, k1 = 0, k2 = 0, k3 = 0;
        const int32_t c0 = cur.next(k0);
        if (c0 < 0) break;
        const int32_t c1 = cur.next(k1), c2 = cur.next(k2), c3 = cur.next(k3);
        const double4 p0 = pos[c0], p1 = pos[c1 < 0 ? c0 : c1], p2 = pos[c2 < 0 ? c0 : c2], p3 = pos[c3 < 0 ? c0 : c3];
        test(c0, k0, p0);
        if (c1 >= 0) test(c1, k1, p1);
        if (c2 >= 0) test(c2, k2, p2);
        if (c3 >= 0) test(c3, k3, p3);
    }
}

// compute_flocking_spatial (flock.py:68-238) + update_physics_numba (flock.py:241-308).
// kPhysics=false: write the four force arrays (caller's boid order) instead of integrating.
// G = GridP or GridPer, PP = FlockP or FlockPN (a noisy step): the walled, noise-free instances are the kernels they
// were.  LDS per block: 18 KiB of runs + 16 KiB of notes = 34 KiB walled (4 blocks = 16 waves per CU), 36 + 16 = 52 KiB
// periodic (3 blocks = 12 waves per CU).
template <bool kPhysics, class G, class PP>
__global__ __launch_bounds__(kBlock) void k_flock(BoidsAoS b, Boids a, const uint2 *__restrict__ occ,
                                                  const int32_t *__restrict__ cell_start, int64_t n, G g, PP P,
                                                  double *__restrict__ o_sep, double *__restrict__ o_ali,
                                                  double *__restrict__ o_coh, double *__restrict__ o_avg,
                                                  int xcd_contiguous) {
    constexpr int kOffBits = RunNotes<G>::kOffBits;
    __shared__ int32_t runs[2 * RunNotes<G>::kRuns][kBlock];  // [2 row, 2 row + 1][thread]: candidate run of the thread's boid in each of its rows
    constexpr int kHitCap = 32;
    __shared__ unsigned short hits[kHitCap][kBlock];  // [k][thread]: the boid's neighbours found so far, (row << kOffBits) | offset in the row's run
    const int64_t r = logical_block(blockIdx.x, gridDim.x, xcd_contiguous) * kBlock + threadIdx.x;
    if (r >= n) return;
    const double4 pi4 = b.p[r], vi4 = b.v[r], ci4 = b.c[r];
    if (kPhysics && b.id[r] < 0) {
        // a ghost (slab mode: a neighbour slab's boid inside the halo): visible to the others, owned elsewhere
        a.px[r] = pi4.x; a.py[r] = pi4.y; a.pz[r] = pi4.z;
        a.vx[r] = vi4.x; a.vy[r] = vi4.y; a.vz[r] = vi4.z;
        a.cr[r] = ci4.x; a.cg[r] = ci4.y; a.cb[r] = ci4.z;
        a.id[r] = b.id[r];
        return;
    }
    FlockSums S;
    // the reference's test of one candidate (flock.py:134-148)
    auto in_sight = [&](const double4 &q) {
        const double4 qp = image_of(pi4, q, g);
        const double dx = pi4.x - qp.x, dy = pi4.y - qp.y, dz = pi4.z - qp.z;
        const double dist_sq = dx * dx + dy * dy + dz * dz;
        return dist_sq < P.perception_sq && dist_sq > 0.0001;
    };
    bool big;
    const int nr = note_runs<kBlock>(pi4, g, occ, cell_start, runs, big);
    // [r4] One flattened candidate loop per boid instead of nine, in two phases.  In the state flocks reach (53
    // candidates per boid instead of 9, two thirds of the cells empty, the rest holding more) the nine per-row
    // loops cost a wave the SUM of the rows' longest runs among its 64 boids; one loop over a lane's nine runs back
    // to back costs the longest TOTAL.  And only one candidate in six is a neighbour (a sphere of one cell size in
    // a cube of three), yet nearly every trip of the loop had SOME lane with one, so the wave ran the expensive
    // half of the body - a float64 square root, four divisions, two dependent 32-byte loads - on every trip with
    // a sixth of its lanes (66 % of the sweep's wave cycles were waits, 85 vector instructions per trip:
    // profiles/r04_boids_steady_state_ab.txt).  Now phase 1 only tests distances, four candidates per trip
    // with their position records requested together, and notes the neighbours (16 bits each: row and offset in
    // the row's run) in a per-lane list in LDS; phase 2 walks that list - every lane busy with a real neighbour,
    // two at a time with all six records in flight.  Same neighbours in the same order: results unchanged bit
    // for bit.  Sweep at 2 M boids: 0.275 -> 0.205 ms on the initial state, 0.783 -> 0.579 ms after 1000 steps.
    // (Measured and dropped: phase 1 on an fp32 copy of the positions relative to the cell centres, eight per trip,
    // float64 re-test inside the fp32 error band - same sets, 0.67 ms: the sweep waits for its gathers, it is not
    // short of arithmetic or bytes.)
    int nh = 0;
    auto flush = [&]() {
        for (int h = 0; h < nh; h += 2) {
            const unsigned e0 = hits[h][threadIdx.x], e1 = hits[h + 1 < nh ? h + 1 : h][threadIdx.x];
            const int32_t q0 = runs[2 * (e0 >> kOffBits)][threadIdx.x] + (int32_t)(e0 & ((1u << kOffBits) - 1u));
            const int32_t q1 = runs[2 * (e1 >> kOffBits)][threadIdx.x] + (int32_t)(e1 & ((1u << kOffBits) - 1u));
            const double4 p0 = b.p[q0], v0 = b.v[q0], c0 = b.c[q0], p1 = b.p[q1], v1 = b.v[q1], c1 = b.c[q1];
            S.add(pi4, image_of(pi4, p0, g), v0, c0, P.separation_sq);
            if (h + 1 < nh) S.add(pi4, image_of(pi4, p1, g), v1, c1, P.separation_sq);
        }
        nh = 0;
    };
    if (big) {
        // a run of more than 4095 boids (three cells!; 2047 on a periodic grid): its offsets do not fit the 16-bit
        // notes - such a boid takes its candidates one by one
        for (int k = 0; k < nr; k++)
            for (int32_t q = runs[2 * k][threadIdx.x]; q < runs[2 * k + 1][threadIdx.x]; q++) {
                if (q == r) continue;
                const double4 qp = b.p[q];
                if (in_sight(qp)) S.add(pi4, image_of(pi4, qp, g), b.v[q], b.c[q], P.separation_sq);
            }
    } else {
        walk_runs<kBlock, kOffBits>(
            b.p, runs, nr, [&]() { if (nh > kHitCap - 4) flush(); },
            [&](int32_t c, unsigned code, const double4 &qp) {
                if (c != r && in_sight(qp)) hits[nh++][threadIdx.x] = (unsigned short)code;
            });
        flush();
    }
    flock_finish<kPhysics>(b, a, r, g, P, pi4, vi4, ci4, S, o_sep, o_ali, o_coh, o_avg);
}

// ---- topological interaction: the k nearest within sight (include/bdmi.h has the specification) ------
// T_i = the first min(k, |N_i|) members of the metric set N_i in ascending (d2, caller's id) order.  The selection below
// keeps, per lane, an ascending list of at most k entries {d2, rank q} in LDS columns [slot][thread]; the sums then run
// over that list in its order, from +0.0, so the forces are a function of the state and the ids alone - not of the cell
// order, the row order or the block order.
constexpr int kTopoMaxK = 16;

// The list of the boid at rank r (position pi4): ld2 / lq [slot][thread], ascending; returns its length.  Candidates come
// from the nine row runs, noted and walked back to back as in k_flock.  The common case of a candidate inside the window
// is a reject against the current k-th d2 (kept in a register); ids are loaded only to break an exact d2 tie.  Ranks are
// stored whole, so a run may have any length.
template <int kCap, int kThreads, class G>
__device__ __forceinline__ int topo_select(const BoidsAoS &b, const uint2 *__restrict__ occ, const int32_t *__restrict__ cell_start,
                                           const G &g, int64_t r, const double4 &pi4, double perception_sq, int k,
                                           int32_t (*runs)[kThreads], double (*ld2)[kThreads], int32_t (*lq)[kThreads]) {
    const int t = threadIdx.x;
    int cnt = 0;
    double worst = INFINITY;  // d2 of the k-th entry once the list is full
    auto insert = [&](double d2, int32_t q) {
        // (d2, id_q) before (pd, id_pq)?  ids differ, so the order is total
        auto before = [&](double pd, int32_t pq) { return d2 < pd || (d2 == pd && b.id[q] < b.id[pq]); };
        int pos;
        if (cnt == k) {
            if (d2 > worst) return;
            if (!before(worst, lq[k - 1][t])) return;
            pos = k - 1;  // the last entry falls out
        } else {
            pos = cnt++;
        }
        while (pos > 0) {
            const double pd = ld2[pos - 1][t];
            const int32_t pq = lq[pos - 1][t];
            if (!before(pd, pq)) break;
            ld2[pos][t] = pd;
            lq[pos][t] = pq;
            pos--;
        }
        ld2[pos][t] = d2;
        lq[pos][t] = q;
        if (cnt == k) worst = ld2[k - 1][t];
    };
    bool big;  // (no 16-bit notes here)
    const int nr = note_runs<kThreads>(pi4, g, occ, cell_start, runs, big);
    walk_runs<kThreads, RunNotes<G>::kOffBits>(
        b.p, runs, nr, [] {},
        [&](int32_t c, unsigned, const double4 &q) {
            if (c == r) return;
            const double4 qp = image_of(pi4, q, g);  // d2 is the image's
            const double dx = pi4.x - qp.x, dy = pi4.y - qp.y, dz = pi4.z - qp.z;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 < perception_sq && d2 > 0.0001) insert(d2, c);
        });
    return cnt;
}

// compute_flocking_spatial with T_i in the place of the neighbour set + update_physics_numba.  kCap = the largest k this
// instance serves: k <= 8 runs 256 threads per block (18 KiB of runs + 24 KiB of list = 42 KiB, 3 blocks = 12 waves per
// CU), k <= 16 runs 128 threads per block (9 + 24 = 33 KiB, 4 blocks = 8 waves per CU).  On a periodic grid the runs
// are twice as many: 36 + 24 = 60 KiB (2 blocks = 8 waves per CU) and 18 + 24 = 42 KiB (3 blocks = 6 waves per CU).
template <bool kPhysics, int kCap, int kThreads, class G, class PP>
__global__ __launch_bounds__(kThreads) void k_flock_topo(BoidsAoS b, Boids a, const uint2 *__restrict__ occ,
                                                         const int32_t *__restrict__ cell_start, int64_t n, G g, PP P,
                                                         int k, double *__restrict__ o_sep, double *__restrict__ o_ali,
                                                         double *__restrict__ o_coh, double *__restrict__ o_avg,
                                                         int xcd_contiguous) {
    __shared__ int32_t runs[2 * RunNotes<G>::kRuns][kThreads];
    __shared__ double ld2[kCap][kThreads];
    __shared__ int32_t lq[kCap][kThreads];
    const int t = threadIdx.x;
    const int64_t r = logical_block(blockIdx.x, gridDim.x, xcd_contiguous) * kThreads + t;
    if (r >= n) return;
    const double4 pi4 = b.p[r], vi4 = b.v[r], ci4 = b.c[r];
    const int cnt = topo_select<kCap, kThreads>(b, occ, cell_start, g, r, pi4, P.perception_sq, k, runs, ld2, lq);
    FlockSums S;
    // the list in its order, two entries at a time with all six records in flight
    for (int h = 0; h < cnt; h += 2) {
        const int32_t q0 = lq[h][t], q1 = lq[h + 1 < cnt ? h + 1 : h][t];
        const double4 p0 = b.p[q0], v0 = b.v[q0], c0 = b.c[q0], p1 = b.p[q1], v1 = b.v[q1], c1 = b.c[q1];
        S.add(pi4, image_of(pi4, p0, g), v0, c0, P.separation_sq);
        if (h + 1 < cnt) S.add(pi4, image_of(pi4, p1, g), v1, c1, P.separation_sq);
    }
    flock_finish<kPhysics>(b, a, r, g, P, pi4, vi4, ci4, S, o_sep, o_ali, o_coh, o_avg);
}

// bdmi_topological_neighbours: the lists themselves, rows in the caller's order, padded with -1 / +inf
template <int kCap, int kThreads, class G>
__global__ __launch_bounds__(kThreads) void k_topo_rows(BoidsAoS b, const uint2 *__restrict__ occ,
                                                        const int32_t *__restrict__ cell_start, int64_t n, G g,
                                                        double perception_sq, int k, int32_t *__restrict__ o_ids,
                                                        double *__restrict__ o_d2, int32_t *__restrict__ o_count) {
    __shared__ int32_t runs[2 * RunNotes<G>::kRuns][kThreads];
    __shared__ double ld2[kCap][kThreads];
    __shared__ int32_t lq[kCap][kThreads];
    const int t = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * kThreads + t;
    if (r >= n) return;
    const int cnt = topo_select<kCap, kThreads>(b, occ, cell_start, g, r, b.p[r], perception_sq, k, runs, ld2, lq);
    const int64_t i = b.id[r];
    for (int s = 0; s < k; s++) {
        o_ids[i * k + s] = s < cnt ? b.id[lq[s][t]] : -1;
        o_d2[i * k + s] = s < cnt ? ld2[s][t] : INFINITY;
    }
    o_count[i] = cnt;
}

__global__ __launch_bounds__(kBlock) void k_split(const double *__restrict__ p, const double *__restrict__ v,
                                                  const double *__restrict__ c, Boids a, int64_t n, int by_id) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const int64_t i = by_id ? (int64_t)a.id[r] : r;
    if (p) { a.px[r] = p[3 * i]; a.py[r] = p[3 * i + 1]; a.pz[r] = p[3 * i + 2]; }
    if (v) { a.vx[r] = v[3 * i]; a.vy[r] = v[3 * i + 1]; a.vz[r] = v[3 * i + 2]; }
    if (c) { a.cr[r] = c[3 * i]; a.cg[r] = c[3 * i + 1]; a.cb[r] = c[3 * i + 2]; }
    if (!by_id) a.id[r] = (int32_t)r;
}

__global__ __launch_bounds__(kBlock) void k_join(const double *__restrict__ x, const double *__restrict__ y,
                                                 const double *__restrict__ z, const int32_t *__restrict__ id, int64_t n,
                                                 double *__restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const int64_t o = 3 * (int64_t)id[r];
    out[o] = x[r]; out[o + 1] = y[r]; out[o + 2] = z[r];
}

__global__ __launch_bounds__(kBlock) void k_cells_out(Boids a, int64_t n, GridP g, int32_t *__restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const int cx = cell_coord(a.px[r], g), cy = cell_coord(a.py[r], g), cz = cell_coord(a.pz[r], g);
    out[a.id[r]] = cx + cy * g.dim + cz * g.dim * g.dim;
}

// bdmi_noise_vectors: xi_i(step) for the caller ids i = 0 .. n - 1
__global__ __launch_bounds__(kBlock) void k_noise_vectors(int64_t n, uint32_t seed_lo, uint32_t seed_hi, uint32_t step_lo,
                                                          uint32_t step_hi, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double x, y, z;
    noise_xi((uint32_t)i, step_lo, step_hi, seed_lo, seed_hi, x, y, z);
    out[3 * i] = x; out[3 * i + 1] = y; out[3 * i + 2] = z;
}

// ---- slab mode (multi-GPU): selections of rows by a predicate, in row order ------------------------------
// what = 0: owned rows (id >= 0); 1: owned rows in the LEFT halo zone (x < x_lo + cell); 2: RIGHT (x >= x_hi - cell)
struct SlabSel {
    const double *px;
    const int32_t *id;
    int what;
    double lo_edge, hi_edge;
    __device__ bool operator()(int64_t r) const {
        if (id[r] < 0) return false;
        if (what == 0) return true;
        return what == 1 ? px[r] < lo_edge : px[r] >= hi_edge;
    }
};
struct SlabMask {
    SlabSel sel;
    __device__ unsigned operator()(int64_t first, int64_t n) const { return scan::item_mask(first, n, sel); }
};
// selected rows -> packed rows {p, v, c, id} of 10 doubles (dst_rows) or -> the SoA arrays `dst` (compaction)
struct EmitRows {
    Boids src, dst;
    double *dst_rows;
    __device__ void operator()(unsigned m, int64_t first, int64_t first_slot) const {
        scan::for_each_item(m, first, first_slot, [&](int64_t r, int64_t slot) {
            if (dst_rows) {
                double *o = dst_rows + 10 * slot;
                o[0] = src.px[r]; o[1] = src.py[r]; o[2] = src.pz[r];
                o[3] = src.vx[r]; o[4] = src.vy[r]; o[5] = src.vz[r];
                o[6] = src.cr[r]; o[7] = src.cg[r]; o[8] = src.cb[r];
                o[9] = (double)src.id[r];
            } else {
                dst.px[slot] = src.px[r]; dst.py[slot] = src.py[r]; dst.pz[slot] = src.pz[r];
                dst.vx[slot] = src.vx[r]; dst.vy[slot] = src.vy[r]; dst.vz[slot] = src.vz[r];
                dst.cr[slot] = src.cr[r]; dst.cg[slot] = src.cg[r]; dst.cb[slot] = src.cb[r];
                dst.id[slot] = src.id[r];
            }
        });
    }
};
// owned rows that have left the slab stay for this step as ghosts (their new owner got a copy)
__global__ __launch_bounds__(kBlock) void k_slab_demote(Boids a, int64_t n, double x_lo, double x_hi) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const double x = a.px[r];
    if (a.id[r] >= 0 && !(x >= x_lo && x < x_hi)) a.id[r] = -1 - a.id[r];
}
// received rows: inside the slab -> owned, else a ghost
__global__ __launch_bounds__(kBlock) void k_slab_append(Boids a, int64_t at, const double *__restrict__ rows, int64_t count,
                                                        double x_lo, double x_hi) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= count) return;
    const double *o = rows + 10 * k;
    const int64_t r = at + k;
    a.px[r] = o[0]; a.py[r] = o[1]; a.pz[r] = o[2];
    a.vx[r] = o[3]; a.vy[r] = o[4]; a.vz[r] = o[5];
    a.cr[r] = o[6]; a.cg[r] = o[7]; a.cb[r] = o[8];
    const int32_t gid = (int32_t)o[9];
    a.id[r] = (o[0] >= x_lo && o[0] < x_hi) ? gid : -1 - gid;
}
__global__ __launch_bounds__(kBlock) void k_set_ids(const int32_t *__restrict__ ids, int32_t *__restrict__ dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) dst[i] = ids[i];
}

// ---- flock analysis: bdmi_flocks / bdmi_flock_catalogue / bdmi_diagnostics / bdmi_neighbour_stats ----------------
// (include/bdmi.h has the definitions, DESIGN.md section 4.21 the measurements.)  All four work on the grid that
// enqueue_grid builds for the current positions: B = the boids in cell order, occ / cell_start = the compact table.
struct FlockStats {
    int32_t *parent = nullptr, *root = nullptr, *minid = nullptr, *cnt = nullptr;  // union-find over ranks; per root
    int32_t *lcnt = nullptr;                                 // members of the flock with this label (at [label])
    uint32_t *lab = nullptr, *lab_s = nullptr;               // label of rank r; the same, sorted
    uint32_t *rank = nullptr, *rank_s = nullptr;             // 0 .. n-1; the ranks in the order a stable sort by label leaves
    uint32_t *qkey = nullptr, *qkey_s = nullptr, *qval = nullptr, *qval_s = nullptr;  // qualifying heads: n - members, position
    unsigned long long *counters = nullptr;                  // links, evals, flocks, neighbour evals
    // catalogue rows, grown on demand: chunk offsets, per-chunk partials of the two passes, the rows themselves
    int32_t *chunk_off = nullptr;
    double *part = nullptr, *rows16 = nullptr;
    int32_t *row_label = nullptr;
    int64_t *row_members = nullptr;
    // ... on a periodic handle also per row: the occupancy words of its three axes, the cuts, the unwrapped centre
    uint32_t *occ_mask = nullptr;
    int32_t *wrap3 = nullptr;
    double *centre = nullptr;
    int64_t rows_cap = 0, chunks_cap = 0;
    // bdmi_velocity_correlation, allocated at its first call: the quantised fluctuations in rank order, the call's words
    int4 *vc_q = nullptr;
    unsigned long long *vc_acc = nullptr;
    double vc_e2[65] = {};  // the squared edges of the call in flight (the source of their upload)
};

// d2(i, j) of the header: three products, two sums, symmetric in its arguments
__device__ __forceinline__ double fs_d2(const double4 &a, const double4 &b) {
    const double dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
    return (dx * dx + dy * dy) + dz * dz;
}
// ... and the d2 of the periodic flock analysis (include/bdmi.h, "Flock analysis on periodic handles"): the DIFFERENCE is
// brought into [-B, B], not the neighbour's position as in image_of, so d2(i, j) and d2(j, i) are the same bits and the
// link relation does not depend on which boid of a pair evaluates it.  Equality does not shift.
template <class G>
__device__ __forceinline__ double fs_dist(const double4 &a, const double4 &b, const G &g) {
    if constexpr (G::kPeriodic) {
        auto axis = [&](double d) { return d > g.B ? d - g.L : (d < -g.B ? d + g.L : d); };
        const double dx = axis(b.x - a.x), dy = axis(b.y - a.y), dz = axis(b.z - a.z);
        return (dx * dx + dy * dy) + dz * dz;
    } else {
        return fs_d2(a, b);
    }
}

__global__ __launch_bounds__(kBlock) void k_fs_init(int64_t n, int32_t *__restrict__ parent, int32_t *__restrict__ minid,
                                                    int32_t *__restrict__ cnt, uint32_t *__restrict__ rank) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    fof_init(r, parent, minid, cnt);
    rank[r] = (uint32_t)r;
}
// The link kernel: one lane per rank r takes the candidates q < r of its nine rows, so every candidate pair is evaluated
// exactly once (by its higher rank) and `links` is the exact number of linked pairs - a pair is NOT skipped because its
// boids are in one set already.  A run of any length is walked in place: there are no 16-bit notes here.  Every access
// to parent[] goes through unionfind.h (agent-scope relaxed atomics, invariants (a)-(d)); no loop waits on another thread.
// G = GridP or GridPer (the up to 18 wrapped runs and fs_dist's d2; dim >= 3 keeps the 27 cells distinct, so a pair is
// still met once): the GridP instance is the kernel it was.
template <class G>
__global__ __launch_bounds__(kBlock) void k_fs_link(const double4 *__restrict__ pos, const uint2 *__restrict__ occ,
                                                    const int32_t *__restrict__ cell_start, int64_t n, G g, double b2,
                                                    int32_t *parent, unsigned long long *counters) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    long long links = 0, evals = 0;
    if (r < n) {
        const double4 pi = pos[r];
        int mine = (int)r;  // an ancestor of r: its own rank at first, then the root the last unite came back with
        for_each_run(pi, g, occ, cell_start, [&](int32_t qb, int32_t qe) {
            const int32_t e = qe < (int32_t)r ? qe : (int32_t)r;
            for (int32_t q = qb; q < e; q++) {
                const double d2 = fs_dist(pi, pos[q], g);
                evals++;
                if (d2 <= b2) {
                    links++;
                    mine = fof_unite(parent, mine, q);
                }
            }
        });
    }
    nbmi::wave_add(counters + 0, links, threadIdx.x & 63);
    nbmi::wave_add(counters + 1, evals, threadIdx.x & 63);
}
// Behind the kernel boundary parent[] is final and read plainly (fof_flatten): root[r], minid[root] = the smallest caller
// index and cnt[root] = the members below it.
__global__ __launch_bounds__(kBlock) void k_fs_flatten(int64_t n, const int32_t *__restrict__ parent,
                                                       const int32_t *__restrict__ id, int32_t *__restrict__ root,
                                                       int32_t *__restrict__ minid, int32_t *__restrict__ cnt) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    fof_flatten(r, n, parent, root, minid, cnt, [&](int64_t q) { return id[q]; });
}
// label of every rank, of every boid in the caller's order, the members per label, and the number of roots
__global__ __launch_bounds__(kBlock) void k_fs_labels(int64_t n, const int32_t *__restrict__ root,
                                                      const int32_t *__restrict__ minid, const int32_t *__restrict__ cnt,
                                                      const int32_t *__restrict__ id, uint32_t *__restrict__ lab,
                                                      int32_t *__restrict__ lcnt, int32_t *__restrict__ labels,
                                                      unsigned long long *__restrict__ n_roots) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool is_root = false;
    if (r < n) {
        const int32_t f = root[r], l = minid[f];
        is_root = f == (int32_t)r;
        lab[r] = (uint32_t)l;
        labels[id[r]] = l;
        if (is_root) lcnt[l] = cnt[r];
    }
    nbmi::wave_add(n_roots, is_root ? 1ll : 0ll, threadIdx.x & 63);
}
// The full sweep of the nine rows per boid: count[i] = #{j != i : d2 <= r2}, nn_d2[i] = the least such d2 or +inf.
// An integer count and a minimum: exact whatever the order.  G as in k_fs_link.
template <class G>
__global__ __launch_bounds__(kBlock) void k_fs_neighbours(const double4 *__restrict__ pos, const int32_t *__restrict__ id,
                                                          const uint2 *__restrict__ occ, const int32_t *__restrict__ cell_start,
                                                          int64_t n, G g, double r2, int32_t *__restrict__ count,
                                                          double *__restrict__ nn_d2, unsigned long long *evals_out) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    long long evals = 0;
    if (r < n) {
        const double4 pi = pos[r];
        int32_t c = 0;
        double least = INFINITY;
        for_each_run(pi, g, occ, cell_start, [&](int32_t qb, int32_t qe) {
            for (int32_t q = qb; q < qe; q++) {
                if (q == (int32_t)r) continue;
                const double d2 = fs_dist(pi, pos[q], g);
                evals++;
                if (d2 <= r2) {
                    c++;
                    least = d2 < least ? d2 : least;
                }
            }
        });
        const int32_t i = id[r];
        count[i] = c;
        nn_d2[i] = least;
    }
    nbmi::wave_add(evals_out, evals, threadIdx.x & 63);
}

// ---- velocity correlation: bdmi_velocity_correlation (include/bdmi.h) ------------------------
// The one boids query that looks further than sight: the cells within m of the boid's own, per axis.  for_each_run_wide is
// for_each_run with that reach, for both grids: the (2m+1)^2 rows (cy+b, cz+c), clamped and skipped where out of a walled
// grid, wrapped on a periodic one; a row's x cells [cx-m, cx+m] are one clamped segment (walled) or up to two wrapped ones
// (periodic; 2m+1 <= dim keeps them apart).  A segment is up to 33 cells = up to three words of the occupancy table.  Same
// shape as run_words / run_bounds: three rows go through each stage together - table words, then the cell_start bounds
// of the first and last non-empty cell, then one run per segment.  m == 1 emits the runs of for_each_run.
__device__ __forceinline__ double fs_heading(const double4 &v, double &ux, double &uy, double &uz);  // with the rows, below
constexpr int kVcMaxBins = 64, kVcMaxReach = 16;
struct WideWords {
    uint32_t x0, x1, x2, y0, y1, y2;  // the words' bits and prefixes (scalars: selected by value, never through an index)
    int lo_bit, hi_bit, nw;           // nw == 0: the segment does not exist
};
__device__ __forceinline__ WideWords wide_words(const uint2 *__restrict__ occ, int64_t c_lo, int64_t c_hi, bool ok) {
    WideWords s;
    s.lo_bit = (int)(c_lo & 31);
    s.hi_bit = (int)(c_hi & 31);
    s.nw = ok ? (int)((c_hi >> 5) - (c_lo >> 5)) + 1 : 0;
    const int64_t w0 = c_lo >> 5;
    const uint2 a = s.nw > 0 ? occ[w0] : make_uint2(0u, 0u);
    const uint2 b = s.nw > 1 ? occ[w0 + 1] : make_uint2(0u, 0u);
    const uint2 c = s.nw > 2 ? occ[w0 + 2] : make_uint2(0u, 0u);
    s.x0 = a.x; s.y0 = a.y; s.x1 = b.x; s.y1 = b.y; s.x2 = c.x; s.y2 = c.y;
    return s;
}
__device__ __forceinline__ void wide_bounds(const WideWords &s, const int32_t *__restrict__ cell_start, int32_t &qb, int32_t &qe) {
    const uint32_t top = ~0u >> (31 - s.hi_bit);
    const uint32_t b0 = s.x0 & (~0u << s.lo_bit) & (s.nw == 1 ? top : ~0u);
    const uint32_t b1 = s.x1 & (s.nw == 2 ? top : ~0u);
    const uint32_t b2 = s.x2 & top;  // (zero words where the segment has fewer than three)
    qb = 0; qe = 0;
    if (b0 | b1 | b2) {
        // first and last non-empty cell of the segment; the words are picked with masks (a conditional between record
        // members became a load through a computed address, and the records stayed in scratch memory)
        const uint32_t f0 = b0 ? ~0u : 0u, f1 = ~f0 & (b1 ? ~0u : 0u), f2 = ~f0 & ~f1;
        const uint32_t l2 = b2 ? ~0u : 0u, l1 = ~l2 & (b1 ? ~0u : 0u), l0 = ~l2 & ~l1;
        const uint32_t fx = (s.x0 & f0) | (s.x1 & f1) | (s.x2 & f2), fy = (s.y0 & f0) | (s.y1 & f1) | (s.y2 & f2);
        const uint32_t fb = (b0 & f0) | (b1 & f1) | (b2 & f2);
        const uint32_t lx = (s.x0 & l0) | (s.x1 & l1) | (s.x2 & l2), ly = (s.y0 & l0) | (s.y1 & l1) | (s.y2 & l2);
        const uint32_t lb = (b0 & l0) | (b1 & l1) | (b2 & l2);
        const int first = __ffs(fb) - 1, last = 31 - __clz(lb);
        qb = cell_start[fy + __popc(fx & ((1u << first) - 1u))];
        qe = cell_start[ly + __popc(lx & ((1u << last) - 1u)) + 1u];
    }
}
template <class G, class Emit>
__device__ __forceinline__ void for_each_run_wide(const double4 &p, const G &g, int m, const uint2 *__restrict__ occ,
                                                  const int32_t *__restrict__ cell_start, Emit emit) {
    const int dim = g.dim;
    const int cx = cell_coord(p.x, g), cy = cell_coord(p.y, g), cz = cell_coord(p.z, g);
    // segment 0 = the cells around cx that are next to each other, segment 1 = those through the x face (periodic only)
    int lo0 = cx - m, hi0 = cx + m, lo1 = 0, hi1 = 0;
    bool second = false;
    if constexpr (G::kPeriodic) {
        if (lo0 < 0) { lo1 = lo0 + dim; hi1 = dim - 1; lo0 = 0; second = true; }
        else if (hi0 > dim - 1) { lo1 = 0; hi1 = hi0 - dim; hi0 = dim - 1; second = true; }
    } else {
        lo0 = lo0 < 0 ? 0 : lo0;
        hi0 = hi0 > dim - 1 ? dim - 1 : hi0;
    }
    for (int c = -m; c <= m; c++) {
        int ncz = cz + c;
        if constexpr (G::kPeriodic) ncz = ncz < 0 ? ncz + dim : (ncz >= dim ? ncz - dim : ncz);
        else if (ncz < 0 || ncz >= dim) continue;
        // the words of row cy + b: its segment 0, or its segment 1 where there is one
        auto words = [&](int b, bool seg1) {
            int ncy = cy + b;
            bool rok = b <= m && (!seg1 || second);
            if constexpr (G::kPeriodic) ncy = ncy < 0 ? ncy + dim : (ncy >= dim ? ncy - dim : ncy);
            else rok = rok && ncy >= 0 && ncy < dim;
            const int64_t row = rok ? (int64_t)ncy * dim + (int64_t)ncz * dim * dim : 0;
            return wide_words(occ, row + (seg1 ? lo1 : lo0), row + (seg1 ? hi1 : hi0), rok);
        };
        for (int b0 = -m; b0 <= m; b0 += 3) {
            // six named records, nothing indexed: what decides whether they stay in registers is wide_bounds' masks
            const WideWords w0 = words(b0, false), w1 = words(b0, true), w2 = words(b0 + 1, false), w3 = words(b0 + 1, true),
                            w4 = words(b0 + 2, false), w5 = words(b0 + 2, true);
            int32_t qb0, qe0, qb1, qe1, qb2, qe2, qb3, qe3, qb4, qe4, qb5, qe5;
            wide_bounds(w0, cell_start, qb0, qe0);
            wide_bounds(w1, cell_start, qb1, qe1);
            wide_bounds(w2, cell_start, qb2, qe2);
            wide_bounds(w3, cell_start, qb3, qe3);
            wide_bounds(w4, cell_start, qb4, qe4);
            wide_bounds(w5, cell_start, qb5, qe5);
            // one copy of emit's body: the run is picked by compares
#pragma unroll 1
            for (int j = 0; j < 6; j += G::kPeriodic ? 1 : 2) {
                const int32_t rb = j == 0 ? qb0 : j == 1 ? qb1 : j == 2 ? qb2 : j == 3 ? qb3 : j == 4 ? qb4 : qb5;
                const int32_t re = j == 0 ? qe0 : j == 1 ? qe1 : j == 2 ? qe2 : j == 3 ? qe3 : j == 4 ? qe4 : qe5;
                if (re > rb) emit(rb, re);
            }
        }
    }
}

// The device words of one call, zeroed on the stream ahead of the kernels: per slot k {pairs, the sum's low part, its high
// part}, then {sum qx, sum qy, sum qz, Q low, Q high}, then evals; behind them the squared edges E[0 .. nb] as doubles.
constexpr int kVcSlots = kVcMaxBins + 1;
constexpr int kVcSelf = 3 * kVcSlots, kVcEvals = kVcSelf + 5, kVcZeroed = kVcEvals + 1, kVcEdges = 208;
constexpr int kVcWords = kVcEdges + kVcSlots;
static_assert(kVcEdges >= kVcZeroed, "the edges lie behind the zeroed words");

// Ranks in a grid-stride loop (cell order when the grid was built: bv / bid are B's; else A's rows as they stand, bv == null):
// q = rint((u - mean) 2^24) per component, 0 where the difference is not finite, as int4 with the caller id in w; and the
// five sums of self5.  Q = qx^2 + qy^2 + qz^2 <= 3 * 2^50 per boid goes in as its low 32 bits and the rest, so that for
// n < 2^31 neither 64-bit sum can wrap.  At most kVcQuantBlocks blocks and five atomics per block: the sums end in five
// words, and one wave per 64 boids adding to them took 1.9 ms at 2 M boids, nearly all of it the atomics on those addresses.
constexpr int kVcQuantBlocks = 512;
__global__ __launch_bounds__(kBlock) void k_vc_quantise(const double4 *__restrict__ bv, const int32_t *__restrict__ bid, Boids a,
                                                        int64_t n, double mx, double my, double mz, int4 *__restrict__ qv,
                                                        unsigned long long *acc) {
    long long sx = 0, sy = 0, sz = 0, q_lo = 0, q_hi = 0;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock) {
        const double4 v = bv ? bv[r] : make_double4(a.vx[r], a.vy[r], a.vz[r], 0.0);
        double ux, uy, uz;
        (void)fs_heading(v, ux, uy, uz);
        auto quant = [](double d) { return isfinite(d) ? (long long)rint(d * 16777216.0) : 0ll; };
        const long long qx = quant(ux - mx), qy = quant(uy - my), qz = quant(uz - mz);
        if (qv) qv[r] = make_int4((int)qx, (int)qy, (int)qz, bv ? bid[r] : a.id[r]);
        const long long Q = qx * qx + qy * qy + qz * qz;
        sx += qx; sy += qy; sz += qz;
        q_lo += Q & 0xffffffffll;
        q_hi += Q >> 32;
    }
    // wave sums by shuffles, the block's four through LDS, then five atomics per block
    __shared__ long long red[5][kBlock / 64];
    long long v[5] = {sx, sy, sz, q_lo, q_hi};
#pragma unroll
    for (int c = 0; c < 5; c++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[c] += __shfl_xor(v[c], o);
        if ((threadIdx.x & 63) == 0) red[c][threadIdx.x >> 6] = v[c];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        long long t = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; w++) t += red[threadIdx.x][w];
        if (t != 0ll)
            (void)__hip_atomic_fetch_add(acc + kVcSelf + threadIdx.x, (unsigned long long)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The pair kernel: one lane per rank r takes the candidates q < r of its runs (k_fs_link's rule: every candidate pair is
// met once, by its higher rank), loads pos[q] and qv[q] together, takes fs_dist, finds the slot by a binary search over the
// E[k] in LDS and adds 1 and g = q_r . q_q to the block's counters: three 64-bit LDS words per slot {pairs, sum of the low
// 32 bits of g, sum of g >> 32}.  g = (g >> 32) 2^32 + (g & 0xffffffff) with an arithmetic shift, so the three are plain
// integer sums.  A lane has fewer than 2^31 candidates: the high word stays below 2^8 * 2^31 * 3 * 2^18 < 2^59; the low word
// could wrap, so its add returns the old value and a wrap carries 2^32 into the high word.  The flush is one agent-scope
// integer atomic per non-empty word into acc[], with the same carry; evals goes through one LDS word and one atomic per
// block.  Integers only: the result does not depend on any order.  No floating-point atomic, no flag, nothing waits on
// another lane.
template <class G>
__global__ __launch_bounds__(kBlock) void k_vc_pairs(const double4 *__restrict__ pos, const int4 *__restrict__ qv,
                                                     const uint2 *__restrict__ occ, const int32_t *__restrict__ cell_start,
                                                     int64_t n, G g, int m, int nb, unsigned long long *acc, int xcd_contiguous) {
    __shared__ double sE[kVcSlots];
    __shared__ unsigned long long s_cnt[kVcSlots], s_lo[kVcSlots], s_hi[kVcSlots], s_evals;
    if (threadIdx.x == 0) s_evals = 0ull;
    if (threadIdx.x <= nb) {
        sE[threadIdx.x] = reinterpret_cast<const double *>(acc + kVcEdges)[threadIdx.x];
        s_cnt[threadIdx.x] = 0ull; s_lo[threadIdx.x] = 0ull; s_hi[threadIdx.x] = 0ull;
    }
    __syncthreads();
    const int64_t r = logical_block((int)blockIdx.x, (int)gridDim.x, xcd_contiguous) * kBlock + threadIdx.x;
    long long evals = 0;
    if (r < n) {
        const double4 pi = pos[r];
        const int4 qi = qv[r];
        const double e_max = sE[nb];
        for_each_run_wide(pi, g, m, occ, cell_start, [&](int32_t qb, int32_t qe) {
            const int32_t e = qe < (int32_t)r ? qe : (int32_t)r;
            for (int32_t q = qb; q < e; q++) {
                const double4 pj = pos[q];
                const int4 qj = qv[q];
                const double d2 = fs_dist(pi, pj, g);
                evals++;
                if (d2 <= e_max) {  // (a NaN d2 is in no slot)
                    int lo = 0, hi = nb;
                    while (lo < hi) {  // the first k with d2 <= E[k]
                        const int mid = (lo + hi) >> 1;
                        if (sE[mid] < d2) lo = mid + 1; else hi = mid;
                    }
                    const long long gg = (long long)qi.x * qj.x + (long long)qi.y * qj.y + (long long)qi.z * qj.z;
                    const unsigned long long low = (unsigned long long)gg & 0xffffffffull;
                    long long high = gg >> 32;
                    atomicAdd(&s_cnt[lo], 1ull);
                    const unsigned long long old = atomicAdd(&s_lo[lo], low);
                    if (old + low < old) high += 1ll << 32;
                    atomicAdd(&s_hi[lo], (unsigned long long)high);
                }
            }
        });
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) evals += __shfl_xor(evals, o);
    if ((threadIdx.x & 63) == 0 && evals) atomicAdd(&s_evals, (unsigned long long)evals);
    __syncthreads();
    if (threadIdx.x == kBlock - 1 && s_evals)
        (void)__hip_atomic_fetch_add(acc + kVcEvals, s_evals, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x <= nb) {
        unsigned long long *out = acc + 3 * threadIdx.x;
        const unsigned long long c = s_cnt[threadIdx.x], low = s_lo[threadIdx.x];
        unsigned long long high = s_hi[threadIdx.x];
        if (c) (void)__hip_atomic_fetch_add(out, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (low) {
            const unsigned long long old = __hip_atomic_fetch_add(out + 1, low, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old + low < old) high += 1ull << 32;
        }
        if (high) (void)__hip_atomic_fetch_add(out + 2, high, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the heads (first member) of the flocks with at least min_members members, in label order
struct FsHeadSel {
    const uint32_t *lab_s;
    const int32_t *lcnt;
    int64_t min_members;
    __device__ unsigned operator()(int64_t first, int64_t n) const {
        return scan::item_mask(first, n, [&](int64_t h) {
            return (h == 0 || lab_s[h - 1] != lab_s[h]) && (int64_t)lcnt[lab_s[h]] >= min_members;
        });
    }
};
struct FsEmitHead {
    const uint32_t *lab_s;
    const int32_t *lcnt;
    int64_t n;
    uint32_t *qkey, *qval;
    __device__ void operator()(unsigned m, int64_t first, int64_t first_slot) const {
        scan::for_each_item(m, first, first_slot, [&](int64_t h, int64_t slot) {
            qkey[slot] = (uint32_t)(n - (int64_t)lcnt[lab_s[h]]);  // ascending = members descending
            qval[slot] = (uint32_t)h;
        });
    }
};

// ---- the rows of 16 doubles ------------------------------------------------------------------------------------------
// Row `row` has the members [head, head + m) of the sorted member list (head = rhead[row], m = n - rkey[row]), member j
// being the boid of rank rank_s[j] (rank j where rank_s is null: bdmi_diagnostics).  The members are cut into chunks of
// 4096; chunk_off[row] = the first chunk of the row in the partials, chunk_off[rows] = their number.  One block per
// chunk: thread t adds the members t, t + 256, .. of the chunk in this order, the 64 lanes of a wave are folded by the
// butterfly over the distances 32, 16, .. 1, the four waves left to right; k_fs_combine then adds a row's chunks in chunk
// order.  Nothing here depends on timing: the same state gives the same bits.
constexpr int kFsChunk = 4096;
constexpr int kFsVals = 16;  // pass 1: Sp[3], Sv[3], Su[3], Ss, lo[3], hi[3]; pass 2: Sw[3]

__device__ __forceinline__ int fs_row_of(const int32_t *__restrict__ chunk_off, int rows, int b) {
    int lo = 0, hi = rows;  // chunk_off[lo] <= b < chunk_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_off[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}
// op 0: sum, 1: min, 2: max
__device__ __forceinline__ double fs_fold(int op, double a, double b) { return op == 0 ? a + b : op == 1 ? (b < a ? b : a) : (b > a ? b : a); }
template <int K>
__device__ __forceinline__ void fs_block_fold(double (&v)[K], const int (&op)[K], double *__restrict__ out) {
    __shared__ double red[K][kBlock / 64];
#pragma unroll
    for (int c = 0; c < K; c++) {
        double x = v[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x = fs_fold(op[c], x, __shfl_xor(x, o));
        if ((threadIdx.x & 63) == 0) red[c][threadIdx.x >> 6] = x;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const int c = threadIdx.x;
        double x = red[c][0];
        for (int w = 1; w < kBlock / 64; w++) x = fs_fold(op[c], x, red[c][w]);
        out[c] = x;
    }
}
// u = v / |v| per component (0 for a boid at rest) and the speed
__device__ __forceinline__ double fs_heading(const double4 &v, double &ux, double &uy, double &uz) {
    const double s = sqrt((v.x * v.x + v.y * v.y) + v.z * v.z);
    ux = uy = uz = 0.0;
    if (s != 0.0) { ux = v.x / s; uy = v.y / s; uz = v.z / s; }
    return s;
}
// Where the positions of a row's members come from: FsBox takes them as they stand (walled handles, and bdmi_diagnostics
// on either kind); FsTorus unwraps them first (bdmi_periodic_flock_catalogue): y = x + L on an axis where the member's cell
// coordinate lies below the row's cut wrap3[3 row + axis] (k_fs_wrap; -1 = the flock spans the axis, nothing is moved),
// the milling pass takes the unwrapped centre c~ kept in centre[3 row ..], and the row's c is c~ brought back into the box.
// A compile-time policy like GridP / GridPer: the FsBox instances are the kernels they were.
struct FsBox {
    static constexpr bool kTorus = false;
};
struct FsTorus {
    static constexpr bool kTorus = true;
    GridPer g;
    const int32_t *wrap3;
    double *centre;
    __device__ __forceinline__ double4 unwrapped(const double4 &p, int row) const {
        const int32_t *s = wrap3 + 3 * (int64_t)row;
        return make_double4(cell_coord(p.x, g) < s[0] ? p.x + g.L : p.x, cell_coord(p.y, g) < s[1] ? p.y + g.L : p.y,
                            cell_coord(p.z, g) < s[2] ? p.z + g.L : p.z, p.w);
    }
};
template <int kPass, class X>
__global__ __launch_bounds__(kBlock) void k_fs_chunks(const double4 *__restrict__ pos, const double4 *__restrict__ vel,
                                                      const uint32_t *__restrict__ rank_s, const uint32_t *__restrict__ rkey,
                                                      const uint32_t *__restrict__ rhead, int64_t n,
                                                      const int32_t *__restrict__ chunk_off, int rows,
                                                      const double *__restrict__ rows16, double *__restrict__ part, X tor) {
    const int row = fs_row_of(chunk_off, rows, (int)blockIdx.x);
    const int64_t m = n - (int64_t)rkey[row], head = rhead[row];
    const int64_t first = head + (int64_t)((int)blockIdx.x - chunk_off[row]) * kFsChunk;
    const int64_t end = first + kFsChunk < head + m ? first + kFsChunk : head + m;
    double *out = part + (int64_t)blockIdx.x * kFsVals;
    auto position = [&](int64_t r) {
        if constexpr (X::kTorus) return tor.unwrapped(pos[r], row);
        else return pos[r];
    };
    if (kPass == 1) {
        double v[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (int64_t j = first + threadIdx.x; j < end; j += kBlock) {
            const int64_t r = rank_s ? (int64_t)rank_s[j] : j;
            const double4 p = position(r), w = vel[r];
            double ux, uy, uz;
            const double s = fs_heading(w, ux, uy, uz);
            v[0] += p.x; v[1] += p.y; v[2] += p.z;
            v[3] += w.x; v[4] += w.y; v[5] += w.z;
            v[6] += ux; v[7] += uy; v[8] += uz;
            v[9] += s;
            v[10] = p.x < v[10] ? p.x : v[10]; v[11] = p.y < v[11] ? p.y : v[11]; v[12] = p.z < v[12] ? p.z : v[12];
            v[13] = p.x > v[13] ? p.x : v[13]; v[14] = p.y > v[14] ? p.y : v[14]; v[15] = p.z > v[15] ? p.z : v[15];
        }
        const int op[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2};
        fs_block_fold(v, op, out);
    } else {
        const double *centre = rows16 + 16 * (int64_t)row + 1;
        if constexpr (X::kTorus) centre = tor.centre + 3 * (int64_t)row;
        const double cx = centre[0], cy = centre[1], cz = centre[2];
        double v[3] = {0, 0, 0};
        for (int64_t j = first + threadIdx.x; j < end; j += kBlock) {
            const int64_t r = rank_s ? (int64_t)rank_s[j] : j;
            const double4 p = position(r), w = vel[r];
            double ux, uy, uz;
            (void)fs_heading(w, ux, uy, uz);
            double rx = p.x - cx, ry = p.y - cy, rz = p.z - cz;
            const double rho = sqrt((rx * rx + ry * ry) + rz * rz);
            if (rho != 0.0) { rx /= rho; ry /= rho; rz /= rho; } else { rx = ry = rz = 0.0; }
            v[0] += ry * uz - rz * uy;
            v[1] += rz * ux - rx * uz;
            v[2] += rx * uy - ry * ux;
        }
        const int op[3] = {0, 0, 0};
        fs_block_fold(v, op, out);
    }
}
// one thread per row: the chunks' partials in chunk order, then the row's fields
template <int kPass, class X>
__global__ __launch_bounds__(kBlock) void k_fs_combine(const uint32_t *__restrict__ lab_s, const uint32_t *__restrict__ rkey,
                                                       const uint32_t *__restrict__ rhead, int64_t n,
                                                       const int32_t *__restrict__ chunk_off, int rows,
                                                       const double *__restrict__ part, double *__restrict__ rows16,
                                                       int32_t *__restrict__ row_label, int64_t *__restrict__ row_members,
                                                       X tor) {
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row >= rows) return;
    const int64_t members = n - (int64_t)rkey[row];
    const double m = (double)members;
    double *o = rows16 + 16 * (int64_t)row;
    const int c0 = chunk_off[row], c1 = chunk_off[row + 1];
    if (kPass == 1) {
        const int op[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2};
        double v[16];
        for (int k = 0; k < 16; k++) v[k] = part[(int64_t)c0 * kFsVals + k];
        for (int c = c0 + 1; c < c1; c++)
            for (int k = 0; k < 16; k++) v[k] = fs_fold(op[k], v[k], part[(int64_t)c * kFsVals + k]);
        o[0] = m;
        if constexpr (X::kTorus) {
            // the unwrapped centre stays for the milling pass; the row gets it brought back into the box
            for (int k = 0; k < 3; k++) {
                const double c = v[k] / m;
                tor.centre[3 * (int64_t)row + k] = c;
                o[1 + k] = c > tor.g.B ? c - tor.g.L : c;
            }
        } else {
            o[1] = v[0] / m; o[2] = v[1] / m; o[3] = v[2] / m;
        }
        o[4] = v[3] / m; o[5] = v[4] / m; o[6] = v[5] / m;
        o[7] = sqrt((v[6] * v[6] + v[7] * v[7]) + v[8] * v[8]) / m;
        o[8] = v[9] / m;
        o[9] = 0.0;
        for (int k = 0; k < 6; k++) o[10 + k] = v[10 + k];
        if (row_label) row_label[row] = (int32_t)lab_s[rhead[row]];
        if (row_members) row_members[row] = members;
    } else {
        double v[3];
        for (int k = 0; k < 3; k++) v[k] = part[(int64_t)c0 * kFsVals + k];
        for (int c = c0 + 1; c < c1; c++)
            for (int k = 0; k < 3; k++) v[k] += part[(int64_t)c * kFsVals + k];
        o[9] = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) / m;
    }
}

// ---- a flock's cut on the torus (include/bdmi.h, "Flock analysis on periodic handles") --------------------------------------
// O_a of a row = one bit per cell coordinate that its members occupy on axis a: `words` = ceil(dim / 32) words per axis,
// mask[(3 row + a) words ..].  One block per chunk of the rows' member list, as k_fs_chunks: the members' bits are ORed
// into an LDS mask (integer atomics: the result does not depend on their order), then the block's non-zero words into the
// row's mask in global memory.  cell_coord clamps into [0, dim - 1] and a periodic handle has dim <= 1290, so a word index
// stays below `words` <= kFsOccWords.
constexpr int kFsOccWords = (1290 + 31) / 32;
__global__ __launch_bounds__(kBlock) void k_fs_occupancy(const double4 *__restrict__ pos, const uint32_t *__restrict__ rank_s,
                                                         const uint32_t *__restrict__ rkey, const uint32_t *__restrict__ rhead,
                                                         int64_t n, const int32_t *__restrict__ chunk_off, int rows, GridPer g,
                                                         int words, uint32_t *__restrict__ mask) {
    __shared__ uint32_t bits[3 * kFsOccWords];
    const int row = fs_row_of(chunk_off, rows, (int)blockIdx.x);
    const int64_t m = n - (int64_t)rkey[row], head = rhead[row];
    const int64_t first = head + (int64_t)((int)blockIdx.x - chunk_off[row]) * kFsChunk;
    const int64_t end = first + kFsChunk < head + m ? first + kFsChunk : head + m;
    for (int k = threadIdx.x; k < 3 * words; k += kBlock) bits[k] = 0u;
    __syncthreads();
    for (int64_t j = first + threadIdx.x; j < end; j += kBlock) {
        const double4 p = pos[rank_s[j]];
        const int c[3] = {cell_coord(p.x, g), cell_coord(p.y, g), cell_coord(p.z, g)};
#pragma unroll
        for (int a = 0; a < 3; a++) atomicOr(&bits[a * words + (c[a] >> 5)], 1u << (c[a] & 31));
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 3 * words; k += kBlock)
        if (bits[k]) atomicOr(&mask[(int64_t)row * 3 * words + k], bits[k]);
}
// One thread per (row, axis): wrap = -1 where all dim coordinates are occupied (the flock spans the axis), else the
// smallest occupied coordinate whose cyclic predecessor is free.  A row has a member, so such a coordinate exists.
__global__ __launch_bounds__(kBlock) void k_fs_wrap(const uint32_t *__restrict__ mask, int rows, int dim, int words,
                                                    int32_t *__restrict__ wrap3) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= 3 * rows) return;
    const uint32_t *w = mask + (int64_t)t * words;
    int occupied = 0;
    for (int k = 0; k < words; k++) occupied += __popc(w[k]);
    int32_t cut = -1;
    if (occupied < dim) {
        uint32_t carry = (w[(dim - 1) >> 5] >> ((dim - 1) & 31)) & 1u;  // the predecessor of coordinate 0 is dim - 1
        for (int k = 0; k < words; k++) {
            const uint32_t starts = w[k] & ~((w[k] << 1) | carry);
            if (starts) { cut = 32 * k + __ffs(starts) - 1; break; }
            carry = w[k] >> 31;
        }
    }
    wrap3[t] = cut;
}

inline int nblocks(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }

}  // namespace

struct bdmi_flock {
    int64_t n = 0;
    int device = 0;
    double params[11] = {};
    GridP grid = {};
    int64_t num_cells = 0;
    int key_bits = 0;
    hipStream_t stream = nullptr;
    Boids A = {};
    BoidsAoS B = {};
    // slab mode (multi-GPU): rows [0, n) = owned boids and this step's ghosts; T = scratch for compactions
    bool slab = false;
    int64_t cap = 0;
    double x_lo = 0, x_hi = 0;
    int has_left = 0, has_right = 0;
    Boids T = {};
    uint32_t *keys = nullptr, *keys_s = nullptr, *idx = nullptr, *perm = nullptr;
    uint2 *occ = nullptr;          // per 32 cells: {occupancy bits, rank of the first non-empty cell}
    int32_t *cell_start = nullptr;    // first sorted boid of the k-th non-empty cell; [count] = n
    uint32_t *tile_cnt = nullptr;     // scan scratch
    int64_t occ_words = 0;
    unsigned long long *occupied = nullptr;
    void *tmp_sort = nullptr;
    size_t tmp_sort_bytes = 0;
    double *stage = nullptr;  // 12 N doubles
    int xcd_contiguous = 1;   // sweep block -> XCD mapping, see logical_block()
    int nb_mode = BDMI_NEIGHBOURS_METRIC, nb_k = 7;  // bdmi_set_neighbour_mode; BDMI_NEIGHBOURS at create
    // bdmi_create_periodic: the box [-box_b, box_b]^3 of edge box_l; `grid` is then the periodic grid
    bool periodic = false;
    double box_b = 0, box_l = 0;
    // bdmi_set_noise; the step counts the substeps since create whether or not eta > 0
    double noise_eta = 0;
    uint64_t noise_seed = 0;
    int64_t noise_step = 0;
    // bdmi_topological_neighbours scratch ((N, topo_cap) ids and d2, (N,) counts), allocated on first use
    int32_t *topo_ids = nullptr, *topo_cnt = nullptr;
    double *topo_d2 = nullptr;
    int topo_cap = 0;
    // render-side reduction scratch (bdmi_visible_vertices), allocated on first use
    uint8_t *vis_flag = nullptr;
    uint32_t *vis_slot = nullptr, *vis_tiles = nullptr;
    float *vis_verts = nullptr, *vis_cols = nullptr;  // 18 floats per boid each
    FlockStats fs = {};  // flock analysis scratch (bdmi_flocks and the calls next to it), allocated on first use
    bool timers = false;
    hipEvent_t ev[4] = {};
    double ms[3] = {0, 0, 0};
    int64_t timed = 0;
    std::vector<void *> allocs;
};

namespace {

template <typename T>
int dev_alloc(bdmi_flock *f, T **p, size_t count) {
    void *q = nullptr;
    NBMI_HIP_CHECK(hipMalloc(&q, (count ? count : 1) * sizeof(T)));
    f->allocs.push_back(q);
    *p = (T *)q;
    return 0;
}
// frees one of the handle's allocations ahead of bdmi_destroy (the caller clears its pointer)
void dev_release(bdmi_flock *f, void *p) {
    if (!p) return;
    for (size_t k = 0; k < f->allocs.size(); k++)
        if (f->allocs[k] == p) { f->allocs.erase(f->allocs.begin() + (long)k); break; }
    (void)hipFree(p);
}
// a scratch buffer that has become too small: released and allocated again (null if that fails).  The caller keeps the
// capacity: 0 ahead of the calls, the new one behind them.
template <typename T>
int dev_regrow(bdmi_flock *f, T **p, size_t count) {
    dev_release(f, *p);
    *p = nullptr;
    return dev_alloc(f, p, count);
}

int alloc_boids(bdmi_flock *f, Boids *b, int64_t n) {
    if (dev_alloc(f, &b->px, n) || dev_alloc(f, &b->py, n) || dev_alloc(f, &b->pz, n) || dev_alloc(f, &b->vx, n) ||
        dev_alloc(f, &b->vy, n) || dev_alloc(f, &b->vz, n) || dev_alloc(f, &b->cr, n) || dev_alloc(f, &b->cg, n) ||
        dev_alloc(f, &b->cb, n) || dev_alloc(f, &b->id, n))
        return -2;
    return 0;
}

int check(bdmi_flock *f) {
    if (!f) { nbmi::set_error("null bdmi_flock handle"); return -1; }
    if (hipSetDevice(f->device) != hipSuccess) { nbmi::set_error("hipSetDevice(%d) failed", f->device); return -2; }
    return 0;
}

FlockP make_params(const bdmi_flock *f, double dt) {
    const double *p = f->params;
    FlockP P;
    P.bounds = p[0]; P.margin = p[1];
    P.max_speed = p[3]; P.max_force = p[4];
    P.wall_force = p[4] * p[2];  // max_force * wall_weight (flock.py:673)
    P.perception_sq = p[5] * p[5];
    P.separation_sq = p[6] * p[6];
    P.sep_w = p[7]; P.ali_w = p[8]; P.coh_w = p[9];
    const double blend = p[10] * dt;  // min(1, color_blend_rate * dt) (flock.py:662)
    P.blend = blend < 1.0 ? blend : 1.0;
    P.dt = dt;
    return P;
}

// cells -> sort -> reorder A->B -> table
int enqueue_grid(bdmi_flock *f, bool timed) {
    const int64_t n = f->n;
    hipStream_t st = f->stream;
    if (timed) NBMI_HIP_CHECK(hipEventRecord(f->ev[0], st));
    k_assign<<<nblocks(n), kBlock, 0, st>>>(f->A, n, f->grid, f->keys, f->idx);
    NBMI_HIP_CHECK(nbmi::radix_sort_pairs_u32(f->tmp_sort, f->tmp_sort_bytes, f->keys, f->keys_s, f->idx, f->perm,
                                              (size_t)n, 0, f->key_bits, st));
    if (timed) NBMI_HIP_CHECK(hipEventRecord(f->ev[1], st));
    k_reorder<<<nblocks(n), kBlock, 0, st>>>(f->A, f->B, f->perm, n);
    NBMI_HIP_CHECK(hipMemsetAsync(f->occ, 0, (size_t)f->occ_words * sizeof(uint2), st));
    scan::enqueue_compact(FirstOfCell{f->keys_s}, n, f->tile_cnt,
                          EmitTable{f->keys_s, n, f->tile_cnt, scan::tiles_for(n), f->occ, f->cell_start}, st);
    if (timed) NBMI_HIP_CHECK(hipEventRecord(f->ev[2], st));
    NBMI_HIP_CHECK(hipGetLastError());
    return 0;
}

// The two instances of the topological kernels (k_flock_topo, k_topo_rows): k <= 8 runs 256 threads per block with a list
// of 8, a larger k 128 threads with a list of kTopoMaxK.  launch(list capacity, threads per block, blocks for n boids),
// the first two as integral constants.
template <class F>
void topo_launch(int k, int64_t n, F launch) {
    if (k <= 8)
        launch(std::integral_constant<int, 8>{}, std::integral_constant<int, 256>{}, (int)((n + 255) / 256));
    else
        launch(std::integral_constant<int, kTopoMaxK>{}, std::integral_constant<int, 128>{}, (int)((n + 127) / 128));
}

GridPer periodic_grid(const bdmi_flock *f) {
    GridPer g;
    g.cell_size = f->grid.cell_size; g.offset = f->grid.offset; g.dim = f->grid.dim;
    g.B = f->box_b; g.L = f->box_l;
    return g;
}

// the sweep of the handle's neighbour mode over the grid enqueue_grid has just built, as the instance of its grid G and
// its parameters PP
template <bool kPhysics, class G, class PP>
void enqueue_sweep_as(bdmi_flock *f, const G &g, const PP &P, double *d0, double *d1, double *d2, double *d3) {
    const int64_t n = f->n;
    if (f->nb_mode != BDMI_NEIGHBOURS_TOPOLOGICAL)
        k_flock<kPhysics, G, PP><<<nblocks(n), kBlock, 0, f->stream>>>(f->B, f->A, f->occ, f->cell_start, n, g, P, d0, d1, d2, d3,
                                                                      f->xcd_contiguous);
    else
        topo_launch(f->nb_k, n, [&](auto cap, auto threads, int blocks) {
            k_flock_topo<kPhysics, decltype(cap)::value, decltype(threads)::value, G, PP>
                <<<blocks, decltype(threads)::value, 0, f->stream>>>(f->B, f->A, f->occ, f->cell_start, n, g, P, f->nb_k, d0, d1,
                                                                     d2, d3, f->xcd_contiguous);
        });
}
// walled or periodic; a step (kPhysics) of a handle with eta > 0 runs the noisy instance with the noise step `step`, every
// other sweep the instance without the term (no "+ 0.0 * xi")
template <bool kPhysics>
void enqueue_sweep(bdmi_flock *f, const FlockP &P, int64_t step, double *d0, double *d1, double *d2, double *d3) {
    auto with_grid = [&](const auto &PP) {
        if (f->periodic) enqueue_sweep_as<kPhysics>(f, periodic_grid(f), PP, d0, d1, d2, d3);
        else enqueue_sweep_as<kPhysics>(f, f->grid, PP, d0, d1, d2, d3);
    };
    if constexpr (kPhysics) {
        if (f->noise_eta > 0) {
            FlockPN N;
            static_cast<FlockP &>(N) = P;
            N.amp = f->noise_eta * P.max_force;
            N.seed_lo = (uint32_t)f->noise_seed; N.seed_hi = (uint32_t)(f->noise_seed >> 32);
            N.step_lo = (uint32_t)(uint64_t)step; N.step_hi = (uint32_t)((uint64_t)step >> 32);
            with_grid(N);
            return;
        }
    }
    with_grid(P);
}

}  // namespace

extern "C" {

const char *bdmi_last_error(void) { return nbmi::get_error(); }

void bdmi_destroy(bdmi_flock *f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    for (void *p : f->allocs) (void)hipFree(p);
    for (auto &e : f->ev)
        if (e) (void)hipEventDestroy(e);
    if (f->stream) (void)hipStreamDestroy(f->stream);
    delete f;
}

static int bd_create_impl(bdmi_flock *f, const double *pos, const double *vel, const double *col) {
    const int64_t n = f->n;
    const int64_t c = f->cap > n ? f->cap : n;  // rows allocated (slab mode keeps head room for ghosts / immigrants)
    NBMI_HIP_CHECK(hipSetDevice(f->device));
    NBMI_HIP_CHECK(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
    for (auto &e : f->ev) NBMI_HIP_CHECK(hipEventCreate(&e));
    f->occ_words = (f->num_cells + 31) / 32;
    if (alloc_boids(f, &f->A, c)) return -2;
    if (f->slab && alloc_boids(f, &f->T, c)) return -2;
    if (dev_alloc(f, &f->B.p, c) || dev_alloc(f, &f->B.v, c) || dev_alloc(f, &f->B.c, c) || dev_alloc(f, &f->B.id, c))
        return -2;
    if (dev_alloc(f, &f->keys, c) || dev_alloc(f, &f->keys_s, c) || dev_alloc(f, &f->idx, c) ||
        dev_alloc(f, &f->perm, c) || dev_alloc(f, &f->occ, (size_t)f->occ_words) ||
        dev_alloc(f, &f->cell_start, (size_t)c + 2) ||
        dev_alloc(f, &f->tile_cnt, (size_t)scan::tiles_for(c) + 2) || dev_alloc(f, &f->occupied, 1) ||
        dev_alloc(f, &f->stage, (size_t)12 * (c ? c : 1)))
        return -2;
    f->tmp_sort_bytes = nbmi::radix_temp_bytes_u32((size_t)c, f->key_bits);
    char *t = nullptr;
    if (dev_alloc(f, &t, f->tmp_sort_bytes + 256)) return -2;
    f->tmp_sort = t;
    NBMI_HIP_CHECK(nbmi::radix_init_temp(t, f->stream));
    if (n > 0) {
        double *dp = f->stage, *dv = dp + 3 * n, *dc = dv + 3 * n;
        NBMI_HIP_CHECK(hipMemcpyAsync(dp, pos, (size_t)n * 24, hipMemcpyHostToDevice, f->stream));
        NBMI_HIP_CHECK(hipMemcpyAsync(dv, vel, (size_t)n * 24, hipMemcpyHostToDevice, f->stream));
        NBMI_HIP_CHECK(hipMemcpyAsync(dc, col, (size_t)n * 24, hipMemcpyHostToDevice, f->stream));
        k_split<<<nblocks(n), kBlock, 0, f->stream>>>(dp, dv, dc, f->A, n, 0);
        NBMI_HIP_CHECK(hipGetLastError());
    }
    NBMI_HIP_CHECK(hipStreamSynchronize(f->stream));
    return 0;
}

// A periodic handle takes only positions inside its box: the first row of (n, 3) positions with a coordinate that is not
// finite or outside [-b, b], or -1
static int64_t first_row_outside(const double *pos, int64_t n, double b) {
    for (int64_t i = 0; i < 3 * n; i++)
        if (!(pos[i] >= -b && pos[i] <= b)) return i / 3;  // NaN fails both
    return -1;
}

static bdmi_flock *bd_create(int64_t n, const double *pos, const double *vel, const double *col, const double *params,
                             int device, bool slab, int64_t capacity, const int32_t *ids, double x_lo, double x_hi,
                             int has_left, int has_right, bool periodic = false) {
    nbmi::clear_error();
    if (n < 0 || n > 1000000000 || !params || (n > 0 && (!pos || !vel || !col))) {
        nbmi::set_error("%s: bad arguments (n=%lld)", periodic ? "bdmi_create_periodic" : "bdmi_create", (long long)n);
        return nullptr;
    }
    const double bounds = params[0], perception = params[5], margin = params[1];
    if (periodic) {
        // wall_margin and wall_weight are ignored; the grid is dim = floor(L / perception) cells of L / dim per axis
        if (!(bounds > 0) || !(perception > 0) || !(bounds < INFINITY)) {
            nbmi::set_error("bdmi_create_periodic: bounds and perception_radius must be finite and > 0");
            return nullptr;
        }
        const double dimf = floor(2 * bounds / perception);
        if (!(dimf >= 3) || dimf > 1290) {
            nbmi::set_error("bdmi_create_periodic: grid dimension floor(2 * bounds / perception_radius) = %.0f must be in "
                            "3..1290 (below 3 the 27 wrapped cells are not distinct)", dimf);
            return nullptr;
        }
        const int64_t bad = first_row_outside(pos, n, bounds);
        if (bad >= 0) {
            nbmi::set_error("bdmi_create_periodic: position row %lld = (%g, %g, %g) is not finite or outside the box [-%g, %g]",
                            (long long)bad, pos[3 * bad], pos[3 * bad + 1], pos[3 * bad + 2], bounds, bounds);
            return nullptr;
        }
    } else if (!(bounds > 0) || !(perception > 0) || !(margin > 0)) {
        nbmi::set_error("bdmi_create: bounds, perception_radius and wall_margin must be > 0");
        return nullptr;
    }
    if (slab && (capacity < n || capacity < 1 || (n > 0 && !ids) || !(x_hi - x_lo >= 2 * perception))) {
        nbmi::set_error("bdmi_create_slab: capacity < n, missing ids, or a slab narrower than two cells");
        return nullptr;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        nbmi::set_error("bdmi_create: no HIP device available");
        return nullptr;
    }
    if (device < 0 || device >= count) {
        nbmi::set_error("bdmi_create: device %d out of range (have %d)", device, count);
        return nullptr;
    }
    bdmi_flock *f = new bdmi_flock();
    if (const char *e = getenv("BDMI_XCD")) f->xcd_contiguous = atoi(e) != 0;  // measurement knob
    // BDMI_NEIGHBOURS=topological or topological:K (K in 1..16, default 7): the initial neighbour mode of ordinary
    // handles, so that unchanged drivers can be run in it; anything else means metric
    if (const char *e = getenv("BDMI_NEIGHBOURS")) {
        int k = 7;
        char tail = 0;
        const bool plain = strcmp(e, "topological") == 0;
        if (!slab && (plain || (sscanf(e, "topological:%d%c", &k, &tail) == 1 && k >= 1 && k <= kTopoMaxK))) {
            f->nb_mode = BDMI_NEIGHBOURS_TOPOLOGICAL;
            f->nb_k = k;
        }
    }
    f->n = n;
    f->device = device;
    f->slab = slab; f->cap = slab ? capacity : 0;
    f->x_lo = x_lo; f->x_hi = x_hi; f->has_left = has_left; f->has_right = has_right;
    memcpy(f->params, params, sizeof(f->params));
    if (periodic) {
        f->periodic = true;
        f->box_b = bounds;
        f->box_l = 2 * bounds;
        f->grid.dim = (int)floor(f->box_l / perception);
        f->grid.cell_size = f->box_l / f->grid.dim;
        f->grid.offset = bounds;
    } else {
        // Flock.__init__ grid (flock.py:478-481)
        f->grid.cell_size = perception;
        const double dimf = ceil(bounds * 2 / perception) + 2;
        if (!(dimf >= 1) || dimf > 1290) {  // dim^3 must fit int32 cell ids
            nbmi::set_error("bdmi_create: grid dimension %.0f out of range", dimf);
            delete f;
            return nullptr;
        }
        f->grid.dim = (int)dimf;
        f->grid.offset = bounds + perception;
    }
    f->num_cells = (int64_t)f->grid.dim * f->grid.dim * f->grid.dim;
    f->key_bits = 1;
    while (((int64_t)1 << f->key_bits) < f->num_cells) f->key_bits++;
    int rc = bd_create_impl(f, pos, vel, col);
    if (rc == 0 && slab && n > 0) {  // global ids instead of row numbers
        hipError_t e = hipMemcpyAsync(f->stage, ids, (size_t)n * 4, hipMemcpyHostToDevice, f->stream);
        if (e == hipSuccess) {
            k_set_ids<<<nblocks(n), kBlock, 0, f->stream>>>((const int32_t *)f->stage, f->A.id, n);
            e = hipStreamSynchronize(f->stream);
        }
        if (e != hipSuccess) { nbmi::set_error("bdmi_create_slab: id upload failed: %s", hipGetErrorString(e)); rc = -2; }
    }
    if (rc != 0) {
        std::string keep = nbmi::get_error();
        bdmi_destroy(f);
        nbmi::set_error("%s", keep.c_str());
        return nullptr;
    }
    return f;
}

bdmi_flock *bdmi_create(int64_t n, const double *pos, const double *vel, const double *col, const double *params,
                        int device) {
    return bd_create(n, pos, vel, col, params, device, false, 0, nullptr, 0.0, 0.0, 0, 0);
}

bdmi_flock *bdmi_create_periodic(int64_t n, const double *pos, const double *vel, const double *col, const double *params,
                                 int device) {
    return bd_create(n, pos, vel, col, params, device, false, 0, nullptr, 0.0, 0.0, 0, 0, true);
}

// ---- slab mode --------------------------------------------------------------------------
bdmi_flock *bdmi_create_slab(int64_t n, const double *pos, const double *vel, const double *col, const int32_t *ids,
                             int64_t capacity, const double *params, double x_lo, double x_hi, int has_left, int has_right,
                             int device) {
    return bd_create(n, pos, vel, col, params, device, true, capacity, ids, x_lo, x_hi, has_left, has_right);
}

namespace {
// rows selected by `sel`, in row order, to packed rows or to the SoA arrays `dst`; the count stays on the device
int enqueue_select(bdmi_flock *f, const SlabSel &sel, int64_t n, Boids dst, double *dst_rows) {
    scan::enqueue_compact(SlabMask{sel}, n, f->tile_cnt, EmitRows{f->A, dst, dst_rows}, f->stream);
    NBMI_HIP_CHECK(hipGetLastError());
    return 0;
}
int slab_check(bdmi_flock *f, const char *what) {
    if (int rc = check(f)) return rc;
    if (!f->slab) { nbmi::set_error("%s: not a slab-mode handle (bdmi_create_slab)", what); return -1; }
    return 0;
}
// The calls that address their buffers by A.id: a slab handle holds GLOBAL ids there (and -1 - id for a ghost), its row
// count changes with every exchange, and it holds only a part of the flock, so a caller-order array has no meaning.
int whole_flock_check(bdmi_flock *f, const char *what) {
    if (int rc = check(f)) return rc;
    if (f->slab) {
        nbmi::set_error("%s: refused on a slab handle (bdmi_create_slab), whose rows carry global ids and ghosts; read a "
                        "slab with bdmi_slab_get", what);
        return -1;
    }
    return 0;
}
// drop the ghosts: owned rows to the front, in row order
int slab_compact_owned(bdmi_flock *f, int64_t *n_owned) {
    uint32_t total = 0;
    if (f->n > 0) {
        const SlabSel own{f->A.px, f->A.id, 0, 0.0, 0.0};
        if (int rc = enqueue_select(f, own, f->n, f->T, nullptr)) return rc;
        NBMI_HIP_CHECK(hipMemcpyAsync(&total, f->tile_cnt + scan::tiles_for(f->n), 4, hipMemcpyDeviceToHost, f->stream));
        NBMI_HIP_CHECK(hipStreamSynchronize(f->stream));
        std::swap(f->A, f->T);
    }
    f->n = total;
    *n_owned = total;
    return 0;
}
}  // namespace

int64_t bdmi_slab_count(bdmi_flock *f) {
    if (!f || !f->slab) return -1;
    int64_t n = 0;
    if (slab_compact_owned(f, &n)) return -1;
    return n;
}

int bdmi_slab_export(bdmi_flock *f, void *dev_left, int64_t *n_left, void *dev_right, int64_t *n_right) {
    if (int rc = slab_check(f, "bdmi_slab_export")) return rc;
    if (!n_left || !n_right || (f->has_left && !dev_left) || (f->has_right && !dev_right)) {
        nbmi::set_error("bdmi_slab_export: null buffer");
        return -1;
    }
    *n_left = *n_right = 0;
    int64_t owned = 0;
    if (int rc = slab_compact_owned(f, &owned)) return rc;  // last step's ghosts are gone
    if (owned == 0) return 0;
    const double cell = f->grid.cell_size;
    uint32_t cl = 0, cr = 0;
    const int64_t ntiles = scan::tiles_for(owned);
    if (f->has_left) {
        const SlabSel sel{f->A.px, f->A.id, 1, f->x_lo + cell, 0.0};
        if (int rc = enqueue_select(f, sel, owned, Boids{}, (double *)dev_left)) return rc;
        NBMI_HIP_CHECK(hipMemcpyAsync(&cl, f->tile_cnt + ntiles, 4, hipMemcpyDeviceToHost, f->stream));
        NBMI_HIP_CHECK(hipStreamSynchronize(f->stream));
    }
    if (f->has_right) {
        const SlabSel sel{f->A.px, f->A.id, 2, 0.0, f->x_hi - cell};
        if (int rc = enqueue_select(f, sel, owned, Boids{}, (double *)dev_right)) return rc;
        NBMI_HIP_CHECK(hipMemcpyAsync(&cr, f->tile_cnt + ntiles, 4, hipMemcpyDeviceToHost, f->stream));
        NBMI_HIP_CHECK(hipStreamSynchronize(f->stream));
    }
    // boids that have left the slab were just handed over: here they are ghosts for this step.  (Slabs at the
    // two ends of the domain keep their outer side: the walls turn those boids back.)
    k_slab_demote<<<nblocks(owned), kBlock, 0, f->stream>>>(f->A, owned, f->has_left ? f->x_lo : -INFINITY,
                                                           f->has_right ? f->x_hi : INFINITY);
    NBMI_HIP_CHECK(hipGetLastError());
    *n_left = cl;
    *n_right = cr;
    return 0;
}

int bdmi_slab_import(bdmi_flock *f, const void *dev_rows, int64_t count) {
    if (int rc = slab_check(f, "bdmi_slab_import")) return rc;
    if (count < 0 || (count > 0 && !dev_rows)) { nbmi::set_error("bdmi_slab_import: bad arguments"); return -1; }
    if (f->n + count > f->cap) {
        nbmi::set_error("bdmi_slab_import: %lld + %lld boids exceed the capacity %lld", (long long)f->n, (long long)count,
                        (long long)f->cap);
        return -4;
    }
    if (count == 0) return 0;
    k_slab_append<<<nblocks(count), kBlock, 0, f->stream>>>(f->A, f->n, (const double *)dev_rows, count,
                                                           f->has_left ? f->x_lo : -INFINITY, f->has_right ? f->x_hi : INFINITY);
    NBMI_HIP_CHECK(hipGetLastError());
    f->n += count;
    return 0;
}

int bdmi_slab_get(bdmi_flock *f, double *rows10, int64_t capacity, int64_t *count) {
    if (int rc = slab_check(f, "bdmi_slab_get")) return rc;
    if (!count) { nbmi::set_error("bdmi_slab_get: null count"); return -1; }
    *count = 0;
    if (f->n == 0) return 0;
    // owned rows {p, v, c, id}, packed, through the staging buffer (12 doubles per row are reserved)
    const SlabSel own{f->A.px, f->A.id, 0, 0.0, 0.0};
    if (int rc = enqueue_select(f, own, f->n, Boids{}, f->stage)) return rc;
    uint32_t total = 0;
    NBMI_HIP_CHECK(hipMemcpyAsync(&total, f->tile_cnt + scan::tiles_for(f->n), 4, hipMemcpyDeviceToHost, f->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(f->stream));
    *count = total;
    const int64_t rows = (int64_t)total < capacity ? (int64_t)total : capacity;
    if (rows > 0) {
        if (!rows10) { nbmi::set_error("bdmi_slab_get: null output"); return -1; }
        NBMI_HIP_CHECK(hipMemcpyAsync(rows10, f->stage, (size_t)rows * 80, hipMemcpyDeviceToHost, f->stream));
        NBMI_HIP_CHECK(hipStreamSynchronize(f->stream));
    }
    return 0;
}

int bdmi_step(bdmi_flock *f, double dt, int substeps) {
    if (int rc = check(f)) return rc;
    if (substeps < 0) { nbmi::set_error("bdmi_step: substeps < 0"); return -1; }
    // A slab handle knows only that its neighbours are at least two cells wide (as it is itself).  The speed clamp
    // bounds a step's displacement by max_speed * |dt|; below two cells a boid that leaves its slab lands inside the
    // adjacent one, which got a copy of it at the exchange.  Beyond that it could land in a slab that never saw it:
    // demoted here, a ghost there, and dropped by every rank at the next export.
    if (f->slab && !(f->params[3] * fabs(dt) < 2.0 * f->params[5])) {
        nbmi::set_error("bdmi_step: on a slab handle max_speed * |dt| = %g must stay below two cells = 2 * "
                        "perception_radius = %g (a boid may only ever move to the adjacent slab)",
                        f->params[3] * fabs(dt), 2.0 * f->params[5]);
        return -1;
    }
    // A periodic handle wraps a boid once per step: the displacement must stay below one box length.
    if (f->periodic && !(f->params[3] * fabs(dt) < f->box_l)) {
        nbmi::set_error("bdmi_step: on a periodic handle max_speed * |dt| = %g must stay below the box length %g (a boid is "
                        "wrapped once per step)", f->params[3] * fabs(dt), f->box_l);
        return -1;
    }
    // (the noise step counts the substeps of ordinary handles; a slab handle has no noise and no counter to keep)
    if (f->n == 0) { if (!f->slab) f->noise_step += substeps; return 0; }
    const FlockP P = make_params(f, dt);
    for (int k = 0; k < substeps; k++) {
        if (int rc = enqueue_grid(f, f->timers)) return rc;
        enqueue_sweep<true>(f, P, f->noise_step, nullptr, nullptr, nullptr, nullptr);
        NBMI_HIP_CHECK(hipGetLastError());
        if (!f->slab) f->noise_step++;
        if (f->timers) {
            NBMI_HIP_CHECK(hipEventRecord(f->ev[3], f->stream));
            NBMI_HIP_CHECK(hipEventSynchronize(f->ev[3]));
            for (int p = 0; p < 3; p++) {
                float ms = 0.f;
                NBMI_HIP_CHECK(hipEventElapsedTime(&ms, f->ev[p], f->ev[p + 1]));
                f->ms[p] += ms;
            }
            f->timed++;
        }
    }
    return 0;
}

// synchronise, then look at the radix sort's sticky error word (a timed-out look-back = a corrupt cell order)
static int sync_checked(bdmi_flock *f) {
    unsigned sort_err = 0u;
    if (f->tmp_sort) NBMI_HIP_CHECK(nbmi::radix_error_word(f->tmp_sort, &sort_err, f->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(f->stream));
    if (sort_err) {
        NBMI_HIP_CHECK(nbmi::radix_init_temp(f->tmp_sort, f->stream));
        NBMI_HIP_CHECK(hipStreamSynchronize(f->stream));
        nbmi::set_error("device radix sort: a look-back spin timed out; the steps since the last synchronisation are invalid");
        return -2;
    }
    return 0;
}

int bdmi_sync(bdmi_flock *f) {
    if (int rc = check(f)) return rc;
    return sync_checked(f);
}

int bdmi_get_state(bdmi_flock *f, double *pos, double *vel, double *col) {
    if (int rc = whole_flock_check(f, "bdmi_get_state")) return rc;
    const int64_t n = f->n;
    if (n == 0) return 0;
    double *dp = f->stage, *dv = dp + 3 * n, *dc = dv + 3 * n;
    const Boids &a = f->A;
    if (pos) {
        k_join<<<nblocks(n), kBlock, 0, f->stream>>>(a.px, a.py, a.pz, a.id, n, dp);
        NBMI_HIP_CHECK(hipMemcpyAsync(pos, dp, (size_t)n * 24, hipMemcpyDeviceToHost, f->stream));
    }
    if (vel) {
        k_join<<<nblocks(n), kBlock, 0, f->stream>>>(a.vx, a.vy, a.vz, a.id, n, dv);
        NBMI_HIP_CHECK(hipMemcpyAsync(vel, dv, (size_t)n * 24, hipMemcpyDeviceToHost, f->stream));
    }
    if (col) {
        k_join<<<nblocks(n), kBlock, 0, f->stream>>>(a.cr, a.cg, a.cb, a.id, n, dc);
        NBMI_HIP_CHECK(hipMemcpyAsync(col, dc, (size_t)n * 24, hipMemcpyDeviceToHost, f->stream));
    }
    NBMI_HIP_CHECK(hipGetLastError());
    return sync_checked(f);
}

int bdmi_set_state(bdmi_flock *f, const double *pos, const double *vel, const double *col) {
    if (int rc = whole_flock_check(f, "bdmi_set_state")) return rc;
    const int64_t n = f->n;
    if (n == 0) return 0;
    if (f->periodic && pos) {
        const int64_t bad = first_row_outside(pos, n, f->box_b);
        if (bad >= 0) {
            nbmi::set_error("bdmi_set_state: position row %lld = (%g, %g, %g) is not finite or outside the periodic box "
                            "[-%g, %g]; nothing was uploaded", (long long)bad, pos[3 * bad], pos[3 * bad + 1], pos[3 * bad + 2],
                            f->box_b, f->box_b);
            return -1;
        }
    }
    double *dp = f->stage, *dv = dp + 3 * n, *dc = dv + 3 * n;
    if (pos) NBMI_HIP_CHECK(hipMemcpyAsync(dp, pos, (size_t)n * 24, hipMemcpyHostToDevice, f->stream));
    if (vel) NBMI_HIP_CHECK(hipMemcpyAsync(dv, vel, (size_t)n * 24, hipMemcpyHostToDevice, f->stream));
    if (col) NBMI_HIP_CHECK(hipMemcpyAsync(dc, col, (size_t)n * 24, hipMemcpyHostToDevice, f->stream));
    k_split<<<nblocks(n), kBlock, 0, f->stream>>>(pos ? dp : nullptr, vel ? dv : nullptr, col ? dc : nullptr, f->A, n, 1);
    NBMI_HIP_CHECK(hipGetLastError());
    NBMI_HIP_CHECK(hipStreamSynchronize(f->stream));
    return 0;
}

int bdmi_get_cell_indices(bdmi_flock *f, int32_t *out) {
    if (int rc = whole_flock_check(f, "bdmi_get_cell_indices")) return rc;
    const int64_t n = f->n;
    if (n == 0) return 0;
    if (!out) { nbmi::set_error("null output"); return -1; }
    int32_t *d = (int32_t *)f->stage;
    k_cells_out<<<nblocks(n), kBlock, 0, f->stream>>>(f->A, n, f->grid, d);
    NBMI_HIP_CHECK(hipGetLastError());
    NBMI_HIP_CHECK(hipMemcpyAsync(out, d, (size_t)n * 4, hipMemcpyDeviceToHost, f->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(f->stream));
    return 0;
}

int bdmi_get_forces(bdmi_flock *f, double *sep, double *ali, double *coh, double *avg) {
    if (int rc = whole_flock_check(f, "bdmi_get_forces")) return rc;
    const int64_t n = f->n;
    if (n == 0) return 0;
    if (!sep || !ali || !coh || !avg) { nbmi::set_error("null output"); return -1; }
    if (int rc = enqueue_grid(f, false)) return rc;
    double *d0 = f->stage, *d1 = d0 + 3 * n, *d2 = d1 + 3 * n, *d3 = d2 + 3 * n;
    const FlockP P = make_params(f, 0.0);
    enqueue_sweep<false>(f, P, 0, d0, d1, d2, d3);
    NBMI_HIP_CHECK(hipGetLastError());
    NBMI_HIP_CHECK(hipMemcpyAsync(sep, d0, (size_t)n * 24, hipMemcpyDeviceToHost, f->stream));
    NBMI_HIP_CHECK(hipMemcpyAsync(ali, d1, (size_t)n * 24, hipMemcpyDeviceToHost, f->stream));
    NBMI_HIP_CHECK(hipMemcpyAsync(coh, d2, (size_t)n * 24, hipMemcpyDeviceToHost, f->stream));
    NBMI_HIP_CHECK(hipMemcpyAsync(avg, d3, (size_t)n * 24, hipMemcpyDeviceToHost, f->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(f->stream));
    return 0;
}

// ---- topological interaction (include/bdmi.h) ---------------------------------------------------------------------
static int topo_k_check(const char *what, int k) {
    if (k < 1 || k > kTopoMaxK) {
        nbmi::set_error("%s: k = %d must be in 1..%d", what, k, kTopoMaxK);
        return -1;
    }
    return 0;
}
static int topo_handle_check(bdmi_flock *f, const char *what) {
    if (!f) { nbmi::set_error("%s: null bdmi_flock handle", what); return -1; }
    return whole_flock_check(f, what);
}

int bdmi_set_neighbour_mode(bdmi_flock *f, int mode, int k) {
    if (int rc = topo_handle_check(f, "bdmi_set_neighbour_mode")) return rc;
    if (mode != BDMI_NEIGHBOURS_METRIC && mode != BDMI_NEIGHBOURS_TOPOLOGICAL) {
        nbmi::set_error("bdmi_set_neighbour_mode: unknown mode %d (BDMI_NEIGHBOURS_METRIC = 0, BDMI_NEIGHBOURS_TOPOLOGICAL = 1)",
                        mode);
        return -1;
    }
    if (mode == BDMI_NEIGHBOURS_TOPOLOGICAL) {
        if (int rc = topo_k_check("bdmi_set_neighbour_mode", k)) return rc;
        f->nb_k = k;
    }
    f->nb_mode = mode;
    return 0;
}

int bdmi_get_neighbour_mode(bdmi_flock *f, int *mode, int *k) {
    if (!f) { nbmi::set_error("bdmi_get_neighbour_mode: null bdmi_flock handle"); return -1; }
    if (mode) *mode = f->nb_mode;
    if (k) *k = f->nb_k;
    return 0;
}

int bdmi_topological_neighbours(bdmi_flock *f, int k, int32_t *ids, double *d2, int32_t *count) {
    if (int rc = topo_handle_check(f, "bdmi_topological_neighbours")) return rc;
    if (int rc = topo_k_check("bdmi_topological_neighbours", k)) return rc;
    const int64_t n = f->n;
    if (n == 0) return 0;
    if (k > f->topo_cap) {
        f->topo_cap = 0;
        if (dev_regrow(f, &f->topo_ids, (size_t)n * k) || dev_regrow(f, &f->topo_d2, (size_t)n * k)) return -2;
        f->topo_cap = k;
    }
    if (!f->topo_cnt && dev_alloc(f, &f->topo_cnt, (size_t)n)) return -2;
    if (int rc = enqueue_grid(f, false)) return rc;
    hipStream_t st = f->stream;
    const double psq = f->params[5] * f->params[5];
    topo_launch(k, n, [&](auto cap, auto threads, int blocks) {
        auto rows = [&](const auto &g) {
            k_topo_rows<decltype(cap)::value, decltype(threads)::value><<<blocks, decltype(threads)::value, 0, st>>>(
                f->B, f->occ, f->cell_start, n, g, psq, k, f->topo_ids, f->topo_d2, f->topo_cnt);
        };
        if (f->periodic) rows(periodic_grid(f)); else rows(f->grid);
    });
    NBMI_HIP_CHECK(hipGetLastError());
    if (ids) NBMI_HIP_CHECK(hipMemcpyAsync(ids, f->topo_ids, (size_t)n * k * 4, hipMemcpyDeviceToHost, st));
    if (d2) NBMI_HIP_CHECK(hipMemcpyAsync(d2, f->topo_d2, (size_t)n * k * 8, hipMemcpyDeviceToHost, st));
    if (count) NBMI_HIP_CHECK(hipMemcpyAsync(count, f->topo_cnt, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    return sync_checked(f);
}

// ---- periodic box and noise (include/bdmi.h) --------------------------------------------------------------------------
int bdmi_get_box(bdmi_flock *f, int *periodic, double *length, double *cell_size) {
    if (int rc = topo_handle_check(f, "bdmi_get_box")) return rc;
    if (periodic) *periodic = f->periodic ? 1 : 0;
    if (length) *length = f->periodic ? f->box_l : 2 * f->params[0];
    if (cell_size) *cell_size = f->grid.cell_size;
    return 0;
}

int bdmi_set_noise(bdmi_flock *f, double eta, uint64_t seed, int64_t step) {
    if (int rc = topo_handle_check(f, "bdmi_set_noise")) return rc;
    if (!(eta >= 0) || !(eta < INFINITY)) {
        nbmi::set_error("bdmi_set_noise: eta = %g must be finite and >= 0", eta);
        return -1;
    }
    if (step < -1) {
        nbmi::set_error("bdmi_set_noise: step = %lld must be >= 0, or -1 to keep the handle's step", (long long)step);
        return -1;
    }
    f->noise_eta = eta;
    f->noise_seed = seed;
    if (step >= 0) f->noise_step = step;
    return 0;
}

int bdmi_get_noise(bdmi_flock *f, double *eta, uint64_t *seed, int64_t *step) {
    if (int rc = topo_handle_check(f, "bdmi_get_noise")) return rc;
    if (eta) *eta = f->noise_eta;
    if (seed) *seed = f->noise_seed;
    if (step) *step = f->noise_step;
    return 0;
}

int bdmi_noise_vectors(bdmi_flock *f, int64_t step, double *out_xyz) {
    if (int rc = topo_handle_check(f, "bdmi_noise_vectors")) return rc;
    if (step < -1) {
        nbmi::set_error("bdmi_noise_vectors: step = %lld must be >= 0, or -1 for the handle's step", (long long)step);
        return -1;
    }
    const int64_t n = f->n;
    if (n == 0) return 0;
    if (!out_xyz) { nbmi::set_error("bdmi_noise_vectors: null output"); return -1; }
    const uint64_t s = (uint64_t)(step >= 0 ? step : f->noise_step);
    k_noise_vectors<<<nblocks(n), kBlock, 0, f->stream>>>(n, (uint32_t)f->noise_seed, (uint32_t)(f->noise_seed >> 32), (uint32_t)s,
                                                         (uint32_t)(s >> 32), f->stage);
    NBMI_HIP_CHECK(hipGetLastError());
    NBMI_HIP_CHECK(hipMemcpyAsync(out_xyz, f->stage, (size_t)n * 24, hipMemcpyDeviceToHost, f->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(f->stream));
    return 0;
}

int bdmi_grid_info(bdmi_flock *f, int32_t *grid_dim, int64_t *num_cells, int64_t *occupied) {
    if (int rc = check(f)) return rc;
    if (grid_dim) *grid_dim = f->grid.dim;
    if (num_cells) *num_cells = f->num_cells;
    if (occupied) {
        unsigned long long h = 0;
        if (f->n > 0) {
            NBMI_HIP_CHECK(hipMemsetAsync(f->occupied, 0, sizeof(unsigned long long), f->stream));
            int gb = nblocks(f->n);
            if (gb > 64) gb = 64;
            k_count_cells<<<gb, kBlock, 0, f->stream>>>(f->keys_s, f->n, f->occupied);
            NBMI_HIP_CHECK(hipGetLastError());
        }
        NBMI_HIP_CHECK(hipMemcpyAsync(&h, f->occupied, sizeof(h), hipMemcpyDeviceToHost, f->stream));
        NBMI_HIP_CHECK(hipStreamSynchronize(f->stream));
        *occupied = (int64_t)h;
    }
    return 0;
}

int bdmi_enable_timers(bdmi_flock *f, int enable) {
    if (int rc = check(f)) return rc;
    f->timers = enable != 0;
    return 0;
}

int bdmi_get_timers(bdmi_flock *f, double *ms3, int64_t *count, int reset) {
    if (int rc = check(f)) return rc;
    if (ms3) memcpy(ms3, f->ms, sizeof(f->ms));
    if (count) *count = f->timed;
    if (reset) { memset(f->ms, 0, sizeof(f->ms)); f->timed = 0; }
    return 0;
}

namespace {
// build_vertices_numba (flock.py:351-447): two triangles (tip/right/left, tip/up/down) per boid,
// float64 arithmetic in the reference's order, one rounding to float32 on store.
struct EmitCones {
    Boids a;
    double cone_length, cone_radius;
    float *verts, *cols;
    __device__ void operator()(int64_t k, int64_t, uint32_t slot) const {
        const double wux = 0.0, wuy = 1.0, wuz = 0.0, wrx = 1.0, wry = 0.0, wrz = 0.0;
        const double px = a.px[slot], py = a.py[slot], pz = a.pz[slot];
        const double vx = a.vx[slot], vy = a.vy[slot], vz = a.vz[slot];
        double speed = sqrt(vx * vx + vy * vy + vz * vz);
        if (speed < 0.0001) speed = 0.0001;
        const double fx = vx / speed, fy = vy / speed, fz = vz / speed;
        double rx = fy * wuz - fz * wuy;
        double ry = fz * wux - fx * wuz;
        double rz = fx * wuy - fy * wux;
        double r_len = sqrt(rx * rx + ry * ry + rz * rz);
        if (r_len < 0.1) {
            rx = fy * wrz - fz * wry;
            ry = fz * wrx - fx * wrz;
            rz = fx * wry - fy * wrx;
            r_len = sqrt(rx * rx + ry * ry + rz * rz);
        }
        if (r_len > 0.0001) { rx /= r_len; ry /= r_len; rz /= r_len; }
        const double ux = ry * fz - rz * fy;
        const double uy = rz * fx - rx * fz;
        const double uz = rx * fy - ry * fx;
        const double r = cone_radius;
        const float tip[3] = {(float)(px + fx * cone_length), (float)(py + fy * cone_length), (float)(pz + fz * cone_length)};
        float *o = verts + 18 * k;
        o[0] = tip[0]; o[1] = tip[1]; o[2] = tip[2];
        o[3] = (float)(px + rx * r); o[4] = (float)(py + ry * r); o[5] = (float)(pz + rz * r);
        o[6] = (float)(px - rx * r); o[7] = (float)(py - ry * r); o[8] = (float)(pz - rz * r);
        o[9] = tip[0]; o[10] = tip[1]; o[11] = tip[2];
        o[12] = (float)(px + ux * r); o[13] = (float)(py + uy * r); o[14] = (float)(pz + uz * r);
        o[15] = (float)(px - ux * r); o[16] = (float)(py - uy * r); o[17] = (float)(pz - uz * r);
        const float cr = (float)a.cr[slot], cg = (float)a.cg[slot], cb = (float)a.cb[slot];
        float *c = cols + 18 * k;
#pragma unroll
        for (int v = 0; v < 6; v++) { c[3 * v] = cr; c[3 * v + 1] = cg; c[3 * v + 2] = cb; }
    }
};
}  // namespace

int bdmi_visible_vertices(bdmi_flock *f, const double *cam12, double tan_h, double tan_v, double fog_end,
                          double cone_length, double cone_radius, float *out_vertices, float *out_colors,
                          int64_t capacity_boids, int64_t *count) {
    if (int rc = whole_flock_check(f, "bdmi_visible_vertices")) return rc;
    if (!cam12 || !count || capacity_boids < 0 || (capacity_boids > 0 && (!out_vertices || !out_colors))) {
        nbmi::set_error("bdmi_visible_vertices: null argument");
        return -1;
    }
    const float *d_verts = nullptr, *d_cols = nullptr;
    if (int rc = nbmi::flock_visible_device(f, cam12, tan_h, tan_v, fog_end, cone_length, cone_radius, &d_verts, &d_cols,
                                            count, nullptr))
        return rc;
    hipStream_t st = f->stream;
    const int64_t rows = *count < capacity_boids ? *count : capacity_boids;
    if (rows > 0) {
        NBMI_HIP_CHECK(hipMemcpyAsync(out_vertices, d_verts, (size_t)rows * 72, hipMemcpyDeviceToHost, st));
        NBMI_HIP_CHECK(hipMemcpyAsync(out_colors, d_cols, (size_t)rows * 72, hipMemcpyDeviceToHost, st));
        NBMI_HIP_CHECK(hipStreamSynchronize(st));
    }
    return 0;
}

// ---- flock analysis (the kernels are above, next to the sweep whose grid they share) ---------------------------------
namespace {
// walled_call = null: `what` is one of the walled calls, which refuse a periodic handle; else `what` is the periodic
// counterpart of walled_call and refuses everything but a periodic handle
int fs_radius_check(bdmi_flock *f, const char *what, const char *name, double v, const char *walled_call = nullptr) {
    if (walled_call && !f) { nbmi::set_error("%s: null bdmi_flock handle", what); return -1; }
    if (int rc = whole_flock_check(f, what)) return rc;
    if (f->periodic && !walled_call) {
        nbmi::set_error("%s: refused on a periodic handle (bdmi_create_periodic): this call does not follow links through the "
                        "faces of the box; bdmi_periodic_flocks, bdmi_periodic_flock_catalogue and "
                        "bdmi_periodic_neighbour_stats do", what);
        return -1;
    }
    if (!f->periodic && walled_call) {
        nbmi::set_error("%s: refused on a walled handle (bdmi_create): it works on the periodic box of bdmi_create_periodic; "
                        "use %s", what, walled_call);
        return -1;
    }
    const double perception = f->params[5];
    if (!(v > 0) || !(v <= perception)) {  // NaN fails the first test, +inf the second
        nbmi::set_error("%s: %s = %g must be finite, > 0 and at most the perception radius %g (the grid cell)", what, name, v,
                        perception);
        return -1;
    }
    return 0;
}
int fs_bits(int64_t n) {
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < n) bits++;
    return bits;
}
// the handle's one sort scratch (whose sticky error word sync_checked reports) must also hold a sort of n pairs on `bits`
int fs_sort_temp(bdmi_flock *f, int64_t n, int bits) {
    const size_t need = nbmi::radix_temp_bytes_u32((size_t)n, bits);
    if (need <= f->tmp_sort_bytes) return 0;
    if (int rc = sync_checked(f)) return rc;
    char *t = (char *)f->tmp_sort;
    f->tmp_sort = nullptr;
    f->tmp_sort_bytes = 0;
    if (dev_regrow(f, &t, need + 256)) return -2;
    f->tmp_sort = t;
    f->tmp_sort_bytes = need;
    NBMI_HIP_CHECK(nbmi::radix_init_temp(t, f->stream));
    return 0;
}
int fs_buffers(bdmi_flock *f) {
    FlockStats &s = f->fs;
    if (s.parent) return 0;
    const size_t n = (size_t)(f->n > 0 ? f->n : 1);
    if (dev_alloc(f, &s.parent, n) || dev_alloc(f, &s.root, n) || dev_alloc(f, &s.minid, n) || dev_alloc(f, &s.cnt, n) ||
        dev_alloc(f, &s.lcnt, n) || dev_alloc(f, &s.lab, n) || dev_alloc(f, &s.lab_s, n) || dev_alloc(f, &s.rank, n) ||
        dev_alloc(f, &s.rank_s, n) || dev_alloc(f, &s.qkey, n) || dev_alloc(f, &s.qkey_s, n) || dev_alloc(f, &s.qval, n) ||
        dev_alloc(f, &s.qval_s, n) || dev_alloc(f, &s.counters, 4))
        return -2;
    return 0;
}
int fs_occ_words(const bdmi_flock *f) { return (f->grid.dim + 31) / 32; }
int fs_row_buffers(bdmi_flock *f, int64_t rows, int64_t chunks) {
    FlockStats &s = f->fs;
    if (rows > s.rows_cap) {
        s.rows_cap = 0;
        if (dev_regrow(f, &s.chunk_off, (size_t)rows + 1) || dev_regrow(f, &s.rows16, (size_t)rows * 16) ||
            dev_regrow(f, &s.row_label, (size_t)rows) || dev_regrow(f, &s.row_members, (size_t)rows))
            return -2;
        if (f->periodic && (dev_regrow(f, &s.occ_mask, (size_t)rows * 3 * fs_occ_words(f)) ||
                            dev_regrow(f, &s.wrap3, (size_t)rows * 3) || dev_regrow(f, &s.centre, (size_t)rows * 3)))
            return -2;
        s.rows_cap = rows;
    }
    if (chunks > s.chunks_cap) {
        s.chunks_cap = 0;
        if (dev_regrow(f, &s.part, (size_t)chunks * kFsVals)) return -2;
        s.chunks_cap = chunks;
    }
    return 0;
}
// grid, union-find over the links, labels: leaves root / minid / cnt / lab / lcnt, the labels in the caller's order in
// the staging buffer and the counters {links, evals, flocks}
int fs_enqueue_flocks(bdmi_flock *f, double b2) {
    const int64_t n = f->n;
    FlockStats &s = f->fs;
    hipStream_t st = f->stream;
    if (int rc = fs_buffers(f)) return rc;
    if (int rc = enqueue_grid(f, false)) return rc;
    NBMI_HIP_CHECK(hipMemsetAsync(s.counters, 0, 4 * sizeof(unsigned long long), st));
    k_fs_init<<<nblocks(n), kBlock, 0, st>>>(n, s.parent, s.minid, s.cnt, s.rank);
    if (f->periodic)
        k_fs_link<<<nblocks(n), kBlock, 0, st>>>(f->B.p, f->occ, f->cell_start, n, periodic_grid(f), b2, s.parent, s.counters);
    else
        k_fs_link<<<nblocks(n), kBlock, 0, st>>>(f->B.p, f->occ, f->cell_start, n, f->grid, b2, s.parent, s.counters);
    k_fs_flatten<<<nblocks(n), kBlock, 0, st>>>(n, s.parent, f->B.id, s.root, s.minid, s.cnt);
    k_fs_labels<<<nblocks(n), kBlock, 0, st>>>(n, s.root, s.minid, s.cnt, f->B.id, s.lab, s.lcnt, (int32_t *)f->stage,
                                               s.counters + 2);
    NBMI_HIP_CHECK(hipGetLastError());
    return 0;
}
// the two passes over `rows` rows whose members (host copy: members[]) are described by rkey / rhead on the device;
// torus = the rows of bdmi_periodic_flock_catalogue: occupancy and cuts first, then the FsTorus instances of the passes
int fs_enqueue_rows(bdmi_flock *f, int64_t rows, const int64_t *members, const uint32_t *rank_s, const uint32_t *lab_s,
                    const uint32_t *rkey, const uint32_t *rhead, bool with_labels, bool torus = false) {
    FlockStats &s = f->fs;
    hipStream_t st = f->stream;
    std::vector<int32_t> off((size_t)rows + 1);
    int64_t chunks = 0;
    for (int64_t i = 0; i < rows; i++) {
        off[(size_t)i] = (int32_t)chunks;
        chunks += (members[i] + kFsChunk - 1) / kFsChunk;
    }
    off[(size_t)rows] = (int32_t)chunks;
    if (int rc = fs_row_buffers(f, rows, chunks)) return rc;
    NBMI_HIP_CHECK(hipMemcpyAsync(s.chunk_off, off.data(), off.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    NBMI_HIP_CHECK(hipStreamSynchronize(st));  // `off` is pageable host memory that ends with this function
    auto passes = [&](const auto &tor) {
        k_fs_chunks<1><<<(int)chunks, kBlock, 0, st>>>(f->B.p, f->B.v, rank_s, rkey, rhead, f->n, s.chunk_off, (int)rows, s.rows16,
                                                      s.part, tor);
        k_fs_combine<1><<<nblocks(rows), kBlock, 0, st>>>(lab_s, rkey, rhead, f->n, s.chunk_off, (int)rows, s.part, s.rows16,
                                                         with_labels ? s.row_label : nullptr,
                                                         with_labels ? s.row_members : nullptr, tor);
        k_fs_chunks<2><<<(int)chunks, kBlock, 0, st>>>(f->B.p, f->B.v, rank_s, rkey, rhead, f->n, s.chunk_off, (int)rows, s.rows16,
                                                      s.part, tor);
        k_fs_combine<2><<<nblocks(rows), kBlock, 0, st>>>(lab_s, rkey, rhead, f->n, s.chunk_off, (int)rows, s.part, s.rows16,
                                                         nullptr, nullptr, tor);
    };
    if (torus) {
        const GridPer g = periodic_grid(f);
        const int words = fs_occ_words(f);
        NBMI_HIP_CHECK(hipMemsetAsync(s.occ_mask, 0, (size_t)rows * 3 * words * sizeof(uint32_t), st));
        k_fs_occupancy<<<(int)chunks, kBlock, 0, st>>>(f->B.p, rank_s, rkey, rhead, f->n, s.chunk_off, (int)rows, g, words,
                                                      s.occ_mask);
        k_fs_wrap<<<nblocks(3 * rows), kBlock, 0, st>>>(s.occ_mask, (int)rows, g.dim, words, s.wrap3);
        passes(FsTorus{g, s.wrap3, s.centre});
    } else {
        passes(FsBox{});
    }
    NBMI_HIP_CHECK(hipGetLastError());
    return 0;
}
}  // namespace

static int fs_flocks(bdmi_flock *f, double link, int32_t *labels, int64_t *n_flocks, int64_t *links, int64_t *evals) {
    const int64_t n = f->n;
    unsigned long long h[4] = {0, 0, 0, 0};
    if (n > 0) {
        if (int rc = fs_enqueue_flocks(f, link * link)) return rc;
        hipStream_t st = f->stream;
        NBMI_HIP_CHECK(hipMemcpyAsync(h, f->fs.counters, sizeof(h), hipMemcpyDeviceToHost, st));
        if (labels) NBMI_HIP_CHECK(hipMemcpyAsync(labels, f->stage, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        if (int rc = sync_checked(f)) return rc;
    }
    if (links) *links = (int64_t)h[0];
    if (evals) *evals = (int64_t)h[1];
    if (n_flocks) *n_flocks = (int64_t)h[2];
    return 0;
}
int bdmi_flocks(bdmi_flock *f, double link, int32_t *labels, int64_t *n_flocks, int64_t *links, int64_t *evals) {
    if (int rc = fs_radius_check(f, "bdmi_flocks", "link", link)) return rc;
    return fs_flocks(f, link, labels, n_flocks, links, evals);
}
int bdmi_periodic_flocks(bdmi_flock *f, double link, int32_t *labels, int64_t *n_flocks, int64_t *links, int64_t *evals) {
    if (int rc = fs_radius_check(f, "bdmi_periodic_flocks", "link", link, "bdmi_flocks")) return rc;
    return fs_flocks(f, link, labels, n_flocks, links, evals);
}

// the catalogue of either kind of handle, behind fs_radius_check; wrap3 (may be null) only on a periodic one
static int fs_catalogue(bdmi_flock *f, const char *what, double link, int64_t min_members, int64_t capacity, int32_t *label,
                        int64_t *members, double *rows16, int32_t *wrap3, int64_t *count) {
    if (min_members < 1 || capacity < 0) {
        nbmi::set_error("%s: min_members = %lld must be >= 1 and capacity = %lld >= 0", what, (long long)min_members,
                        (long long)capacity);
        return -1;
    }
    if (!count || (capacity > 0 && (!label || !members || !rows16))) {
        nbmi::set_error("%s: null count, or null output with capacity > 0", what);
        return -1;
    }
    const int64_t n = f->n;
    if (n == 0) { *count = 0; return 0; }
    const int bits = fs_bits(n);
    if (int rc = fs_sort_temp(f, n, bits)) return rc;
    if (int rc = fs_enqueue_flocks(f, link * link)) return rc;
    FlockStats &s = f->fs;
    hipStream_t st = f->stream;
    // the ranks by label, stable; the heads of the qualifying flocks in label order; those by n - members, stable
    NBMI_HIP_CHECK(nbmi::radix_sort_pairs_u32(f->tmp_sort, f->tmp_sort_bytes, s.lab, s.lab_s, s.rank, s.rank_s, (size_t)n, 0, bits,
                                              st));
    scan::enqueue_compact(FsHeadSel{s.lab_s, s.lcnt, min_members}, n, f->tile_cnt, FsEmitHead{s.lab_s, s.lcnt, n, s.qkey, s.qval},
                          st);
    NBMI_HIP_CHECK(hipGetLastError());
    uint32_t total = 0;
    NBMI_HIP_CHECK(hipMemcpyAsync(&total, f->tile_cnt + scan::tiles_for(n), 4, hipMemcpyDeviceToHost, st));
    if (int rc = sync_checked(f)) return rc;
    const int64_t rows = (int64_t)total < capacity ? (int64_t)total : capacity;
    if (rows > 0) {
        if (int rc = fs_sort_temp(f, (int64_t)total, bits)) return rc;
        NBMI_HIP_CHECK(nbmi::radix_sort_pairs_u32(f->tmp_sort, f->tmp_sort_bytes, s.qkey, s.qkey_s, s.qval, s.qval_s, (size_t)total,
                                                  0, bits, st));
        std::vector<uint32_t> hkey((size_t)rows);
        NBMI_HIP_CHECK(hipMemcpyAsync(hkey.data(), s.qkey_s, (size_t)rows * 4, hipMemcpyDeviceToHost, st));
        if (int rc = sync_checked(f)) return rc;
        for (int64_t i = 0; i < rows; i++) members[i] = n - (int64_t)hkey[(size_t)i];
        if (int rc = fs_enqueue_rows(f, rows, members, s.rank_s, s.lab_s, s.qkey_s, s.qval_s, true, f->periodic)) return rc;
        NBMI_HIP_CHECK(hipMemcpyAsync(rows16, s.rows16, (size_t)rows * 16 * sizeof(double), hipMemcpyDeviceToHost, st));
        NBMI_HIP_CHECK(hipMemcpyAsync(label, s.row_label, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (f->periodic && wrap3)
            NBMI_HIP_CHECK(hipMemcpyAsync(wrap3, s.wrap3, (size_t)rows * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (int rc = sync_checked(f)) return rc;
    }
    *count = (int64_t)total;
    return 0;
}
int bdmi_flock_catalogue(bdmi_flock *f, double link, int64_t min_members, int64_t capacity, int32_t *label, int64_t *members,
                         double *rows16, int64_t *count) {
    if (int rc = fs_radius_check(f, "bdmi_flock_catalogue", "link", link)) return rc;
    return fs_catalogue(f, "bdmi_flock_catalogue", link, min_members, capacity, label, members, rows16, nullptr, count);
}
int bdmi_periodic_flock_catalogue(bdmi_flock *f, double link, int64_t min_members, int64_t capacity, int32_t *label,
                                  int64_t *members, double *rows16, int32_t *wrap3, int64_t *count) {
    if (int rc = fs_radius_check(f, "bdmi_periodic_flock_catalogue", "link", link, "bdmi_flock_catalogue")) return rc;
    return fs_catalogue(f, "bdmi_periodic_flock_catalogue", link, min_members, capacity, label, members, rows16, wrap3, count);
}

int bdmi_diagnostics(bdmi_flock *f, double *row16) {
    if (int rc = whole_flock_check(f, "bdmi_diagnostics")) return rc;
    if (!row16) { nbmi::set_error("bdmi_diagnostics: null output"); return -1; }
    const int64_t n = f->n;
    if (n == 0) { memset(row16, 0, 16 * sizeof(double)); return 0; }
    if (int rc = fs_buffers(f)) return rc;
    if (int rc = enqueue_grid(f, false)) return rc;
    FlockStats &s = f->fs;
    hipStream_t st = f->stream;
    // one row of all the boids in rank order: head 0, key n - n = 0
    NBMI_HIP_CHECK(hipMemsetAsync(s.qkey, 0, 4, st));
    NBMI_HIP_CHECK(hipMemsetAsync(s.qval, 0, 4, st));
    if (int rc = fs_enqueue_rows(f, 1, &n, nullptr, nullptr, s.qkey, s.qval, false)) return rc;
    NBMI_HIP_CHECK(hipMemcpyAsync(row16, s.rows16, 16 * sizeof(double), hipMemcpyDeviceToHost, st));
    return sync_checked(f);
}

static int fs_neighbour_stats(bdmi_flock *f, double radius, int32_t *count, double *nn_d2, int64_t *evals) {
    const int64_t n = f->n;
    unsigned long long h = 0;
    if (n > 0) {
        if (int rc = fs_buffers(f)) return rc;
        if (int rc = enqueue_grid(f, false)) return rc;
        hipStream_t st = f->stream;
        int32_t *d_count = (int32_t *)f->stage;
        double *d_nn = f->stage + n;  // behind the n int32 counts (n doubles hold them twice over)
        NBMI_HIP_CHECK(hipMemsetAsync(f->fs.counters + 3, 0, sizeof(unsigned long long), st));
        if (f->periodic)
            k_fs_neighbours<<<nblocks(n), kBlock, 0, st>>>(f->B.p, f->B.id, f->occ, f->cell_start, n, periodic_grid(f),
                                                           radius * radius, d_count, d_nn, f->fs.counters + 3);
        else
            k_fs_neighbours<<<nblocks(n), kBlock, 0, st>>>(f->B.p, f->B.id, f->occ, f->cell_start, n, f->grid, radius * radius,
                                                           d_count, d_nn, f->fs.counters + 3);
        NBMI_HIP_CHECK(hipGetLastError());
        if (count) NBMI_HIP_CHECK(hipMemcpyAsync(count, d_count, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        if (nn_d2) NBMI_HIP_CHECK(hipMemcpyAsync(nn_d2, d_nn, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        NBMI_HIP_CHECK(hipMemcpyAsync(&h, f->fs.counters + 3, sizeof(h), hipMemcpyDeviceToHost, st));
        if (int rc = sync_checked(f)) return rc;
    }
    if (evals) *evals = (int64_t)h;
    return 0;
}
int bdmi_neighbour_stats(bdmi_flock *f, double radius, int32_t *count, double *nn_d2, int64_t *evals) {
    if (int rc = fs_radius_check(f, "bdmi_neighbour_stats", "radius", radius)) return rc;
    return fs_neighbour_stats(f, radius, count, nn_d2, evals);
}
int bdmi_periodic_neighbour_stats(bdmi_flock *f, double radius, int32_t *count, double *nn_d2, int64_t *evals) {
    if (int rc = fs_radius_check(f, "bdmi_periodic_neighbour_stats", "radius", radius, "bdmi_neighbour_stats")) return rc;
    return fs_neighbour_stats(f, radius, count, nn_d2, evals);
}

// C(r) beyond sight (include/bdmi.h): checks first, then quantise (+ grid and pair kernel when there are bins), then the
// three words per slot normalised into (hi, lo)
int bdmi_velocity_correlation(bdmi_flock *f, int nb, const double *edges, const double *mean3, int64_t *pairs, int64_t *dot,
                              int64_t *self5, int64_t *evals) {
    const char *what = "bdmi_velocity_correlation";
    if (!f) { nbmi::set_error("%s: null bdmi_flock handle", what); return -1; }
    if (int rc = whole_flock_check(f, what)) return rc;
    if (nb < 0 || nb > kVcMaxBins) { nbmi::set_error("%s: nb = %d must be in 0..%d", what, nb, kVcMaxBins); return -1; }
    if (nb > 0 && !edges) { nbmi::set_error("%s: null edges with nb = %d", what, nb); return -1; }
    if (!mean3) { nbmi::set_error("%s: null mean3", what); return -1; }
    for (int c = 0; c < 3; c++)
        if (!(fabs(mean3[c]) <= 1.0)) {  // NaN and +-inf fail too
            nbmi::set_error("%s: mean3[%d] = %g must be finite and at most 1 in magnitude", what, c, mean3[c]);
            return -1;
        }
    double e2[kVcSlots];
    int m = 0;
    if (nb > 0) {
        for (int k = 0; k <= nb; k++) {
            const double e = edges[k];
            e2[k] = e * e;
            const bool ok = e >= 0 && e2[k] < INFINITY && (k == 0 || (e > edges[k - 1] && e2[k] > e2[k - 1]));
            if (!ok) {
                nbmi::set_error("%s: edges[%d] = %g: the edges must be finite, >= 0 and strictly increasing, and so must their "
                                "squares", what, k, e);
                return -1;
            }
        }
        const double cell = f->grid.cell_size;
        const int dim = f->grid.dim;
        const int m_max = f->periodic && (dim - 1) / 2 < kVcMaxReach ? (dim - 1) / 2 : kVcMaxReach;
        const double mf = ceil(edges[nb] / cell);
        if (!(mf >= 1) || mf > m_max) {
            nbmi::set_error("%s: reach m = ceil(%g / %g) = %.0f cells must be in 1..%d%s (dim = %d); the largest admissible last "
                            "edge is %g", what, edges[nb], cell, mf, m_max,
                            f->periodic ? " (at most 16, and 2 m + 1 <= dim on a periodic handle)" : "", dim, m_max * cell);
            return -1;
        }
        m = (int)mf;
    }
    const int64_t n = f->n;
    unsigned long long h[kVcZeroed];
    memset(h, 0, sizeof(h));
    if (n > 0) {
        FlockStats &s = f->fs;
        if (!s.vc_acc && (dev_alloc(f, &s.vc_q, (size_t)n) || dev_alloc(f, &s.vc_acc, (size_t)kVcWords))) return -2;
        hipStream_t st = f->stream;
        if (nb > 0) {
            if (int rc = enqueue_grid(f, false)) return rc;
            memcpy(s.vc_e2, e2, (size_t)(nb + 1) * sizeof(double));
            NBMI_HIP_CHECK(hipMemcpyAsync(s.vc_acc + kVcEdges, s.vc_e2, (size_t)(nb + 1) * sizeof(double), hipMemcpyHostToDevice, st));
        }
        NBMI_HIP_CHECK(hipMemsetAsync(s.vc_acc, 0, kVcZeroed * sizeof(unsigned long long), st));
        k_vc_quantise<<<nblocks(n) < kVcQuantBlocks ? nblocks(n) : kVcQuantBlocks, kBlock, 0, st>>>(nb > 0 ? f->B.v : nullptr, f->B.id, f->A, n, mean3[0], mean3[1], mean3[2],
                                                    nb > 0 ? s.vc_q : nullptr, s.vc_acc);
        if (nb > 0 && f->periodic)
            k_vc_pairs<<<nblocks(n), kBlock, 0, st>>>(f->B.p, s.vc_q, f->occ, f->cell_start, n, periodic_grid(f), m, nb, s.vc_acc,
                                                      f->xcd_contiguous);
        else if (nb > 0)
            k_vc_pairs<<<nblocks(n), kBlock, 0, st>>>(f->B.p, s.vc_q, f->occ, f->cell_start, n, f->grid, m, nb, s.vc_acc,
                                                      f->xcd_contiguous);
        NBMI_HIP_CHECK(hipGetLastError());
        NBMI_HIP_CHECK(hipMemcpyAsync(h, s.vc_acc, sizeof(h), hipMemcpyDeviceToHost, st));
        if (int rc = sync_checked(f)) return rc;
    }
    // S = high 2^32 + low with low < 2^64: the unique (hi, lo) with 0 <= lo < 2^32
    auto norm = [](unsigned long long high, unsigned long long low, int64_t *out) {
        out[0] = (int64_t)high + (int64_t)(low >> 32);
        out[1] = (int64_t)(low & 0xffffffffull);
    };
    for (int k = 0; k <= nb && nb > 0; k++) {
        if (pairs) pairs[k] = (int64_t)h[3 * k];
        if (dot) norm(h[3 * k + 2], h[3 * k + 1], dot + 2 * k);
    }
    if (self5) {
        for (int c = 0; c < 3; c++) self5[c] = (int64_t)h[kVcSelf + c];
        norm(h[kVcSelf + 4], h[kVcSelf + 3], self5 + 3);
    }
    if (evals) *evals = (int64_t)h[kVcEvals];
    return 0;
}

}  // extern "C"


// ---- triangle rasteriser (raster.hip) reads a flock handle through these -----------------------------------
int nbmi::flock_source(bdmi_flock *f, int64_t *n, int *device, int *slab) {
    if (int rc = check(f)) return rc;
    *n = f->n; *device = f->device; *slab = f->slab ? 1 : 0;
    return 0;
}

// The device part of bdmi_visible_vertices: mark, count, scan, emit cones into the handle's scratch, then the
// number of visible boids.  `done` (may be null) is recorded on the flock's stream behind the last kernel.
int nbmi::flock_visible_device(bdmi_flock *f, const double *cam12, double tan_h, double tan_v, double fog_end,
                               double cone_length, double cone_radius, const float **d_verts, const float **d_cols,
                               int64_t *count, hipEvent_t done) {
    if (int rc = check(f)) return rc;
    const int64_t n = f->n;
    *count = 0;
    *d_verts = *d_cols = nullptr;
    if (n == 0) return 0;
    const int64_t ntiles = scan::tiles_for(n);
    if (!f->vis_flag) {
        if (dev_alloc(f, &f->vis_flag, vis::flag_bytes(n)) || dev_alloc(f, &f->vis_slot, (size_t)ntiles * scan::kTile) ||
            dev_alloc(f, &f->vis_tiles, ntiles + 1) || dev_alloc(f, &f->vis_verts, (size_t)n * 18) ||
            dev_alloc(f, &f->vis_cols, (size_t)n * 18))
            return -2;
        NBMI_HIP_CHECK(hipMemsetAsync(f->vis_flag, 0, vis::flag_bytes(n), f->stream));
    }
    vis::Camera c;
    for (int k = 0; k < 3; k++) { c.p[k] = cam12[k]; c.f[k] = cam12[3 + k]; c.r[k] = cam12[6 + k]; c.u[k] = cam12[9 + k]; }
    c.tan_h = tan_h; c.tan_v = tan_v; c.z_near = 0.5; c.z_far = fog_end; c.margin = 1.0;
    const Boids &a = f->A;
    hipStream_t st = f->stream;
    vis::k_mark<<<nblocks(n), kBlock, 0, st>>>(a.px, a.py, a.pz, a.id, n, c, f->vis_flag, f->vis_slot);
    vis::enqueue_visible(f->vis_flag, f->vis_slot, n, f->vis_tiles,
                         EmitCones{a, cone_length, cone_radius, f->vis_verts, f->vis_cols}, st);
    NBMI_HIP_CHECK(hipGetLastError());
    if (done) NBMI_HIP_CHECK(hipEventRecord(done, st));
    uint32_t total = 0;
    NBMI_HIP_CHECK(hipMemcpyAsync(&total, f->vis_tiles + ntiles, 4, hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    *count = total;
    *d_verts = f->vis_verts;
    *d_cols = f->vis_cols;
    return 0;
}
