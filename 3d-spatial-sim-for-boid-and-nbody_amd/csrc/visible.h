// Render-side reductions shared by libnbmi's two handles: frustum test per body,
// then an order-preserving compaction in the caller's ORIGINAL body order, so that only what a
// viewer would upload crosses PCIe.  The bodies live on the device in key / cell order with their
// original index in `id`, hence: mark by id -> the tile compaction of scan.h over the ids (count
// per tile, scan the tile counts, emit).  All float64, same operation order as the reference's
// functions (built with -ffp-contract=off): the masks are bit-identical to a CPython run of
//   compute_visibility_points   nbody/simulation.py:403-434   (z_near 0.1, margin 1.2)
//   compute_visibility_numba    boids/flock.py:311-348        (z_near 0.5, margin 1.0)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan.h"

namespace vis {

struct Camera {
    double p[3], f[3], r[3], u[3];
    double tan_h, tan_v, z_near, z_far, margin;
};

__device__ __forceinline__ bool frustum_visible(const Camera &c, double px, double py, double pz) {
    const double dx = px - c.p[0], dy = py - c.p[1], dz = pz - c.p[2];
    const double z = dx * c.f[0] + dy * c.f[1] + dz * c.f[2];
    if (z < c.z_near || z > c.z_far) return false;
    const double x = dx * c.r[0] + dy * c.r[1] + dz * c.r[2];
    const double y = dx * c.u[0] + dy * c.u[1] + dz * c.u[2];
    const double half_width = z * c.tan_h * c.margin;   // margin 1.0 multiplies exactly
    const double half_height = z * c.tan_v * c.margin;
    return fabs(x) < half_width && fabs(y) < half_height;
}

// slot = where the body is stored now; id[slot] = its original index
static __global__ __launch_bounds__(scan::kBlock) void k_mark(const double *__restrict__ x, const double *__restrict__ y,
                                                        const double *__restrict__ z, const int32_t *__restrict__ id,
                                                        int64_t n, Camera c, uint8_t *__restrict__ flag,
                                                        uint32_t *__restrict__ slot_of) {
    const int64_t s = (int64_t)blockIdx.x * scan::kBlock + threadIdx.x;
    if (s >= n) return;
    const int32_t i = id[s];
    flag[i] = frustum_visible(c, x[s], y[s], z[s]) ? 1 : 0;
    slot_of[i] = (uint32_t)s;
}

// the compaction's predicate: the 8 flags of a thread as a bit mask, one 8-byte load (flag[] is padded to a multiple
// of 8 and zero beyond n)
struct Flagged {
    const uint8_t *flag;
    __device__ unsigned operator()(int64_t first, int64_t n) const {
        const unsigned long long w = *reinterpret_cast<const unsigned long long *>(flag + first);
        unsigned m = 0;
#pragma unroll
        for (int k = 0; k < scan::kItems; k++) m |= (unsigned)((w >> (8 * k)) & 1ull) << k;
        return first < n ? m : 0u;
    }
};

// the compaction's emit: Emit(k, i, slot) writes output row k for original index i stored at `slot`
template <class Emit>
struct EmitVisible {
    const uint32_t *slot_of;
    Emit emit;
    __device__ void operator()(unsigned m, int64_t first, int64_t k) const {
        scan::for_each_item(m, first, k, [&](int64_t i, int64_t row) { emit(row, i, slot_of[i]); });
    }
};

// flag / slot_of (from k_mark) -> the visible bodies' rows in original order; tiles[tiles_for(n)] = their number
template <class Emit>
void enqueue_visible(const uint8_t *flag, const uint32_t *slot_of, int64_t n, uint32_t *tiles, const Emit &emit, hipStream_t st) {
    scan::enqueue_compact(Flagged{flag}, n, tiles, EmitVisible<Emit>{slot_of, emit}, st);
}

inline size_t flag_bytes(int64_t n) { return (size_t)scan::tiles_for(n) * scan::kTile + 8; }

}  // namespace vis
