// The one place that knows how a workgroup scans: the block scan, the single-workgroup scan of per-tile values, and
// the order-preserving tile compaction ("count per tile, scan the tile counts, emit") built on them.
//
// ORDER CONTRACT of block_scan (floating-point callers - the octree build's Mom4 and double-double SubVal - depend on
// it bit for bit; integer callers do not care):
//   1. inside a wave a Kogge-Stone scan over the distances 1, 2, 4, .. 32, each step applied as
//      own = op(value from the lane `distance` below, own);
//   2. lane 63 writes the wave's total to LDS; one barrier;
//   3. front = seed, then front = op(front, total of wave q) for the waves q in front of this one, left to right;
//      total = the wave totals folded left to right from wave 0's (the seed is NOT part of it);
//   4. incl = op(front, the lane's value of step 1);  excl = front in lane 0, else the incl of the lane below.
// `seed` is what lies in front of the whole workgroup: the operator's identity for a plain scan, the running carry for
// a scan continued over several rounds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace scan {

struct Sum {
    template <class T>
    __device__ T operator()(const T &a, const T &b) const { return a + b; }
};
struct Min {
    template <class T>
    __device__ T operator()(const T &a, const T &b) const { return b < a ? b : a; }
};

// The value of the lane d below.  A value type that is not a scalar supplies its own overload next to its definition.
template <class T>
__device__ __forceinline__ T lane_up(const T &v, int d) { return __shfl_up(v, d); }

template <class T>
struct Scanned {
    T excl, incl, total;
};

// Scan over the NT threads of a workgroup (every thread calls it).  The LDS is the function's own; the trailing
// barrier lets the caller scan again at once.
template <int NT, class T, class Op>
__device__ __forceinline__ Scanned<T> block_scan(const T &v, const T &seed, Op op) {
    static_assert(NT % 64 == 0 && NT <= 1024, "whole waves of one workgroup");
    __shared__ T wave_total[NT / 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: the fold below branches on the scalar unit
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T below = lane_up(inc, d);
        if (lane >= d) inc = op(below, inc);
    }
    if (lane == 63) wave_total[wave] = inc;
    __syncthreads();
    T front = seed, total = wave_total[0];
#pragma unroll
    for (int q = 0; q < NT / 64; q++) {
        if (q < wave) front = op(front, wave_total[q]);
        if (q > 0) total = op(total, wave_total[q]);
    }
    __syncthreads();
    inc = op(front, inc);
    T ex = lane_up(inc, 1);
    if (lane == 0) ex = front;
    return Scanned<T>{ex, inc, total};
}

// Exclusive scan of m per-tile values in ONE workgroup, NT values per round with the carry in registers:
// out[i] = op over in[0 .. i), out[m] = the total.  blockIdx.y selects one of several arrays `stride` entries apart.
// In place (out == in, same element size) is fine: a thread overwrites only the entry it has read itself.
constexpr int kScanThreads = 1024;
template <class TI, class TO, class Op>
static __global__ __launch_bounds__(kScanThreads) void k_scan_values(const TI *in, TO *out, int64_t m, int64_t stride,
                                                                    TO ident, Op op) {
    in += (int64_t)blockIdx.y * stride;
    out += (int64_t)blockIdx.y * stride;
    TO carry = ident;
    for (int64_t base = 0; base < m; base += kScanThreads) {
        const int64_t i = base + threadIdx.x;
        const TO v = i < m ? (TO)in[i] : ident;
        const Scanned<TO> s = block_scan<kScanThreads>(v, carry, op);
        if (i < m) out[i] = s.excl;
        carry = op(carry, s.total);
    }
    if (threadIdx.x == 0) out[m] = carry;
}

// ---- tile compaction -------------------------------------------------------------------------------------------
// First output slot of a thread that emits c outputs, given the scanned offsets of the tiles (one tile per workgroup).
template <int NT, class TO>
__device__ __forceinline__ int64_t tile_slot(const TO *__restrict__ tile_off, unsigned c) {
    return (int64_t)tile_off[blockIdx.x] + block_scan<NT>(c, 0u, Sum()).excl;
}

// The 256 x 8 layout: a thread owns 8 consecutive items.
constexpr int kBlock = 256;
constexpr int kItems = 8;
constexpr int kTile = kBlock * kItems;
inline int64_t tiles_for(int64_t n) { return (n + kTile - 1) / kTile; }

// bit k = item first + k exists and f(first + k) holds
template <class F>
__device__ __forceinline__ unsigned item_mask(int64_t first, int64_t n, F f) {
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < kItems; k++) m |= (first + k < n && f(first + k) ? 1u : 0u) << k;
    return m;
}
// f(item, slot) for the set bits of m, the slots counting up from `slot`
template <class F>
__device__ __forceinline__ void for_each_item(unsigned m, int64_t first, int64_t slot, F f) {
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        if (!((m >> k) & 1u)) continue;
        f(first + k, slot);
        slot++;
    }
}

// pred(first, n): the mask of the thread's 8 items that are selected (item_mask for a per-item test)
template <class Pred>
static __global__ __launch_bounds__(kBlock) void k_count(Pred pred, int64_t n, uint32_t *__restrict__ tile_cnt) {
    const int64_t first = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kItems;
    const unsigned total = block_scan<kBlock>((unsigned)__popc(pred(first, n)), 0u, Sum()).total;
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}
// emit(mask, first, slot): the thread's selected items go to the output slots from `slot` on (for_each_item, or
// whatever batches better across the 8 items)
template <class Pred, class Emit>
static __global__ __launch_bounds__(kBlock) void k_emit(Pred pred, int64_t n, const uint32_t *__restrict__ tile_off,
                                                        Emit emit) {
    const int64_t first = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kItems;
    const unsigned m = pred(first, n);
    emit(m, first, tile_slot<kBlock>(tile_off, (unsigned)__popc(m)));
}

// count, scan, emit on stream st; tile_cnt: tiles_for(n) + 1 entries, the last one receives the number selected
template <class Pred, class Emit>
void enqueue_compact(const Pred &pred, int64_t n, uint32_t *tile_cnt, const Emit &emit, hipStream_t st) {
    const int64_t ntiles = tiles_for(n);
    k_count<<<(int)ntiles, kBlock, 0, st>>>(pred, n, tile_cnt);
    k_scan_values<<<1, kScanThreads, 0, st>>>(tile_cnt, tile_cnt, ntiles, (int64_t)0, 0u, Sum());
    k_emit<<<(int)ntiles, kBlock, 0, st>>>(pred, n, tile_cnt, emit);
}

}  // namespace scan
