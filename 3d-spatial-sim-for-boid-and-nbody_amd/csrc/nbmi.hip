// libnbmi.so - MI355X (gfx950) N-body backend: Barnes-Hut octree + stackless wave-shared tree
// walk with fused kick-drift, and the LDS-tiled direct O(N^2) fallback.  C ABI in include/nbmi.h.
//
// Reference behaviour being reproduced (file:line in /root/reference):
//   compute_bounds                nbody/simulation.py:308-317
//   get_octant / _center          nbody/simulation.py:38-60      (key digits)
//   build_octree                  nbody/simulation.py:63-198     (one body per leaf; cell SET is
//                                                                  insertion-order independent)
//   compute_forces_barnes_hut     nbody/simulation.py:201-278
//   update_positions_velocities   nbody/simulation.py:281-305
//   compute_colors_by_velocity    nbody/simulation.py:320-400
//   compute_forces_*_cuda, update_bodies_cuda   nbody/gpu_backend.py:145-257
//
// Design (DESIGN.md has the full story):
//   * master state float64 SoA in HBM, kept in key-sorted order (re-sorted every step; the
//     permutation is nearly the identity so the gather is almost coalesced); `id` maps a
//     sorted rank back to the caller's body index.
//   * keys: per-body replay of the reference's compare/halve recurrence in float64, 42 levels
//     (2 x 63 bit), so the cell set equals the reference's bit for bit.
//   * tree: for key-sorted bodies, delta[r] = common octal prefix length of bodies r, r+1.
//     Body r starts internal cells at levels (delta[r-1], delta[r]] and owns one leaf at level
//     max(delta[r-1], delta[r]) + 1.  Nodes are emitted in DFS pre-order with a `next` (skip
//     subtree) index, COM from float64 prefix sums of {m, m x} over the sorted bodies.
//   * walk: one wave64 per 64 consecutive sorted bodies walks the pre-order array with a single
//     wave-uniform cursor (scalar loads); every lane applies the reference's own per-body
//     opening test; the wave descends if ANY lane opens, lanes that accepted an ancestor sit
//     out until the cursor leaves that subtree.  Each lane's accepted set == the reference's.
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/nbmi.h"
#include "common.h"
#include "radix_hist.h"
#include "hilbert.h"
#include "visible.h"
#include "unionfind.h"

namespace nbmi {
static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char *get_error() { return g_err; }
void clear_error() { g_err[0] = 0; }
}  // namespace nbmi

using nbmi::Moment;

namespace {

constexpr int kBlock = 256;
constexpr int kMaxLevel = 42;  // key digits available (2 x 21)

// 24-byte octree node, DFS pre-order, read by the walk with scalar loads.  The node that follows in
// memory (first child, or for a leaf the next sibling) is always at own offset + 24, so only the
// "skip my subtree" link is stored; 24 instead of 32 bytes per node is 25 % more nodes per cache
// line (the walk slows by 30 % when the record is padded to 64 bytes: it is that sensitive).
struct alignas(8) Node {
    float cx, cy, cz;   // centre of mass (leaf: the body's position)
    float gm;           // G * mass
    float s2t;          // (2*half_size)^2 / theta^2 (accept when s2t < dist_sq); 0 for leaves
    unsigned next_off;  // BYTE offset (index * 24) of the first node after this node's subtree
};
constexpr unsigned kNodeBytes = 24;
// Float64 twin of an internal cell, row = node index: centre of mass and half size as the reference holds
// them (node_com / node_half_sizes, simulation.py:478-484).  Read only when the fp32 opening test lands
// inside its uncertainty band (K9); leaves have no row content (a leaf is always accepted).
struct alignas(16) Node64 {
    double cx, cy, cz, hs;
};
// [r3] The float64 node record, one per node (leaves too), read by the waves that compute their forces in float64
// (k_walk, "force precision"): centre of mass / body position and G m as the float64 state has them, the opening
// threshold and the skip link.  Same pre-order as `Node`; links are byte offsets in units of THIS record.
struct alignas(8) NodeD {
    double cx, cy, cz, gm;
    float s2t;          // as Node::s2t
    unsigned next_off;  // index * 40
};
constexpr unsigned kNodeDBytes = 40;
constexpr unsigned kBand64 = 2;  // half width (ulps of fp32 d^2) of the float64 loop's uncertainty band, see k_emit_tile
static_assert(sizeof(NodeD) == kNodeDBytes, "NodeD must be 40 bytes");
constexpr int64_t kMaxNodeDRows = 107000000;  // 32-bit byte offsets: 2^32 / 40
// Node links are 32-bit byte offsets: at most 2^32 / 24 rows.  The reference allocates min(8 M, 4N)
// rows (simulation.py:477) and uses ~1.5 N; this build allocates 4N + 4096 rows up to that ceiling,
// which still leaves 1.7 N rows at the largest supported body count.
constexpr int64_t kMaxNodeRows = 178000000;
constexpr int64_t kMaxBodies = 100000000;  // the reference's largest presets have 50 M bodies
inline int64_t node_rows_for(int64_t n) { return 4 * n + 4096 < kMaxNodeRows ? 4 * n + 4096 : kMaxNodeRows; }
// Node `num_nodes` is a sentinel that loops onto itself (next = own offset, zero mass, at
// "infinity", never opened): the unrolled walk may step onto it a few times after the traversal
// has ended.
static_assert(sizeof(Node) == kNodeBytes, "Node must be 24 bytes");

struct Bodies {
    double *x, *y, *z, *vx, *vy, *vz, *m;
    int32_t *id;
};

struct TreeInfo {
    unsigned long long maxabs_bits;  // max |coordinate| (non-negative double bit pattern)
    double bounds;                   // root half size
    long long num_nodes;             // N + number of internal cells (reference numbering)
    long long walk_nodes;            // nodes the walk covers: num_nodes, plus received trees in owner mode
    int max_level;                   // deepest leaf level
    int error;                       // 1 = node capacity exceeded
    int max_run;                     // longest run of bodies equal in the radix-sorted key prefix (> 64 only)
    int pad0;
    unsigned long long maxabs_next;  // max |coordinate| of the positions this step's integrating walk WRITES: the next
                                     // step's maxabs_bits without a pass over the bodies (k_header)
    unsigned long long wave_visits, lane_visits, lane_accepts;
    unsigned long long win_miss[4];  // counted walk: node-window misses for windows of 8/16/32/64 nodes
    unsigned long long jumps;        // cursor moves other than to the next node in memory
    unsigned long long xcd_visits[8];  // counted walk: wave-level visits executed on each XCD
    unsigned long long band_visits;    // counted walk: lane visits decided by the float64 re-test (near-ties)
    unsigned band2;                    // width (ulps of d^2) of the opening test's uncertainty band, see K9
    // Sticky: set together with `error`, but outside the range every step clears.  While it is set the
    // walk does not advance the state (the bodies keep the last good step), so an overflow in substep 3
    // of 10 is still there when the host looks (nbmi_sync / getters), which reports and clears it.
    int sticky_error;
    long long sticky_nodes;  // num_nodes of the build that overflowed
    // force precision "auto": 1 while a large part of the system asks for float64 - then every wave computes in it.
    // Entered when more than a third of the step's waves ask, left when fewer than a quarter do (hysteresis: a system
    // hovering at the threshold must not flip the whole walk between the two loops step by step).  [r4] Round 3
    // entered above one half: the held-out 1 M collision at dt 0.25 (36 % of the waves asking at the start, 61 % after
    // 100 steps) then ended at 3.1e-5 - 3 x inside the bound - where every wave in float64 ends at 2.5e-14 and costs
    // nothing extra (the waves that ask are the ones that visit most nodes: with 48 % of them in float64 the walk
    // already takes the all-float64 time; profiles/r04_precision_cases.jsonl).  Decided by k_scan_subtiles from
    // (ask_waves, n_waves) of the handle's own bodies; in owner mode with several ranks the host sums the ranks'
    // votes and sets the verdict for all of them (nbmi_owner_set_all64) - one system, one decision, whatever the
    // world size.  Outside the ranges the per-step header reset clears: the value of the last step is the state.
    int force_all64;
    int ask_waves, n_waves;  // this build's votes: waves whose own density asked for float64 / waves
    int pad1;
    // owner mode [r3]: the own tree in its global form (k_chain_fix) - how many of its first nodes are copies of cells
    // that begin on a lower rank (not walked, not exported), and where the walk array begins behind the jump node
    int own_skip, own_added;
    long long walk_first;
};

// ---------------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------------
// The build did not fit (this build, or an earlier one that nobody has reported yet): a kernel that reads the tree does
// nothing, the host reports it.
__device__ __forceinline__ bool tree_frozen(const TreeInfo *info) {
    return info->error != 0 || info->sticky_error != 0;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// XCD-aware block remap.  Hardware deals consecutive blocks round-robin over the 8 XCDs (blocks b
// and b+8 share an XCD and its L2).  Neighbouring body groups walk nearly the same nodes, so every
// XCD should get CONTIGUOUS runs of logical blocks; runs of `chunk` blocks are interleaved over
// the XCDs so that dense and sparse regions of the key order are spread evenly (chunk = 0: one
// contiguous eighth per XCD; chunk < 0: identity).  Speed only, never correctness.
__device__ __forceinline__ int logical_block(int b, int nb, int chunk) {
    if (chunk < 0) return b;
    const int xcd = b & 7, j = b >> 3;
    if (chunk == 0) {
        const int q = nb >> 3, rem = nb & 7;
        return xcd * q + (xcd < rem ? xcd : rem) + j;
    }
    const int span = 8 * chunk;
    const int full = (nb / span) * span;  // blocks covered by complete rounds of 8 chunks
    if (b >= full) return b;
    return ((j / chunk) * 8 + xcd) * chunk + (j % chunk);
}

__device__ __forceinline__ int cpl_digits(uint64_t ahi, uint64_t alo, uint64_t bhi, uint64_t blo) {
    const uint64_t xh = ahi ^ bhi;
    if (xh) return (__clzll((long long)xh) - 1) / 3;
    const uint64_t xl = alo ^ blo;
    if (xl) return 21 + (__clzll((long long)xl) - 1) / 3;
    return kMaxLevel;
}

// ---------------------------------------------------------------------------------------
// K1: max |coordinate|  (compute_bounds, simulation.py:308-317; max is order independent)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_maxabs(const double *__restrict__ x, const double *__restrict__ y,
                                                   const double *__restrict__ z, int64_t n, TreeInfo *info) {
    __shared__ double red[kBlock / 64];
    double mx = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        mx = fmax(mx, fabs(x[i]));
        mx = fmax(mx, fabs(y[i]));
        mx = fmax(mx, fabs(z[i]));
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; w++) mx = fmax(mx, red[w]);
        atomicMax(&info->maxabs_bits, (unsigned long long)__double_as_longlong(mx));
    }
}

// The step's tree header when the previous step's integrating walk has already left max |coordinate| of the
// positions it wrote in maxabs_next: take it over and clear the rest (instead of a memset + a pass over the bodies).
__global__ void k_header(TreeInfo *info) {
    if (threadIdx.x != 0) return;
    info->maxabs_bits = info->maxabs_next;
    info->maxabs_next = 0ull;
    info->bounds = 0.0;
    info->num_nodes = 0;
    info->walk_nodes = 0;
    info->max_level = 0;
    info->error = 0;
    info->max_run = 0;
    info->pad0 = 0;
}

// ---------------------------------------------------------------------------------------
// K2: octant-path keys.  Replays get_octant/get_octant_center (simulation.py:38-60) from the
// root cube [-bounds, bounds]^3: digit = x>=cx | (y>=cy)<<1 | (z>=cz)<<2, centre +- hs/2.
// Only compares, adds and exact halvings: bit-identical to the float64 reference.
// ---------------------------------------------------------------------------------------
// [r2] The digits are then RELABELLED along the 3-D Hilbert curve (hilbert.h: digit and next orientation from the
// octant and the cell's orientation, a 24-state machine carried down the 42 levels).  Which bodies share a
// level-L cell - every common-prefix length, hence the cell set, the node count, every cell's bodies - is
// untouched; what changes is the order of a cell's eight children in the sorted array, and with it which 64
// bodies share a wave: waves along the Hilbert curve are more compact and visit 7 % fewer nodes (1 M galaxy;
// 5 % at the 10 M collision; scripts/analysis/hilbert_groups.py).  nbmi_get_keys / nbmi_get_cells decode back
// to the reference's octant digits.  kHilbert = false (NBMI_HILBERT=0): plain octant digits.
// The packed sort word: (upper key word >> shift) << 24 | body index.  It holds while the sorted prefix has at most
// 40 bits and the index fits in 24 (packed_sort_ok() is the one place that decides).
constexpr int kPackIdxBits = 24, kPackMaxSortBits = 64 - kPackIdxBits;
constexpr uint64_t kPackIdxMask = (1ull << kPackIdxBits) - 1ull;

// 21 levels of the descent from the cell (cx, cy, cz, hs) in orientation st: one key word.  hd / hn: the Hilbert tables
// (k_keys: its copy in LDS; key_low_word: the constant tables).
template <bool kHilbert, typename TD, typename TN>
__device__ __forceinline__ uint64_t key_word(double px, double py, double pz, double &cx, double &cy, double &cz, double &hs,
                                             unsigned &st, const TD *hd, const TN *hn) {
    uint64_t kk = 0;
    for (int l = 0; l < 21; l++) {
        const double q = hs * 0.5;
        const bool bx = px >= cx, by = py >= cy, bz = pz >= cz;
        cx = bx ? cx + q : cx - q;
        cy = by ? cy + q : cy - q;
        cz = bz ? cz + q : cz - q;
        hs = q;
        const unsigned oct = (bx ? 1u : 0u) | (by ? 2u : 0u) | (bz ? 4u : 0u);
        if (kHilbert) {
            kk = (kk << 3) | (uint64_t)((hd[st] >> (3u * oct)) & 7u);
            st = (unsigned)(hn[st] >> (5u * oct)) & 31u;
        } else {
            kk = (kk << 3) | (uint64_t)oct;
        }
    }
    return kk;
}

// The low key word (levels 22 - 42) of one body, recomputed from its float64 position: the lean stepping build
// (k_keys<., true>) does not store it, and the three places that read it - members of a tie run whose upper words
// agree (k_tiefix), neighbours with equal upper words (k_gather_scan), cells below level 21 that reach beyond their
// tile (k_emit_tile) - meet such bodies essentially never (two bodies inside one cell of edge 2 bounds / 2^21).  The
// same recurrence, the same tables, the same bounds as k_keys: the same bits.
__device__ __noinline__ uint64_t key_low_word(bool hilbert, double px, double py, double pz, double bounds) {
    double cx = 0.0, cy = 0.0, cz = 0.0, hs = bounds;
    unsigned st = 0u;
    if (hilbert) {
        (void)key_word<true>(px, py, pz, cx, cy, cz, hs, st, nbmi::kHilDigit, nbmi::kHilNext);
        return key_word<true>(px, py, pz, cx, cy, cz, hs, st, nbmi::kHilDigit, nbmi::kHilNext);
    }
    (void)key_word<false>(px, py, pz, cx, cy, cz, hs, st, nbmi::kHilDigit, nbmi::kHilNext);
    return key_word<false>(px, py, pz, cx, cy, cz, hs, st, nbmi::kHilDigit, nbmi::kHilNext);
}
// where the low word of body b comes from: the stored array, or (lean build: key_lo == null) the position
__device__ __forceinline__ uint64_t low_word_of(const uint64_t *__restrict__ key_lo, const Bodies &cur, uint32_t b, int hilbert,
                                                const TreeInfo *info) {
    return key_lo ? key_lo[b] : key_low_word(hilbert != 0, cur.x[b], cur.y[b], cur.z[b], info->bounds);
}

// kLean: the upper word only, 21 levels, key_lo not written (the stepping build of a plain handle)
// k_keys_hist (packed path only): the kernel also counts the digits of the sorted prefix for every pass of the sort that
// follows, which then needs no read of `packed` for its histogram.  Its workgroups are 1 024 threads and cover `rounds`
// x 1 024 consecutive bodies each, at least 2 048 and few enough workgroups (keys_hist_grid) that the flush of their
// LDS counters - up to a thousand per pass, mostly ones after 256 bodies, every one a device-scope atomic on the same
// few cache lines - stays small: 256-thread workgroups of 2 048 bodies made 2.9 M such atomics at 10 M bodies and the
// kernel 0.057 ms slower, and left a SIMD two waves to hide the key recurrence's latency behind at 1 M (0.040 against
// 0.024 ms; profiles/sort_wide_ab.txt).  The Hilbert tables are copied once per workgroup.  Per body the same
// arithmetic either way.
constexpr int kKeysHistBlock = 1024, kKeysHistMaxGrid = 512;
constexpr int kKeysHistCounters = 4096;  // passes << digit bits of a packed field: 5 x 256 or 4 x 1 024 at the most
// Counting costs k_keys_hist what k_radix_hist costs on its own (the LDS atomics of a wave whose keys hold two or three
// values of a digit serialise in either); what the fusion saves is a launch, the read of `packed` and an emptier chip:
// keys + sort 0.150 -> 0.141 ms at 1 M bodies, but 0.741 -> 0.749 at 10 M (profiles/sort_wide_ab.txt).  Measured at those
// two sizes only; the boundary is the sort's own between its two large forms, an estimate.
static inline bool fused_hist_pays(int64_t n) { return n <= 2097152; }
static inline int keys_hist_grid(int64_t n) {
    const int64_t g = (n + 2 * kKeysHistBlock - 1) / (2 * kKeysHistBlock);
    return (int)(g < 1 ? 1 : (g > kKeysHistMaxGrid ? kKeysHistMaxGrid : g));
}
// one body's key words, index and (packed != null) packed sort word; returns the upper word
template <bool kHilbert, bool kLean>
__device__ __forceinline__ uint64_t keys_of_body(int64_t i, const double *__restrict__ x, const double *__restrict__ y,
                                                 const double *__restrict__ z, double bounds, uint64_t *__restrict__ key_hi,
                                                 uint64_t *__restrict__ key_lo, uint32_t *__restrict__ idx,
                                                 uint64_t *__restrict__ packed, int shift, const uint32_t *hd, const uint64_t *hn) {
    const double px = x[i], py = y[i], pz = z[i];
    double cx = 0.0, cy = 0.0, cz = 0.0, hs = bounds;
    uint64_t k[2];
    unsigned st = 0u;  // orientation of the current cell (root: 0)
    k[0] = key_word<kHilbert>(px, py, pz, cx, cy, cz, hs, st, hd, hn);
    key_hi[i] = k[0];
    if (!kLean) {
        k[1] = key_word<kHilbert>(px, py, pz, cx, cy, cz, hs, st, hd, hn);
        key_lo[i] = k[1];
    }
    // packed sort (enqueue_local_sort): the sorted prefix with the body index below it, ONE word for the keys-only sort
    if (packed) packed[i] = ((k[0] >> shift) << kPackIdxBits) | (uint64_t)i;
    else idx[i] = (uint32_t)i;
    return k[0];
}

template <bool kHilbert, bool kLean = false>
__global__ __launch_bounds__(kBlock) void k_keys(const double *__restrict__ x, const double *__restrict__ y,
                                                 const double *__restrict__ z, int64_t n, TreeInfo *info,
                                                 uint64_t *__restrict__ key_hi, uint64_t *__restrict__ key_lo,
                                                 uint32_t *__restrict__ idx, const uint8_t *__restrict__ dead = nullptr,
                                                 uint64_t *__restrict__ packed = nullptr, int shift = 0) {
    __shared__ uint32_t hd[nbmi::kHilStates];
    __shared__ uint64_t hn[nbmi::kHilStates];
    if (kHilbert) {
        if (threadIdx.x < nbmi::kHilStates) {
            hd[threadIdx.x] = nbmi::kHilDigit[threadIdx.x];
            hn[threadIdx.x] = nbmi::kHilNext[threadIdx.x];
        }
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    // bounds = max_extent * 1.1 + 10.0 with two roundings (no FMA contraction)
    const double maxabs = __longlong_as_double((long long)info->maxabs_bits);
    const double bounds = __dadd_rn(__dmul_rn(maxabs, 1.1), 10.0);
    if (i == 0) info->bounds = bounds;
    if (i >= n) return;
    if (dead && dead[i]) {  // owner mode: this row's body now lives on another rank; all ones sorts behind every key
        key_hi[i] = ~0ull;
        key_lo[i] = ~0ull;
        idx[i] = (uint32_t)i;
        return;
    }
    (void)keys_of_body<kHilbert, kLean>(i, x, y, z, bounds, key_hi, key_lo, idx, packed, shift, hd, hn);
}

// Out of line for k_keys_hist: inlined into its loop over the rounds the same code takes 95 VGPRs (128 and a spill with
// the low word) instead of k_keys' 46, and two workgroups of 1 024 threads no longer fit a CU.
template <bool kHilbert, bool kLean>
__device__ __noinline__ uint64_t keys_of_body_call(int64_t i, const double *__restrict__ x, const double *__restrict__ y,
                                                   const double *__restrict__ z, double bounds, uint64_t *__restrict__ key_hi,
                                                   uint64_t *__restrict__ key_lo, uint64_t *__restrict__ packed, int shift,
                                                   const uint32_t *hd, const uint64_t *hn) {
    return keys_of_body<kHilbert, kLean>(i, x, y, z, bounds, key_hi, key_lo, nullptr, packed, shift, hd, hn);
}

// k_keys of the packed path with the sort's histogram (see above): no dead rows, `packed` is written
template <bool kHilbert, bool kLean>
__global__ __launch_bounds__(kKeysHistBlock) void k_keys_hist(const double *__restrict__ x, const double *__restrict__ y,
                                                              const double *__restrict__ z, int64_t n, TreeInfo *info,
                                                              uint64_t *__restrict__ key_hi, uint64_t *__restrict__ key_lo,
                                                              uint64_t *__restrict__ packed, int shift, nbmi::RadixHist hist,
                                                              int rounds) {
    __shared__ uint32_t hd[nbmi::kHilStates];
    __shared__ uint64_t hn[nbmi::kHilStates];
    __shared__ unsigned hcnt[kKeysHistCounters];
    for (int c = threadIdx.x; c < (hist.passes << hist.digit_bits); c += kKeysHistBlock) hcnt[c] = 0u;
    if (kHilbert && threadIdx.x < nbmi::kHilStates) {
        hd[threadIdx.x] = nbmi::kHilDigit[threadIdx.x];
        hn[threadIdx.x] = nbmi::kHilNext[threadIdx.x];
    }
    __syncthreads();
    const double maxabs = __longlong_as_double((long long)info->maxabs_bits);
    const double bounds = __dadd_rn(__dmul_rn(maxabs, 1.1), 10.0);
    if (blockIdx.x == 0 && threadIdx.x == 0) info->bounds = bounds;
#pragma unroll 1
    for (int r = 0; r < rounds; r++) {
        const int64_t i = ((int64_t)blockIdx.x * rounds + r) * kKeysHistBlock + threadIdx.x;
        if (i >= n) break;
        const uint64_t hi = keys_of_body_call<kHilbert, kLean>(i, x, y, z, bounds, key_hi, key_lo, packed, shift, hd, hn);
        nbmi::radix_hist_count(hcnt, hi >> shift, hist.bits, hist.digit_bits, hist.passes);
    }
    __syncthreads();
    nbmi::radix_hist_flush(hcnt, hist.counts, hist.digit_bits, hist.passes, kKeysHistBlock);
}

// ---------------------------------------------------------------------------------------
// K4: finish the order.  The radix sort only looks at the top `sort_bits` bits of the upper key word
// (13 levels by default: 5 digit passes instead of 8); bodies that agree on those bits form a run - none or
// pairs in the bench systems, thousands inside one cell once an escaper has inflated the root cube - and
// are put in order of their full 126-bit key here.  One thread per body; a body inside a run finds the
// run's ends by galloping + binary search on the sorted prefixes and its place by counting the run's
// members that sort before it: L reads per member, all members in parallel, so a run of 10^5 bodies costs
// about a millisecond (a one-thread insertion sort of it took minutes).  Equal keys keep the input order
// (the sort is stable and idx ascends), like the reference's insertion order.  Writes the final
// permutation and the fully sorted upper words; the longest run is recorded so that the host can widen
// the sorted prefix for the following steps (and the stepping build goes back to full keys: a lean build
// recomputes the low words of a run's members, key_low_word, which is for runs of a few bodies).
// ---------------------------------------------------------------------------------------
// kPacked: `srt` holds the sorted PACKED words (k_keys) instead of the sorted upper words, and there is no `perm`: the
// body is the word's low 24 bits, the prefix the bits above them, and the full upper word comes from key_hi[body]
// (the unsorted array; nearly sequential, the state being kept in last step's order).  Same perm_out / hi_out / max_run.
template <bool kPacked>
__global__ __launch_bounds__(kBlock) void k_tiefix(const uint64_t *__restrict__ srt, const uint64_t *__restrict__ key_hi,
                                                   const uint64_t *__restrict__ key_lo,
                                                   const uint32_t *__restrict__ perm, int shift,
                                                   uint32_t *__restrict__ perm_out, uint64_t *__restrict__ hi_out, int64_t n,
                                                   TreeInfo *info, Bodies cur, int hilbert,
                                                   const int32_t *__restrict__ dead_rank = nullptr, int64_t n_dead = 0) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    // sorted prefix / body / full upper word of rank t
    auto prefix = [&](int64_t t) { return kPacked ? srt[t] >> kPackIdxBits : srt[t] >> shift; };
    auto body = [&](int64_t t) { return kPacked ? (uint32_t)(srt[t] & kPackIdxMask) : perm[t]; };
    auto upper = [&](int64_t t, uint32_t b) { return kPacked ? key_hi[b] : srt[t]; };
    const uint32_t p = body(r);
    const uint64_t h = upper(r, p), hp = prefix(r);
    if (!kPacked && dead_rank && h == ~0ull) {
        // owner mode: the row of a body that has left (all-ones key, larger than any real one): the n_dead of them
        // take the last n_dead places, in row order - no run to search, however many there are
        const int64_t slot = n - n_dead + dead_rank[p];
        perm_out[slot] = p;
        hi_out[slot] = h;
        return;
    }
    const bool tie = (r + 1 < n && prefix(r + 1) == hp) || (r > 0 && prefix(r - 1) == hp);
    if (!tie) {
        perm_out[r] = p;
        hi_out[r] = h;
        return;
    }
    // run = [s, e): first / one past the last rank with this prefix
    int64_t lo_ok = r, lo_bad, step = 1;
    for (;;) {  // backwards
        const int64_t t = r - step;
        if (t < 0) { lo_bad = -1; break; }
        if (prefix(t) == hp) { lo_ok = t; step <<= 1; } else { lo_bad = t; break; }
    }
    while (lo_ok - lo_bad > 1) {
        const int64_t mid = lo_bad + ((lo_ok - lo_bad) >> 1);
        if (prefix(mid) == hp) lo_ok = mid; else lo_bad = mid;
    }
    int64_t hi_ok = r, hi_bad;
    step = 1;
    for (;;) {  // forwards
        const int64_t t = r + step;
        if (t >= n) { hi_bad = n; break; }
        if (prefix(t) == hp) { hi_ok = t; step <<= 1; } else { hi_bad = t; break; }
    }
    while (hi_bad - hi_ok > 1) {
        const int64_t mid = hi_ok + ((hi_bad - hi_ok) >> 1);
        if (prefix(mid) == hp) hi_ok = mid; else hi_bad = mid;
    }
    const int64_t s = lo_ok, e = hi_bad;
    if (r == s && e - s > 64 && !(!kPacked && dead_rank && srt[e - 1] == ~0ull)) atomicMax(&info->max_run, (int)(e - s < 0x7fffffff ? e - s : 0x7fffffff));
    // key_lo == null (lean build): the low words are recomputed, and only once a member with this upper word shows up
    uint64_t la = key_lo ? key_lo[p] : 0ull;
    bool have_la = key_lo != nullptr;
    int64_t before = 0;
    for (int64_t j = s; j < e; j++) {
        const uint32_t pj = body(j);
        const uint64_t hj = upper(j, pj);
        if (hj != h) {
            before += hj < h ? 1 : 0;
        } else {
            if (pj == p) continue;
            if (!have_la) { la = low_word_of(key_lo, cur, p, hilbert, info); have_la = true; }
            const uint64_t lj = low_word_of(key_lo, cur, pj, hilbert, info);
            before += (lj < la || (lj == la && pj < p)) ? 1 : 0;
        }
    }
    perm_out[s + before] = p;
    hi_out[s + before] = h;
}

// ---------------------------------------------------------------------------------------
// K5 - K7 [r3]: ONE pass puts the bodies in key order and lays the ground for every cell's mass and centre of mass.
// A workgroup owns a tile (SUB-TILE of the prefix sums) of kScanTile = 2048 sorted ranks, swept in 8 rounds of 256:
//   * gather through the sort permutation: fp32 {x,y,z,G m} (walk / leaf data), the low key word;
//   * from the sorted keys of the two neighbours
//       delta[r] = common prefix digits of sorted bodies r and r+1 (delta[N-1] = -1),
//       cnt[r]   = number of internal cells whose first body is r = max(0, delta[r] - delta[r-1]);
//   * exclusive prefix sums INSIDE the tile (plain float64, straight from the float64 state):
//       S[r]    = sum over the sub-tile's bodies before r of {G m, G m x, G m y, G m z}     (32 bytes)
//       PexL[r] = the same for cnt
//     and the sub-tile's totals (sub_tot / sub_cnt).
// k_scan_subtiles then turns the totals into exclusive prefixes over the sub-tiles (T: double-double, subPex).
// A cell's moments are   (T[sub(e)] - T[sub(r)])  +  (S[e] - S[r])   for its body range [r, e):
// the first difference is exact to 1e-32 (double-double), the second is between sums of at most 2047 terms, so a
// cell's centre of mass is good to ~1e-13 of the coordinate wherever the cell sits in the array.  (A plain float64
// running sum over 10^6 bodies loses 1e-8, the size of the opening-test ties K9 re-decides in float64; round 2
// carried double-double sums through a three-phase scan of 64-byte records instead - 1.0 GB more traffic at 10 M
// bodies and three more kernels.)  Pre-order index helpers: pex_at(r) = subPex[r / 256] + PexL[r].
// ---------------------------------------------------------------------------------------
constexpr int kScanItems = 8;                      // rounds (sub-tiles) per workgroup
constexpr int kScanTile = kBlock * kScanItems;     // 2048 ranks per workgroup
constexpr int kSubShift = 11;                      // sub-tile = the workgroup's 2048 ranks
static_assert(kScanTile == (1 << kSubShift), "a sub-tile is one workgroup's tile");

// double-double (unevaluated sum of two float64)
struct dd {
    double h, l;
};
__device__ __forceinline__ dd dd_add(const dd &a, const dd &b) {
    const double s = a.h + b.h;
    const double bb = s - a.h;
    double e = (a.h - (s - bb)) + (b.h - bb);
    e += a.l + b.l;
    const double h = s + e;
    return dd{h, e - (h - s)};
}
__device__ __forceinline__ double dd_diff(const dd &a, const dd &b) {  // a - b, rounded once
    const dd d = dd_add(a, dd{-b.h, -b.l});
    return d.h + d.l;
}

__device__ __forceinline__ int64_t pex_at(const int32_t *__restrict__ PexL, const int32_t *__restrict__ subPex, int64_t r) {
    return (int64_t)subPex[r >> kSubShift] + PexL[r];
}

struct Mom4 {
    double m, x, y, z;
    int c;
};
__device__ __forceinline__ Mom4 operator+(const Mom4 &a, const Mom4 &b) { return Mom4{a.m + b.m, a.x + b.x, a.y + b.y, a.z + b.z, a.c + b.c}; }
__device__ __forceinline__ Mom4 lane_up(const Mom4 &v, int d) {  // scan.h's lane shift for this type
    return Mom4{__shfl_up(v.m, d), __shfl_up(v.x, d), __shfl_up(v.y, d), __shfl_up(v.z, d), __shfl_up(v.c, d)};
}

// lane exchange inside a row of 16 lanes as a DPP operand (CTRL: 0xB1 / 0x4E quad_perm [1,0,3,2] / [2,3,0,1], 0x141
// row_half_mirror, 0x140 row_mirror)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float add_f(float a, float b) { return a + b; }

template <bool kLean>
__global__ __launch_bounds__(kBlock) void k_gather_scan(Bodies cur, const uint32_t *__restrict__ perm,
                                                        const uint64_t *__restrict__ hi_s, const uint64_t *__restrict__ key_lo,
                                                        int64_t n, double G, float4 *__restrict__ posm_s,
                                                        double4 *__restrict__ p64_s /* may be null */, uint64_t *__restrict__ lo_s,
                                                        int32_t *__restrict__ delta, double4 *__restrict__ S,
                                                        int32_t *__restrict__ PexL, double4 *__restrict__ sub_tot,
                                                        int32_t *__restrict__ sub_cnt, unsigned char *__restrict__ wave_flag,
                                                        int32_t *__restrict__ sub_flag, float dens_thr, float edge_floor,
                                                        const TreeInfo *__restrict__ info, int hilbert) {
    // kLean (lean build; key_lo and lo_s are null): no low word is gathered or stored; the rare neighbours with equal
    // upper words get theirs from key_low_word
    __shared__ int wflag[kBlock / 64];
    int nflag = 0;  // (lane 0 of each wave) the wave's rounds whose density asks for float64 forces
    __shared__ int dl[kBlock + 1];  // delta of the round's ranks, dl[0] = delta of the rank before the round
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    Mom4 carry{0.0, 0.0, 0.0, 0.0, 0};  // the rounds before this one (plain float64: at most 2047 terms)
#pragma unroll 1
    for (int k = 0; k < kScanItems; k++) {
        const int64_t r0 = (int64_t)blockIdx.x * kScanTile + (int64_t)k * kBlock;
        if (r0 > n) break;  // entry n (the totals' slot) is the last one anybody reads
        const int64_t r = r0 + t;
        Mom4 v{0.0, 0.0, 0.0, 0.0, 0};
        int d = -1;
        uint64_t h = 0, l = 0;
        float fx = 0.f, fy = 0.f, fz = 0.f;
        if (r < n) {
            const uint32_t j = perm[r];
            const double x = cur.x[j], y = cur.y[j], z = cur.z[j], gm = G * cur.m[j];
            fx = (float)x; fy = (float)y; fz = (float)z;
            posm_s[r] = make_float4((float)x, (float)y, (float)z, (float)gm);
            if (p64_s) p64_s[r] = make_double4(x, y, z, gm);
            h = hi_s[r];
            if (!kLean) {
                l = key_lo[j];
                lo_s[r] = l;
            }
            if (r + 1 < n) {
                const uint64_t hn = hi_s[r + 1];
                uint64_t ln = 0ull;
                uint64_t lr = l;
                if (hn == h) {
                    if (kLean) lr = low_word_of(nullptr, cur, j, hilbert, info);
                    ln = kLean ? low_word_of(nullptr, cur, perm[r + 1], hilbert, info) : key_lo[perm[r + 1]];
                }
                d = cpl_digits(h, lr, hn, ln);
            }
            delta[r] = d;
            v = Mom4{gm, gm * x, gm * y, gm * z, 0};
        }
        if (wave_flag) {
            // [r3] force precision "auto", decided here where the sorted bodies pass through registers: G rho of the
            // DENSEST quarter of the wave (16 key-adjacent bodies: sum of G m over the volume of their bounding box, every
            // edge at least one softening length) against tau / dt^2.  Not the whole wave's box: 64 consecutive bodies
            // of the key order can straddle a gap (the two disks of the collision preset, a cell boundary high up in the
            // tree) and their common box then says nothing about where they sit.
            const bool have = r < n;
            const float big = 3.0e38f;
            float lox = have ? fx : big, hix = have ? fx : -big, loy = have ? fy : big, hiy = have ? fy : -big;
            float loz = have ? fz : big, hiz = have ? fz : -big, gsum = have ? (float)v.m : 0.f;
            // butterflies inside a row of 16 lanes as DPP operands (quad swaps, half-row mirror, row mirror: min, max and
            // the sum are symmetric) - one vector instruction each, where __shfl_xor is an LDS round trip (28 of them per
            // round cost 0.15 ms at 10 M bodies)
#define NBMI_ROW16(V, OP)                      \
    V = OP(V, dpp_f<0xB1>(V));                 \
    V = OP(V, dpp_f<0x4E>(V));                 \
    V = OP(V, dpp_f<0x141>(V));                \
    V = OP(V, dpp_f<0x140>(V));
            NBMI_ROW16(lox, fminf) NBMI_ROW16(hix, fmaxf) NBMI_ROW16(loy, fminf) NBMI_ROW16(hiy, fmaxf)
            NBMI_ROW16(loz, fminf) NBMI_ROW16(hiz, fmaxf) NBMI_ROW16(gsum, add_f)
#undef NBMI_ROW16
            const float vol = fmaxf(hix - lox, edge_floor) * fmaxf(hiy - loy, edge_floor) * fmaxf(hiz - loz, edge_floor);
            float dens = gsum > 0.f ? gsum / vol : 0.f;
            dens = fmaxf(dens, __shfl_xor(dens, 16));
            dens = fmaxf(dens, __shfl_xor(dens, 32));
            const int flag = dens > dens_thr ? 1 : 0;
            if (lane == 0) {
                if (r0 + 64 * w < n) wave_flag[(r0 >> 6) + w] = (unsigned char)flag;
                nflag += (r0 + 64 * w < n) ? flag : 0;
            }
        }
        dl[t + 1] = d;
        if (t == 0) {
            int dp = -1;
            if (r > 0 && r < n) {
                const uint64_t hp = hi_s[r - 1];
                uint64_t lp = 0ull, lr = l;
                if (hp == h) {
                    if (kLean) lr = low_word_of(nullptr, cur, perm[r], hilbert, info);
                    lp = kLean ? low_word_of(nullptr, cur, perm[r - 1], hilbert, info) : key_lo[perm[r - 1]];
                }
                dp = cpl_digits(hp, lp, h, lr);
            }
            dl[0] = dp;
        }
        __syncthreads();
        if (r < n) {
            const int dp = dl[t];
            v.c = d > dp ? d - dp : 0;
        }
        // scan over the 256 ranks of the round, continued from the rounds before it.  The exclusive value is the
        // neighbour's inclusive one, not inclusive - own (own is exactly representable in the sum only for cnt).
        // The scan's trailing barrier also covers the reuse of dl by the next round.
        const scan::Scanned<Mom4> sc = scan::block_scan<kBlock>(v, carry, scan::Sum());
        carry = carry + sc.total;
        if (r <= n) {
            S[r] = make_double4(sc.excl.m, sc.excl.x, sc.excl.y, sc.excl.z);
            PexL[r] = sc.excl.c;
        }
    }
    if (wave_flag) {
        if (lane == 0) wflag[w] = nflag;
        __syncthreads();
    }
    if (t == 0) {
        sub_tot[blockIdx.x] = make_double4(carry.m, carry.x, carry.y, carry.z);
        sub_cnt[blockIdx.x] = carry.c;
        if (wave_flag) sub_flag[blockIdx.x] = wflag[0] + wflag[1] + wflag[2] + wflag[3];
    }
}

// Exclusive prefixes over the sub-tile totals: T (double-double moments, 64 bytes) and subPex.  One workgroup of
// 1024 threads: a thread adds up a contiguous chunk, the chunk sums are scanned across the workgroup, a second
// sweep writes the prefixes.  (39 k sub-tiles at 10 M bodies: 1.6 MB in, 2.7 MB out.)
constexpr int kSubScanThreads = 1024;
struct SubVal {
    dd m, x, y, z;
    long long c;
};
__device__ __forceinline__ SubVal operator+(const SubVal &a, const SubVal &b) {
    return SubVal{dd_add(a.m, b.m), dd_add(a.x, b.x), dd_add(a.y, b.y), dd_add(a.z, b.z), a.c + b.c};
}
__device__ __forceinline__ SubVal sub_zero() { return SubVal{{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, 0}; }
__device__ __forceinline__ dd dd_shfl_up(const dd &v, int d) { return dd{__shfl_up(v.h, d), __shfl_up(v.l, d)}; }
__device__ __forceinline__ SubVal lane_up(const SubVal &v, int d) {  // scan.h's lane shift for this type
    return SubVal{dd_shfl_up(v.m, d), dd_shfl_up(v.x, d), dd_shfl_up(v.y, d), dd_shfl_up(v.z, d), __shfl_up(v.c, d)};
}
// the system-wide half of force precision "auto" (TreeInfo::force_all64): enter above a third of the waves, leave below a quarter
constexpr int kAll64Enter = 333, kAll64Leave = 250;
// (thresholds in per mille of the waves: kAll64Enter / kAll64Leave; NBMI_ALL64_ENTER / NBMI_ALL64_LEAVE for experiments)
__host__ __device__ inline int all64_rule(int prev, long long ask, long long waves, int enter_pm, int leave_pm) {
    return prev ? (1000 * ask >= (long long)leave_pm * waves ? 1 : 0) : (1000 * ask > (long long)enter_pm * waves ? 1 : 0);
}
__global__ void k_set_all64(TreeInfo *info, int v) { info->force_all64 = v; }

__global__ __launch_bounds__(kSubScanThreads) void k_scan_subtiles(const double4 *__restrict__ sub_tot,
                                                                   const int32_t *__restrict__ sub_cnt, int64_t nsub,
                                                                   Moment *__restrict__ T, int32_t *__restrict__ subPex,
                                                                   const int32_t *__restrict__ sub_flag, int64_t nwaves,
                                                                   int enter_pm, int leave_pm, TreeInfo *info) {
    __shared__ long long fsum[kSubScanThreads / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t chunk = (nsub + kSubScanThreads - 1) / kSubScanThreads;
    const int64_t b = (int64_t)t * chunk, e = b + chunk < nsub ? b + chunk : nsub;
    SubVal acc = sub_zero();
    long long fl = 0;
    for (int64_t i = b; i < e; i++) {
        const double4 q = sub_tot[i];
        acc = acc + SubVal{{q.x, 0.0}, {q.y, 0.0}, {q.z, 0.0}, {q.w, 0.0}, (long long)sub_cnt[i]};
        if (sub_flag) fl += sub_flag[i];
    }
    if (sub_flag) {
        // [r3, thresholds r4] force precision "auto": while a large part of the waves ask for float64 (all64_rule: entered
        // above a third, left below a quarter), every wave gets it - where much of the system needs float64, the sparse rest
        // interacts with the same massive cells (10 M collision at dt 0.25: the 5 % of the waves below any density threshold
        // end at 3.8e-4 after 50 steps in fp32, at 1e-10 in float64; at the 1 M galaxy a quarter of the waves ask at first and
        // the fp32 rest stays at 2e-6 after 100 steps)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) fl += __shfl_xor(fl, o);
        if (lane == 0) fsum[w] = fl;
    }
    // exclusive prefix of this thread's chunk
    SubVal run = scan::block_scan<kSubScanThreads>(acc, sub_zero(), scan::Sum()).excl;
    if (sub_flag && t == 0) {
        long long tot = 0;
        for (int q = 0; q < kSubScanThreads / 64; q++) tot += fsum[q];
        info->ask_waves = (int)tot;
        info->n_waves = (int)nwaves;
        info->force_all64 = all64_rule(info->force_all64, tot, nwaves, enter_pm, leave_pm);
    }
    for (int64_t i = b; i < e; i++) {
        T[i] = Moment{run.m.h, run.m.l, run.x.h, run.x.l, run.y.h, run.y.l, run.z.h, run.z.l};
        subPex[i] = (int32_t)run.c;
        const double4 q = sub_tot[i];
        run = run + SubVal{{q.x, 0.0}, {q.y, 0.0}, {q.z, 0.0}, {q.w, 0.0}, (long long)sub_cnt[i]};
    }
}

// Half width K (ulps of d^2) of the opening test's uncertainty band; derivation at K9.
__device__ __forceinline__ unsigned band_half_ulps(double maxabs, double eps) {
    double k = 8.0 + 7.0 * maxabs / eps;  // eps == 0: inf
    if (!(k < 2097152.0)) k = 2097152.0;  // cap 2^21 (band 2^22 ulps = a factor 1.5 ... 2 in d^2)
    return (unsigned)k + 1u;
}

// ---------------------------------------------------------------------------------------
// K8 [r3]: emit the nodes in DFS pre-order, one workgroup per tile of TILE sorted ranks (kEmitTile / kEmitTileSmall).
// Pre-order index of a node "started" by sorted body r (dp = delta[r-1], d = delta[r], cnt = max(0, d - dp)):
//   internal cell k of r (level dp+1+k, k < cnt) -> r + pex(r) + k,     leaf of r -> r + pex(r) + cnt.
// A cell (r, lev) holds the bodies [r, e), e - 1 = the first j >= r with delta[j] < lev ("nearest smaller value to
// the right").  Round 2 found e with a gallop + binary search on the sorted KEYS in global memory, one thread per
// cell: ~2 log2(size) dependent 16-byte probes each, 527 us at 10 M bodies (64 % of the wave cycles parked at
// s_waitcnt).  Now the tile's delta values sit in LDS as bytes under a min-tree (heap layout); the query "first
// j >= r with delta[j] < lev" climbs from leaf r to the first subtree on its right whose minimum is small enough
// and descends to its leftmost such leaf - a handful of LDS byte reads for the small cells that make up the
// bulk.  Only cells that reach beyond their tile (<= depth of the tree per tile boundary) fall back to the key
// search, started at the tile's end.  The same workgroup writes the leaves and lists the tile's cells in LDS
// (chunks of kCellChunk), so the cell list never travels through global memory.
// Mass / centre of mass of [r, e): see K5-K7.
// ---------------------------------------------------------------------------------------
constexpr int kEmitTile = 512, kEmitTileSmall = 256;
constexpr int64_t kEmitSmallBodies = 262144;  // up to here the small tile (>= 1024 workgroups from 262 k bodies on either way)

// moments (G m, G m x, G m y, G m z summed) of the bodies at sorted ranks [r, e): in-tile prefix differences, plus
// the double-double tile prefixes where the range crosses tiles
__device__ __forceinline__ void range_moments(const double4 *__restrict__ S, const Moment *__restrict__ T, int64_t r, int64_t e,
                                              double &M, double &mx, double &my, double &mz) {
    const double4 s0 = S[r], s1 = S[e];
    M = s1.x - s0.x; mx = s1.y - s0.y; my = s1.z - s0.z; mz = s1.w - s0.w;
    const int64_t ur = r >> kSubShift, ue = e >> kSubShift;
    if (ue != ur) {
        const Moment a = T[ur], b = T[ue];
        M += dd_diff(dd{b.m, b.ml}, dd{a.m, a.ml});
        mx += dd_diff(dd{b.x, b.xl}, dd{a.x, a.xl});
        my += dd_diff(dd{b.y, b.yl}, dd{a.y, a.yl});
        mz += dd_diff(dd{b.z, b.zl}, dd{a.z, a.zl});
    }
}

__device__ __forceinline__ void write_sentinel(Node *__restrict__ nodes, int32_t *__restrict__ node_ref, int64_t total,
                                               int64_t link_base = 0) {
    Node sn;
    sn.cx = sn.cy = sn.cz = 1.0e30f;
    sn.gm = 0.f; sn.s2t = 0.f;
    sn.next_off = (unsigned)(total + link_base) * kNodeBytes;
    nodes[total] = sn;
    if (node_ref) node_ref[total] = -1;
}

// [r4] TILE is a template parameter.  Round 3 used 2 048 ranks per workgroup throughout; measured this round
// (profiles/r04_emit_tile_sweep.txt): tree phase at 1 M bodies 0.147 ms with 2 048, 0.134 / 0.133 / 0.135 with 1 024 / 512 /
// 256; at 10 M 1.32 / 1.18 / 1.16 / 1.26 ms; at 10 k bodies five workgroups of 2 048 ranks took 58 us (the tile's serial
// phases, an empty chip), forty of 256 a quarter of that.  512 ships, 256 up to 262 k bodies.  Only the decomposition
// changes (a cell that reaches beyond its tile is found by the key search either way): the nodes written are the same.
template <int TILE>
__global__ __launch_bounds__(kBlock) void k_emit_tile(const int32_t *__restrict__ delta, const int32_t *__restrict__ PexL,
                                                      const int32_t *__restrict__ subPex, const double4 *__restrict__ S,
                                                      const Moment *__restrict__ T, const float4 *__restrict__ posm_s,
                                                      const uint64_t *__restrict__ hi_s,
                                                      const uint64_t *__restrict__ lo_s, int64_t n, int64_t capacity,
                                                      double eps, double inv_theta2, Node *__restrict__ nodes,
                                                      Node64 *__restrict__ nodes64, uint8_t *__restrict__ node_level,
                                                      int32_t *__restrict__ node_ref, double4 *__restrict__ diag64,
                                                      NodeD *__restrict__ nodesd /* may be null */, Bodies cur,
                                                      const uint32_t *__restrict__ perm, double G, TreeInfo *info, int hilbert,
                                                      int64_t link_base /* owner mode: the arrays passed in begin at this row of
                                                                           the walk array, and the links count from ITS start */) {
    __shared__ uint8_t tree[2 * TILE];   // heap: tree[TILE + i] = delta[base + i] + 1, inner nodes = min of children
    __shared__ uint8_t dprev;                 // delta[base - 1] + 1
    __shared__ uint32_t cells[(2 * TILE)];    // node slot -> (local body index << 6) | k (k-th node of that body)
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * TILE;
    const int64_t total = n + pex_at(PexL, subPex, n);
    if (blockIdx.x == 0 && t == 0) {
        info->num_nodes = total;
        info->walk_nodes = total;
        info->band2 = 2u * band_half_ulps(__longlong_as_double((long long)info->maxabs_bits), eps);
        if (total + 1 > capacity) {  // + 1: the sentinel
            info->error = 1;
            if (info->sticky_error == 0) {
                info->sticky_error = 1;
                info->sticky_nodes = total;
            }
        } else {
            write_sentinel(nodes, node_ref, total, link_base);
            if (nodesd) nodesd[total] = NodeD{1.0e30, 1.0e30, 1.0e30, 0.0, 0.0f, (unsigned)(total + link_base) * kNodeDBytes};
        }
    }
    if (total + 1 > capacity) return;
    // delta of the tile as bytes (ranks >= n - 1 count as -1: nothing reaches across the end of the array)
    for (int i = t; i < TILE; i += kBlock) {
        const int64_t r = base + i;
        tree[TILE + i] = (uint8_t)((r < n ? delta[r] : -1) + 1);
    }
    if (t == 0) dprev = (uint8_t)((base > 0 ? delta[base - 1] : -1) + 1);
    __syncthreads();
    for (int width = TILE / 2; width >= 1; width >>= 1) {
        for (int i = t; i < width; i += kBlock) {
            const uint8_t a = tree[2 * (width + i)], b = tree[2 * (width + i) + 1];
            tree[width + i] = a < b ? a : b;
        }
        __syncthreads();
    }
    const int64_t q_tile = pex_at(PexL, subPex, base < n ? base : n);
    const int64_t tile_end = base + TILE < n ? base + TILE : n;
    const int64_t ncell = pex_at(PexL, subPex, tile_end) - q_tile;  // cells started inside this tile
    const int64_t nnode = (tile_end - base) + ncell;                // the tile's nodes: one contiguous run of indices
    const int64_t idx0 = base + q_tile;                             // ... starting here
    const double bounds = info->bounds;
    const unsigned bandk = band_half_ulps(__longlong_as_double((long long)info->maxabs_bits), eps);
    // The tile's nodes are written in INDEX order, consecutive lanes = consecutive nodes (a wave's stores of the
    // 24 / 40 / 32-byte records then cover one contiguous stretch of each array; a thread per body / per cell wrote
    // every record into a different cache line: 2.3 TB/s of mostly partial-line traffic at 10 M bodies).  Which
    // (body, k) a node index belongs to comes from a table in LDS that the bodies fill, (2 * TILE) slots at a time:
    // local node slot of body i's k-th node (its cnt cells, then its leaf) = i + (pex(r) - q_tile) + k.
    for (int64_t c0 = 0; c0 < nnode; c0 += (2 * TILE)) {
        for (int i = t; i < TILE; i += kBlock) {
            const int64_t r = base + i;
            if (r >= n) break;
            const int d = (int)tree[TILE + i] - 1;
            const int dp = (int)(i > 0 ? tree[TILE + i - 1] : dprev) - 1;
            const int cnt = d > dp ? d - dp : 0;
            const int64_t s0 = i + (pex_at(PexL, subPex, r) - q_tile) - c0;
            for (int k = 0; k <= cnt; k++) {
                const int64_t c = s0 + k;
                if (c >= 0 && c < (2 * TILE)) cells[c] = ((uint32_t)i << 6) | (uint32_t)k;
            }
        }
        __syncthreads();
        const int64_t here = nnode - c0 < (2 * TILE) ? nnode - c0 : (2 * TILE);
        for (int64_t c = t; c < here; c += kBlock) {
            const uint32_t cl = cells[c];
            const int i = (int)(cl >> 6), k = (int)(cl & 63u);
            const int64_t r = base + i;
            const int64_t idx = idx0 + c0 + c;
            const int d = (int)tree[TILE + i] - 1;
            const int dp = (int)(i > 0 ? tree[TILE + i - 1] : dprev) - 1;
            const int cnt = d > dp ? d - dp : 0;
            if (k == cnt) {  // the body's leaf
                const float4 p = posm_s[r];
                Node lf;
                lf.cx = p.x; lf.cy = p.y; lf.cz = p.z; lf.gm = p.w;
                lf.s2t = 0.0f;
                lf.next_off = (unsigned)(idx + 1 + link_base) * kNodeBytes;
                nodes[idx] = lf;
                if (diag64) {  // the body as the float64 state has it
                    const uint32_t j = perm[r];
                    diag64[idx] = make_double4(cur.x[j], cur.y[j], cur.z[j], G * cur.m[j]);
                }
                if (nodesd) {  // the body as the float64 state has it (nearly sequential: the state is in last step's key order)
                    const uint32_t j = perm[r];
                    nodesd[idx] = NodeD{cur.x[j], cur.y[j], cur.z[j], G * cur.m[j], 0.0f, (unsigned)(idx + 1 + link_base) * kNodeDBytes};
                }
                if (node_ref) {  // queries and the owner-mode kernels only: a plain step does not pay for them
                    node_ref[idx] = (int32_t)r;
                    node_level[idx] = (uint8_t)((d > dp ? d : dp) + 1);
                }
                continue;
            }
            const int lev = dp + 1 + k;
            // first local index j >= i with delta[j] + 1 <= lev
            unsigned h = (unsigned)(TILE + i);
            bool found = false;
            for (;;) {
                if ((int)tree[h] <= lev) { found = true; break; }
                while ((h & 1u) && h > 1u) h >>= 1;
                if (h == 1u) break;
                h += 1u;
            }
            int64_t e;
            if (found) {
                while (h < (unsigned)TILE) {
                    h <<= 1;
                    if ((int)tree[h] > lev) h += 1u;
                }
                e = base + (int64_t)(h - (unsigned)TILE) + 1;
            } else {
                // the cell reaches beyond the tile: gallop + binary search on the sorted keys from the tile's end on
                // (lo_s == null, lean build: a low word matters only to a cell below level 21 and only where the upper
                // words agree; it is recomputed there)
                const uint64_t kh = hi_s[r];
                const bool deep = lev > 21;
                const uint64_t kl = lo_s ? lo_s[r] : (deep ? low_word_of(nullptr, cur, perm[r], hilbert, info) : 0ull);
                auto reaches = [&](int64_t u) {
                    const uint64_t hu = hi_s[u];
                    const uint64_t lu = lo_s ? lo_s[u] : (deep && hu == kh ? low_word_of(nullptr, cur, perm[u], hilbert, info) : 0ull);
                    return cpl_digits(kh, kl, hu, lu) >= lev;
                };
                int64_t ok = base + TILE - 1, bad, step = 1;
                for (;;) {
                    const int64_t u = ok + step;
                    if (u >= n) { bad = n; break; }
                    if (reaches(u)) { ok = u; step <<= 1; }
                    else { bad = u; break; }
                }
                while (bad - ok > 1) {
                    const int64_t mid = ok + ((bad - ok) >> 1);
                    if (reaches(mid)) ok = mid; else bad = mid;
                }
                e = bad;
            }
            double M, mx, my, mz;
            range_moments(S, T, r, e, M, mx, my, mz);
            double cx = 0.0, cy = 0.0, cz = 0.0;
            if (M > 0.0) { cx = mx / M; cy = my / M; cz = mz / M; }
            const double size = ldexp(bounds, 1 - lev);  // 2 * bounds / 2^lev, exact
            Node nd;
            nd.cx = (float)cx; nd.cy = (float)cy; nd.cz = (float)cz;
            nd.gm = (float)M;  // the moments are sums of G*m
            // upper edge of the uncertainty band: bits((2 hs)^2 / theta^2) + K  (theta == 0: +inf, never accepted)
            const float s2t = (float)(size * size * inv_theta2);
            nd.s2t = __int_as_float(__float_as_int(s2t) + (int)bandk);
            const int64_t nxt = e + pex_at(PexL, subPex, e) + link_base;
            nd.next_off = (unsigned)nxt * kNodeBytes;
            nodes[idx] = nd;
            // [r3] the float64 loop tests a correctly rounded d^2: its uncertainty band is 2 ulps on either side of the
            // threshold, not the K the fp32 loop needs for its rounded coordinates (re-decisions in float64 waves: 1 000 x fewer)
            if (nodesd) nodesd[idx] = NodeD{cx, cy, cz, M, __int_as_float(__float_as_int(s2t) + (int)kBand64), (unsigned)nxt * kNodeDBytes};
            nodes64[idx] = Node64{cx, cy, cz, ldexp(bounds, -lev)};
            if (diag64) diag64[idx] = make_double4(cx, cy, cz, M);
            if (node_ref) {
                node_ref[idx] = (int32_t)r;
                node_level[idx] = (uint8_t)lev;
            }
        }
        __syncthreads();
    }
}

// deepest leaf level = max(delta) + 1; only run when nbmi_tree_stats() asks (same-address
// atomics cost ~11 ns each: one per block here, never in the per-step path)
__global__ __launch_bounds__(kBlock) void k_max_level(const int32_t *__restrict__ delta, int64_t n, TreeInfo *info) {
    __shared__ int red[kBlock / 64];
    int m = -1;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int d = delta[i];
        m = d > m ? d : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(m, o);
        m = other > m ? other : m;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; w++) m = red[w] > m ? red[w] : m;
        atomicMax(&info->max_level, m + 1);
    }
}

// ---------------------------------------------------------------------------------------
// K9: the walk.  One wave64 = 64 consecutive sorted bodies; wave-uniform cursor over the
// pre-order node array (scalar loads of the 24-byte record); per lane the reference's test
// (simulation.py:245-274):
//     d = com - p; dist_sq = |d|^2 + eps^2;
//     accept if leaf or 2 hs / dist < theta          [== (2hs)^2/theta^2 < dist_sq; leaves carry 0]
//     accepted && mass>0 && dist_sq > eps^2  ->  a += G m d / dist^3
// The reference's explicit "skip my own leaf" needs no instruction here: the own leaf has d = 0
// exactly, so its term is 0 (eps > 0) or fails the dist_sq > eps^2 guard (kGuard, eps == 0).
// `resume` = first node index at which the lane takes part again (it accepted an ancestor of
// everything before that).  The cursor moves to the next node in memory if any lane opens the node, else to
// next_off.  Fused epilogue: v = (v + a dt) * damping; x += v dt  (simulation.py:291-305),
// written at the body's NEW sorted rank (state re-ordering is fused into this kernel).
//
// Opening-test ties.  The test runs in fp32 on fp32-rounded positions, the reference's in float64; a
// (body, node) pair whose d^2 lies within the rounding error of the threshold can be decided the other
// way, and such a body then carries a different (equally legitimate) Barnes-Hut approximation - enough
// to miss the 1e-4 position bound after 100 steps at 1 M bodies.  So the node stores the UPPER edge of
// an uncertainty band, bits(s2t) + K, the walk derives the lower edge bits(s2t) - K, and a lane whose
// d^2 falls between the two is re-decided exactly as the reference does it (simulation.py:252-258):
// float64 body position, float64 centre of mass (double-double prefix sums, see k_scan_*), sqrt and
// divide.  K (ulps of d^2) bounds the fp32 error: both positions are rounded by <= 2^-24 maxabs, so
// d^2 is off by <= 2 sqrt(3) d 2^-23 maxabs + a few ulps, i.e. by <= 6.93 maxabs / d + 4 ulps (one ulp
// is >= 2^-24 of d^2); the test only matters where d >= eps (smaller cells pass it through eps^2
// alone), hence K = 8 + 7 maxabs / eps (TreeInfo.band2 = 2 K; 6.5 k ulps = 4e-4 ... 8e-4 of d^2 for the
// 1 M-body galaxy).  One extra compare per visit; the float64 path runs for ~1.5e-4 of the lane visits.
// ---------------------------------------------------------------------------------------
struct WalkParams {
    int64_t rank_begin, rank_end;  // shard of sorted ranks handled by this launch

    float eps2;
    int xcd_chunk;  // see logical_block()
    int balance;    // 1: blocks are dealt to the XCDs by last step's measured times (WalkTable::xcd_bounds)
    int pair;       // one-wave walk with two cursors (the two halves of the array)
    double dt, damping;
    int curbuf;  // which of WalkTable.buf holds the current state
    int force_prec;  // 0 = per wave by local density (see k_walk), 1 = fp32 pair forces everywhere, 2 = float64 everywhere
    float prec_tau;  // force_prec 0: a wave takes float64 when G rho dt^2 of its bodies exceeds this
};

// Per-handle constants the walk needs only rarely (float64 re-decision) or only at its end (the state
// pointers of the fused kick-drift).  They live in device memory, not in kernel arguments: arguments sit
// in SGPRs for the whole kernel, and with 16 state pointers among them the walk needed 92 SGPRs - over
// the 80 at which the hardware still admits eight 256-thread blocks per CU.
struct WalkTable {
    Bodies buf[2];
    const Node64 *n64;
    const NodeD *nodesd;  // float64 node records (null: the handle computes every force in fp32)
    const int *xcd_bounds;   // [9] logical walk blocks [b[x], b[x + 1]) belong to XCD x (balance mode)
    unsigned *wave_cycles;   // [4 per logical block] how long each wave of the last walk took (shader clocks)
    unsigned char *wave_flag;  // [one per wave] 1 = the wave's own density asked for float64 forces (auto mode)
    const int32_t *pex, *subpex;  // leaf of the body at sorted rank r = node r + pex_at(pex, subpex, r + 1)
    unsigned long long *maxabs_next;  // TreeInfo::maxabs_next
    double theta, eps2;
    long long own_base;  // owner mode: row of the walk array at which the handle's own tree begins (0 otherwise)
    // [leapfrog] which epilogue the integrating walks run: 0 = the reference's kick-drift, kLeapClose / kLeapPrime (see
    // leap_epilogue).  The handle keeps one table per value (nbmi_sim::wtab[3]) and passes the one it wants: no kernel
    // argument, no upload per step.
    int leap;
    double *ax, *ay, *az;  // acceleration columns beside the rows of the current state (leapfrog; null before its first step)
};
constexpr int kLeapClose = 1;  // closing half-kick, state and a written at the body's new rank of the other buffer
constexpr int kLeapPrime = 2;  // a = F(x) written beside the body's row of the current buffer, state untouched

// where a lane finds its body's float64 position (only read on the re-decision path)
struct Body64 {
    const WalkTable *tab;
    int curbuf;
    uint32_t j;
};

// the reference's own test in float64 (simulation.py:249-258), operation for operation
__device__ __forceinline__ bool exact_take_idx(unsigned idx, const Body64 &b) {
    const WalkTable *t = b.tab;
    // (Measured and dropped [r3]: taking the centre of mass from the NodeD row and the half size from bounds / 2^level,
    // so that Node64 need not be written - 0.1 ms less build at 10 M bodies, but the walk lost 0.5 ms: a wave leaves the
    // loop for ~12 re-decisions per walk and each one waits for this function's dependent loads; one more level of them
    // is 4 % of the walk.)
    const Node64 c = t->n64[idx];
    const Bodies &cur = t->buf[b.curbuf];
    const double dx = c.cx - cur.x[b.j], dy = c.cy - cur.y[b.j], dz = c.cz - cur.z[b.j];
    const double dist_sq = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)), t->eps2);
    const double dist = sqrt(dist_sq);
    return (c.hs * 2.0) / dist < t->theta;
}

// THE opening decision: every walk, of whatever arithmetic and stride, asks it here, so the force, quadrupole and
// potential walks accept the same (body, node) sets and a visit decides alike in the hand-scheduled loops' C++ twins.
// `d2` is the fp32 dist_sq (the float64 walks pass their (float)d2), `s2t` the record's threshold (0: a leaf, always
// taken).  Non-negative floats compare as integers; hi / lo are the edges of the uncertainty band, `band2` ulps wide.
// A lane inside the band (or one the caller names in `also`: field_walk's near pairs) that takes part in the
// visit is re-decided in float64 - rare, divergent.  geom: the lane takes node `idx` if it takes part.
struct Opening {
    bool geom, band;
};
__device__ __forceinline__ Opening opening(float d2, float s2t, unsigned band2, bool active, unsigned idx, const Body64 &b64,
                                           bool also = false) {
    const int d2b = __float_as_int(d2), hi = __float_as_int(s2t), lo = hi - (int)band2;
    bool geom = hi < d2b;
    const bool band = active && ((!geom && lo < d2b) || also);
    if (band) geom = (hi == 0) || exact_take_idx(idx, b64);
    return Opening{geom, band};
}
// What follows the decision in the lock-step walks: a lane that takes the node skips its subtree (resume), and the
// wave's cursor steps into the subtree if any lane opens it, past it otherwise.  kStride: kNodeBytes / kNodeDBytes.
template <unsigned kStride>
__device__ __forceinline__ unsigned advance(bool active, bool geom, unsigned off, unsigned next_off, unsigned &resume, bool &take) {
    take = active && geom;
    resume = take ? next_off : resume;
    const unsigned long long any_open = __builtin_amdgcn_ballot_w64(active && !geom);
    return any_open ? off + kStride : next_off;
}

// One node visit (C++ form: counted / eps == 0 kernels, seek(), and the product walk's re-decision visits).
// `off` is the cursor as a byte offset into the node array; `resume` likewise.  Returns the next cursor.
template <bool kGuard>
__device__ __forceinline__ unsigned visit(const Node *__restrict__ nodes, unsigned off,
                                          float px, float py, float pz, const Body64 &b64, const WalkParams &P,
                                          unsigned band2, unsigned &resume, float &ax, float &ay, float &az,
                                          bool &active_out, bool &force_out, bool &jumped, bool &band_out) {
    off = __builtin_amdgcn_readfirstlane(off);
    const Node nd = *reinterpret_cast<const Node *>(reinterpret_cast<const char *>(nodes) + off);
    const float dx = nd.cx - px, dy = nd.cy - py, dz = nd.cz - pz;
    const float dist_sq = fmaf(dz, dz, fmaf(dy, dy, fmaf(dx, dx, P.eps2)));
    const bool active = resume <= off;
    const Opening o = opening(dist_sq, nd.s2t, band2, active, off / kNodeBytes, b64);
    bool take;
    const unsigned next = advance<kNodeBytes>(active, o.geom, off, nd.next_off, resume, take);
    bool force = take;
    if (kGuard) force = take && (dist_sq > P.eps2);
    // same association as the hand-scheduled loop, (G m / d) (1 / d^2): a body's sums must not depend on
    // which of its visits went through this C++ form (that depends on the other bodies of its wave)
    const float inv = __builtin_amdgcn_rsqf(dist_sq);
    const float f = force ? (nd.gm * inv) * (inv * inv) : 0.f;
    ax = fmaf(dx, f, ax);
    ay = fmaf(dy, f, ay);
    az = fmaf(dz, f, az);
    active_out = active;
    force_out = take && (dist_sq > P.eps2);
    band_out = o.band;
    jumped = next != off + kNodeBytes;
    return next;
}

// Hand-scheduled walk loop for the product kernel (eps > 0, no counters): 16 VALU + 3 SALU + 2 SMEM
// instructions on a visit nobody opens (80 % of them).  s_load_dwordx4 + s_load_dwordx2 at an SGPR byte offset.
// The two deciding compares are v_cmpx: EXEC narrows to the lanes that take part in the visit, then to those
// that TAKE the node, so the force instructions and the `resume` update need no per-lane selects; s_andn2 of
// the two masks leaves "some lane opens" in SCC.  Nobody opens: the cursor follows next_off.  Somebody opens
// (20 % of the visits): a branch to an out-of-line block behind the loop (NBMI_OPEN_X), which holds everything
// only such a visit needs - the near-tie check (only an opener can lie inside the uncertainty band: one v_cmp
// of the openers against the lower band edge s2t - band2; a hit leaves the loop BEFORE the visit has changed
// anything - cursor, resume, sums - the caller performs that one visit in C++ with the float64 test and
// re-enters) and the step to the next node in memory - and comes back.  (Measured: walk 1.071 -> 1.053 ms at
// 1 M, 10.23 -> 10.06 ms at 10 M against the check on every visit.)  EXEC is all-ones again before the next
// visit (every launched wave is full; lanes without a body carry resume = ~0 and never take part).  The node
// record of the NEXT visit is requested as soon as its offset is known - before the nine force instructions of
// the current visit are issued - into the other of two SGPR banks (A = s[36:41], B = s[48:53]: cx cy cz gm s2t
// next_off), which takes those instructions' issue time out of the per-wave dependent chain.  The whole loop
// is one asm statement (4 visits per trip, banks A B A B) so that no compiler-generated code runs while a load
// is in flight; a self-looping sentinel node after the last one makes overshooting harmless.
#define NBMI_VISIT_X(OFF, RES, ACC, WAIT, CX, CY, CZ, GM, S2T, NXT, NEXTLO, NEXTHI, LOPEN, LJOIN, LSKIP) \
    "v_cmpx_ge_u32_e64 s[44:45], " OFF ", " RES "\n"           \
    WAIT                                                       \
    "v_sub_f32_e32 %[dx], " CX ", %[px]\n"                     \
    "v_sub_f32_e32 %[dy], " CY ", %[py]\n"                     \
    "v_sub_f32_e32 %[dz], " CZ ", %[pz]\n"                     \
    "v_fma_f32 %[d2], %[dx], %[dx], %[eps2]\n"                 \
    "v_fmac_f32_e32 %[d2], %[dy], %[dy]\n"                     \
    "v_fmac_f32_e32 %[d2], %[dz], %[dz]\n"                     \
    "v_cmpx_lt_i32_e64 s[46:47], " S2T ", %[d2]\n"             \
    "s_andn2_b64 s[56:57], s[44:45], s[46:47]\n"               \
    "s_cbranch_scc1 " LOPEN "f\n"                              \
    "s_mov_b32 " OFF ", " NXT "\n"                             \
    LJOIN ":\n"                                                \
    "s_load_dwordx4 " NEXTLO ", %[base], " OFF "\n"            \
    "s_load_dwordx2 " NEXTHI ", %[base], " OFF " offset:16\n"  \
    "v_rsq_f32_e32 %[inv], %[d2]\n"                            \
    "v_mov_b32_e32 " RES ", " NXT "\n"                         \
    "v_mul_f32_e32 %[f], " GM ", %[inv]\n"                     \
    "v_mul_f32_e32 %[t], %[inv], %[inv]\n"                     \
    "v_mul_f32_e32 %[f], %[f], %[t]\n"                         \
    "v_fmac_f32_e32 %[ax" ACC "], %[dx], %[f]\n"               \
    "v_fmac_f32_e32 %[ay" ACC "], %[dy], %[f]\n"               \
    "v_fmac_f32_e32 %[az" ACC "], %[dz], %[f]\n"               \
    "s_mov_b64 exec, -1\n"                                    \
    LSKIP ":\n"
// the out-of-line half of a visit that some lane opens (s[56:57] = openers, s[46:47] = takers; 20 % of the visits):
// only an opener can lie inside the uncertainty band, so the near-tie check lives here - one v_cmp of the openers
// against the lower band edge; a hit leaves the loop BEFORE the visit has changed anything, otherwise the cursor
// moves to the next node in memory and the visit goes on
#define NBMI_OPEN_X(OFF, S2T, NEXTLO, NEXTHI, LOPEN, LJOIN, LSKIP, EXITL)   \
    LOPEN ":\n"                                      \
    "s_sub_u32 s54, " S2T ", %[band2]\n"             \
    "s_mov_b64 exec, s[56:57]\n"                     \
    "v_cmp_lt_i32_e64 s[42:43], s54, %[d2]\n"        \
    "s_mov_b64 exec, s[46:47]\n"                     \
    "s_cmp_lg_u64 s[42:43], 0\n"                     \
    "s_cbranch_scc1 " EXITL "\n"                     \
    "s_add_u32 " OFF ", " OFF ", 24\n"               \
    "s_cmp_lg_u64 s[46:47], 0\n"                     \
    "s_cbranch_scc1 " LJOIN "b\n"                    \
    /* [r3] nobody takes the node (every lane that takes part opens it): request the next record and skip the */ \
    /* eight force instructions */                   \
    "s_load_dwordx4 " NEXTLO ", %[base], " OFF "\n"  \
    "s_load_dwordx2 " NEXTHI ", %[base], " OFF " offset:16\n" \
    "s_mov_b64 exec, -1\n"                           \
    "s_branch " LSKIP "b\n"
#define NBMI_WAIT "s_waitcnt lgkmcnt(0)\n"
#define NBMI_VISIT_A(LO, LJ, LS) \
    NBMI_VISIT_X("%[off]", "%[resume]", "", NBMI_WAIT, "s36", "s37", "s38", "s39", "s40", "s41", "s[48:51]", "s[52:53]", LO, LJ, LS)
#define NBMI_VISIT_B(LO, LJ, LS) \
    NBMI_VISIT_X("%[off]", "%[resume]", "", NBMI_WAIT, "s48", "s49", "s50", "s51", "s52", "s53", "s[36:39]", "s[40:41]", LO, LJ, LS)
#define NBMI_OPEN_A(LO, LJ, LS) NBMI_OPEN_X("%[off]", "s40", "s[48:51]", "s[52:53]", LO, LJ, LS, "7f")
#define NBMI_OPEN_B(LO, LJ, LS) NBMI_OPEN_X("%[off]", "s52", "s[36:39]", "s[40:41]", LO, LJ, LS, "7f")
// two cursors in one wave (walk_pair_asm): cursor 1 uses banks s[36:41] / s[48:53], cursor 2 uses
// s[60:65] / s[68:73]; the trip waits ONCE for both cursors' records
#define NBMI_VISIT_1A NBMI_VISIT_A
#define NBMI_VISIT_1B NBMI_VISIT_B
#define NBMI_VISIT_2A(LO, LJ, LS) \
    NBMI_VISIT_X("%[off2]", "%[resume2]", "2", "", "s60", "s61", "s62", "s63", "s64", "s65", "s[68:71]", "s[72:73]", LO, LJ, LS)
#define NBMI_VISIT_2B(LO, LJ, LS) \
    NBMI_VISIT_X("%[off2]", "%[resume2]", "2", "", "s68", "s69", "s70", "s71", "s72", "s73", "s[60:63]", "s[64:65]", LO, LJ, LS)
#define NBMI_OPEN_2A(LO, LJ, LS) NBMI_OPEN_X("%[off2]", "s64", "s[68:71]", "s[72:73]", LO, LJ, LS, "8f")
#define NBMI_OPEN_2B(LO, LJ, LS) NBMI_OPEN_X("%[off2]", "s72", "s[60:63]", "s[64:65]", LO, LJ, LS, "8f")
// Two-level sums: the loops add into fp32 accumulators (one instruction per component and visit); every few
// trips those are emptied into float64 sums (NBMI_FLUSH: convert, add, clear), so an fp32 running sum never grows
// beyond a dozen terms.  Measured at 1 M bodies against the float64 oracle, per-body relative acceleration error:
// fp32 running sums over the whole walk rms 5.4e-7 (median 4.1e-7), every contribution summed in float64 1.1e-7
// (5.4e-8) - the running sums were four fifths of the error.  The flush blocks sit behind the loops (reached by a
// branch once per NBMI_FLUSH_TRIPS trips).
#define NBMI_FLUSH(AX, AY, AZ)                      \
    "v_cvt_f64_f32_e32 %[t64], " AX "\n"            \
    "v_add_f64 %[sx], %[sx], %[t64]\n"              \
    "v_mov_b32_e32 " AX ", 0\n"                     \
    "v_cvt_f64_f32_e32 %[t64], " AY "\n"            \
    "v_add_f64 %[sy], %[sy], %[t64]\n"              \
    "v_mov_b32_e32 " AY ", 0\n"                     \
    "v_cvt_f64_f32_e32 %[t64], " AZ "\n"            \
    "v_add_f64 %[sz], %[sz], %[t64]\n"              \
    "v_mov_b32_e32 " AZ ", 0\n"
// at the loop-back point: count the trip down; on underflow empty the accumulators (label 40, returns to 41)
#define NBMI_TRIP_COUNT                 \
    "s_sub_u32 %[cnt], %[cnt], 1\n"     \
    "s_cbranch_scc1 40f\n"              \
    "41:\n"
#define NBMI_EXITS(OPENS, FLUSHES, TRIPS) \
    "s_branch 9f\n" OPENS               \
    "40:\n" FLUSHES                     \
    "s_mov_b32 %[cnt], " TRIPS "\n"     \
    "s_branch 41b\n"                    \
    "7:\n"                              \
    "s_mov_b64 exec, -1\n"              \
    "s_mov_b32 %[which], 1\n"           \
    "s_branch 9f\n"                     \
    "8:\n"                              \
    "s_mov_b64 exec, -1\n"              \
    "s_mov_b32 %[which], 2\n"           \
    "9:\n"                              \
    "s_waitcnt lgkmcnt(0)\n"
#define NBMI_CLOBBERS                                                                                               \
    "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50", "s51", \
        "s52", "s53", "s54", "s55", "s56", "s57", "s58", "vcc", "scc", "memory"

// walks from `off` until the cursor reaches `end` (the end of the array: 4 visits per loop test, the
// sentinel absorbs the overshoot) or a near-tie stops it (which = 1, cursor on the tied node)
__device__ __forceinline__ void walk4_asm(const Node *nodes, unsigned &off, unsigned end, float px, float py, float pz,
                                          float eps2, unsigned band2, unsigned &resume, float &ax, float &ay, float &az,
                                          double &sx, double &sy, double &sz, unsigned &which) {
    float dx, dy, dz, d2, inv, f, t;
    double t64;
    unsigned cnt;
    asm volatile("s_mov_b32 %[cnt], 3\n"
                 "s_load_dwordx4 s[36:39], %[base], %[off]\n"
                 "s_load_dwordx2 s[40:41], %[base], %[off] offset:16\n"
                 "1:\n" NBMI_VISIT_A("21", "31", "51") NBMI_VISIT_B("22", "32", "52") NBMI_VISIT_A("23", "33", "53") NBMI_VISIT_B("24", "34", "54") NBMI_TRIP_COUNT
                 "s_cmp_lt_u32 %[off], %[end]\n"
                 "s_cbranch_scc1 1b\n"
                 NBMI_EXITS(NBMI_OPEN_A("21", "31", "51") NBMI_OPEN_B("22", "32", "52") NBMI_OPEN_A("23", "33", "53") NBMI_OPEN_B("24", "34", "54"),
                            NBMI_FLUSH("%[ax]", "%[ay]", "%[az]"), "3")
                 : [off] "+s"(off), [which] "+s"(which), [resume] "+v"(resume), [ax] "+v"(ax), [ay] "+v"(ay),
                   [az] "+v"(az), [sx] "+v"(sx), [sy] "+v"(sy), [sz] "+v"(sz), [t64] "=&v"(t64), [cnt] "=&s"(cnt),
                   [dx] "=&v"(dx), [dy] "=&v"(dy), [dz] "=&v"(dz), [d2] "=&v"(d2), [inv] "=&v"(inv),
                   [f] "=&v"(f), [t] "=&v"(t)
                 : [base] "s"(nodes), [px] "v"(px), [py] "v"(py), [pz] "v"(pz), [eps2] "s"(eps2), [end] "s"(end),
                   [band2] "s"(band2)
                 : NBMI_CLOBBERS);
}

// one visit per loop test: a part must not step past its end (the next part starts there)
__device__ __forceinline__ void walk1_asm(const Node *nodes, unsigned &off, unsigned end, float px, float py, float pz,
                                          float eps2, unsigned band2, unsigned &resume, float &ax, float &ay, float &az,
                                          double &sx, double &sy, double &sz, unsigned &which) {
    float dx, dy, dz, d2, inv, f, t;
    double t64;
    unsigned cnt;
    asm volatile("s_mov_b32 %[cnt], 7\n"
                 "s_load_dwordx4 s[36:39], %[base], %[off]\n"
                 "s_load_dwordx2 s[40:41], %[base], %[off] offset:16\n"
                 "1:\n" NBMI_VISIT_A("21", "31", "51")
                 "s_cmp_lt_u32 %[off], %[end]\n"
                 "s_cbranch_scc0 9f\n" NBMI_VISIT_B("22", "32", "52") NBMI_TRIP_COUNT
                 "s_cmp_lt_u32 %[off], %[end]\n"
                 "s_cbranch_scc1 1b\n"
                 NBMI_EXITS(NBMI_OPEN_A("21", "31", "51") NBMI_OPEN_B("22", "32", "52"), NBMI_FLUSH("%[ax]", "%[ay]", "%[az]"), "7")
                 : [off] "+s"(off), [which] "+s"(which), [resume] "+v"(resume), [ax] "+v"(ax), [ay] "+v"(ay),
                   [az] "+v"(az), [sx] "+v"(sx), [sy] "+v"(sy), [sz] "+v"(sz), [t64] "=&v"(t64), [cnt] "=&s"(cnt),
                   [dx] "=&v"(dx), [dy] "=&v"(dy), [dz] "=&v"(dz), [d2] "=&v"(d2), [inv] "=&v"(inv),
                   [f] "=&v"(f), [t] "=&v"(t)
                 : [base] "s"(nodes), [px] "v"(px), [py] "v"(py), [pz] "v"(pz), [eps2] "s"(eps2), [end] "s"(end),
                   [band2] "s"(band2)
                 : NBMI_CLOBBERS);
}

// Two cursors in one wave: the same 64 bodies walk [off1, end1) and [off2, end2) of the array at
// once, one visit of each per trip.  A wave issues in order and a scalar load can only be awaited with
// lgkmcnt(0), so the trip waits once, for both records, and both cursors' next loads are in flight
// while the other cursor's instructions issue: two dependent load chains per wave instead of one.
// Runs while BOTH cursors are inside their ranges: the first is checked after every trip (it must not
// step into the second's range), the second after every other trip (its range ends with the
// self-looping sentinel, one idle visit at worst); the caller finishes the longer one alone.
__device__ __forceinline__ void walk_pair_asm(const Node *nodes, unsigned &off1, unsigned end1, unsigned &off2,
                                              unsigned end2, float px, float py, float pz, float eps2, unsigned band2,
                                              unsigned &resume1, unsigned &resume2, float &ax, float &ay, float &az,
                                              float &ax2, float &ay2, float &az2, double &sx, double &sy, double &sz,
                                              unsigned &which) {
    float dx, dy, dz, d2, inv, f, t;
    double t64;
    unsigned cnt;
    asm volatile("s_mov_b32 %[cnt], 3\n"
                 "s_load_dwordx4 s[36:39], %[base], %[off]\n"
                 "s_load_dwordx2 s[40:41], %[base], %[off] offset:16\n"
                 "s_load_dwordx4 s[60:63], %[base], %[off2]\n"
                 "s_load_dwordx2 s[64:65], %[base], %[off2] offset:16\n"
                 "1:\n" NBMI_VISIT_1A("21", "31", "51") NBMI_VISIT_2A("22", "32", "52")
                 "s_cmp_lt_u32 %[off], %[end]\n"
                 "s_cbranch_scc0 9f\n" NBMI_VISIT_1B("23", "33", "53") NBMI_VISIT_2B("24", "34", "54")
                 "s_cmp_lt_u32 %[off], %[end]\n"
                 "s_cbranch_scc0 9f\n" NBMI_TRIP_COUNT
                 "s_cmp_lt_u32 %[off2], %[end2]\n"
                 "s_cbranch_scc1 1b\n"
                 NBMI_EXITS(NBMI_OPEN_A("21", "31", "51") NBMI_OPEN_2A("22", "32", "52") NBMI_OPEN_B("23", "33", "53") NBMI_OPEN_2B("24", "34", "54"),
                            NBMI_FLUSH("%[ax]", "%[ay]", "%[az]") NBMI_FLUSH("%[ax2]", "%[ay2]", "%[az2]"), "3")
                 : [off] "+s"(off1), [off2] "+s"(off2), [which] "+s"(which), [resume] "+v"(resume1),
                   [resume2] "+v"(resume2), [ax] "+v"(ax), [ay] "+v"(ay), [az] "+v"(az), [ax2] "+v"(ax2),
                   [ay2] "+v"(ay2), [az2] "+v"(az2), [sx] "+v"(sx), [sy] "+v"(sy), [sz] "+v"(sz), [t64] "=&v"(t64),
                   [cnt] "=&s"(cnt), [dx] "=&v"(dx), [dy] "=&v"(dy), [dz] "=&v"(dz), [d2] "=&v"(d2),
                   [inv] "=&v"(inv), [f] "=&v"(f), [t] "=&v"(t)
                 : [base] "s"(nodes), [px] "v"(px), [py] "v"(py), [pz] "v"(pz), [eps2] "s"(eps2), [end] "s"(end1),
                   [end2] "s"(end2), [band2] "s"(band2)
                 : NBMI_CLOBBERS, "s60", "s61", "s62", "s63", "s64", "s65", "s68", "s69", "s70", "s71", "s72", "s73");
}

// ---------------------------------------------------------------------------------------
// [r3] The float64 visit.  Why it exists (scripts/experiments/walk_prec_modes.patch, profiles/r03_precision/): at 1 M
// bodies x 100 steps the position error against the float64 reference is made by fp32 pair arithmetic, and not by
// its random roundings but by its SYSTEMATIC ones - G m rounded to fp32 (alone: max 6.6e-5 of the largest
// coordinate), v_rsq_f32's one-ulp error pattern (alone: 9.5e-5), fp32-rounded coordinates of near pairs - which act
// like a slightly different force law step after step on the bodies of the dense inner disk, where a difference,
// once it flips an opening decision, cascades.  With the force of every accepted visit in float64 (same accepted
// sets) the GPU follows the reference to 3e-14 over the 100 steps.  Same lock-step scheme as the fp32 loop, operands
// of the 40-byte NodeD record in SGPR pairs:
//   d = c - p, d2 = |d|^2 + eps^2 in float64;  the opening test on fp32(d2) against the same s2t / band as the fp32
//   loop (fp32(d2) is within half an ulp of the true value: well inside what the band allows for, so the accepted
//   sets are the reference's here too);  y0 = v_rsq_f32(fp32(d2)), e = 1 - d2 y0^2 (one FMA, exact to 1e-16),
//   G m d2^(-3/2) = G m y0^3 (1 + 1.5 e) [+ O(e^2) = 1e-14];  three float64 FMAs into the sums.
// 17 float64-rate + 4 fp32-rate vector instructions per visit (the fp32 visit: 16 fp32-rate).
// ---------------------------------------------------------------------------------------
#define NBMI_V64_X(CX, CY, CZ, GM, S2T, NXT, NEXT8, NEXT2, LOPEN, LJOIN, LSKIP) \
    "v_cmpx_ge_u32_e64 s[58:59], %[off], %[resume]\n"          \
    "s_waitcnt lgkmcnt(0)\n"                                   \
    "v_add_f64 %[dx], " CX ", -%[px]\n"                        \
    "v_add_f64 %[dy], " CY ", -%[py]\n"                        \
    "v_add_f64 %[dz], " CZ ", -%[pz]\n"                        \
    "v_fma_f64 %[d2], %[dx], %[dx], %[eps2]\n"                 \
    "v_fma_f64 %[d2], %[dy], %[dy], %[d2]\n"                   \
    "v_fma_f64 %[d2], %[dz], %[dz], %[d2]\n"                   \
    "v_cvt_f32_f64_e32 %[d2f], %[d2]\n"                        \
    "v_cmpx_lt_i32_e64 s[60:61], " S2T ", %[d2f]\n"            \
    "s_andn2_b64 s[62:63], s[58:59], s[60:61]\n"               \
    "s_cbranch_scc1 " LOPEN "f\n"                              \
    "s_mov_b32 %[off], " NXT "\n"                              \
    LJOIN ":\n"                                                \
    "s_load_dwordx8 " NEXT8 ", %[base], %[off]\n"              \
    "s_load_dwordx2 " NEXT2 ", %[base], %[off] offset:32\n"    \
    "v_rsq_f32_e32 %[d2f], %[d2f]\n"                           \
    "v_mov_b32_e32 %[resume], " NXT "\n"                       \
    "v_cvt_f64_f32_e32 %[y0], %[d2f]\n"                        \
    "v_mul_f64 %[t], %[y0], %[y0]\n"                           \
    "v_mul_f64 %[w], " GM ", %[y0]\n"                          \
    "v_fma_f64 %[d2], -%[d2], %[t], 1.0\n"                     \
    "v_mul_f64 %[w], %[w], %[t]\n"                             \
    "v_mul_f64 %[d2], %[d2], %[c15]\n"                         \
    "v_fma_f64 %[w], %[w], %[d2], %[w]\n"                      \
    "v_fma_f64 %[sx], %[dx], %[w], %[sx]\n"                    \
    "v_fma_f64 %[sy], %[dy], %[w], %[sy]\n"                    \
    "v_fma_f64 %[sz], %[dz], %[w], %[sz]\n"                    \
    "s_mov_b64 exec, -1\n"                                    \
    LSKIP ":\n"
#define NBMI_O64_X(S2T, NEXT8, NEXT2, LOPEN, LJOIN, LSKIP) \
    LOPEN ":\n"                                      \
    "s_sub_u32 s66, " S2T ", %[band2]\n"             \
    "s_mov_b64 exec, s[62:63]\n"                     \
    "v_cmp_lt_i32_e64 s[64:65], s66, %[d2f]\n"       \
    "s_mov_b64 exec, s[60:61]\n"                     \
    "s_cmp_lg_u64 s[64:65], 0\n"                     \
    "s_cbranch_scc1 7f\n"                            \
    "s_add_u32 %[off], %[off], 40\n"                 \
    "s_cmp_lg_u64 s[60:61], 0\n"                     \
    "s_cbranch_scc1 " LJOIN "b\n"                    \
    /* nobody takes the node: request the next record, skip the force block */ \
    "s_load_dwordx8 " NEXT8 ", %[base], %[off]\n"    \
    "s_load_dwordx2 " NEXT2 ", %[base], %[off] offset:32\n" \
    "s_mov_b64 exec, -1\n"                           \
    "s_branch " LSKIP "b\n"
#define NBMI_V64_A(LO, LJ, LS) \
    NBMI_V64_X("s[36:37]", "s[38:39]", "s[40:41]", "s[42:43]", "s44", "s45", "s[48:55]", "s[56:57]", LO, LJ, LS)
#define NBMI_V64_B(LO, LJ, LS) \
    NBMI_V64_X("s[48:49]", "s[50:51]", "s[52:53]", "s[54:55]", "s56", "s57", "s[36:43]", "s[44:45]", LO, LJ, LS)
#define NBMI_O64_A(LO, LJ, LS) NBMI_O64_X("s44", "s[48:55]", "s[56:57]", LO, LJ, LS)
#define NBMI_O64_B(LO, LJ, LS) NBMI_O64_X("s56", "s[36:43]", "s[44:45]", LO, LJ, LS)

// walks from `off` to the end of the NodeD array (4 visits per loop test, the sentinel absorbs the overshoot) or
// until a near-tie stops it (which = 1, cursor on the tied node)
__device__ __forceinline__ void walk4_asm64(const NodeD *nodesd, unsigned &off, unsigned end, double px, double py,
                                            double pz, double eps2, unsigned band2, unsigned &resume, double &sx,
                                            double &sy, double &sz, unsigned &which) {
    double dx, dy, dz, d2, y0, t, w;
    float d2f;
    const double c15 = 1.5;
    asm volatile("s_load_dwordx8 s[36:43], %[base], %[off]\n"
                 "s_load_dwordx2 s[44:45], %[base], %[off] offset:32\n"
                 "1:\n" NBMI_V64_A("21", "31", "51") NBMI_V64_B("22", "32", "52") NBMI_V64_A("23", "33", "53") NBMI_V64_B("24", "34", "54")
                 "s_cmp_lt_u32 %[off], %[end]\n"
                 "s_cbranch_scc1 1b\n"
                 "s_branch 9f\n"
                 NBMI_O64_A("21", "31", "51") NBMI_O64_B("22", "32", "52") NBMI_O64_A("23", "33", "53") NBMI_O64_B("24", "34", "54")
                 "7:\n"
                 "s_mov_b64 exec, -1\n"
                 "s_mov_b32 %[which], 1\n"
                 "9:\n"
                 "s_waitcnt lgkmcnt(0)\n"
                 : [off] "+s"(off), [which] "+s"(which), [resume] "+v"(resume), [sx] "+v"(sx), [sy] "+v"(sy), [sz] "+v"(sz),
                   [dx] "=&v"(dx), [dy] "=&v"(dy), [dz] "=&v"(dz), [d2] "=&v"(d2), [y0] "=&v"(y0), [t] "=&v"(t),
                   [w] "=&v"(w), [d2f] "=&v"(d2f)
                 : [base] "s"(nodesd), [px] "v"(px), [py] "v"(py), [pz] "v"(pz), [eps2] "s"(eps2), [c15] "s"(c15),
                   [end] "s"(end), [band2] "s"(band2)
                 : "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50",
                   "s51", "s52", "s53", "s54", "s55", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65",
                   "s66", "vcc", "scc", "memory");
}

// the same with one visit per loop test: a part of the array must not be stepped past (split walk)
__device__ __forceinline__ void walk1_asm64(const NodeD *nodesd, unsigned &off, unsigned end, double px, double py,
                                            double pz, double eps2, unsigned band2, unsigned &resume, double &sx,
                                            double &sy, double &sz, unsigned &which) {
    double dx, dy, dz, d2, y0, t, w;
    float d2f;
    const double c15 = 1.5;
    asm volatile("s_load_dwordx8 s[36:43], %[base], %[off]\n"
                 "s_load_dwordx2 s[44:45], %[base], %[off] offset:32\n"
                 "1:\n" NBMI_V64_A("21", "31", "51")
                 "s_cmp_lt_u32 %[off], %[end]\n"
                 "s_cbranch_scc0 9f\n" NBMI_V64_B("22", "32", "52")
                 "s_cmp_lt_u32 %[off], %[end]\n"
                 "s_cbranch_scc1 1b\n"
                 "s_branch 9f\n"
                 NBMI_O64_A("21", "31", "51") NBMI_O64_B("22", "32", "52")
                 "7:\n"
                 "s_mov_b64 exec, -1\n"
                 "s_mov_b32 %[which], 1\n"
                 "9:\n"
                 "s_waitcnt lgkmcnt(0)\n"
                 : [off] "+s"(off), [which] "+s"(which), [resume] "+v"(resume), [sx] "+v"(sx), [sy] "+v"(sy), [sz] "+v"(sz),
                   [dx] "=&v"(dx), [dy] "=&v"(dy), [dz] "=&v"(dz), [d2] "=&v"(d2), [y0] "=&v"(y0), [t] "=&v"(t),
                   [w] "=&v"(w), [d2f] "=&v"(d2f)
                 : [base] "s"(nodesd), [px] "v"(px), [py] "v"(py), [pz] "v"(pz), [eps2] "s"(eps2), [c15] "s"(c15),
                   [end] "s"(end), [band2] "s"(band2)
                 : "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50",
                   "s51", "s52", "s53", "s54", "s55", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65",
                   "s66", "vcc", "scc", "memory");
}

// The float64 monopole factor G m / d^3 as NBMI_V64_X computes it: v_rsq_f32 of the rounded d^2 as the seed, one
// Newton step in float64.  A body's sums do not depend on which of its visits came through the C++ visits below.
__device__ __forceinline__ double monopole64(double gm, double d2, float d2f) {
    const double y0 = (double)__builtin_amdgcn_rsqf(d2f);
    const double t = y0 * y0;
    double w = gm * y0;
    const double e = __builtin_fma(-d2, t, 1.0);
    w = w * t;
    const double h = e * 1.5;
    return __builtin_fma(w, h, w);
}

// one float64 visit in C++ with the float64 re-decision of the lanes inside the band (the asm loop stopped on this
// node)
__device__ __forceinline__ unsigned tie_visit64(const NodeD *nodesd, unsigned off, double qx, double qy, double qz,
                                                double eps2, unsigned band2, const Body64 &b64, unsigned &resume,
                                                double &sx, double &sy, double &sz) {
    off = __builtin_amdgcn_readfirstlane(off);
    const NodeD *np = reinterpret_cast<const NodeD *>(reinterpret_cast<const char *>(nodesd) + off);
    const bool active = resume <= off;
    bool geom;
    {   // the decision first, in a scope of its own: the float64 re-test is register hungry, and nothing of the
        // force arithmetic below needs to be alive across it (the pointer is laundered so that it is recomputed)
        const double dx = np->cx - qx, dy = np->cy - qy, dz = np->cz - qz;
        const float d2f = (float)__builtin_fma(dz, dz, __builtin_fma(dy, dy, __builtin_fma(dx, dx, eps2)));
        geom = opening(d2f, np->s2t, band2, active, off / kNodeDBytes, b64).geom;
    }
    asm volatile("" : "+s"(np));
    const NodeD nd = *np;
    const double dx = nd.cx - qx, dy = nd.cy - qy, dz = nd.cz - qz;
    const double d2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, __builtin_fma(dx, dx, eps2)));
    const double w = monopole64(nd.gm, d2, (float)d2);
    bool take;
    const unsigned next = advance<kNodeDBytes>(active, geom, off, nd.next_off, resume, take);
    if (take) {
        sx = __builtin_fma(dx, w, sx); sy = __builtin_fma(dy, w, sy); sz = __builtin_fma(dz, w, sz);
    }
    return __builtin_amdgcn_readfirstlane(next);
}

// The float64 visit of the guarded walk (k_walk<*, *, true>: eps == 0, or an eps so small that the fp32 self-term
// overflows): tie_visit64 plus the reference's dist_sq > eps^2 rule on the float64 d^2 (simulation.py:260) as
// k_potential_tree applies it: the own leaf has d = 0 exactly, and so has a coincident body.
__device__ __forceinline__ unsigned guard_visit64(const NodeD *nodesd, unsigned off, double qx, double qy, double qz,
                                                  double eps2, const Body64 &b64, unsigned &resume, double &sx,
                                                  double &sy, double &sz) {
    off = __builtin_amdgcn_readfirstlane(off);
    const NodeD nd = *reinterpret_cast<const NodeD *>(reinterpret_cast<const char *>(nodesd) + off);
    const double dx = nd.cx - qx, dy = nd.cy - qy, dz = nd.cz - qz;
    const double d2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, __builtin_fma(dx, dx, eps2)));
    const float d2f = (float)d2;
    const bool active = resume <= off;
    const bool geom = opening(d2f, nd.s2t, 2u * kBand64, active, off / kNodeDBytes, b64).geom;
    bool take;
    const unsigned next = advance<kNodeDBytes>(active, geom, off, nd.next_off, resume, take);
    if (take && d2 > eps2) {
        const double w = monopole64(nd.gm, d2, d2f);
        sx = __builtin_fma(dx, w, sx); sy = __builtin_fma(dy, w, sy); sz = __builtin_fma(dz, w, sz);
    }
    return __builtin_amdgcn_readfirstlane(next);
}

// a wave-uniform 64-bit value the compiler no longer knows to be uniform (loaded behind something it treats as a
// possible store, e.g. the cycle counter read of the balance mode) back into scalar registers
__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
// Everything a lane carries through a walk.  lane_prologue() fills it for every walk kernel alike: which body the lane
// has, what a lane without one looks like (resume = ~0: it never takes part, so every launched wave is full), and what a
// pending capacity error does (frozen: nothing is walked, the epilogues leave the state as it is).
struct WalkCtx {
    const Node *nodes;
    bool valid, frozen;
    uint32_t j;  // the body's row of the current state
    float px, py, pz;
    Body64 b64;
    unsigned resume;  // the cursor value from which the lane takes part: 0 at the start
    unsigned band2;
    unsigned rows;  // the walk ends behind this many node records
};
// a pending capacity error ends every walk before its first visit
__device__ __forceinline__ unsigned walk_rows(const TreeInfo *info_in, bool frozen) {
    return frozen ? 0u : (unsigned)info_in->walk_nodes;
}
__device__ __forceinline__ WalkCtx lane_prologue(const Node *nodes, const float4 *__restrict__ posm_s,
                                                 const uint32_t *__restrict__ perm, int64_t rank, int64_t rank_end,
                                                 const TreeInfo *info_in, const WalkTable *tab, int curbuf) {
    WalkCtx C;
    C.nodes = nodes;
    C.valid = rank < rank_end;
    C.frozen = tree_frozen(info_in);
    C.rows = walk_rows(info_in, C.frozen);
    C.band2 = __builtin_amdgcn_readfirstlane(info_in->band2);
    C.px = C.py = C.pz = 0.f;
    C.j = 0;
    if (C.valid) {
        const float4 p = posm_s[rank];
        C.px = p.x; C.py = p.y; C.pz = p.z;
        C.j = perm[rank];
    }
    C.b64 = Body64{tab, curbuf, C.j};
    C.resume = C.valid ? 0u : 0xffffffffu;
    return C;
}
// what the float64 walks need besides: the body's float64 position and the wave-uniform eps^2
struct Lane64 {
    double qx, qy, qz, eps2;
};
__device__ __forceinline__ Lane64 lane_f64(const WalkCtx &C) {
    const WalkTable *tab = C.b64.tab;
    Lane64 L{0.0, 0.0, 0.0, 0.0};
    if (C.valid) {
        const Bodies &cur = tab->buf[C.b64.curbuf];
        L.qx = cur.x[C.j]; L.qy = cur.y[C.j]; L.qz = cur.z[C.j];
    }
    L.eps2 = __longlong_as_double((long long)uniform_u64((unsigned long long)__double_as_longlong(tab->eps2)));
    return L;
}

// [r3] Force precision of a wave (see NBMI_V64_X); rank = any rank of the wave, its first lane's counts.  force_prec 0: float64 where the
// bodies' own neighbourhood is dense enough that an error, once made, is amplified within a few hundred steps (decided
// wave by wave in k_gather_scan, which has the sorted bodies in registers anyway), or where most of the system is
// (k_scan_subtiles).  All lanes of a wave agree; which 64 ranks form a wave does not depend on the sharding.
// per_wave = false (a force pass without a step, whose dt the per-wave decision needs): float64 only if every wave takes it.
__device__ __forceinline__ bool wave_uses_f64(const WalkTable *tab, const TreeInfo *info, const WalkParams &P, int64_t rank,
                                              bool per_wave = true) {
    bool use64 = false;
    if (tab->nodesd && P.force_prec != 1) {
        if (P.force_prec == 2) return true;
        if (per_wave) use64 = tab->wave_flag[rank >> 6] != 0 || info->force_all64 != 0;
        use64 = __builtin_amdgcn_readfirstlane((int)use64) != 0;
    }
    return use64;
}

// Two-level sums: the fp32 accumulators of a C++ loop are emptied into the float64 ones every 12 visits, as NBMI_FLUSH
// does every 3 trips of 4 visits.
__device__ __forceinline__ void flush12(int &since_flush, float &ax, float &ay, float &az, double &sx, double &sy, double &sz) {
    if (++since_flush != 12) return;
    sx += (double)ax; sy += (double)ay; sz += (double)az;
    ax = ay = az = 0.f;
    since_flush = 0;
}

// epilogue of the walks that do not integrate: the acceleration in the caller's body order
__device__ __forceinline__ void store_acc(double *__restrict__ acc_out, const Bodies &cur, uint32_t j, double x, double y, double z) {
    const int64_t o = 3 * (int64_t)cur.id[j];
    acc_out[o] = x; acc_out[o + 1] = y; acc_out[o + 2] = z;
}

// one visit with the float64 re-decision (the asm loop stopped on this node)
__device__ __forceinline__ unsigned tie_visit(const WalkCtx &C, const WalkParams &P, unsigned off, unsigned &resume,
                                              float &ax, float &ay, float &az) {
    bool a_, f_, j_, b_;
    return __builtin_amdgcn_readfirstlane(
        visit<false>(C.nodes, off, C.px, C.py, C.pz, C.b64, P, C.band2, resume, ax, ay, az, a_, f_, j_, b_));
}

// the cursor `off` walks until it reaches `end`; kToEnd: `end` is the end of the array (unrolled loop)
template <bool kToEnd>
__device__ __forceinline__ void walk_span(const WalkCtx &C, const WalkParams &P, unsigned off, unsigned end,
                                          unsigned &resume, float &ax, float &ay, float &az, double &sx, double &sy,
                                          double &sz) {
    off = __builtin_amdgcn_readfirstlane(off);
    while (off < end) {
        unsigned which = 0u;
        if (kToEnd) walk4_asm(C.nodes, off, end, C.px, C.py, C.pz, P.eps2, C.band2, resume, ax, ay, az, sx, sy, sz, which);
        else walk1_asm(C.nodes, off, end, C.px, C.py, C.pz, P.eps2, C.band2, resume, ax, ay, az, sx, sy, sz, which);
        off = __builtin_amdgcn_readfirstlane(off);
        if (!__builtin_amdgcn_readfirstlane(which)) break;
        off = tie_visit(C, P, off, resume, ax, ay, az);
    }
}

// Split / pair walks start a cursor in the middle of the array, at offset S.  The lane's `resume` there
// is what the full walk would have left: only the ancestors of S can have set it beyond S, so seek()
// replays the opening test down that chain (no forces: an ancestor lies before S and belongs to
// another part).  Returns the first offset >= S the walk visits.
__device__ __forceinline__ unsigned seek(const WalkCtx &C, const WalkParams &P, unsigned S, unsigned &resume) {
    unsigned off = 0u;
    while (off < S) {
        off = __builtin_amdgcn_readfirstlane(off);
        const Node nd = *reinterpret_cast<const Node *>(reinterpret_cast<const char *>(C.nodes) + off);
        const float dx = nd.cx - C.px, dy = nd.cy - C.py, dz = nd.cz - C.pz;
        const float dist_sq = fmaf(dz, dz, fmaf(dy, dy, fmaf(dx, dx, P.eps2)));
        const bool active = resume <= off;
        bool take;
        const unsigned next = advance<kNodeBytes>(active, opening(dist_sq, nd.s2t, C.band2, active, off / kNodeBytes, C.b64).geom,
                                                  off, nd.next_off, resume, take);
        if (next == nd.next_off) {
            off = next;  // nobody opens this ancestor: the walk never enters it
            continue;
        }
        // descend to the child whose subtree contains S
        unsigned c = next;
        for (;;) {
            c = __builtin_amdgcn_readfirstlane(c);
            const unsigned nxt = reinterpret_cast<const Node *>(reinterpret_cast<const char *>(C.nodes) + c)->next_off;
            if (nxt > S) break;
            c = nxt;
        }
        off = c;
    }
    return off;
}

// [leapfrog] Epilogue of the synchronized kick-drift-kick step.  The state rows the walk reads
// (P.curbuf) were written by k_kick_drift: x already drifted, v after the opening half-kick.
//   kLeapClose: v = (v + a dt/2) damping, written with x, m, id and a at the body's new rank of the other buffer - the
//               buffer k_kick_drift read, so after the step the current buffer is the same one again.
//   kLeapPrime: a written beside the body's own row of the current buffer (the walk ran on the current state).
// Frozen (a capacity error is pending): nothing is written, the pre-step rows (x, v, a) stay the state.
__device__ __forceinline__ void leap_epilogue(const WalkTable *tab, int leap, uint32_t j, int64_t rank, double ax, double ay,
                                              double az, const WalkParams &P, bool frozen) {
    if (frozen) return;
    if (leap == kLeapPrime) {
        tab->ax[j] = ax; tab->ay[j] = ay; tab->az[j] = az;
        return;
    }
    const Bodies cur = tab->buf[P.curbuf], nxt = tab->buf[1 - P.curbuf];
    const double h = 0.5 * P.dt;
    nxt.vx[rank] = (cur.vx[j] + ax * h) * P.damping;
    nxt.vy[rank] = (cur.vy[j] + ay * h) * P.damping;
    nxt.vz[rank] = (cur.vz[j] + az * h) * P.damping;
    nxt.x[rank] = cur.x[j]; nxt.y[rank] = cur.y[j]; nxt.z[rank] = cur.z[j];
    nxt.m[rank] = cur.m[j];
    nxt.id[rank] = cur.id[j];
    tab->ax[rank] = ax; tab->ay[rank] = ay; tab->az[rank] = az;
}

// fused kick-drift (simulation.py:291-305) of the body at sorted rank `rank`, written at that rank of the
// other buffer; frozen (a capacity error is pending): the body moves to its rank unchanged.  kLeap (the leapfrog
// instantiations of the walks): leap_epilogue as tab->leap says (returns 0: the positions the next build reads are
// published by k_kick_drift).  A template parameter, not a branch on tab->leap alone: the kick-drift instantiations keep
// their code, registers and occupancy exactly.
template <bool kLeap>
__device__ __forceinline__ double integrate(const WalkTable *tab, uint32_t j, int64_t rank, double ax,
                                            double ay, double az, const WalkParams &P, bool frozen) {
    if (kLeap) {
        leap_epilogue(tab, tab->leap, j, rank, ax, ay, az, P, frozen);
        return 0.0;
    }
    const Bodies cur = tab->buf[P.curbuf], nxt = tab->buf[1 - P.curbuf];
    double vx = cur.vx[j], vy = cur.vy[j], vz = cur.vz[j];
    double x0 = cur.x[j], y0 = cur.y[j], z0 = cur.z[j];
    const double m0 = cur.m[j];
    const int32_t id0 = cur.id[j];
    if (!frozen) {
        vx += ax * P.dt; vy += ay * P.dt; vz += az * P.dt;
        vx *= P.damping; vy *= P.damping; vz *= P.damping;
        x0 += vx * P.dt; y0 += vy * P.dt; z0 += vz * P.dt;
    }
    nxt.vx[rank] = vx; nxt.vy[rank] = vy; nxt.vz[rank] = vz;
    nxt.x[rank] = x0; nxt.y[rank] = y0; nxt.z[rank] = z0;
    nxt.m[rank] = m0;
    nxt.id[rank] = id0;
    return fmax(fmax(fabs(x0), fabs(y0)), fabs(z0));
}

// The largest |coordinate| a wave has just written joins TreeInfo::maxabs_next (all lanes of the wave call this;
// lanes without a body pass 0).  Most waves find a value at least as large already there and skip the atomic.
__device__ __forceinline__ void publish_maxabs(const WalkTable *tab, double lane_max) {
    const double m = wave_max(lane_max);
    if ((threadIdx.x & 63) == 0) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(m);
        unsigned long long *dst = tab->maxabs_next;
        if (bits > __atomic_load_n(dst, __ATOMIC_RELAXED)) atomicMax(dst, bits);
    }
}

// [r3] Cuts for the balance mode of k_walk: XCD x gets the logical blocks [b[x], b[x + 1]) such that every range
// holds about an eighth of last step's total wave time (bodies move little between steps), at most `jmax` blocks
// (the launch has 8 jmax workgroups) and at least one.  One workgroup: per-thread chunk sums, scan, the seven
// thread(s) whose chunk holds a cut find it.  All-zero times (first step) give equal ranges.
// What the walk relies on is the covering property: b[0] = 0, b[8] = nb and 1 <= b[k + 1] - b[k] <= jmax, so that the
// workgroups (xcd, jb < jmax) with b[xcd] + jb < b[xcd + 1] walk every logical block exactly once.
// PRECONDITION: nb >= kXcdMinBlocks (with fewer blocks than XCDs no range can hold "at least one": the need_after clamp
// pushes the cuts below 0 - nb = 5 gives 0 -2 -1 0 1 2 3 4 5 - and an XCD would start at a negative block) and
// 8 jmax >= nb (xcd_jmax(nb) gives that).  The callers check both: enqueue_walk's gate and the two debug hooks.
constexpr int kXcdMinBlocks = 8;
// workgroups per XCD of a balanced launch over nb logical blocks: half as many again as an equal eighth, so that a cheap
// range can hold that much more than its share (64 bits: the hooks test a caller's nb before anything is narrowed)
inline int64_t xcd_jmax(int64_t nb) { return ((nb + 7) / 8) * 3 / 2 + 1; }
__global__ __launch_bounds__(1024) void k_xcd_bounds(const unsigned *__restrict__ wave_cycles, int nb, int jmax, int *__restrict__ bounds) {
    __shared__ int cut[9];
    const int t = threadIdx.x;
    const int chunk = (nb + 1023) / 1024;
    const int b = t * chunk < nb ? t * chunk : nb, e = b + chunk < nb ? b + chunk : nb;
    unsigned long long acc = 0;
    for (int i = b; i < e; i++) {
        const uint4 q = reinterpret_cast<const uint4 *>(wave_cycles)[i];
        acc += (unsigned long long)q.x + q.y + q.z + q.w + 1ull;  // + 1: all-zero input still cuts into equal parts
    }
    const scan::Scanned<unsigned long long> sc = scan::block_scan<1024>(acc, 0ull, scan::Sum());
    const unsigned long long ex = sc.excl, inc = sc.incl;  // work before this thread's chunk, and with it
    if (t == 0) { cut[0] = 0; cut[8] = nb; }
    for (int k = 1; k < 8; k++) {
        const unsigned long long target = sc.total / 8ull * (unsigned long long)k;
        if (b < e && ex <= target && target < inc) {
            unsigned long long run = ex;
            int i = b;
            for (; i < e; i++) {
                const uint4 q = reinterpret_cast<const uint4 *>(wave_cycles)[i];
                run += (unsigned long long)q.x + q.y + q.z + q.w + 1ull;
                if (run > target) break;
            }
            cut[k] = i + 1 < nb ? i + 1 : nb;
        }
    }
    __syncthreads();
    if (t == 0) {
        // ranges of 1 .. jmax blocks, in order; what the clamps push out goes to the later XCDs
        int prev = 0;
        for (int k = 1; k < 8; k++) {
            int c = cut[k];
            const int lo = prev + 1, hi = prev + jmax;
            const int need_after = (8 - k);  // blocks the remaining XCDs need at least ...
            const int room_after = (8 - k) * jmax;  // ... and can take at most
            if (c < lo) c = lo;
            if (c > hi) c = hi;
            if (nb - c < need_after) c = nb - need_after;
            if (nb - c > room_after) c = nb - room_after;
            bounds[k] = c;
            prev = c;
        }
        bounds[0] = 0;
        bounds[8] = nb;
    }
}

// The walk kernel.  kCount = parity/measurement build (C++ visit, work counters);
// otherwise the hand-scheduled loop (eps > 0) or the C++ visit with the distance guard (kGuard: eps == 0 or tiny, see
// guarded()), whose float64 waves visit through guard_visit64.
template <bool kIntegrate, bool kCount, bool kGuard, bool kLeap = false>
__global__ __launch_bounds__(kBlock) void k_walk(const Node *__restrict__ nodes, const WalkTable *tab,
                                                 const TreeInfo *info_in, const float4 *__restrict__ posm_s,
                                                 const uint32_t *__restrict__ perm,
                                                 double *__restrict__ acc_out, WalkParams P, TreeInfo *info_out) {
    // [r3] Which logical block (= which 256 consecutive ranks) this workgroup walks.  Hardware deals workgroups to the
    // eight XCDs round-robin; logical_block() gives every XCD one contiguous eighth of the blocks (neighbouring
    // groups walk the same nodes: L2 locality) - equal in blocks, not in work: the XCD that got the densest part
    // of the system sets the kernel's time (10 M collision: the busiest XCD has 5.5 % more visits than the mean).
    // Balance mode keeps the contiguous ranges but cuts them where last step's measured wave times say an eighth of
    // the WORK ends (k_xcd_bounds); a workgroup beyond its XCD's range has nothing to do.
    int lb;
    if (kIntegrate && P.balance) {
        const int xcd = blockIdx.x & 7, jb = blockIdx.x >> 3;
        const int b0 = __builtin_amdgcn_readfirstlane(tab->xcd_bounds[xcd]);
        const int b1 = __builtin_amdgcn_readfirstlane(tab->xcd_bounds[xcd + 1]);
        lb = b0 + jb;
        if (lb >= b1) return;
    } else {
        lb = logical_block(blockIdx.x, gridDim.x, P.xcd_chunk);
    }
    const int lane = threadIdx.x & 63;
    const int64_t rank = P.rank_begin + (int64_t)lb * blockDim.x + threadIdx.x;
    const WalkCtx C = lane_prologue(nodes, posm_s, perm, rank, P.rank_end, info_in, tab, P.curbuf);
    const bool valid = C.valid, frozen = C.frozen;
    const uint32_t j = C.j;
    const unsigned nn = C.rows * kNodeBytes;  // end offset
    unsigned resume = C.resume;
    float ax = 0.f, ay = 0.f, az = 0.f;  // fp32 accumulators of the loops ...
    double sx = 0.0, sy = 0.0, sz = 0.0;  // ... emptied into these every few trips (two-level sums, NBMI_FLUSH)

    const bool use64 = !kCount && kIntegrate && wave_uses_f64(tab, info_in, P, rank);
    // (the clock is read here, behind the prologue's loads: the compiler treats the read as a possible store and
    // turns every scalar load that follows it into a vector load)
    const unsigned long long t_start = (kIntegrate && P.balance) ? __builtin_readcyclecounter() : 0ull;
    if (use64) {
        const NodeD *nodesd = reinterpret_cast<const NodeD *>(uniform_u64(reinterpret_cast<unsigned long long>(tab->nodesd)));
        const Lane64 L = lane_f64(C);
        // (read again, not kept from the prologue: one SGPR less, and the product instantiation sits at the 80 beyond which a
        // CU holds one block fewer)
        const unsigned nnd = __builtin_amdgcn_readfirstlane(walk_rows(info_in, frozen) * kNodeDBytes);
        unsigned off = 0u;
        // (the guarded walk: every visit in C++, skipping the pairs at dist_sq <= eps^2)
        if (kGuard) {
            while (off < nnd) off = guard_visit64(nodesd, off, L.qx, L.qy, L.qz, L.eps2, C.b64, resume, sx, sy, sz);
        }
        while (!kGuard && off < nnd) {
            unsigned which = 0u;
            walk4_asm64(nodesd, off, nnd, L.qx, L.qy, L.qz, L.eps2, 2u * kBand64, resume, sx, sy, sz, which);
            off = __builtin_amdgcn_readfirstlane(off);
            if (!__builtin_amdgcn_readfirstlane(which)) break;
            off = tie_visit64(nodesd, off, L.qx, L.qy, L.qz, L.eps2, 2u * kBand64, C.b64, resume, sx, sy, sz);
        }
    } else if (!kCount && !kGuard) {
        if (nn && P.pair) {
            // two cursors: [0, mid) and [mid, nn); the second needs the lanes' state at mid (seek).
            // Where to cut: a wave spends ~40 % of its visits inside the 1/64 of the array around its own bodies
            // (scripts/analysis/range_balance.py), so equal halves keep both cursors busy for only a fifth of the
            // visits; cutting at the leaf of the wave's middle body does for two thirds of them.
            // (owner mode: the array begins with a jump node and unused rows up to walk_first)
            unsigned mid = __builtin_amdgcn_readfirstlane((unsigned)((info_in->walk_first + info_in->walk_nodes) / 2) * kNodeBytes);
            if (P.pair == 2) {
                const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
                const int64_t r0 = P.rank_begin + (int64_t)lb * blockDim.x + wv * 64;
                const int64_t rl = r0 + 64 < P.rank_end ? r0 + 64 : P.rank_end;  // the wave's bodies: [r0, rl)
                const int64_t rm = r0 < rl ? r0 + (rl - r0) / 2 : 0;
                const unsigned home = __builtin_amdgcn_readfirstlane((unsigned)(rm + pex_at(tab->pex, tab->subpex, rm + 1) + tab->own_base) * kNodeBytes);
                mid = (r0 < rl && home > 0u && home < nn) ? home : mid;
            }
            // (each half sums into its own accumulator, added at the end: a body's result does not depend on how the two
            // cursors' visits interleave.  With the home cut it does depend on which 64 ranks form the wave - the same
            // ones for every sharding whose ranges start at multiples of 64 ranks)
            unsigned resume2 = resume;
            float bx = 0.f, by = 0.f, bz = 0.f;
            unsigned o1 = 0u, o2 = __builtin_amdgcn_readfirstlane(mid ? seek(C, P, mid, resume2) : 0u);
            while (mid && o1 < mid && o2 < nn) {
                unsigned which = 0u;
                walk_pair_asm(nodes, o1, mid, o2, nn, C.px, C.py, C.pz, P.eps2, C.band2, resume, resume2, ax, ay, az,
                              bx, by, bz, sx, sy, sz, which);
                o1 = __builtin_amdgcn_readfirstlane(o1);
                o2 = __builtin_amdgcn_readfirstlane(o2);
                which = __builtin_amdgcn_readfirstlane(which);
                if (which == 1u) o1 = tie_visit(C, P, o1, resume, ax, ay, az);
                else if (which == 2u) o2 = tie_visit(C, P, o2, resume2, bx, by, bz);
                else break;
            }
            if (o1 < mid) walk_span<false>(C, P, o1, mid, resume, ax, ay, az, sx, sy, sz);
            if (o2 < nn && o2 >= mid) walk_span<true>(C, P, o2, nn, resume2, bx, by, bz, sx, sy, sz);
            sx += (double)bx; sy += (double)by; sz += (double)bz;
        } else if (nn) {
            walk_span<true>(C, P, 0u, nn, resume, ax, ay, az, sx, sy, sz);
        }
    } else {
        unsigned long long wv = 0, lv = 0, la = 0, jm = 0, bd = 0;
        unsigned long long wm[4] = {0, 0, 0, 0};
        int wbase[4] = {-1000, -1000, -1000, -1000};
        unsigned off = 0u;
        int since_flush = 0;  // guarded integrating walk: visits since the fp32 sums were emptied (two-level sums)
        while (off < nn) {
            bool a_, f_, j_, b_;
            const int c_old = (int)(off / kNodeBytes);
            off = visit<kGuard>(nodes, off, C.px, C.py, C.pz, C.b64, P, C.band2, resume, ax, ay, az, a_, f_, j_, b_);
            if (kGuard && !kCount) flush12(since_flush, ax, ay, az, sx, sy, sz);
            if (kCount) {
                wv += 1; lv += a_ ? 1 : 0; la += f_ ? 1 : 0; jm += j_ ? 1 : 0; bd += b_ ? 1 : 0;
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    if (c_old < wbase[w] || c_old >= wbase[w] + (8 << w)) { wm[w]++; wbase[w] = c_old; }
                }
            }
        }
        if (kCount) {
            // wave_visits counted once per wave (lane 0), lane counters summed over lanes
            if (lane == 0) {
                const unsigned xcc = __builtin_amdgcn_s_getreg((20 /*HW_REG_XCC_ID*/) | (0 << 6) | ((4 - 1) << 11)) & 7u;
                atomicAdd(&info_out->xcd_visits[xcc], wv);
                atomicAdd(&info_out->wave_visits, wv);
                for (int w = 0; w < 4; w++) atomicAdd(&info_out->win_miss[w], wm[w]);
                atomicAdd(&info_out->jumps, jm);
            }
            atomicAdd(&info_out->lane_visits, lv);
            atomicAdd(&info_out->lane_accepts, la);
            if (bd) atomicAdd(&info_out->band_visits, bd);
        }
    }
    if (kIntegrate) {
        publish_maxabs(tab, valid ? integrate<kLeap>(tab, j, rank, sx + (double)ax, sy + (double)ay, sz + (double)az, P, frozen) : 0.0);
        if (P.balance && lane == 0) {
            const unsigned long long dtc = __builtin_readcyclecounter() - t_start;
            tab->wave_cycles[4 * lb + (threadIdx.x >> 6)] = (unsigned)(dtc > 0xffffffffull ? 0xffffffffull : dtc);
        }
    } else if (valid) {
        store_acc(acc_out, tab->buf[P.curbuf], j, (double)ax, (double)ay, (double)az);
    }
}

// ---------------------------------------------------------------------------------------
// Split walk for small systems.  Below ~250 k bodies there are fewer groups than wave slots and the
// step time is ONE wave's serial chain of ~1 700 dependent visits (0.32 ms at 100 k bodies, where
// the same work spread over the chip would take 0.1 ms).  Here a block of K waves shares one group
// of 64 bodies and wave w walks the w-th K-th of the pre-order array, [w N/K, (w+1) N/K) nodes.
// (Measured at 100 k bodies, K = 4: equal quarters 0.179 ms; quarters centred on the group's own
// leaves with a near range of 1/8 ... 1/8192 of the array 0.204 ... 0.257 ms - a galaxy's far field
// is where most visits are, so plain equal parts balance best, and they do not depend on the
// group.)  A part that starts at S gets its lanes' `resume` from seek().  The K partial
// sums meet in LDS and are added in fixed order, then the usual fused kick-drift.  Same accepted
// (body, node) set as the one-wave walk; the fp32 sums associate differently (by fixed node ranges,
// so a body's result still does not depend on its group or on the sharding).
// ---------------------------------------------------------------------------------------
template <int K, bool kLeap = false>
__global__ __launch_bounds__(64 * K) void k_walk_split(const Node *__restrict__ nodes, const WalkTable *tab,
                                                       const TreeInfo *info_in, const float4 *__restrict__ posm_s,
                                                       const uint32_t *__restrict__ perm, WalkParams P) {
    __shared__ double part[K][3][64];
    const int lb = logical_block(blockIdx.x, gridDim.x, P.xcd_chunk);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t rank = P.rank_begin + (int64_t)lb * 64 + lane;
    const WalkCtx C = lane_prologue(nodes, posm_s, perm, rank, P.rank_end, info_in, tab, P.curbuf);
    const bool valid = C.valid, frozen = C.frozen;
    const uint32_t j = C.j;
    const int64_t num_nodes = C.rows;
    unsigned resume = C.resume;
    float ax = 0.f, ay = 0.f, az = 0.f;
    double sx = 0.0, sy = 0.0, sz = 0.0;  // two-level sums, see NBMI_FLUSH
    // wave-uniform range (w is the wave index): tell the compiler so
    // (owner mode: rows [1, walk_first) behind the jump node at row 0 are unused; the parts divide the rest)
    const int64_t first = frozen ? 0 : info_in->walk_first, span = num_nodes - first;
    // ([r4] measured and dropped: parts graded by distance from the group's own leaves - the K waves sharing the two sides
    // of the home leaf in proportion to their octaves of distance, a side's parts ending at home +- 48 * 2^(t octaves / parts)
    // nodes.  Walk 0.076 -> 0.096 ms at 10 k bodies, 0.157 -> 0.182 at 30 k, 0.216 -> 0.244 at 100 k, 0.475 -> 0.454 at
    // 262 k: a galaxy's visits are spread over the far field more evenly than one per octave, equal K-ths stay.)
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(w == 0 ? 0 : first + span * w / K) * kNodeBytes);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(first + span * (w + 1) / K) * kNodeBytes);
    // [r3] force precision of the group (all K waves of the workgroup walk the same 64 bodies)
    const bool use64 = wave_uses_f64(tab, info_in, P, P.rank_begin + (int64_t)lb * 64);
    if (lo < hi) {
        // (seek works on the fp32 records in both cases: it only replays opening decisions, and those are the same)
        const unsigned c0 = __builtin_amdgcn_readfirstlane(lo == 0u ? 0u : seek(C, P, lo, resume));
        if (c0 < hi && !use64) {
            walk_span<false>(C, P, c0, hi, resume, ax, ay, az, sx, sy, sz);
        } else if (c0 < hi) {
            const NodeD *nodesd = reinterpret_cast<const NodeD *>(uniform_u64(reinterpret_cast<unsigned long long>(tab->nodesd)));
            const Lane64 L = lane_f64(C);
            // offsets of the 24-byte records -> offsets of the 40-byte ones (same node indices)
            unsigned off = c0 / kNodeBytes * kNodeDBytes;
            const unsigned end = hi / kNodeBytes * kNodeDBytes;
            unsigned res64 = resume == 0xffffffffu ? resume : resume / kNodeBytes * kNodeDBytes;
            while (off < end) {
                unsigned which = 0u;
                walk1_asm64(nodesd, off, end, L.qx, L.qy, L.qz, L.eps2, 2u * kBand64, res64, sx, sy, sz, which);
                off = __builtin_amdgcn_readfirstlane(off);
                if (!__builtin_amdgcn_readfirstlane(which)) break;
                off = tie_visit64(nodesd, off, L.qx, L.qy, L.qz, L.eps2, 2u * kBand64, C.b64, res64, sx, sy, sz);
            }
        }
    }
    part[w][0][lane] = sx + (double)ax; part[w][1][lane] = sy + (double)ay; part[w][2][lane] = sz + (double)az;
    __syncthreads();
    if (w != 0) return;
    sx = part[0][0][lane]; sy = part[0][1][lane]; sz = part[0][2][lane];
#pragma unroll
    for (int k = 1; k < K; k++) {
        sx += part[k][0][lane]; sy += part[k][1][lane]; sz += part[k][2][lane];
    }
    publish_maxabs(tab, valid ? integrate<kLeap>(tab, j, rank, sx, sy, sz, P, frozen) : 0.0);
}

// ---------------------------------------------------------------------------------------
// Direct O(N^2): a_i = sum_{j != i} G m_j d (|d|^2 + eps^2)^(-3/2)   (gpu_backend.py:145-240)
// 256-thread blocks, IB bodies per thread, 256-body tiles of {x,y,z,G m} staged in LDS and read
// back as wave-uniform broadcasts.  fp32 pair arithmetic, per-tile fp32 partial sums folded
// into float64 accumulators.  The j == i term is exactly zero when eps > 0 (d = 0); with
// kGuard (eps == 0, or so small that the fp32 j == i term would be 0 * inf: guarded()) the pairs whose
// fp32 r2 does not exceed eps^2 are skipped, the reference's rule for its self and coincident pairs.  Fused update_bodies_cuda
// (gpu_backend.py:243-257): v = (v + a dt) * damping; x += v dt, new positions go to `nxt`.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_pack_posm(Bodies cur, int64_t n, double G, float4 *__restrict__ posm) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    posm[i] = make_float4((float)cur.x[i], (float)cur.y[i], (float)cur.z[i], (float)(G * cur.m[i]));
}

// [leapfrog] Opening half-kick and drift of every row of the current buffer, written to the same
// row of the other buffer: v' = v + a dt/2, x' = x + v' dt; m and id travel along.  The pre-step rows stay untouched
// (a step whose octree does not fit leaves them the state).  Barnes-Hut: max |x'| joins TreeInfo::maxabs_next, which the
// build's k_header takes over (no pass of its own over the bodies); one atomic per block, so the grid is capped by the
// caller.  Direct: the new positions and G m are also packed for k_direct (k_pack_posm's job).
__global__ __launch_bounds__(kBlock) void k_kick_drift(Bodies cur, Bodies nxt, const double *__restrict__ ax,
                                                       const double *__restrict__ ay, const double *__restrict__ az, int64_t n,
                                                       double dt, double G, float4 *__restrict__ posm,
                                                       unsigned long long *__restrict__ maxabs) {
    __shared__ double red[kBlock / 64];
    const double h = 0.5 * dt;
    double mx = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const double vx = cur.vx[i] + ax[i] * h, vy = cur.vy[i] + ay[i] * h, vz = cur.vz[i] + az[i] * h;
        const double x = cur.x[i] + vx * dt, y = cur.y[i] + vy * dt, z = cur.z[i] + vz * dt;
        const double m = cur.m[i];
        nxt.vx[i] = vx; nxt.vy[i] = vy; nxt.vz[i] = vz;
        nxt.x[i] = x; nxt.y[i] = y; nxt.z[i] = z;
        nxt.m[i] = m;
        nxt.id[i] = cur.id[i];
        if (posm) posm[i] = make_float4((float)x, (float)y, (float)z, (float)(G * m));
        mx = fmax(mx, fmax(fmax(fabs(x), fabs(y)), fabs(z)));
    }
    if (!maxabs) return;
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; w++) mx = fmax(mx, red[w]);
        const unsigned long long bits = (unsigned long long)__double_as_longlong(mx);
        if (bits > __atomic_load_n(maxabs, __ATOMIC_RELAXED)) atomicMax(maxabs, bits);
    }
}

// [r4] kUniform: every body has the same mass (the reference's presets set masses = 1: tools/presets.py), so G m is ONE number:
// it leaves the pair loop - f = inv^3 instead of G m inv^3, 12 vector instructions per pair instead of 13 - and multiplies
// the float64 sums once per body.
// [leapfrog] kLeap (with kIntegrate): the epilogue of leap_epilogue in index order - kLeapClose reads the rows k_kick_drift
// wrote (cur) and writes x, the closed v, m, id to `nxt` and a to the columns acc_out[i], acc_out[n + i], acc_out[2n + i];
// kLeapPrime only writes a there.
template <int IB, bool kGuard, bool kIntegrate, bool kUniform, int kLeap = 0>
__global__ __launch_bounds__(kBlock) void k_direct(const float4 *__restrict__ posm, int64_t n, int64_t ibeg, int64_t iend,
                                                   float eps2, Bodies cur, Bodies nxt, double *__restrict__ acc_out,
                                                   double dt, double damping, double uniform_gm) {
    // bodies [ibeg, iend) (this launch's shard) against all n
    __shared__ float4 tile[kBlock];
    const int64_t i0 = ibeg + (int64_t)blockIdx.x * (kBlock * IB) + threadIdx.x;
    float px[IB], py[IB], pz[IB];
    double ax[IB], ay[IB], az[IB];
#pragma unroll
    for (int k = 0; k < IB; k++) {
        const int64_t i = i0 + (int64_t)k * kBlock;
        const float4 p = i < iend ? posm[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        px[k] = p.x; py[k] = p.y; pz[k] = p.z;
        ax[k] = ay[k] = az[k] = 0.0;
    }
    const int64_t ntiles = (n + kBlock - 1) / kBlock;
    for (int64_t t = 0; t < ntiles; t++) {
        const int64_t j = t * kBlock + threadIdx.x;
        // pads of the last tile: zero mass - or, where the mass is not part of the pair arithmetic, so far away that
        // d^2 overflows to +inf and v_rsq_f32 returns exactly 0
        tile[threadIdx.x] = j < n ? posm[j] : (kUniform ? make_float4(1.0e20f, 1.0e20f, 1.0e20f, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f));
        __syncthreads();
        float sx[IB], sy[IB], sz[IB];
#pragma unroll
        for (int k = 0; k < IB; k++) sx[k] = sy[k] = sz[k] = 0.f;
        // [r4] The j-bodies are fetched a chunk AHEAD: the next eight LDS reads are issued before the current eight bodies'
        // arithmetic, so no read is waited for where it is issued (the compiler's 8-unrolled form of the plain loop put an
        // s_waitcnt lgkmcnt(0) behind each of its last four ds_read_b128).  Same operations in the same order: results
        // unchanged bit for bit.  62.8 -> 73.3 TFLOP/s at 1 M bodies (318 -> 273 ms per step) (scripts/ubench/direct_valu_sched.hip:
        // 47.3 -> 41.2 cycles per 64 pairs per SIMD; chunks of 4: 41.9; more bodies per thread: no better).
        constexpr int CH = 8;
        float4 cur[CH], nxt[CH];
#pragma unroll
        for (int c = 0; c < CH; c++) cur[c] = tile[c];
#pragma unroll 1
        for (int jj = 0; jj < kBlock; jj += CH) {
            const int nb = jj + CH < kBlock ? jj + CH : 0;
#pragma unroll
            for (int c = 0; c < CH; c++) nxt[c] = tile[nb + c];
#pragma unroll
            for (int c = 0; c < CH; c++) {
                const float4 q = cur[c];
#pragma unroll
                for (int k = 0; k < IB; k++) {
                    const float dx = q.x - px[k], dy = q.y - py[k], dz = q.z - pz[k];
                    const float r2 = fmaf(dz, dz, fmaf(dy, dy, fmaf(dx, dx, eps2)));
                    const float inv = __builtin_amdgcn_rsqf(r2);
                    float f = kUniform ? inv * inv * inv : q.w * inv * inv * inv;
                    if (kGuard) f = (r2 > eps2) ? f : 0.f;
                    sx[k] = fmaf(f, dx, sx[k]);
                    sy[k] = fmaf(f, dy, sy[k]);
                    sz[k] = fmaf(f, dz, sz[k]);
                }
            }
#pragma unroll
            for (int c = 0; c < CH; c++) cur[c] = nxt[c];
        }
#pragma unroll
        for (int k = 0; k < IB; k++) {
            ax[k] += (double)sx[k]; ay[k] += (double)sy[k]; az[k] += (double)sz[k];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < IB; k++) {
        const int64_t i = i0 + (int64_t)k * kBlock;
        if (i >= iend) continue;
        if (kUniform) { ax[k] *= uniform_gm; ay[k] *= uniform_gm; az[k] *= uniform_gm; }
        if (kIntegrate && kLeap != 0) {
            if (kLeap == kLeapClose) {
                const double h = 0.5 * dt;
                nxt.vx[i] = (cur.vx[i] + ax[k] * h) * damping;
                nxt.vy[i] = (cur.vy[i] + ay[k] * h) * damping;
                nxt.vz[i] = (cur.vz[i] + az[k] * h) * damping;
                nxt.x[i] = cur.x[i]; nxt.y[i] = cur.y[i]; nxt.z[i] = cur.z[i];
                nxt.m[i] = cur.m[i];
                nxt.id[i] = cur.id[i];
            }
            acc_out[i] = ax[k]; acc_out[n + i] = ay[k]; acc_out[2 * n + i] = az[k];
        } else if (kIntegrate) {
            const double vx = (cur.vx[i] + ax[k] * dt) * damping;
            const double vy = (cur.vy[i] + ay[k] * dt) * damping;
            const double vz = (cur.vz[i] + az[k] * dt) * damping;
            nxt.vx[i] = vx; nxt.vy[i] = vy; nxt.vz[i] = vz;
            nxt.x[i] = cur.x[i] + vx * dt;
            nxt.y[i] = cur.y[i] + vy * dt;
            nxt.z[i] = cur.z[i] + vz * dt;
            nxt.m[i] = cur.m[i];
            nxt.id[i] = cur.id[i];
        } else {
            const int64_t o = 3 * (int64_t)cur.id[i];
            acc_out[o] = ax[k]; acc_out[o + 1] = ay[k]; acc_out[o + 2] = az[k];
        }
    }
}

// ---------------------------------------------------------------------------------------
// colour ramp (simulation.py:320-400 == gpu_backend.py:259-325), float64 maths, f32 stores,
// rows written in the caller's body order.
// ---------------------------------------------------------------------------------------
// (shared by k_colors and k_frame_snapshot: one ramp, so a snapshot's colours are nbmi_compute_colors' bit for bit)
// the ramp itself, a function of t (values above 1 are the caller's to clamp): the speed colours enter with
// t = speed / max_speed, the density colours (K16) with t = the position of log10(rho) in its range
__device__ __forceinline__ void color_ramp_t(double t, float &out_r, float &out_g, float &out_b) {
    double cr, cg, cb, s, s2;
    if (t < 0.55) {
        if (t < 0.15) {
            s = t / 0.15;
            cr = __dsub_rn(0.4, __dmul_rn(0.2, s)); cg = __dadd_rn(0.2, __dmul_rn(0.2, s)); cb = __dadd_rn(0.8, __dmul_rn(0.1, s));
        } else if (t < 0.30) {
            s = (t - 0.15) / 0.15;
            cr = __dadd_rn(0.2, __dmul_rn(0.1, s)); cg = __dadd_rn(0.4, __dmul_rn(0.1, s)); cb = __dadd_rn(0.9, __dmul_rn(0.05, s));
        } else {
            s = (t - 0.30) / 0.25;
            if (s < 0.6) {
                s2 = s / 0.6;
                cr = __dsub_rn(0.3, __dmul_rn(0.1, s2)); cg = __dadd_rn(0.5, __dmul_rn(0.3, s2)); cb = __dadd_rn(0.95, __dmul_rn(0.05, s2));
            } else {
                s2 = (s - 0.6) / 0.4;
                cr = __dadd_rn(0.2, __dmul_rn(0.8, s2)); cg = __dadd_rn(0.8, __dmul_rn(0.2, s2)); cb = 1.0;
            }
        }
    } else if (t < 0.90) {
        cr = 1.0; cg = 1.0; cb = 1.0;
    } else if (t < 0.95) {
        s = (t - 0.90) / 0.05;
        cr = 1.0; cg = __dsub_rn(1.0, __dmul_rn(0.05, s)); cb = __dsub_rn(1.0, __dmul_rn(1.0, s));
    } else if (t < 0.99) {
        s = (t - 0.95) / 0.04;
        cr = 1.0; cg = __dsub_rn(0.95, __dmul_rn(0.45, s)); cb = 0.0;
    } else {
        s = (t - 0.99) / 0.01;
        cr = 1.0; cg = __dsub_rn(0.5, __dmul_rn(0.5, s)); cb = 0.0;
    }
    out_r = (float)cr; out_g = (float)cg; out_b = (float)cb;
}
__device__ __forceinline__ void color_ramp(double vx, double vy, double vz, double max_speed, float &out_r, float &out_g,
                                           float &out_b) {
    const double speed = sqrt(__dadd_rn(__dadd_rn(__dmul_rn(vx, vx), __dmul_rn(vy, vy)), __dmul_rn(vz, vz)));
    double t = speed / max_speed;
    t = t > 1.0 ? 1.0 : t;
    color_ramp_t(t, out_r, out_g, out_b);
}
// density colours (nbmi_set_color_mode): rho = the mass inside the k-th neighbour sphere over
// its volume, +inf where the sphere has no radius; t = where log10(rho) lies in [lo, hi].  Shared by k_colors_density
// and k_frame_snapshot, like the ramp.
__device__ __forceinline__ double knn_density(double r2, double mass) {
    if (r2 == 0.0) return INFINITY;
    return mass / __dmul_rn(4.1887902047863905, __dmul_rn(r2, sqrt(r2)));
}
__device__ __forceinline__ void color_density(double r2, double mass, double lo, double hi, float &out_r, float &out_g,
                                              float &out_b) {
    double t = __dsub_rn(log10(knn_density(r2, mass)), lo) / __dsub_rn(hi, lo);
    t = t > 1.0 ? 1.0 : t;
    t = t < 0.0 ? 0.0 : t;
    color_ramp_t(t, out_r, out_g, out_b);
}
__global__ __launch_bounds__(kBlock) void k_colors_density(Bodies cur, int64_t n, const double *__restrict__ r2,
                                                           const double *__restrict__ mass, double lo, double hi,
                                                           float *__restrict__ colors) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    float cr, cg, cb;
    color_density(r2[r], mass[r], lo, hi, cr, cg, cb);
    const int64_t o = 3 * (int64_t)cur.id[r];
    colors[o] = cr; colors[o + 1] = cg; colors[o + 2] = cb;
}
__global__ __launch_bounds__(kBlock) void k_colors(Bodies cur, int64_t n, double max_speed, bool by_rank,
                                                   float *__restrict__ colors) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    float cr, cg, cb;
    color_ramp(cur.vx[r], cur.vy[r], cur.vz[r], max_speed, cr, cg, cb);
    const int64_t o = 3 * (by_rank ? r : (int64_t)cur.id[r]);  // owner mode: rows stay in rank order
    colors[o] = cr; colors[o + 1] = cg; colors[o + 2] = cb;
}

// ---- un-permuting getters ------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_unperm3_f32(const double *__restrict__ a, const double *__restrict__ b,
                                                        const double *__restrict__ c, const int32_t *__restrict__ id,
                                                        int64_t n, float *__restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const int64_t o = 3 * (id ? (int64_t)id[r] : r);  // owner mode: rows stay in rank order
    out[o] = (float)a[r]; out[o + 1] = (float)b[r]; out[o + 2] = (float)c[r];
}
__global__ __launch_bounds__(kBlock) void k_unperm3_f64(const double *__restrict__ a, const double *__restrict__ b,
                                                        const double *__restrict__ c, const int32_t *__restrict__ id,
                                                        int64_t n, double *__restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const int64_t o = 3 * (id ? (int64_t)id[r] : r);
    out[o] = a[r]; out[o + 1] = b[r]; out[o + 2] = c[r];
}
// ---- frame codec on the device (tools/record.py:231-326) ------------------------------------------
// Format-2 payload of a .zstd frame: int16((cur - prev) * 1000) against the PREVIOUS DECODED frame
// (record.py:254-262; decoder :313-322), float32 arithmetic like NumPy's, C-cast wrap beyond +-32.767 kept
// [quirk].  `prev` (float32, caller's body order) lives in HBM and is advanced to what the decoder will
// reconstruct, prev + int16 / 1000, so only 6 bytes per body and array cross PCIe instead of 12.
// (shared by k_frame_delta and k_frame_snapshot) the int16 of one value; `p` becomes what the decoder reconstructs
__device__ __forceinline__ int16_t frame_quantize(float cur, float &p) {
    const float t = __fmul_rn(__fsub_rn(cur, p), 1000.0f);
    // float -> int32 (truncation toward zero) -> low 16 bits: what ndarray.astype(np.int16) does on x86-64
    const int16_t q = (int16_t)(int)t;
    p = __fadd_rn(p, __fdiv_rn((float)q, 1000.0f));
    return q;
}
__global__ __launch_bounds__(kBlock) void k_frame_delta(const float *__restrict__ cur, float *__restrict__ prev, int64_t count,
                                                        int16_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    float p = prev[i];
    out[i] = frame_quantize(cur[i], p);
    prev[i] = p;
}

// ---- asynchronous frames (nbmi_frame_begin) -------------------------------------------------
// What the snapshot copies of the device-side error words, so that nbmi_frame_wait can report them without touching the
// compute stream.  64 bytes in front of a slot's payload.
struct FrameHeader {
    int error, sticky_error, max_run;
    unsigned sort_error;
    long long num_nodes, sticky_nodes;
    long long pad[4];
};
static_assert(sizeof(FrameHeader) == 64, "slot payloads start 64 bytes into the slot");
// One pass over the state in its own (key-sorted) order: colour (k_colors' ramp) and float32 position (k_unperm3_f32's
// conversion) of every body go to row `id` of the slot - and the colour to `colors`, as nbmi_compute_colors leaves it.
//   NBMI_FRAME_F32        first = positions, second = colours, float32
//   NBMI_FRAME_KEY        the same, and the row also becomes the previous decoded frame
//   NBMI_FRAME_DELTA_I16  positions go to the float32 staging rows; two k_frame_delta launches then write the int16 deltas
//                         of positions and colours against the previous decoded frame into the slot and advance it
// Nothing that a later step writes is read after this kernel: the copy to the host reads the slot only.
template <int KIND>
__global__ __launch_bounds__(kBlock) void k_frame_snapshot(Bodies cur, int64_t n, double max_speed, float *__restrict__ colors,
                                                           float *__restrict__ prev, void *__restrict__ first,
                                                           void *__restrict__ second, const TreeInfo *__restrict__ info,
                                                           const unsigned *__restrict__ sort_error,
                                                           FrameHeader *__restrict__ header,
                                                           const double *__restrict__ knn_r2 /* null: speed colours */,
                                                           const double *__restrict__ knn_mass, double rho_lo, double rho_hi) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r == 0) {
        header->error = info->error;
        header->sticky_error = info->sticky_error;
        header->max_run = info->max_run;
        header->sort_error = sort_error ? *sort_error : 0u;
        header->num_nodes = info->num_nodes;
        header->sticky_nodes = info->sticky_nodes;
    }
    if (r >= n) return;
    float c[3], p[3];
    if (knn_r2) color_density(knn_r2[r], knn_mass[r], rho_lo, rho_hi, c[0], c[1], c[2]);  // (k_colors_density's colours)
    else color_ramp(cur.vx[r], cur.vy[r], cur.vz[r], max_speed, c[0], c[1], c[2]);
    p[0] = (float)cur.x[r]; p[1] = (float)cur.y[r]; p[2] = (float)cur.z[r];
    const int64_t o = 3 * (int64_t)cur.id[r];
    for (int k = 0; k < 3; k++) colors[o + k] = c[k];
    if (KIND == NBMI_FRAME_DELTA_I16) {
        // `first` is the float32 staging row here: the quantisation against `prev` follows as k_frame_delta over the rows in
        // memory order.  (Quantising here, per body, was measured at 249 us for 1 M bodies and 2.95 ms for 10 M against
        // 65 / 565 us for the four kernels of the synchronous path: every access to prev and to the int16 rows is then a
        // scattered partial line, seven scattered streams instead of two.)
        float *fp = (float *)first;
        for (int k = 0; k < 3; k++) fp[o + k] = p[k];
    } else {
        float *fp = (float *)first, *fc = (float *)second;
        for (int k = 0; k < 3; k++) {
            fp[o + k] = p[k];
            fc[o + k] = c[k];
            if (KIND == NBMI_FRAME_KEY) {
                prev[o + k] = p[k];
                prev[3 * n + o + k] = c[k];
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_split_state(const double *__restrict__ pos, const double *__restrict__ vel,
                                                        const double *__restrict__ mass, Bodies cur, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    cur.x[i] = pos[3 * i]; cur.y[i] = pos[3 * i + 1]; cur.z[i] = pos[3 * i + 2];
    cur.vx[i] = vel[3 * i]; cur.vy[i] = vel[3 * i + 1]; cur.vz[i] = vel[3 * i + 2];
    if (mass) cur.m[i] = mass[i];
    cur.id[i] = (int32_t)i;
}
// like k_split_state but keeps the current ordering: row of body id[r] goes to rank r
__global__ __launch_bounds__(kBlock) void k_set_state_perm(const double *__restrict__ pos, const double *__restrict__ vel,
                                                           Bodies cur, int64_t n) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const int64_t i = cur.id[r];
    cur.x[r] = pos[3 * i]; cur.y[r] = pos[3 * i + 1]; cur.z[r] = pos[3 * i + 2];
    cur.vx[r] = vel[3 * i]; cur.vy[r] = vel[3 * i + 1]; cur.vz[r] = vel[3 * i + 2];
}
// the reference's octant digits back from the sort key: `levels` digits of (hi, lo) decoded (hilbert.h), the rest 0
__device__ __forceinline__ void octant_digits(uint64_t hi, uint64_t lo, int levels, uint64_t &ohi, uint64_t &olo) {
    unsigned st = 0u;
    ohi = 0ull; olo = 0ull;
    for (int l = 0; l < levels; l++) {
        const uint64_t w = l < 21 ? hi : lo;
        const unsigned d = (unsigned)(w >> (3 * (20 - (l < 21 ? l : l - 21)))) & 7u;
        const unsigned oct = (nbmi::kHilOctant[st] >> (3u * d)) & 7u;
        st = (unsigned)(nbmi::kHilNextByDigit[st] >> (5u * d)) & 31u;
        if (l < 21) ohi |= (uint64_t)oct << (3 * (20 - l));
        else olo |= (uint64_t)oct << (3 * (41 - l));
    }
}
// keys in the caller's body order; decode: as the reference's octant-path digits, else the raw sort keys
__global__ __launch_bounds__(kBlock) void k_keys_to_orig(const uint64_t *__restrict__ hi_s, const uint64_t *__restrict__ lo_s,
                                                         const uint32_t *__restrict__ perm, const int32_t *__restrict__ id,
                                                         int64_t n, int decode, uint64_t *__restrict__ out_hi,
                                                         uint64_t *__restrict__ out_lo) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const int64_t o = id[perm[r]];
    uint64_t h = hi_s[r], l = lo_s[r];
    if (decode) octant_digits(h, l, kMaxLevel, h, l);
    out_hi[o] = h;
    out_lo[o] = l;
}
__global__ __launch_bounds__(kBlock) void k_order(const uint32_t *__restrict__ perm, const int32_t *__restrict__ id,
                                                  int64_t n, int32_t *__restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r < n) out[r] = id[perm[r]];
}

__global__ __launch_bounds__(kBlock) void k_cells(const int32_t *__restrict__ node_ref, const uint8_t *__restrict__ node_level,
                                                  const uint64_t *__restrict__ hi_s, int64_t num_nodes, int decode,
                                                  int32_t *__restrict__ level, uint64_t *__restrict__ key) {
    const int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (u >= num_nodes) return;
    const int r = node_ref[u];  // first body of the node's range
    const int lev = node_level[u];
    level[u] = lev;
    uint64_t h = hi_s[r], l = 0ull;
    if (decode && lev <= 21) octant_digits(h, 0ull, lev, h, l);  // the cell's path in the reference's octant digits
    key[u] = lev <= 21 ? (lev == 0 ? 0ull : (h >> (63 - 3 * lev))) : ~0ull;
}
// multi-GPU row pack / unpack: {x,y,z,vx,vy,vz,m,id}
__global__ __launch_bounds__(kBlock) void k_pack_rows(Bodies cur, int64_t begin, int64_t end, double *__restrict__ rows) {
    const int64_t r = begin + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= end) return;
    double *o = rows + 8 * (r - begin);
    o[0] = cur.x[r]; o[1] = cur.y[r]; o[2] = cur.z[r];
    o[3] = cur.vx[r]; o[4] = cur.vy[r]; o[5] = cur.vz[r];
    o[6] = cur.m[r]; o[7] = (double)cur.id[r];
}
__global__ __launch_bounds__(kBlock) void k_unpack_rows(Bodies cur, int64_t begin, int64_t end, const double *__restrict__ rows) {
    const int64_t r = begin + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= end) return;
    const double *o = rows + 8 * (r - begin);
    cur.x[r] = o[0]; cur.y[r] = o[1]; cur.z[r] = o[2];
    cur.vx[r] = o[3]; cur.vy[r] = o[4]; cur.vz[r] = o[5];
    cur.m[r] = o[6]; cur.id[r] = (int32_t)o[7];
}

inline int nblocks(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }

}  // namespace

namespace {
// =========================================================================================
// Multi-GPU stage 2 ("owner mode"): every rank OWNS the bodies of one octant-key range, builds the octree
// of its own bodies inside the GLOBAL root cube and receives from every other rank only the part of that
// rank's tree its own bodies can open (a locally essential tree).  Kernels for: the key samples the
// splitters come from, the destination of every body, the body bounding box, and the extraction /
// appending of locally essential trees.  The collectives themselves are the host framework's (RCCL).
// =========================================================================================
constexpr int kMaxWorld = 64;
constexpr int kSampleCap = 4096;  // world x samples_per_rank, ranked in LDS

// `nvalid` regular samples of the (nearly key-ordered) local keys; the other slots are all ones (ignored: they sort to
// the very end).  [r3] A rank emits samples IN PROPORTION to the bodies it holds: with the same number from every rank
// the pooled samples describe "one W-th of the bodies per rank" whatever the ranks actually hold, equal quantiles then
// reproduce the current counts, and an imbalance, once there, stays (measured: 27 k ... 49 k bodies per rank after 500
// steps of a 300 k-body collision on 8 ranks).
__global__ __launch_bounds__(kBlock) void k_key_samples(const uint64_t *__restrict__ key_hi, int64_t n, int nsamples, int nvalid,
                                                        uint64_t *__restrict__ out) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= nsamples) return;
    out[k] = (n > 0 && k < nvalid) ? key_hi[(int64_t)((2 * (int64_t)k + 1) * n / (2 * (int64_t)nvalid))] : ~0ull;
}

// world - 1 splitters at equal quantiles of the valid samples: every sample finds its rank among all of them by
// counting (all samples in LDS, broadcast reads), and the ones whose rank is a quantile write themselves.
// Rank j owns the keys in [split[j-1], split[j]).  Any number of workgroups (one sample per thread).
__global__ __launch_bounds__(kBlock) void k_splitters(const uint64_t *__restrict__ samples, int total, int world,
                                                      uint64_t *__restrict__ split) {
    __shared__ uint64_t a[kSampleCap];
    __shared__ int s_valid;
    if (threadIdx.x == 0) s_valid = 0;
    __syncthreads();
    int cnt = 0;
    for (int i = threadIdx.x; i < total; i += kBlock) {
        const uint64_t v = samples[i];
        a[i] = v;
        cnt += v != ~0ull ? 1 : 0;
    }
    if (cnt) atomicAdd(&s_valid, cnt);
    __syncthreads();
    const int valid = s_valid;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (valid == 0) {
        if (i < world - 1) split[i] = ~0ull;
        return;
    }
    if (i >= total) return;
    const uint64_t x = a[i];
    if (x == ~0ull) return;
    int rank = 0;
#pragma unroll 16
    for (int j = 0; j < total; j++) {
        const uint64_t y = a[j];
        rank += (y < x || (y == x && j < i)) ? 1 : 0;
    }
    for (int j = 0; j < world - 1; j++)
        if ((int)((int64_t)(j + 1) * valid / world) == rank) split[j] = x;
}

// destination rank of every body: number of splitters <= its upper key word (bodies that agree on all 21
// upper digits always travel together)
__global__ __launch_bounds__(kBlock) void k_dest(const uint64_t *__restrict__ key_hi, int64_t n, const uint64_t *__restrict__ split,
                                                 int world, uint32_t *__restrict__ dest, uint32_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = key_hi[i];
    int lo = 0, hi = world - 1;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (split[mid] <= k) lo = mid + 1; else hi = mid; }
    dest[i] = (uint32_t)lo;
    idx[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kBlock) void k_dead_flags(const uint8_t *__restrict__ dead, int64_t n, int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) flag[i] = dead[i] ? 1 : 0;
}
// owner mode, migration: flag row j of destination d = 1 if body i goes to rank d (d != me); dead[i] = leaves
__global__ __launch_bounds__(kBlock) void k_emigrant_flags(const uint32_t *__restrict__ dest, int64_t n, int world, int me,
                                                           int64_t stride, int32_t *__restrict__ flag, uint8_t *__restrict__ dead) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int d = (int)dest[i];
    for (int j = 0; j < world; j++) flag[(int64_t)j * stride + i] = (j == d && j != me) ? 1 : 0;
    dead[i] = d != me ? 1 : 0;
}
// emigrants' rows, grouped by destination (segment offsets from k_let_counts), current order inside a group
__global__ __launch_bounds__(kBlock) void k_pack_emigrants(Bodies cur, const uint32_t *__restrict__ dest, int64_t n, int me,
                                                           int64_t stride, const int32_t *__restrict__ slot,
                                                           const int64_t *__restrict__ seg_off, double *__restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int d = (int)dest[i];
    if (d == me) return;
    double *o = rows + 8 * (seg_off[d] + slot[(int64_t)d * stride + i]);
    o[0] = cur.x[i]; o[1] = cur.y[i]; o[2] = cur.z[i];
    o[3] = cur.vx[i]; o[4] = cur.vy[i]; o[5] = cur.vz[i];
    o[6] = cur.m[i]; o[7] = (double)cur.id[i];
}

// Where a rank's bodies are, for the pruning of the trees the others send it: tight bounding boxes of the
// bodies inside octree cells of the rank's OWN tree - the cells of level kBoxLevel, refined down to
// kBoxLevelMax along the two cells that hold the rank's first and last body (a rank's key range ends in the
// middle of cells; unrefined, those two boxes would overlap the neighbours' whole working set).  (Bounding
// boxes of equal chunks of the key order do not work: a chunk that crosses a high-level cell boundary spans
// two distant corners of the system, and one such box keeps everything alive.)  The boxes come out in key
// order (slot = exclusive scan of the emit flags over the pre-order array), so every kSuper consecutive ones
// are neighbours in space and get a common "super box" for a two-level test.
constexpr int kChainLevels = 43;  // cell levels 0 .. 42 (21 digits of the upper key word, 21 of the lower)
constexpr int kBoxLevel = 4, kBoxLevelMax = 11;
constexpr int kBoxesPerRank = 2048, kSuper = 32, kSupersPerRank = kBoxesPerRank / kSuper;
constexpr int kMegasPerRank = 8, kSupersPerMega = kSupersPerRank / kMegasPerRank;

// flag[i] = 1 if node i is one of the cells / leaves whose bodies get a box
__global__ __launch_bounds__(kBlock) void k_box_flags(const Node *__restrict__ nodes, const uint8_t *__restrict__ node_level,
                                                      const int32_t *__restrict__ node_ref, const uint64_t *__restrict__ hi_s,
                                                      const uint64_t *__restrict__ lo_s, const TreeInfo *__restrict__ info,
                                                      int64_t n, int64_t rows, int32_t *__restrict__ flag,
                                                      int32_t *__restrict__ chainR, int64_t link_base) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= rows) return;  // the grid is rounded up to whole blocks: nothing behind the row budget is written
    const int64_t num_nodes = info->error ? 0 : info->num_nodes;
    if (i >= num_nodes) {
        flag[i] = 0;  // launched for the row budget: rows behind the tree count nothing
        return;
    }
    const int l = node_level[i];
    int f = 0;
    {   // [r3] the cells whose subtree ends with the array hold the rank's last body: one per level (k_chain_table)
        const Node nd = nodes[i];
        if (__float_as_int(nd.s2t) != 0 && (int64_t)(nd.next_off / kNodeBytes) - link_base == num_nodes && l < kChainLevels) chainR[l] = (int32_t)i;
    }
    if (l <= kBoxLevelMax) {
        const Node nd = nodes[i];
        const bool leaf = __float_as_int(nd.s2t) == 0;
        const int64_t a = node_ref[i];
        const int64_t nx = (int64_t)(nd.next_off / kNodeBytes) - link_base;
        const int64_t b = nx < num_nodes ? node_ref[nx] : n;
        const bool boundary = a == 0 || b == n;  // holds the rank's first or last body
        if (l < kBoxLevel) {
            f = leaf ? 1 : 0;
        } else if (l == kBoxLevel) {
            f = (!boundary || leaf) ? 1 : 0;
        } else {
            // only below the two boundary chains: the parent (level l - 1) holds body 0 or body n - 1
            const uint64_t h = hi_s[a], lo = lo_s[a];
            const bool under = cpl_digits(h, lo, hi_s[0], lo_s[0]) >= l - 1 || cpl_digits(h, lo, hi_s[n - 1], lo_s[n - 1]) >= l - 1;
            f = (under && (!boundary || leaf || l == kBoxLevelMax)) ? 1 : 0;
        }
    }
    flag[i] = f;
}
// body ranges of the flagged nodes, in key order
__global__ __launch_bounds__(kBlock) void k_box_ranges(const Node *__restrict__ nodes, const int32_t *__restrict__ node_ref,
                                                       const int32_t *__restrict__ flag, const int32_t *__restrict__ slot,
                                                       const TreeInfo *__restrict__ info, int64_t rows, int64_t n,
                                                       int32_t *__restrict__ ranges /* 2 x kBoxesPerRank */, int64_t link_base) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t num_nodes = info->error ? 0 : info->num_nodes;
    if (i >= num_nodes || !flag[i]) return;
    const int k = slot[i];
    if (k >= kBoxesPerRank) return;  // more cells than boxes: the last box takes everything from its cell on
    const int64_t nx = (int64_t)(nodes[i].next_off / kNodeBytes) - link_base;
    ranges[2 * k] = node_ref[i];
    ranges[2 * k + 1] = (k == kBoxesPerRank - 1 && slot[rows] > kBoxesPerRank) ? (int32_t)n
                                                                                    : (int32_t)(nx < num_nodes ? node_ref[nx] : n);
}
// tight bounding boxes of the bodies of every range (empty box: lo = +inf > hi = -inf).  The ranges are
// consecutive in key order and very unequal (a level-4 cell of a galaxy core holds 10^5 bodies, a refined
// boundary cell a handful), so the work is cut by BODIES: a wave takes kBoxChunk consecutive bodies, finds the
// ranges that overlap them and adds its part of each with float64 atomic min / max.
constexpr int kBoxChunk = 1024;
__global__ void k_boxes_init(double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 6 * kBoxesPerRank) out[i] = (i % 6) < 3 ? INFINITY : -INFINITY;
}
__global__ __launch_bounds__(kBlock) void k_range_boxes(const double4 *__restrict__ p64_s, const int32_t *__restrict__ ranges,
                                                        const int32_t *__restrict__ total, int64_t n, double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t c0 = wave * kBoxChunk, c1 = c0 + kBoxChunk < n ? c0 + kBoxChunk : n;
    if (c0 >= n) return;
    const int nb = *total < kBoxesPerRank ? *total : kBoxesPerRank;
    int lo = 0, hi = nb;  // first range that ends behind c0
    while (lo < hi) { const int mid = (lo + hi) >> 1; if ((int64_t)ranges[2 * mid + 1] > c0) hi = mid; else lo = mid + 1; }
    for (int k = lo; k < nb; k++) {
        const int64_t r0 = ranges[2 * k], r1 = ranges[2 * k + 1];
        if (r0 >= c1) break;
        const int64_t a = r0 > c0 ? r0 : c0, b = r1 < c1 ? r1 : c1;
        double v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (int64_t i = a + lane; i < b; i += 64) {
            const double4 q = p64_s[i];
            v[0] = fmin(v[0], q.x); v[1] = fmin(v[1], q.y); v[2] = fmin(v[2], q.z);
            v[3] = fmax(v[3], q.x); v[4] = fmax(v[4], q.y); v[5] = fmax(v[5], q.z);
        }
#pragma unroll
        for (int c = 0; c < 6; c++) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double t = __shfl_xor(v[c], o);
                v[c] = c < 3 ? fmin(v[c], t) : fmax(v[c], t);
            }
        }
        if (lane < 6 && a < b) {
            double r = v[0];
#pragma unroll
            for (int c = 1; c < 6; c++) r = lane == c ? v[c] : r;
            if (lane < 3) atomicMin(&out[6 * k + lane], r);
            else atomicMax(&out[6 * k + lane], r);
        }
    }
}
// super box = union of kSuper consecutive boxes (of every rank)
__global__ void k_super_boxes(const double *__restrict__ boxes, int nsupers, double *__restrict__ supers) {
    const int sidx = blockIdx.x * blockDim.x + threadIdx.x;
    if (sidx >= nsupers) return;
    double v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < kSuper; k++) {
        const double *b = boxes + 6 * ((int64_t)sidx * kSuper + k);
        if (!(b[0] <= b[3])) continue;
        for (int c = 0; c < 3; c++) { v[c] = fmin(v[c], b[c]); v[3 + c] = fmax(v[3 + c], b[3 + c]); }
    }
    for (int c = 0; c < 6; c++) supers[6 * sidx + c] = v[c];
}

// ---- plain int32 exclusive scan (three phases: tile sums, scan::k_scan_values over them, apply); blockIdx.y selects
// one of several equally long arrays `stride` elements apart (one per destination rank) -------------------
__global__ __launch_bounds__(kBlock) void k_iscan_reduce(const int32_t *__restrict__ in, int64_t n, int64_t stride,
                                                         int32_t *__restrict__ tile_sum, int64_t tstride) {
    in += (int64_t)blockIdx.y * stride;
    tile_sum += (int64_t)blockIdx.y * tstride;
    const int64_t base = (int64_t)blockIdx.x * kScanTile;
    int acc = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        const int64_t i = base + (int64_t)k * kBlock + threadIdx.x;
        acc += i < n ? in[i] : 0;
    }
    const int total = scan::block_scan<kBlock>(acc, 0, scan::Sum()).total;
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}
// out[i] = sum of in[0..i); entry n receives the total
__global__ __launch_bounds__(kBlock) void k_iscan_apply(const int32_t *__restrict__ in, int64_t n, int64_t stride,
                                                        const int32_t *__restrict__ tile_off, int64_t tstride,
                                                        int32_t *__restrict__ out) {
    in += (int64_t)blockIdx.y * stride;
    out += (int64_t)blockIdx.y * stride;
    tile_off += (int64_t)blockIdx.y * tstride;
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    int v[kScanItems], sum = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) { v[k] = base + k < n ? in[base + k] : 0; sum += v[k]; }
    int run = scan::block_scan<kBlock>(sum, tile_off[blockIdx.x], scan::Sum()).excl;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        if (base + k <= n) out[base + k] = run;
        run += v[k];
    }
}

// ---- locally essential tree -----------------------------------------------------------------
// [r3] One GLOBAL octree, cut into the ranks' pieces.  A rank's build (k_emit_tile) makes the octree of its own
// bodies; the octree of ALL bodies differs from the ranks' trees side by side only along the rank boundaries:
//   * cells that contain a rank's last body AND bodies of higher ranks: one cell in the global tree (first body on
//     some rank A, the "owner"), a partial copy in every rank it reaches into;
//   * cells that exist only because a rank's last body and the next rank's first body share more key digits than
//     either shares with its neighbour on its own rank ("boundary-born" cells).
// Round 2 walked the partial copies as they were - valid Barnes-Hut, but a DIFFERENT approximation than the
// single-GPU tree: 2e-6 of the largest coordinate after 10 steps, 1.2e-4 after 50, 1.7e-3 after 100 at 1 M bodies
// on 8 ranks, whatever the force precision (profiles/r03_owner_100_steps.jsonl).  Now every rank publishes a small
// table about its two ends (ChainTable, all-gathered with the bounding boxes), and k_chain_fix turns the own tree
// into the rank's piece of the global pre-order array:
//   * the copies of cells that begin on a lower rank (always the FIRST own_skip nodes of the array) are dropped;
//   * the cells along the path to the last body that reach into higher ranks get the global moments, the
//     boundary-born ones are inserted in front of the last leaf (the last node of the array: nothing moves);
//   * skip links that leave the rank name (rank, node) and are resolved where the pieces are put together.
// Concatenated in rank order the pieces ARE the global pre-order array: every rank walks its own piece in full and a
// pruned copy of the others', in rank order, i.e. the reference's accepted sets in the reference's order.
constexpr unsigned kLinkTag = 0xFFFFFF00u;  // next_off >= this: a link that leaves the rank, slot = low byte (k_chain_fix)
constexpr int kLinkEnd = 0xFE, kLinkLocal = 0xFF;
struct ChainTable {
    long long n;       // bodies of the rank (0: every other field is meaningless)
    long long nodes;   // nodes of its tree as built (before k_chain_fix)
    unsigned long long first_hi, first_lo, last_hi, last_lo;  // keys of its first / last body
    long long d0, dR;  // common key digits of its first two / last two bodies (-1: a single body)
    // level by level: how many of the rank's FIRST bodies share `level` digits with its first body (Lc), the node
    // behind them in the rank's array (Ln; = nodes if all do) and their moments (Ls); the same from the end (Rc, Rs)
    long long Lc[kChainLevels], Ln[kChainLevels], Rc[kChainLevels];
    double Ls[kChainLevels][4], Rs[kChainLevels][4];
};
static_assert(sizeof(ChainTable) % 8 == 0, "ChainTable travels as doubles");
constexpr int kChainDoubles = (int)(sizeof(ChainTable) / 8);

__device__ __forceinline__ int chain_prev(const ChainTable *T, int x) {
    for (int p = x - 1; p >= 0; p--) if (T[p].n > 0) return p;
    return -1;
}
__device__ __forceinline__ int chain_next(const ChainTable *T, int W, int x) {
    for (int z = x + 1; z < W; z++) if (T[z].n > 0) return z;
    return -1;
}
// key digits the last body of rank x shares with the first body of rank y
__device__ __forceinline__ int chain_cpl(const ChainTable *T, int x, int y) {
    return cpl_digits(T[x].last_hi, T[x].last_lo, T[y].first_hi, T[y].first_lo);
}
// how many of rank x's first nodes are copies of cells that begin on a lower rank
__device__ __forceinline__ int chain_skip(const ChainTable *T, int x) {
    const int p = chain_prev(T, x);
    if (p < 0) return 0;
    const int db = chain_cpl(T, p, x), d0 = (int)T[x].d0;
    return (db < d0 ? db : d0) + 1;
}
struct ChainCell {
    double M, mx, my, mz;
    int link_rank;        // rank on which the cell's subtree ends (kLinkEnd: with the last body of the last rank)
    long long link_node;  // ... and the node (in that rank's numbering as built) that follows it
};
// The level-`lev` cell that holds the LAST body of rank x and reaches into the next rank.  The same function with
// the same gathered tables on every rank that needs the cell (its owner for the record, the ranks it reaches into
// for their pruning decisions): bit-identical moments everywhere.
__device__ ChainCell chain_cell(const ChainTable *T, int W, int x, int lev) {
    int a = x;  // the owner: leftwards while the whole rank lies inside the cell and the cell comes from further left
    while (T[a].Rc[lev] == T[a].n) {
        const int p = chain_prev(T, a);
        if (p < 0 || chain_cpl(T, p, a) < lev) break;
        a = p;
    }
    ChainCell c;
    c.M = T[a].Rs[lev][0]; c.mx = T[a].Rs[lev][1]; c.my = T[a].Rs[lev][2]; c.mz = T[a].Rs[lev][3];
    int y = a;
    for (;;) {
        const int z = chain_next(T, W, y);
        if (z < 0) { c.link_rank = kLinkEnd; c.link_node = 0; break; }
        if (chain_cpl(T, y, z) < lev) { c.link_rank = z; c.link_node = chain_skip(T, z); break; }
        c.M += T[z].Ls[lev][0]; c.mx += T[z].Ls[lev][1]; c.my += T[z].Ls[lev][2]; c.mz += T[z].Ls[lev][3];
        if (T[z].Lc[lev] < T[z].n) { c.link_rank = z; c.link_node = T[z].Ln[lev]; break; }
        y = z;
    }
    return c;
}
// what follows a rank's last leaf in the global array: the first node the next rank keeps
__device__ __forceinline__ void chain_after(const ChainTable *T, int W, int x, int &link_rank, long long &link_node) {
    const int z = chain_next(T, W, x);
    link_rank = z < 0 ? kLinkEnd : z;
    link_node = z < 0 ? 0 : chain_skip(T, z);
}

// the rank's table (one wave, lane = level).  chainR[l] = node of the level-l cell that holds the last body
// (k_box_flags notes them: the cells whose subtree ends with the array).
__global__ void k_chain_table(const Node *__restrict__ nodes, const int32_t *__restrict__ node_ref, const int32_t *__restrict__ delta,
                              const double4 *__restrict__ S, const Moment *__restrict__ T, const uint64_t *__restrict__ hi_s,
                              const uint64_t *__restrict__ lo_s, int64_t n, const TreeInfo *__restrict__ info,
                              const int32_t *__restrict__ chainR, int64_t link_base, ChainTable *__restrict__ out) {
    const int lev = threadIdx.x;
    const int64_t N = info->error ? 0 : info->num_nodes;
    if (N == 0) n = 0;  // (a build that overflowed: the rank takes no part in this step's global tree; the error is sticky)
    const int d0 = n >= 2 ? delta[0] : -1, dR = n >= 2 ? delta[n - 2] : -1;
    if (lev == 0) {
        out->n = n; out->nodes = N;
        out->first_hi = n > 0 ? hi_s[0] : 0; out->first_lo = n > 0 ? lo_s[0] : 0;
        out->last_hi = n > 0 ? hi_s[n - 1] : 0; out->last_lo = n > 0 ? lo_s[n - 1] : 0;
        out->d0 = d0; out->dR = dR;
    }
    if (lev >= kChainLevels || n == 0) return;
    int64_t Lc, Ln, Rc;
    if (lev <= d0) {  // node `lev` is the level-lev cell of the first body (its cells are the first nodes of the array)
        const int64_t nx = (int64_t)(nodes[lev].next_off / kNodeBytes) - link_base;
        Lc = nx < N ? node_ref[nx] : n;
        Ln = nx;
    } else {
        Lc = 1;
        Ln = n >= 2 ? d0 + 2 : N;
    }
    if (lev <= dR) Rc = n - node_ref[chainR[lev]];
    else Rc = 1;
    out->Lc[lev] = Lc; out->Ln[lev] = Ln; out->Rc[lev] = Rc;
    double M, mx, my, mz;
    range_moments(S, T, 0, Lc, M, mx, my, mz);
    out->Ls[lev][0] = M; out->Ls[lev][1] = mx; out->Ls[lev][2] = my; out->Ls[lev][3] = mz;
    range_moments(S, T, n - Rc, n, M, mx, my, mz);
    out->Rs[lev][0] = M; out->Rs[lev][1] = mx; out->Rs[lev][2] = my; out->Rs[lev][3] = mz;
}

struct OwnLink { int node; int rank; long long target; };  // node of the own array, (rank, node there) it links to
constexpr int kOwnLinks = kChainLevels + 1;                  // a slot per level, one for the last leaf

// The own tree becomes the rank's piece of the global array (see above).  One workgroup of 64, lane = level.
__global__ void k_chain_fix(const ChainTable *__restrict__ T, int W, int me, Node *__restrict__ nodes, Node64 *__restrict__ n64,
                            NodeD *__restrict__ nodesd, uint8_t *__restrict__ node_level, int32_t *__restrict__ node_ref,
                            const int32_t *__restrict__ chainR, double inv_theta2, int64_t capacity, OwnLink *__restrict__ links,
                            TreeInfo *info) {
    const int lev = threadIdx.x;
    const ChainTable &t = T[me];
    const int64_t n = t.n, N = t.nodes;
    if (lev < kOwnLinks) links[lev] = OwnLink{-1, 0, 0};
    if (n == 0 || info->error) {
        if (lev == 0) { info->own_skip = 0; info->own_added = 0; }
        return;
    }
    const int p = chain_prev(T, me), z = chain_next(T, W, me);
    const int dprev = p >= 0 ? chain_cpl(T, p, me) : -1, dnext = z >= 0 ? chain_cpl(T, me, z) : -1;
    const int dR = (int)t.dR;
    const int lo_new = n == 1 ? (dprev > dR ? dprev : dR) : dR;  // levels above this one and up to dnext are boundary-born
    const int c = dnext > lo_new ? dnext - lo_new : 0;
    if (N + c + 1 > capacity) {
        if (lev == 0) {
            info->error = 1;
            if (info->sticky_error == 0) { info->sticky_error = 1; info->sticky_nodes = N + c; }
        }
        return;
    }
    // the last leaf first (the new cells take its place)
    const Node leaf = nodes[N - 1];
    const uint8_t leaf_level = node_level[N - 1];
    NodeD leafd = NodeD{0.0, 0.0, 0.0, 0.0, 0.0f, 0u};
    if (nodesd) leafd = nodesd[N - 1];
    __syncthreads();
    const bool exists = lev < kChainLevels && lev <= dR, born = lev < kChainLevels && lev > lo_new && lev <= dnext;
    if (exists || born) {
        const int64_t i = exists ? chainR[lev] : (N - 1) + (lev - lo_new - 1);
        const bool from_left = t.Rc[lev] == n && dprev >= lev;  // begins on a lower rank: that rank's to describe
        if (!from_left) {
            int lr; long long ln;
            if (lev <= dnext) {
                const ChainCell cc = chain_cell(T, W, me, lev);
                lr = cc.link_rank; ln = cc.link_node;
                double cx = 0.0, cy = 0.0, cz = 0.0;
                if (cc.M > 0.0) { cx = cc.mx / cc.M; cy = cc.my / cc.M; cz = cc.mz / cc.M; }
                const double bounds = info->bounds;
                const double size = ldexp(bounds, 1 - lev);
                const float s2t = (float)(size * size * inv_theta2);
                Node nd;
                nd.cx = (float)cx; nd.cy = (float)cy; nd.cz = (float)cz; nd.gm = (float)cc.M;
                nd.s2t = __int_as_float(__float_as_int(s2t) + (int)(info->band2 >> 1));
                nd.next_off = kLinkTag | (unsigned)lev;
                nodes[i] = nd;
                n64[i] = Node64{cx, cy, cz, ldexp(bounds, -lev)};
                if (nodesd) nodesd[i] = NodeD{cx, cy, cz, cc.M, __int_as_float(__float_as_int(s2t) + (int)kBand64), kLinkTag | (unsigned)lev};
                if (born) { node_level[i] = (uint8_t)lev; node_ref[i] = (int32_t)(n - 1); }
            } else {  // ends with the rank's last body: only its skip link leaves the rank
                chain_after(T, W, me, lr, ln);
                nodes[i].next_off = kLinkTag | (unsigned)lev;
                if (nodesd) nodesd[i].next_off = kLinkTag | (unsigned)lev;
            }
            links[lev] = OwnLink{(int)i, lr, ln};
        }
    }
    if (lev == kChainLevels) {  // the last leaf, behind the boundary-born cells
        const int64_t i = N - 1 + c;
        Node lf = leaf;
        lf.next_off = kLinkTag | (unsigned)kChainLevels;
        nodes[i] = lf;
        if (nodesd) { leafd.next_off = kLinkTag | (unsigned)kChainLevels; nodesd[i] = leafd; }
        node_ref[i] = (int32_t)(n - 1);
        node_level[i] = leaf_level + (uint8_t)c;
        int lr; long long ln;
        chain_after(T, W, me, lr, ln);
        links[kChainLevels] = OwnLink{(int)i, lr, ln};
        info->num_nodes = N + c;
        info->own_skip = chain_skip(T, me);
        info->own_added = c;
    }
}

// A cell can only be opened by a body of another rank if the opening test can fail somewhere in one of that
// rank's bounding boxes; if it cannot (for any other rank), nobody else ever looks below it and its subtree
// stays home.  Conservative by a 1e-9 margin on both sides of the float64 test.  diff[] marks the dropped
// pre-order ranges (+1 at the first node of the subtree, -1 behind it): a node is kept iff the running sum
// over diff up to and including it is zero.
__device__ __forceinline__ bool box_may_open(const double *__restrict__ b, const Node64 &c, double eps2, double thr) {
    if (!(b[0] <= b[3])) return false;  // empty
    const double dx = fmax(0.0, fmax(b[0] - c.cx, c.cx - b[3]));
    const double dy = fmax(0.0, fmax(b[1] - c.cy, c.cy - b[4]));
    const double dz = fmax(0.0, fmax(b[2] - c.cz, c.cz - b[5]));
    return (dx * dx + dy * dy + dz * dz + eps2) * (1.0 - 1e-9) <= thr;  // some point of the box may fail "size / dist < theta"
}
// may a body of rank j open the cell?  Four-level test: the union box of the rank, its mega boxes, super boxes, boxes.
__device__ __forceinline__ bool rank_may_open(int j, const Node64 &c, double eps2, double thr, const double *__restrict__ boxes,
                                              const double *__restrict__ supers, const double *__restrict__ megas,
                                              const double *__restrict__ rankbox) {
    if (!box_may_open(rankbox + 6 * j, c, eps2, thr)) return false;
    for (int g = j * kMegasPerRank; g < (j + 1) * kMegasPerRank; g++) {
        if (!box_may_open(megas + 6 * g, c, eps2, thr)) continue;
        for (int sb = g * kSupersPerMega; sb < (g + 1) * kSupersPerMega; sb++) {
            if (!box_may_open(supers + 6 * sb, c, eps2, thr)) continue;
            for (int k = 0; k < kSuper; k++)
                if (box_may_open(boxes + 6 * ((int64_t)sb * kSuper + k), c, eps2, thr)) return true;
        }
    }
    return false;
}
// one pass over the own tree decides for EVERY destination rank: diff row j marks the pre-order ranges rank j
// does not need.
__global__ __launch_bounds__(kBlock) void k_let_mark(const Node *__restrict__ nodes, const Node64 *__restrict__ n64,
                                                     int64_t num_nodes, const double *__restrict__ boxes,
                                                     const double *__restrict__ supers, const double *__restrict__ megas,
                                                     const double *__restrict__ rankbox, int world, int me, double theta, double eps2,
                                                     int32_t *__restrict__ diff, int64_t stride, const TreeInfo *__restrict__ info,
                                                     int64_t link_base) {
    // (a wave-uniform form of these loops - a level entered if ANY lane needs it, box data by scalar loads -
    // was slower, 266 vs 190 us at 8 ranks: the lanes' early exits are worth more than the cheaper loads)
    // `num_nodes` is the host's launch bound (it may be an estimate from the previous step); the tree's own count is
    // on the device
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t N = info->num_nodes;
    if (i >= num_nodes || i >= N || i < info->own_skip) return;  // (the first own_skip nodes: k_let_mark_left speaks for them)
    const Node nd = nodes[i];
    if (__float_as_int(nd.s2t) == 0) return;  // a leaf: nothing below it
    const Node64 c = n64[i];
    const double size = c.hs * 2.0;
    const bool all = !(theta > 0.0);  // theta == 0: every cell is opened by everybody
    const double thr = all ? 0.0 : (size / theta) * (size / theta) * (1.0 + 1e-9);
    const int64_t nx = nd.next_off >= kLinkTag ? N : (int64_t)(nd.next_off / kNodeBytes) - link_base;  // (a subtree that leaves the rank: to the end of the array)
    if (nx <= i + 1) return;
    // [r4] A cell whose PARENT no body of rank j can open lies inside the range the parent drops for j: it has nothing to
    // add (13 of 14 marks of a deep cell were of that kind: two atomics each).  The parent is the cube of edge 2 size around
    // this cell; its centre of mass and ours both lie in it, at most its diagonal 2 sqrt(3) size apart, so every point b of
    // rank j's box is at least d(b, our centre of mass) - 2 sqrt(3) size from the parent's: the parent passes the opening
    // test for all of rank j when d^2 > reach^2.  (Skipping a mark can only keep a node that could have been dropped -
    // the exported piece stays correct whatever this test does; the parent's own test is the exact one.)
    const double far = sqrt(fmax(0.0, 4.0 * thr * (1.0 + 1e-6) - eps2)) + 3.4642 * size;
    const double reach2 = i > 0 ? far * far : INFINITY;
    for (int j = 0; j < world; j++) {
        if (j == me) continue;
        if (!all) {
            const double *rb = rankbox + 6 * j;
            if (rb[0] <= rb[3]) {
                const double dx = fmax(0.0, fmax(rb[0] - c.cx, c.cx - rb[3])), dy = fmax(0.0, fmax(rb[1] - c.cy, c.cy - rb[4])),
                             dz = fmax(0.0, fmax(rb[2] - c.cz, c.cz - rb[5]));
                if (dx * dx + dy * dy + dz * dz > reach2) continue;
            }
        }
        if (!all && !rank_may_open(j, c, eps2, thr, boxes, supers, megas, rankbox)) {
            int32_t *d = diff + (int64_t)j * stride;
            atomicAdd(&d[i + 1], 1);
            atomicAdd(&d[nx], -1);
        }
    }
}
// The cells that begin on a lower rank and reach into this one: their owner decides with the global moments whether
// a destination needs their subtree; this rank takes the same decision from the same numbers (chain_cell) for the
// part of the subtree that lies in ITS array: nodes [0, Ln[level]).  One wave per destination rank, lane = level.
__global__ void k_let_mark_left(const ChainTable *__restrict__ T, int world, int me, const double *__restrict__ boxes,
                                const double *__restrict__ supers, const double *__restrict__ megas,
                                const double *__restrict__ rankbox, double theta, double eps2, int32_t *__restrict__ diff,
                                int64_t stride, const TreeInfo *__restrict__ info) {
    const int lev = threadIdx.x;
    const ChainTable &t = T[me];
    if (lev >= kChainLevels || t.n == 0 || info->error) return;
    const int p = chain_prev(T, me);
    if (p < 0 || chain_cpl(T, p, me) < lev) return;
    if (!(theta > 0.0)) return;  // everybody opens everything
    const ChainCell cc = chain_cell(T, world, p, lev);
    Node64 c{0.0, 0.0, 0.0, ldexp(info->bounds, -lev)};
    if (cc.M > 0.0) { c.cx = cc.mx / cc.M; c.cy = cc.my / cc.M; c.cz = cc.mz / cc.M; }
    const double size = c.hs * 2.0;
    const double thr = (size / theta) * (size / theta) * (1.0 + 1e-9);
    const int64_t end = t.Lc[lev] < t.n ? t.Ln[lev] : info->num_nodes;
    const int j = blockIdx.x;
    if (j == me) return;
    if (!rank_may_open(j, c, eps2, thr, boxes, supers, megas, rankbox)) {
        int32_t *d = diff + (int64_t)j * stride;
        atomicAdd(&d[0], 1);
        atomicAdd(&d[end], -1);
    }
}
__global__ __launch_bounds__(kBlock) void k_let_keep(const int32_t *__restrict__ diff, const int32_t *__restrict__ diff_ex,
                                                     int64_t num_nodes, int64_t stride, int32_t *__restrict__ keep,
                                                     const TreeInfo *__restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t o = (int64_t)blockIdx.y * stride;
    if (i < num_nodes) keep[o + i] = (i >= info->own_skip && i < info->num_nodes && (diff_ex[o + i] + diff[o + i]) == 0) ? 1 : 0;
}
// kept nodes move to their new index in the destination's segment; links are re-based to the compacted
// numbering (a kept node's successor is always kept: it hangs off one of the node's own ancestors - on whichever
// rank that is: all ranks decide about a cell from the same numbers).  A row of the exchange buffer is 48 bytes,
// everything in float64 (LetRow): the receiver rounds the fp32 walk record out of it exactly as the sender's build
// did, and rebuilds the float64 record of the float64 force loop from the same numbers ([r3]; round 2 shipped the
// 24-byte fp32 record + a 32-byte float64 twin and owner mode had fp32 forces only).
struct LetRow {
    double cx, cy, cz, gm;  // centre of mass / body position, G * mass
    float s2t;              // as in Node (the fp32 loop's band included; 0: a leaf)
    unsigned next;          // skip link: node index in the compacted segment (link_rank = kLinkLocal), or the node of
                            // rank link_rank (in that rank's numbering behind ITS dropped copies) that follows the subtree
    unsigned orig;          // the node's index in the sender's array, behind the sender's dropped copies
    uint8_t level;          // cell level (half size = root half size / 2^level)
    uint8_t link_rank;
    uint16_t pad;
};
static_assert(sizeof(LetRow) == 48, "LetRow is a 48-byte wire row");
constexpr int kLetRow = 48;
__global__ __launch_bounds__(kBlock) void k_let_compact(const Node *__restrict__ nodes, const Node64 *__restrict__ n64,
                                                        const NodeD *__restrict__ nodesd /* may be null */,
                                                        const uint8_t *__restrict__ node_level, const OwnLink *__restrict__ links,
                                                        const ChainTable *__restrict__ T,
                                                        const int32_t *__restrict__ keep, const int32_t *__restrict__ newidx,
                                                        int64_t num_nodes, int64_t stride, int64_t capacity, int me,
                                                        const int64_t *__restrict__ seg_off, char *__restrict__ out,
                                                        const TreeInfo *__restrict__ info, int64_t link_base) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int j = blockIdx.y;
    if (j == me || i >= num_nodes || i >= info->num_nodes) return;
    const int64_t o = (int64_t)j * stride;
    if (!keep[o + i]) return;
    const int64_t k = seg_off[j] + newidx[o + i];
    if (k >= capacity) return;  // reported through the counts
    const Node nd = nodes[i];
    const bool leaf = __float_as_int(nd.s2t) == 0;
    LetRow row;
    row.s2t = nd.s2t;
    row.orig = (unsigned)(i - info->own_skip);
    row.level = node_level[i];
    row.pad = 0;
    if (nd.next_off >= kLinkTag) {
        const OwnLink L = links[nd.next_off & 0xffu];
        row.link_rank = (uint8_t)L.rank;
        row.next = L.rank == kLinkEnd ? 0u : (unsigned)(L.target - chain_skip(T, L.rank));
    } else {
        row.link_rank = (uint8_t)kLinkLocal;
        row.next = (unsigned)newidx[o + (int64_t)(nd.next_off / kNodeBytes) - link_base];
    }
    if (nodesd) {  // the float64 record has the unrounded numbers of leaves and cells alike
        const NodeD d = nodesd[i];
        row.cx = d.cx; row.cy = d.cy; row.cz = d.cz; row.gm = d.gm;
    } else if (!leaf) {
        const Node64 c = n64[i];
        row.cx = c.cx; row.cy = c.cy; row.cz = c.cz; row.gm = (double)nd.gm;
    } else {  // an fp32-only handle keeps no float64 copy of a leaf
        row.cx = (double)nd.cx; row.cy = (double)nd.cy; row.cz = (double)nd.cz; row.gm = (double)nd.gm;
    }
    *reinterpret_cast<LetRow *>(out + k * kLetRow) = row;
}
// rows per destination and where each destination's segment starts in the (packed) send buffer
__global__ void k_let_counts(const int32_t *__restrict__ newidx, int64_t num_nodes, int64_t stride, int world, int me,
                             int64_t *__restrict__ counts /* [world] counts, then [world] offsets */) {
    if (threadIdx.x != 0) return;
    int64_t off = 0;
    for (int j = 0; j < world; j++) {
        const int64_t c = j == me ? 0 : newidx[(int64_t)j * stride + num_nodes];
        counts[j] = c;
        counts[world + j] = off;
        off += c;
    }
}
// two more levels above the super boxes: kMegasPerRank "mega boxes" (kSupersPerMega consecutive super boxes each)
// and the union box of the rank.  One workgroup, one thread per mega box.
__global__ __launch_bounds__(kMaxWorld * kMegasPerRank) void k_rank_boxes(const double *__restrict__ supers, int world,
                                                                          double *__restrict__ megas, double *__restrict__ rankbox) {
    __shared__ double m[kMaxWorld * kMegasPerRank][6];
    const int t = threadIdx.x, j = t / kMegasPerRank;
    double v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (j < world) {
        for (int k = 0; k < kSupersPerMega; k++) {
            const double *b = supers + 6 * ((int64_t)t * kSupersPerMega + k);
            if (!(b[0] <= b[3])) continue;
            for (int c = 0; c < 3; c++) { v[c] = fmin(v[c], b[c]); v[3 + c] = fmax(v[3 + c], b[3 + c]); }
        }
        for (int c = 0; c < 6; c++) { megas[6 * t + c] = v[c]; m[t][c] = v[c]; }
    }
    __syncthreads();
    if (j < world && t % kMegasPerRank == 0) {
        for (int g = 1; g < kMegasPerRank; g++)
            for (int c = 0; c < 3; c++) { v[c] = fmin(v[c], m[t + g][c]); v[3 + c] = fmax(v[3 + c], m[t + g][3 + c]); }
        for (int c = 0; c < 6; c++) rankbox[6 * j + c] = v[c];
    }
}
// Where the pieces lie in a rank's walk array, in rank order:
//   row 0: a jump node (a massless leaf everybody accepts, its skip link leads to walk_first)
//   [walk_first, own_base + own_skip): the received pieces of the lower ranks, packed up against
//   [own_base + own_skip, own_base + num_nodes): the own piece, where k_emit_tile / k_chain_fix built it
//   behind it the received pieces of the higher ranks, then the sentinel.
struct Pieces {
    const char *src[kMaxWorld];  // received rows of each rank (null: none / the own rank)
    long long count[kMaxWorld];
    long long base[kMaxWorld];   // first row of the rank's piece in the walk array (own rank: own_base + own_skip)
    long long total;             // row of the sentinel
    int me;
};
// a link (rank, node behind that rank's dropped copies) -> row of the walk array.  The rows of a received piece are
// in pre-order, so the first row at or behind the node is looked up.  A link whose target was pruned belongs to a
// node nobody here can reach (a cell above both of them is never opened - deep cells below theta * softening are
// opened by nobody, not even by the bodies inside them); it then leads to the next node that IS here, which is
// where a walk leaves that never-entered subtree anyway.  The pieces follow each other without gaps in rank order,
// so "behind the last row of a piece" is the first row of the next.
__device__ __forceinline__ long long piece_row(const Pieces &P, int rank, long long node) {
    if (rank == kLinkEnd) return P.total;
    if (rank == P.me) return P.base[rank] + node;
    long long lo = 0, hi = P.count[rank];
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        const unsigned o = reinterpret_cast<const LetRow *>(P.src[rank] + mid * kLetRow)->orig;
        if (o < (unsigned)node) lo = mid + 1; else hi = mid;
    }
    return P.base[rank] + lo;
}
__global__ __launch_bounds__(kBlock) void k_let_append(Pieces P, int from, Node *__restrict__ nodes, Node64 *__restrict__ n64,
                                                       NodeD *__restrict__ nodesd /* may be null */, TreeInfo *info) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= P.count[from]) return;
    const LetRow row = *reinterpret_cast<const LetRow *>(P.src[from] + k * kLetRow);
    const long long base = P.base[from];
    const long long nx = row.link_rank == kLinkLocal ? base + row.next : piece_row(P, row.link_rank, row.next);
    const bool leaf = __float_as_int(row.s2t) == 0;
    Node nd;
    nd.cx = (float)row.cx; nd.cy = (float)row.cy; nd.cz = (float)row.cz; nd.gm = (float)row.gm;
    nd.s2t = row.s2t;
    nd.next_off = (unsigned)nx * kNodeBytes;
    nodes[base + k] = nd;
    n64[base + k] = Node64{row.cx, row.cy, row.cz, leaf ? 0.0 : ldexp(info->bounds, -(int)row.level)};
    if (nodesd) {
        // the float64 loop's narrow band instead of the fp32 loop's (every rank derives the same band from the
        // global extent, k_emit_tile)
        const int bits = __float_as_int(row.s2t);
        const float s2d = bits == 0 ? 0.0f : __int_as_float(bits - (int)(info->band2 >> 1) + (int)kBand64);
        nodesd[base + k] = NodeD{row.cx, row.cy, row.cz, row.gm, s2d, (unsigned)nx * kNodeDBytes};
    }
}
// the own piece's links that leave the rank, the jump node, the sentinel (one wave)
__global__ void k_let_finish(Pieces P, const OwnLink *__restrict__ links, const ChainTable *__restrict__ T, long long own_base,
                             long long walk_first, Node *__restrict__ nodes, NodeD *__restrict__ nodesd, TreeInfo *info) {
    const int t = threadIdx.x;
    if (t < kOwnLinks && links[t].node >= 0) {
        const int lr = links[t].rank;
        const long long nx = piece_row(P, lr, lr == kLinkEnd ? 0 : links[t].target - chain_skip(T, lr));
        const long long i = own_base + links[t].node;
        nodes[i].next_off = (unsigned)nx * kNodeBytes;
        if (nodesd) nodesd[i].next_off = (unsigned)nx * kNodeDBytes;
    }
    if (t == 0) {
        Node sn;
        sn.cx = sn.cy = sn.cz = 1.0e30f;
        sn.gm = 0.f; sn.s2t = 0.f;
        sn.next_off = (unsigned)P.total * kNodeBytes;
        nodes[P.total] = sn;
        if (nodesd) nodesd[P.total] = NodeD{1.0e30, 1.0e30, 1.0e30, 0.0, 0.0f, (unsigned)P.total * kNodeDBytes};
        sn.next_off = (unsigned)walk_first * kNodeBytes;  // the jump node: accepted by every lane, adds nothing
        nodes[0] = sn;
        if (nodesd) nodesd[0] = NodeD{1.0e30, 1.0e30, 1.0e30, 0.0, 0.0f, (unsigned)walk_first * kNodeDBytes};
        info->walk_nodes = P.total;
        info->walk_first = walk_first;
    }
}
// world 1: nothing was received, the walk array is the own tree as built (its sentinel is in place)
__global__ void k_let_finish_alone(TreeInfo *info) {
    info->walk_nodes = info->num_nodes;
    info->walk_first = 0;
}
__global__ void k_copy_ids(const int32_t *__restrict__ ids, int32_t *__restrict__ dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = ids[i];
}

// ---------------------------------------------------------------------------------------
// K14: conservation diagnostics (nbmi_diagnostics / nbmi_get_potentials_f64; include/nbmi.h).
// Float64 throughout; every sum has a fixed order (no floating-point atomics), so two calls on one state agree bit
// for bit.
// ---------------------------------------------------------------------------------------
// The float64 probe walk: the one walk of the potentials (K14), nbmi_field_at (K19) and the tracers (K20).  The walk of
// K9 in its C++ form, one wave per 64 key-adjacent lanes, one wave-uniform cursor over the same pre-order array and skip
// links, and per lane the force walks' opening decision (opening()): the fp32 test on the Node record, re-decided in
// float64 through Node64 where d^2 falls inside the uncertainty band.  A lane's accepted set does not depend on the other
// lanes of its wave (it takes part in every node none of its own accepted ancestors covers), so at a body it is the force
// walk's set, and which probes share a wave decides the speed of a call and never a bit of its result.  What differs is
// the term: the node's float64 row pot[idx] = {cx, cy, cz, G M} (written by k_emit_tile into the diag64 slot for this
// build only: a cell's double-double moments, a leaf's body as the float64 state has it), and the reference's guard
// (simulation.py:260) on the float64 dist_sq.  A body's own leaf has d = 0 exactly, so the guard skips it as the
// reference's explicit test does.
// The lane.  (qx, qy, qz) is its float64 position and `b64` says where opening()'s float64 re-decision reads the same
// three numbers: a body's row perm[rank] of the current state (lane_prologue), or row `rank` of buffer 0 of a table that
// names the probe columns there (probe_alloc) - either way it computes, operation for operation, what it computes for a
// body at that place.  (px, py, pz) is the same position in fp32, for the fp32 test: a probe's caller rounds q, a
// body's has it from posm_s - a coalesced load, so the first visit need not wait for the gathered float64 row (with
// the rounding in here the potential measured 0.4 - 0.7 % slower).  A lane with valid == false walks nothing and
// returns zeros.
// The band.  The node records carry the upper edge bits(s2t) + K of the band for K = band_half_ulps(maxabs of the
// bodies): the fp32 error of d^2 grows with the larger of |p| and |c|, and a probe may lie far outside the root cube.
// kWiden (probes; pmax: the largest |coordinate| among them, eps: the softening): the walk widens the band to K' =
// band_half_ulps(max(maxabs, pmax)) about the same centre - upper edge + (K' - K), width 2 K'.  pmax <= maxabs: K' = K.
// Without kWiden (bodies: nothing lies outside maxabs) the band is the build's own by construction, pmax and eps are not
// looked at, and a visit pays nothing for the widening.  (Either way a decision is the float64 one; the band only settles
// which visits compute it.)
// Near pairs.  The band's half width is capped at 2^21 ulps (band_half_ulps): enough for the fp32 error of d^2, (6.93
// maxabs / d + 4) ulps, only while d >= 3.3e-6 maxabs.  At eps == 0 (or an eps below that) closer pairs exist, and their
// fp32 d^2 says nothing about the test: a cell closer than 8e-6 maxabs (twice the limit plus the rounding of d itself;
// maxabs: the larger of the bodies' and pmax) is decided in float64 whatever the fp32 test said, so that `terms` stays
// the reference's count there too.
// kAcc: the acceleration is summed beside phi and the term count; without it the lane carries neither the sums nor
// their arithmetic.
// kQuad (quadrupole mode): an applied internal cell (leaves are skipped) also adds the
// second-order terms, with u = dist_sq and the cell's float64 second moments P = quad[9 idx + 3 .. 9 idx + 8]
// (k_quad_level), in a scope of their own:
//   phi += 1/2 [tr P u^-3/2 - 3 (d^T P d) u^-5/2],   a += [7.5 (d^T P d) u^-7/2 - 1.5 tr P u^-5/2] d - 3 u^-5/2 P d.
// kTidal (nbmi_tidal_at / nbmi_get_tidal_f64, K27): the lane carries the six sums of the tidal
// tensor T = da/dx and the term count, and neither the acceleration nor phi (kAcc is false); the result is a TidalSum.
// With w = G M / (dist u), w5 = (3 w) / u an applied node adds  T_aa += (d_a d_a) w5 - w,  T_ab += (d_a d_b) w5;  an
// applied internal cell in quadrupole mode, with g = P d, q = d^T P d, i7 = i5 / u, i9 = i7 / u,
//   A = 1.5 tr i5 - 7.5 q i7,  B = 52.5 q i9 - 7.5 tr i7,  C = 3 i5,  D = 15 i7:
//   T_ab += ((A delta_ab + B (d_a d_b)) + C P_ab) - D (g_a d_b + d_a g_b).
// Without kTidal none of it is instantiated: the other walks are the code they were.
struct FieldSum {
    double ax, ay, az, phi;
    int32_t terms;
};
struct TidalSum {
    double xx, yy, zz, xy, xz, yz;
    int32_t terms;
};
template <bool kTidal>
struct WalkSum { using type = FieldSum; };
template <>
struct WalkSum<true> { using type = TidalSum; };
template <bool kQuad, bool kAcc, bool kWiden, bool kTidal = false>
__device__ __forceinline__ typename WalkSum<kTidal>::type field_walk(const Node *__restrict__ nodes, const double4 *__restrict__ pot, const TreeInfo *info,
                                               const Body64 &b64, double qx, double qy, double qz, float px, float py, float pz,
                                               bool valid, float eps2f, double eps, double pmax,
                                               const double *__restrict__ quad) {
    const unsigned nn = __builtin_amdgcn_readfirstlane((unsigned)info->num_nodes * kNodeBytes);
    const double eps2 = __longlong_as_double((long long)uniform_u64((unsigned long long)__double_as_longlong(b64.tab->eps2)));
    double maxabs = __longlong_as_double((long long)info->maxabs_bits);
    int dk = 0;
    unsigned band2 = __builtin_amdgcn_readfirstlane(info->band2);
    if (kWiden) {
        maxabs = fmax(maxabs, pmax);
        const unsigned kb = info->band2 >> 1;
        unsigned kp = band_half_ulps(maxabs, eps);
        kp = kp > kb ? kp : kb;
        dk = __builtin_amdgcn_readfirstlane((int)(kp - kb));
        band2 = __builtin_amdgcn_readfirstlane(2u * kp);
    }
    float near2 = 0.f;
    if (band2 >= 2u * 2097153u) {
        const double r = 8.0e-6 * maxabs;
        near2 = eps2f + (float)(r * r);
    }
    unsigned resume = valid ? 0u : 0xffffffffu;
    static_assert(!(kTidal && kAcc), "the tidal walk carries no acceleration");
    double ax = 0.0, ay = 0.0, az = 0.0, phi = 0.0;
    double txx = 0.0, tyy = 0.0, tzz = 0.0, txy = 0.0, txz = 0.0, tyz = 0.0;  // (kTidal only)
    int32_t terms = 0;
    unsigned off = 0u;
    while (off < nn) {
        off = __builtin_amdgcn_readfirstlane(off);
        const unsigned idx = off / kNodeBytes;
        const Node nd = nodes[idx];
        const bool cell = __float_as_int(nd.s2t) != 0;
        const float s2t = kWiden && cell ? __int_as_float(__float_as_int(nd.s2t) + dk) : nd.s2t;  // (a leaf keeps its 0)
        const float dx = nd.cx - px, dy = nd.cy - py, dz = nd.cz - pz;
        const float dist_sq = fmaf(dz, dz, fmaf(dy, dy, fmaf(dx, dx, eps2f)));
        const bool active = resume <= off;
        const bool near = cell && dist_sq < near2;
        const bool geom = opening(dist_sq, s2t, band2, active, idx, b64, near).geom;
        bool take;
        const unsigned next = advance<kNodeBytes>(active, geom, off, nd.next_off, resume, take);
        if (take) {
            const double4 q = pot[idx];
            const double ex = q.x - qx, ey = q.y - qy, ez = q.z - qz;
            const double d2 = ex * ex + ey * ey + ez * ez + eps2;  // (-ffp-contract=off: the reference's roundings)
            if (q.w > 0.0 && d2 > eps2) {
                const double dist = sqrt(d2);
                if (!kTidal) phi -= q.w / dist;
                terms++;
                if (kAcc) {
                    const double w = q.w / (dist * d2);
                    ax += ex * w; ay += ey * w; az += ez * w;
                }
                if (kTidal) {
                    const double w = q.w / (dist * d2), w5 = (3.0 * w) / d2;
                    txx += (ex * ex) * w5 - w; tyy += (ey * ey) * w5 - w; tzz += (ez * ez) * w5 - w;
                    txy += (ex * ey) * w5; txz += (ex * ez) * w5; tyz += (ey * ez) * w5;
                }
                if (kQuad && nd.next_off != off + kNodeBytes) {  // an internal cell
                    const double *pq = quad + 9 * (size_t)idx + 3;
                    const double pxx = pq[0], pyy = pq[1], pzz = pq[2], pxy = pq[3], pxz = pq[4], pyz = pq[5];
                    const double dpd = ex * (pxx * ex + 2.0 * (pxy * ey + pxz * ez)) + ey * (pyy * ey + 2.0 * (pyz * ez)) + ez * (pzz * ez);
                    const double tr = pxx + pyy + pzz;
                    const double i1 = 1.0 / dist, i3 = i1 / d2, i5 = i3 / d2;
                    if (!kTidal) phi += 0.5 * (tr * i3 - 3.0 * dpd * i5);
                    if (kTidal) {
                        const double gx = pxx * ex + pxy * ey + pxz * ez, gy = pxy * ex + pyy * ey + pyz * ez;
                        const double gz = pxz * ex + pyz * ey + pzz * ez;
                        const double i7 = i5 / d2, i9 = i7 / d2;
                        const double A = 1.5 * tr * i5 - 7.5 * dpd * i7, B = 52.5 * dpd * i9 - 7.5 * tr * i7;
                        const double Cc = 3.0 * i5, D = 15.0 * i7;
                        txx += ((A + B * (ex * ex)) + Cc * pxx) - D * (gx * ex + ex * gx);
                        tyy += ((A + B * (ey * ey)) + Cc * pyy) - D * (gy * ey + ey * gy);
                        tzz += ((A + B * (ez * ez)) + Cc * pzz) - D * (gz * ez + ez * gz);
                        txy += (B * (ex * ey) + Cc * pxy) - D * (gx * ey + ex * gy);
                        txz += (B * (ex * ez) + Cc * pxz) - D * (gx * ez + ex * gz);
                        tyz += (B * (ey * ez) + Cc * pyz) - D * (gy * ez + ey * gz);
                    }
                    if (kAcc) {
                        const double sc = 7.5 * dpd * (i5 / d2) - 1.5 * tr * i5, t3 = 3.0 * i5;
                        ax += sc * ex - t3 * (pxx * ex + pxy * ey + pxz * ez);
                        ay += sc * ey - t3 * (pxy * ex + pyy * ey + pyz * ez);
                        az += sc * ez - t3 * (pxz * ex + pyz * ey + pzz * ez);
                    }
                }
            }
        }
        off = next;
    }
    if constexpr (kTidal) return TidalSum{txx, tyy, tzz, txy, txz, tyz, terms};
    else return FieldSum{ax, ay, az, phi, terms};
}

// Tree potential: the probe walk with a body in the lane - the build's band, phi and the term count only.  Both land at
// the body's state row j = perm[rank].
template <bool kQuad>
__global__ __launch_bounds__(kBlock) void k_potential_tree(const Node *__restrict__ nodes, const double4 *__restrict__ pot,
                                                           const WalkTable *tab, const TreeInfo *info,
                                                           const float4 *__restrict__ posm_s, const uint32_t *__restrict__ perm,
                                                           int curbuf, float eps2f, int64_t n, double *__restrict__ phi,
                                                           int32_t *__restrict__ cnt, const double *__restrict__ quad) {
    if (tree_frozen(info)) return;  // the tree did not fit: the caller reports it
    const int64_t rank = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const WalkCtx C = lane_prologue(nodes, posm_s, perm, rank, n, info, tab, curbuf);
    const Lane64 L = lane_f64(C);
    const FieldSum f = field_walk<kQuad, false, false>(nodes, pot, info, C.b64, L.qx, L.qy, L.qz, C.px, C.py, C.pz, C.valid, eps2f, 0.0,
                                                       0.0, quad);
    if (C.valid) {
        phi[C.j] = f.phi;
        cnt[C.j] = f.terms;
    }
}

// ---------------------------------------------------------------------------------------
// K15: quadrupole mode (nbmi_set_multipole, include/nbmi.h).
// ---------------------------------------------------------------------------------------
// Second moments of an internal cell about its centre of mass, G folded in; a leaf's (and the sentinel's) row is zero.
// 24 bytes, the stride of Node: the walk's byte cursor addresses both arrays.
struct alignas(8) NodeQ {
    float pxx, pyy, pzz, pxy, pxz, pyz;
};
static_assert(sizeof(NodeQ) == kNodeBytes, "NodeQ rows lie beside the Node rows");
constexpr int kQuadDoubles = 9;  // float64 work row of a cell: bottom-up centre of mass (3), second moments (6)
constexpr int kQuadGrid = 2048;  // workgroups of the passes over the node rows (grid-stride)

// One level of the bottom-up pass: every internal cell of level `lev` from its (up to eight) children, which are
// leaves or cells of level lev + 1 that the previous launch finished.  With child k's mass M_k, centre c_k and moments
// P_k (a leaf: its float64 position, P = 0):
//   c = c_0 + sum M_k (c_k - c_0) / M,     P = sum [ P_k + M_k (c_k - c)(c_k - c)^T ]
// Only DIFFERENCES of nearby points are formed, so a cell 1e-3 across at coordinate 700 gets its moments to a few
// ulps of their own size; sums about the origin (the prefix sums of K5-K7 with six more columns) lose them entirely
// there.  The centre carried upwards is the pass's own (good to an ulp of the coordinate), not the build's prefix-sum
// centre (good to 1e-13 of the largest coordinate in the tile: a first-order error 2 M |c_k - c| 1e-13 maxabs, which
// exceeds the tolerance for cells below ~1e-4 across); about which of the two P is taken differs by G M |dc|^2, nothing.
// pot = the build's float64 rows {cx, cy, cz, G M} (leaf: x, y, z, G m); links are Node::next_off.
__global__ __launch_bounds__(kBlock) void k_quad_level(const Node *__restrict__ nodes, const uint8_t *__restrict__ node_level,
                                                       const double4 *__restrict__ pot, const TreeInfo *__restrict__ info,
                                                       int lev, double *__restrict__ work, NodeQ *__restrict__ nq) {
    if (info->error != 0 || lev >= info->max_level) return;  // max_level = the deepest LEAF level (k_max_level)
    const int64_t rows = info->num_nodes;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < rows; i += (int64_t)gridDim.x * kBlock) {
        if (node_level[i] != (uint8_t)lev) continue;
        const unsigned end = nodes[i].next_off / kNodeBytes;
        if (end == (unsigned)i + 1u) continue;  // a leaf
        // first sweep: the centre
        unsigned c = (unsigned)i + 1u;
        const double4 first = pot[c];
        const bool first_leaf = nodes[c].next_off / kNodeBytes == c + 1u;
        const double ox = first_leaf ? first.x : work[kQuadDoubles * (size_t)c], oy = first_leaf ? first.y : work[kQuadDoubles * (size_t)c + 1],
                     oz = first_leaf ? first.z : work[kQuadDoubles * (size_t)c + 2];
        double M = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
        while (c < end) {
            const unsigned nx = nodes[c].next_off / kNodeBytes;
            const double4 q = pot[c];
            const bool leaf = nx == c + 1u;
            const double *w = work + kQuadDoubles * (size_t)c;
            const double cx = leaf ? q.x : w[0], cy = leaf ? q.y : w[1], cz = leaf ? q.z : w[2];
            M += q.w; sx += q.w * (cx - ox); sy += q.w * (cy - oy); sz += q.w * (cz - oz);
            c = nx;
        }
        double cx = ox, cy = oy, cz = oz;
        if (M > 0.0) { cx += sx / M; cy += sy / M; cz += sz / M; }
        double pxx = 0.0, pyy = 0.0, pzz = 0.0, pxy = 0.0, pxz = 0.0, pyz = 0.0;
        c = (unsigned)i + 1u;
        while (c < end) {
            const unsigned nx = nodes[c].next_off / kNodeBytes;
            const double4 q = pot[c];
            const bool leaf = nx == c + 1u;
            const double *w = work + kQuadDoubles * (size_t)c;
            const double dx = (leaf ? q.x : w[0]) - cx, dy = (leaf ? q.y : w[1]) - cy, dz = (leaf ? q.z : w[2]) - cz;
            pxx += q.w * dx * dx; pyy += q.w * dy * dy; pzz += q.w * dz * dz;
            pxy += q.w * dx * dy; pxz += q.w * dx * dz; pyz += q.w * dy * dz;
            if (!leaf) { pxx += w[3]; pyy += w[4]; pzz += w[5]; pxy += w[6]; pxz += w[7]; pyz += w[8]; }
            c = nx;
        }
        double *o = work + kQuadDoubles * (size_t)i;
        o[0] = cx; o[1] = cy; o[2] = cz;
        o[3] = pxx; o[4] = pyy; o[5] = pzz; o[6] = pxy; o[7] = pxz; o[8] = pyz;
        nq[i] = NodeQ{(float)pxx, (float)pyy, (float)pzz, (float)pxy, (float)pxz, (float)pyz};
    }
}

// nbmi_get_cell_moments: the fp32 records widened, rows as k_cells numbers them (a leaf's record is never written
// and never read by the walks: zeros here)
__global__ __launch_bounds__(kBlock) void k_quad_export(const Node *__restrict__ nodes, const NodeQ *__restrict__ nq,
                                                        int64_t num_nodes, double *__restrict__ out) {
    const int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (u >= num_nodes) return;
    const bool leaf = nodes[u].next_off == (unsigned)(u + 1) * kNodeBytes;
    const NodeQ q = leaf ? NodeQ{0.f, 0.f, 0.f, 0.f, 0.f, 0.f} : nq[u];
    double *o = out + 6 * u;
    o[0] = q.pxx; o[1] = q.pyy; o[2] = q.pzz; o[3] = q.pxy; o[4] = q.pxz; o[5] = q.pyz;
}

// The second-order part of one applied cell term, fp32: with e = d u^-1/2 (inv = u^-1/2),
//   q = u^-2 [ (7.5 e^T P e - 1.5 tr P) e - 3 P e ]
// - nothing beyond u^-2 is formed (u^-7/2 leaves fp32 at d ~ 1e-5 when eps = 0), and P meets the first u^-1 before the
// second: P / u <= G M theta^2 for an accepted cell, so the term is finite wherever the monopole term is.  inv = 0
// switches the term off.
__device__ __forceinline__ void quad_term(const NodeQ &Q, float dx, float dy, float dz, float inv, float &ax, float &ay, float &az) {
    const float ex = dx * inv, ey = dy * inv, ez = dz * inv;
    const float i2 = inv * inv;
    const float wx = fmaf(Q.pxz, ez, fmaf(Q.pxy, ey, Q.pxx * ex)) * i2;
    const float wy = fmaf(Q.pyz, ez, fmaf(Q.pyy, ey, Q.pxy * ex)) * i2;
    const float wz = fmaf(Q.pzz, ez, fmaf(Q.pyz, ey, Q.pxz * ex)) * i2;
    const float epe = fmaf(ez, wz, fmaf(ey, wy, ex * wx));
    const float tr = ((Q.pxx + Q.pyy) + Q.pzz) * i2;
    const float s = fmaf(7.5f, epe, -1.5f * tr) * i2, t = -3.0f * i2;
    ax += fmaf(s, ex, t * wx);
    ay += fmaf(s, ey, t * wy);
    az += fmaf(s, ez, t * wz);
}

// The quadrupole walk.  k_potential_tree's shape: one wave per 64 key-adjacent bodies, one wave-uniform cursor, the Node
// and the NodeQ record fetched at the same uniform byte offset (scalar loads), opening() and visit()'s fp32 monopole
// (its association, (G m / d) (1 / d^2)); float64 waves (wave_uses_f64) take the decision and monopole64() from the NodeD
// row and start the correction from the float64 difference rounded to fp32.  fp32 partial sums: flush12().
// Epilogues: k_walk's.  !kIntegrate: accelerations in the caller's order and the lane-accept count (nbmi_walk_counters).
// Empty asm statements (the idiom of tie_visit64; no instruction is emitted) that pin every word of both records
// behind their loads: the loads are all requested first and one wait covers them.  Without the pins the compiler sinks
// the NodeQ load behind the leaf test, and a cell visit waits for scalar memory twice.
#define NBMI_PIN_Q(Q) asm volatile("" : "+s"(Q.pxx), "+s"(Q.pyy), "+s"(Q.pzz), "+s"(Q.pxy), "+s"(Q.pxz), "+s"(Q.pyz))
#define NBMI_PIN_N(N) asm volatile("" : "+s"(N.cx), "+s"(N.cy), "+s"(N.cz), "+s"(N.gm), "+s"(N.s2t), "+s"(N.next_off))
#define NBMI_PIN_D(N) asm volatile("" : "+s"(N.cx), "+s"(N.cy), "+s"(N.cz), "+s"(N.gm), "+s"(N.s2t), "+s"(N.next_off))
template <bool kIntegrate, bool kGuard, bool kLeap>
__global__ __launch_bounds__(kBlock) void k_walk_quad(const Node *__restrict__ nodes, const NodeQ *__restrict__ nodesq,
                                                      const NodeD *__restrict__ nodesd /* null: fp32 forces only */,
                                                      const WalkTable *tab, const TreeInfo *info_in,
                                                      const float4 *__restrict__ posm_s, const uint32_t *__restrict__ perm,
                                                      double *__restrict__ acc_out, WalkParams P, TreeInfo *info_out) {
    const int lb = logical_block(blockIdx.x, gridDim.x, P.xcd_chunk);
    const int64_t rank = P.rank_begin + (int64_t)lb * blockDim.x + threadIdx.x;
    const WalkCtx C = lane_prologue(nodes, posm_s, perm, rank, P.rank_end, info_in, tab, P.curbuf);
    const unsigned rows = __builtin_amdgcn_readfirstlane(C.rows);
    unsigned resume = C.resume;
    float ax = 0.f, ay = 0.f, az = 0.f;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    unsigned long long accepts = 0;
    const bool use64 = wave_uses_f64(tab, info_in, P, rank, kIntegrate);
    int since_flush = 0;
    if (use64) {
        // (the float64 records come as a kernel argument, not through the table as in k_walk: a pointer loaded from
        // memory is a generic one to the compiler, and its loads become vector loads)
        const Lane64 L = lane_f64(C);
        const double qx = L.qx, qy = L.qy, qz = L.qz, eps2 = L.eps2;
        unsigned idx = 0u;
        while (idx < rows) {
            idx = __builtin_amdgcn_readfirstlane(idx);
            NodeD nd = nodesd[idx];
            NodeQ Q = *reinterpret_cast<const NodeQ *>(reinterpret_cast<const char *>(nodesq) + idx * kNodeBytes);
            NBMI_PIN_D(nd);
            NBMI_PIN_Q(Q);
            const unsigned offd = idx * kNodeDBytes;
            const double dx = nd.cx - qx, dy = nd.cy - qy, dz = nd.cz - qz;
            const double d2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, __builtin_fma(dx, dx, eps2)));
            const float d2f = (float)d2;
            const bool active = resume <= offd;
            const bool geom = opening(d2f, nd.s2t, 2u * kBand64, active, idx, C.b64).geom;
            bool take;
            const unsigned next = advance<kNodeDBytes>(active, geom, offd, nd.next_off, resume, take);
            const bool force = kGuard ? (take && d2 > eps2) : take;
            if (!kIntegrate) accepts += (take && d2 > eps2) ? 1u : 0u;
            if (force) {
                const double w = monopole64(nd.gm, d2, d2f);
                sx = __builtin_fma(dx, w, sx); sy = __builtin_fma(dy, w, sy); sz = __builtin_fma(dz, w, sz);
            }
            // (a leaf record, s2t == 0, carries no moments: a wave-uniform skip)
            if (__float_as_int(nd.s2t) != 0)
                quad_term(Q, (float)dx, (float)dy, (float)dz, force ? __builtin_amdgcn_rsqf(d2f) : 0.f, ax, ay, az);
            flush12(since_flush, ax, ay, az, sx, sy, sz);
            idx = next / kNodeDBytes;
        }
    } else {
        const unsigned nn = rows * kNodeBytes;
        unsigned off = 0u;
        while (off < nn) {
            off = __builtin_amdgcn_readfirstlane(off);
            Node nd = *reinterpret_cast<const Node *>(reinterpret_cast<const char *>(nodes) + off);
            NodeQ Q = *reinterpret_cast<const NodeQ *>(reinterpret_cast<const char *>(nodesq) + off);
            NBMI_PIN_N(nd);
            NBMI_PIN_Q(Q);
            const float dx = nd.cx - C.px, dy = nd.cy - C.py, dz = nd.cz - C.pz;
            const float dist_sq = fmaf(dz, dz, fmaf(dy, dy, fmaf(dx, dx, P.eps2)));
            const bool active = resume <= off;
            const bool geom = opening(dist_sq, nd.s2t, C.band2, active, off / kNodeBytes, C.b64).geom;
            bool take;
            const unsigned next = advance<kNodeBytes>(active, geom, off, nd.next_off, resume, take);
            const bool force = kGuard ? (take && dist_sq > P.eps2) : take;
            if (!kIntegrate) accepts += (take && dist_sq > P.eps2) ? 1u : 0u;
            const float inv = force ? __builtin_amdgcn_rsqf(dist_sq) : 0.f;
            const float f = (nd.gm * inv) * (inv * inv);
            ax = fmaf(dx, f, ax);
            ay = fmaf(dy, f, ay);
            az = fmaf(dz, f, az);
            if (__float_as_int(nd.s2t) != 0) quad_term(Q, dx, dy, dz, inv, ax, ay, az);  // (a leaf record carries no moments: a wave-uniform skip)
            flush12(since_flush, ax, ay, az, sx, sy, sz);
            off = next;
        }
    }
    sx += (double)ax; sy += (double)ay; sz += (double)az;
    if (kIntegrate) {
        publish_maxabs(tab, C.valid ? integrate<kLeap>(tab, C.j, rank, sx, sy, sz, P, C.frozen) : 0.0);
    } else {
        if (C.valid) store_acc(acc_out, tab->buf[P.curbuf], C.j, sx, sy, sz);
        atomicAdd(&info_out->lane_accepts, accepts);
    }
}

// The tile loop of every direct sum over the bodies (potential, field, tidal tensor): the float64 bodies staged through
// `tile` (kBlock rows of shared memory) as {x, y, z, G m}, kBlock at a time, and term(row, j) for every body j in index
// order.  Every thread of the block calls it; guard and arithmetic are the caller's.
template <class Term>
__device__ __forceinline__ void direct_tiles(const Bodies &cur, int64_t n, double G, double4 *tile, Term term) {
    const int t = threadIdx.x;
    for (int64_t base = 0; base < n; base += kBlock) {
        const int64_t jj = base + t;
        tile[t] = jj < n ? make_double4(cur.x[jj], cur.y[jj], cur.z[jj], G * cur.m[jj]) : make_double4(0.0, 0.0, 0.0, 0.0);
        __syncthreads();
        const int lim = n - base < kBlock ? (int)(n - base) : kBlock;
        for (int k = 0; k < lim; k++) {
            const double4 q = tile[k];
            term(q, base + k);
        }
        __syncthreads();
    }
}

// Direct potential: phi_i = -sum_{j != i} G m_j / sqrt(|x_j - x_i|^2 + eps^2), every thread one body, j in index order
// (direct_tiles).  eps == 0: pairs at zero distance are skipped (k_direct's guard).  (Not field_direct_sum: this guard
// counts a coincident distinct body when eps > 0, the probe sum's skips it.)
__global__ __launch_bounds__(kBlock) void k_potential_direct(Bodies cur, int64_t n, double G, double eps2,
                                                             double *__restrict__ phi, int32_t *__restrict__ cnt) {
    __shared__ double4 tile[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = i < n;
    double x = 0.0, y = 0.0, z = 0.0;
    if (valid) { x = cur.x[i]; y = cur.y[i]; z = cur.z[i]; }
    double acc = 0.0;
    int32_t terms = 0;
    direct_tiles(cur, n, G, tile, [&](const double4 &q, int64_t j) {
        const double ex = q.x - x, ey = q.y - y, ez = q.z - z;
        const double d2 = ex * ex + ey * ey + ez * ez + eps2;
        // j != i, on the low words: rows stay below kMaxBodies + kBlock < 2^32.  (The 64-bit comparison keeps both halves
        // of i and of the tile's base in registers through the loop: 36 VGPRs / 38 SGPRs for 34 / 36.)
        if ((uint32_t)j != (uint32_t)i && d2 > 0.0) {
            acc -= q.w / sqrt(d2);
            terms++;
        }
    });
    if (valid) {
        phi[i] = acc;
        cnt[i] = terms;
    }
}

// Body sums, in the order of the state rows: per block a contiguous range of rows, per thread a strided part of it,
// then a fixed tree over the block's threads.  Sums: m, m x (3), m v (3), m x X v (3), m |v|^2, m phi; and the
// applied terms as an integer.
constexpr int kDiagSums = 12;
constexpr int kDiagBlocksMax = 1024;
__device__ __forceinline__ void diag_block_sum(double (*sh)[kBlock], long long *shc, double *v, long long c,
                                               double *__restrict__ out, long long *__restrict__ outc) {
    const int t = threadIdx.x;
    for (int k = 0; k < kDiagSums; k++) sh[k][t] = v[k];
    shc[t] = c;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if (t < w) {
            for (int k = 0; k < kDiagSums; k++) sh[k][t] += sh[k][t + w];
            shc[t] += shc[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        for (int k = 0; k < kDiagSums; k++) out[k] = sh[k][0];
        *outc = shc[0];
    }
}

__global__ __launch_bounds__(kBlock) void k_diag_partial(Bodies cur, const double *__restrict__ phi,
                                                         const int32_t *__restrict__ cnt, int64_t n, int64_t per_block,
                                                         double *__restrict__ part, long long *__restrict__ partc) {
    __shared__ double sh[kDiagSums][kBlock];
    __shared__ long long shc[kBlock];
    double v[kDiagSums];
    for (int k = 0; k < kDiagSums; k++) v[k] = 0.0;
    long long c = 0;
    const int64_t b0 = (int64_t)blockIdx.x * per_block;
    const int64_t b1 = b0 + per_block < n ? b0 + per_block : n;
    for (int64_t i = b0 + threadIdx.x; i < b1; i += kBlock) {
        const double m = cur.m[i], x = cur.x[i], y = cur.y[i], z = cur.z[i];
        const double vx = cur.vx[i], vy = cur.vy[i], vz = cur.vz[i];
        v[0] += m;
        v[1] += m * x; v[2] += m * y; v[3] += m * z;
        v[4] += m * vx; v[5] += m * vy; v[6] += m * vz;
        v[7] += m * (y * vz - z * vy);
        v[8] += m * (z * vx - x * vz);
        v[9] += m * (x * vy - y * vx);
        v[10] += m * (vx * vx + vy * vy + vz * vz);
        if (phi) {
            v[11] += m * phi[i];
            c += cnt[i];
        }
    }
    diag_block_sum(sh, shc, v, c, part + (int64_t)blockIdx.x * kDiagSums, partc + blockIdx.x);
}

// one block: the partial sums of k_diag_partial's `nb` blocks, in block order per thread, then the same tree
__global__ __launch_bounds__(kBlock) void k_diag_final(const double *__restrict__ part, const long long *__restrict__ partc,
                                                       int nb, double *__restrict__ out, long long *__restrict__ outc) {
    __shared__ double sh[kDiagSums][kBlock];
    __shared__ long long shc[kBlock];
    double v[kDiagSums];
    for (int k = 0; k < kDiagSums; k++) v[k] = 0.0;
    long long c = 0;
    for (int b = threadIdx.x; b < nb; b += kBlock) {
        for (int k = 0; k < kDiagSums; k++) v[k] += part[(int64_t)b * kDiagSums + k];
        c += partc[b];
    }
    diag_block_sum(sh, shc, v, c, out, outc);
}

// phi from state rows to the caller's order (id: state row -> caller index)
__global__ __launch_bounds__(kBlock) void k_unperm1_f64(const double *__restrict__ a, const int32_t *__restrict__ id, int64_t n,
                                                        double *__restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r < n) out[id[r]] = a[r];
}

// ---------------------------------------------------------------------------------------
// K16 - K18: the exact tree queries - k nearest neighbours, friends-of-friends groups, binned pair counts (include/nbmi.h,
// DESIGN.md sections 4.14 - 4.16).  Float64 throughout, every sum in a fixed order: two calls on one state agree bit for
// bit.  First what all three share: the node rows and the waves' first leaves, d2 and its lower
// bound, the wave's prologue, the walk, the half search inside a wave and the sum of a counter over it.
// ---------------------------------------------------------------------------------------
// A query's own row per node of its build, written after the emission from what the build left behind (the build
// itself is untouched): node_ref gives the node's first body in key order, perm its state row.
//   leaf           {x, y, z, m}   the body as the float64 state has it; m is the MASS (cur.m), not G m
//   internal cell  {x, y, z, w}   the cell's FIRST body (the "anchor") and the reach w = 2 hs + 2^-44 bounds
// Why the anchor and not the centre of mass: the bodies of a level-L cell share L key digits, so per axis they lie
// between two of the centres k_keys computed on the way down - 2 hs apart in exact arithmetic, and at most
// 43 roundings of half an ulp(bounds) each further apart as computed (hence the 2^-44 bounds, 2^9 times that).  So
// every body of the cell is within w of the anchor on every axis, and that statement has no rounding of a sum of
// masses in it.  (The computed centre of mass has: its error grows with the mass ratio of the sub-tile to the cell,
// without bound relative to the cell's size.)
// Also, for every wave of 64 key ranks, wleaf = the node index of its first body's leaf (the node array is in key order:
// everything of a higher rank lies behind that leaf), where K17 and K18 start their walks.
constexpr int kQueryBlock = 64;  // one wave per workgroup (K16: its k x 512 bytes of LDS are then the allocation unit)
__global__ __launch_bounds__(kBlock) void k_query_rows(const Node *__restrict__ nodes, const Node64 *__restrict__ n64,
                                                       const int32_t *__restrict__ node_ref, const uint32_t *__restrict__ perm,
                                                       Bodies cur, const TreeInfo *__restrict__ info, int64_t capacity,
                                                       double4 *__restrict__ rows, uint32_t *__restrict__ wleaf) {
    if (tree_frozen(info)) return;  // the tree did not fit: the caller reports it
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= info->num_nodes || idx >= capacity) return;
    const int32_t r = node_ref[idx];
    const uint32_t j = perm[r];
    const bool leaf = __float_as_int(nodes[idx].s2t) == 0;
    const double w = leaf ? cur.m[j] : __dadd_rn(__dmul_rn(2.0, n64[idx].hs), __dmul_rn(info->bounds, 0x1p-44));
    rows[idx] = make_double4(cur.x[j], cur.y[j], cur.z[j], w);
    if (leaf && (r & 63) == 0) wleaf[r >> 6] = (uint32_t)idx;
}
// After a query (or the diagnostics' potential): the tree header as it stood before its own build - except that a capacity
// error of that build stays behind in the sticky words, to be reported by the next call that looks, as a step's is.
__global__ void k_query_restore(TreeInfo *info, const TreeInfo *__restrict__ saved) {
    if (threadIdx.x != 0) return;
    const int err = info->error | info->sticky_error;
    const long long nodes = info->sticky_error ? info->sticky_nodes : info->num_nodes;
    *info = *saved;
    if (err && info->sticky_error == 0) {
        info->sticky_error = 1;
        info->sticky_nodes = nodes;
    }
}

// d2(i, j) as the header defines it: float64, this association, no FMA
__device__ __forceinline__ double query_d2(double bx, double by, double bz, double qx, double qy, double qz) {
    const double dx = __dsub_rn(bx, qx), dy = __dsub_rn(by, qy), dz = __dsub_rn(bz, qz);
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}
// A lower bound on the COMPUTED d2 between q and every body within `w` per axis of the anchor (ax, ay, az).  Per axis the
// true gap is G = |q - a| - w (or 0).  t = fl|q - a| is within u t of it (u = 2^-53), fl(t - w) within u t of t - w (when
// it is positive, w < t), the stored w within u w < u t of the reach, the last subtraction within u t again: g <=
// G - (2^-49 - 4 u) t < G.  A body's computed |dx| is >= G (1 - u), its computed d2 >= (sum G^2)(1 - u)^5; the bound
// below is <= (sum g^2)(1 + u)^3 (1 - 2^-48).  2^-48 = 32 u leaves a factor four.  Below 2^-960 the products may be
// subnormal and the relative bounds no longer hold: such a bound counts as 0 (never prunes).
// Nothing above uses that q is a body or lies in the root cube: every step is a relative rounding bound on t = fl|q - a|,
// and with |q| <= 1e18 (nbmi_pair_counts_at's points) and the bodies inside the cube no difference, square or sum
// overflows, so the bound holds for such a point unrestricted.
__device__ __forceinline__ double query_lower(double4 a, double qx, double qy, double qz) {
    const double tx = fabs(__dsub_rn(a.x, qx)), ty = fabs(__dsub_rn(a.y, qy)), tz = fabs(__dsub_rn(a.z, qz));
    double gx = __dsub_rn(__dsub_rn(tx, a.w), __dmul_rn(tx, 0x1p-49));
    double gy = __dsub_rn(__dsub_rn(ty, a.w), __dmul_rn(ty, 0x1p-49));
    double gz = __dsub_rn(__dsub_rn(tz, a.w), __dmul_rn(tz, 0x1p-49));
    gx = gx > 0.0 ? gx : 0.0; gy = gy > 0.0 ? gy : 0.0; gz = gz > 0.0 ? gz : 0.0;
    const double lo = __dmul_rn(__dadd_rn(__dadd_rn(__dmul_rn(gx, gx), __dmul_rn(gy, gy)), __dmul_rn(gz, gz)), 1.0 - 0x1p-48);
    return lo > 0x1p-960 ? lo : 0.0;
}
__device__ __forceinline__ double query_bcast(double v, int lane) {  // lane is wave-uniform
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, lane), hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned long long)(unsigned)lo);
}
// the 64 bodies at the key ranks base .. base + 63, one per lane (ranks outside [0, n) hold zeros and are never used)
struct QueryGroup {
    double x, y, z, m;
    int64_t base;
};
__device__ __forceinline__ QueryGroup query_group(const Bodies &cur, const uint32_t *__restrict__ perm, int64_t base, int64_t n) {
    QueryGroup g{0.0, 0.0, 0.0, 0.0, base};
    const int64_t r = base + (int64_t)(threadIdx.x & 63);
    if (r >= 0 && r < n) {
        const uint32_t j = perm[r];
        g.x = cur.x[j]; g.y = cur.y[j]; g.z = cur.z[j]; g.m = cur.m[j];
    }
    return g;
}
// What a lane of a query kernel starts from - one wave per 64 key-adjacent bodies, one body per lane: its key rank (valid:
// it has a body), the end offset of the node array, the wave's own 64 bodies and among them its own, the query point.
// frozen: the build did not fit (the caller reports it): the kernel returns at once.
struct QueryCtx {
    bool frozen, valid;
    int lane;
    int64_t count, w0, rank;  // count: the bodies or points of the grid, 0 where frozen (such a wave has no valid lane)
    unsigned nn;
    QueryGroup own;
    double qx, qy, qz;
};
// What does not depend on whose point the lane has - frozen, count, lane, w0, rank, valid, nn - for a grid over `count`
// bodies or points.  `own` and the query point are the caller's to fill.
__device__ __forceinline__ QueryCtx query_wave(const TreeInfo *__restrict__ info, int64_t count) {
    QueryCtx C;
    C.frozen = tree_frozen(info);
    C.count = C.frozen ? 0 : count;
    C.lane = threadIdx.x;
    C.w0 = (int64_t)blockIdx.x * kQueryBlock;
    C.rank = C.w0 + C.lane;
    C.valid = C.rank < C.count;
    C.nn = __builtin_amdgcn_readfirstlane((unsigned)info->num_nodes * kNodeBytes);
    return C;
}
// a body in the lane: the query point is the wave's own body of that lane
__device__ __forceinline__ QueryCtx query_prologue(const TreeInfo *__restrict__ info, const Bodies &cur,
                                                   const uint32_t *__restrict__ perm, int64_t n) {
    QueryCtx C = query_wave(info, n);
    C.own = query_group(cur, perm, C.w0, C.count);  // (a frozen wave loads nothing)
    C.qx = C.own.x; C.qy = C.own.y; C.qz = C.own.z;
    return C;
}
// One pass over the tree for one wave, k_potential_tree's skeleton: a wave-uniform byte cursor over `Node` and its
// skip links, per lane `resume` = the offset up to which it sits out because it pruned an ancestor; the wave
// descends while any active lane cannot prune.  `bound` is what a lane prunes against, strictly: a subtree is
// skipped only if the lower bound EXCEEDS it, so bodies AT the bound are always reached.
// The cursor starts at byte offset `start` (0: the root; the offset of a leaf: everything behind it in key order -
// the cells that hold that leaf lie in front of it and are never tested, so nothing of theirs is pruned).
// Leaves of the ranks [ex_lo, ex_hi) are skipped: the caller has dealt with those bodies (the wave's own among them,
// which is how self is excluded by identity).  leaf(d2, row, rank) sees every other leaf a lane reaches and may
// lower `bound`.  cell(idx, row, next_off) decides an internal cell for an active lane: true = the lane keeps it open,
// false = it is done with the whole subtree (K16 / K17: pruned; K18 may also have counted it).
template <class Cell, class Leaf>
__device__ __forceinline__ void query_walk_cells(const Node *__restrict__ nodes, const double4 *__restrict__ rows,
                                                 const int32_t *__restrict__ node_ref, unsigned start, const QueryCtx &C,
                                                 int64_t ex_lo, int64_t ex_hi, long long &evals, Cell cell, Leaf leaf) {
    unsigned resume = C.valid ? 0u : 0xffffffffu;
    unsigned off = start;
    while (off < C.nn) {
        off = __builtin_amdgcn_readfirstlane(off);
        const unsigned idx = off / kNodeBytes;
        const Node nd = nodes[idx];
        const double4 row = rows[idx];
        const bool active = resume <= off;
        if (__float_as_int(nd.s2t) == 0) {  // a leaf
            const int64_t r = node_ref[idx];
            if (active && (r < ex_lo || r >= ex_hi)) {
                const double d2 = query_d2(row.x, row.y, row.z, C.qx, C.qy, C.qz);
                evals++;
                leaf(d2, row, r);
            }
            off += kNodeBytes;
        } else {
            bool open = false;
            if (active) {
                open = cell(idx, row, nd.next_off);
                if (!open) resume = nd.next_off;
            }
            off = __builtin_amdgcn_ballot_w64(open) ? off + kNodeBytes : nd.next_off;
        }
    }
}
// K16 / K17: a cell is open unless its lower bound exceeds `bound`
template <class Leaf>
__device__ __forceinline__ void query_walk(const Node *__restrict__ nodes, const double4 *__restrict__ rows,
                                           const int32_t *__restrict__ node_ref, unsigned start, const QueryCtx &C,
                                           int64_t ex_lo, int64_t ex_hi, const double &bound, long long &evals, Leaf leaf) {
    query_walk_cells(nodes, rows, node_ref, start, C, ex_lo, ex_hi, evals,
                     [&](unsigned, const double4 &row, unsigned) { return !(query_lower(row, C.qx, C.qy, C.qz) > bound); }, leaf);
}
// K17 / K18, the half search inside the wave: the wave's own bodies go round by readlane and each pair is tested once - the
// higher lane tests the lower.  f(d2, rank of the lower body) sees every such pair, in one branch for the lanes above it.
template <class Pair>
__device__ __forceinline__ void query_half_search(const QueryCtx &C, int64_t n, long long &evals, Pair f) {
    for (int i = 0; i < 63; i++) {
        if (C.w0 + i >= n) break;
        const double d2 = query_d2(query_bcast(C.own.x, i), query_bcast(C.own.y, i), query_bcast(C.own.z, i), C.qx, C.qy, C.qz);
        if (C.valid && C.lane > i) {
            evals++;
            f(d2, C.w0 + i);
        }
    }
}

// ---- K16: k nearest neighbours (nbmi_knn / nbmi_get_densities_f64 / density colours) --------
constexpr int kKnnMaxK = 64;
// A lane's candidate list: a binary max-heap of its k smallest d2 so far, slot s of lane l at h[64 s] (h = the
// wave's array + l).  The column of a lane is 8 bytes wide, so whatever slots the 64 lanes address, a 32-lane group
// of a ds_read_b64 touches 32 distinct bank pairs and a 16-lane group of a ds_write_b64 sixteen: no conflicts although
// every lane sifts along its own path.  Replaces the root (the current k-th smallest) by v < root.
__device__ __forceinline__ void knn_push(double *__restrict__ h, int k, double v) {
    int i = 0;
    for (;;) {
        int c = 2 * i + 1;
        if (c >= k) break;
        double a = h[64 * c];
        const double b = c + 1 < k ? h[64 * (c + 1)] : -1.0;  // (every d2 is >= 0)
        if (b > a) { a = b; c = c + 1; }
        if (!(a > v)) break;
        h[64 * i] = a;
        i = c;
    }
    h[64 * i] = v;
}
// The seeded ranks: every other body of the three groups (the wave's own 64 bodies and the 64 before and after them in key
// order), exchanged through readlane.  f(d2, mass of that body).
template <class Body>
__device__ __forceinline__ void knn_seed(const QueryGroup (&grp)[3], const QueryCtx &C, int64_t n, long long &evals, Body f) {
#pragma unroll
    for (int g = 0; g < 3; g++) {
        for (int i = 0; i < 64; i++) {
            const int64_t r = grp[g].base + i;
            if (r < 0 || r >= n) continue;
            const double d2 = query_d2(query_bcast(grp[g].x, i), query_bcast(grp[g].y, i), query_bcast(grp[g].z, i), C.qx, C.qy, C.qz);
            const double m = query_bcast(grp[g].m, i);
            if (C.valid && r != C.rank) {
                evals++;
                f(d2, m);
            }
        }
    }
}
// K16's two passes:
//   kSum = false  bound = the lane's current k-th candidate (the heap's root), leaves are pushed
//   kSum = true   bound = r2_k, fixed; leaves with d2 <= r2_k add their mass to `acc`
template <bool kSum>
__device__ __forceinline__ void knn_walk(const Node *__restrict__ nodes, const double4 *__restrict__ rows,
                                         const int32_t *__restrict__ node_ref, const QueryCtx &C, int64_t ex_lo, int64_t ex_hi,
                                         double *__restrict__ h, int k, double &bound, double &acc, long long &evals) {
    query_walk(nodes, rows, node_ref, 0u, C, ex_lo, ex_hi, bound, evals, [&](double d2, const double4 &row, int64_t) {
        if (kSum) {
            if (d2 <= bound) acc = __dadd_rn(acc, row.w);
        } else if (d2 < bound) {
            knn_push(h, k, d2);
            bound = h[0];
        }
    });
}
// One wave per 64 key-adjacent bodies, in one launch:
//   seed     exact distances to the wave's own 64 bodies and the 64 before and after them in key order (Hilbert
//            neighbours, exchanged through readlane) fill the lists, so the first bound is already tight
//   phase 1  walk, pushing every other body's d2 that beats the k-th candidate: the root is then r2_k, the k-th smallest
//            of the multiset (each body is looked at once: no duplicates; ties only ever compare by value)
//   phase 2  mass_k = m_i + the masses at d2 <= r2_k: the seeded ranks again, then a second walk against the fixed bound
// Results land at the body's state row j = perm[rank]; evals (may be null) counts the distances of all three parts.
__global__ __launch_bounds__(kQueryBlock) void k_knn(const Node *__restrict__ nodes, const double4 *__restrict__ rows,
                                                     const int32_t *__restrict__ node_ref, const TreeInfo *__restrict__ info,
                                                     const uint32_t *__restrict__ perm, Bodies cur, int64_t n, int k,
                                                     double *__restrict__ r2_out, double *__restrict__ mass_out,
                                                     unsigned long long *__restrict__ evals_out) {
    extern __shared__ double knn_lds[];  // [k][64]
    const QueryCtx C = query_prologue(info, cur, perm, n);
    if (C.frozen) return;
    const int64_t w0 = C.w0;
    double *h = knn_lds + C.lane;
    for (int s = 0; s < k; s++) h[64 * s] = INFINITY;
    const QueryGroup grp[3] = {C.own, query_group(cur, perm, w0 - 64, n), query_group(cur, perm, w0 + 64, n)};
    const int64_t ex_lo = w0 - 64 > 0 ? w0 - 64 : 0, ex_hi = w0 + 128 < n ? w0 + 128 : n;
    long long evals = 0;
    double bound = INFINITY, acc = 0.0;
    knn_seed(grp, C, n, evals, [&](double d2, double) {
        if (d2 < bound) {
            knn_push(h, k, d2);
            bound = h[0];
        }
    });
    knn_walk<false>(nodes, rows, node_ref, C, ex_lo, ex_hi, h, k, bound, acc, evals);
    const double r2k = bound;
    acc = C.own.m;
    knn_seed(grp, C, n, evals, [&](double d2, double m) {
        if (d2 <= r2k) acc = __dadd_rn(acc, m);
    });
    knn_walk<true>(nodes, rows, node_ref, C, ex_lo, ex_hi, h, k, bound, acc, evals);
    if (C.valid) {
        const uint32_t j = perm[C.rank];
        r2_out[j] = r2k;
        mass_out[j] = acc;
    }
    if (evals_out) nbmi::wave_add(evals_out, evals, C.lane);
}
// state rows -> the caller's order (id), any of the three outputs
__global__ __launch_bounds__(kBlock) void k_knn_out(const double *__restrict__ r2, const double *__restrict__ mass,
                                                    const int32_t *__restrict__ id, int64_t n, double *__restrict__ out_r2,
                                                    double *__restrict__ out_mass, double *__restrict__ out_rho) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const int64_t o = id[r];
    if (out_r2) out_r2[o] = r2[r];
    if (out_mass) out_mass[o] = mass[r];
    if (out_rho) out_rho[o] = knn_density(r2[r], mass[r]);
}


// ---------------------------------------------------------------------------------------
// K17: friends-of-friends groups (nbmi_fof / nbmi_fof_catalogue / nbmi_compute_group_colors; include/nbmi.h, DESIGN.md
// section 4.15).  On top of the shared part: the fixed-radius pair search, a lock-free union-find over key ranks and the
// per-group reductions.
// ---------------------------------------------------------------------------------------
// parent / minid / cnt of every rank
__global__ __launch_bounds__(kBlock) void k_fof_init(int64_t n, int32_t *__restrict__ parent, int32_t *__restrict__ minid,
                                                     int32_t *__restrict__ cnt) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    fof_init(r, parent, minid, cnt);
}
// The pair search: one wave per 64 key-adjacent bodies.  Pairs inside the wave are tested directly (query_half_search);
// every other pair is found by the walk against the fixed bound b2 - a cell is pruned only if query_lower EXCEEDS b2, so a
// pair AT the linking length is always reached.  The cursor starts at the leaf of the wave's first body and the wave's own
// ranks are skipped: the wave sees exactly the bodies of a higher rank, every pair of two waves is found once, by the lower
// wave.
// Every link found goes to fof_link_lanes, which unites the two sets.  evals (may be null) counts the distances evaluated.
__global__ __launch_bounds__(kQueryBlock) void k_fof_link(const Node *__restrict__ nodes, const double4 *__restrict__ rows,
                                                          const int32_t *__restrict__ node_ref, const TreeInfo *__restrict__ info,
                                                          const uint32_t *__restrict__ perm, Bodies cur, int64_t n, double b2,
                                                          const uint32_t *__restrict__ wleaf, int32_t *parent,
                                                          unsigned long long *__restrict__ evals_out) {
    const QueryCtx C = query_prologue(info, cur, perm, n);
    if (C.frozen) return;
    long long evals = 0;
    int mine = (int)C.rank;  // an ancestor of this lane's rank (fof_link_lanes)
    query_half_search(C, n, evals, [&](double d2, int64_t r) { fof_link_lanes(parent, d2 <= b2, mine, (int)r); });
    const unsigned start = __builtin_amdgcn_readfirstlane(wleaf[blockIdx.x]) * kNodeBytes;
    query_walk(nodes, rows, node_ref, start, C, (int64_t)0, C.w0 + kQueryBlock, b2, evals,
               [&](double d2, const double4 &, int64_t r) { fof_link_lanes(parent, d2 <= b2, mine, (int)r); });
    if (evals_out) nbmi::wave_add(evals_out, evals, C.lane);
}
// Behind the kernel boundary parent[] is final and read plainly (fof_flatten): root[r] = the root of r's tree,
// minid[root] = the smallest caller index and cnt[root] = the number of bodies below it.
__global__ __launch_bounds__(kBlock) void k_fof_flatten(const TreeInfo *__restrict__ info, int64_t n,
                                                        const int32_t *__restrict__ parent, const uint32_t *__restrict__ perm,
                                                        const int32_t *__restrict__ id, int32_t *__restrict__ root,
                                                        int32_t *__restrict__ minid, int32_t *__restrict__ cnt) {
    if (tree_frozen(info)) return;
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    fof_flatten(r, n, parent, root, minid, cnt, [&](int64_t q) { return id[perm[q]]; });
}
// label of every body in the caller's order (may be null), and the number of roots
__global__ __launch_bounds__(kBlock) void k_fof_labels(const TreeInfo *__restrict__ info, int64_t n,
                                                       const int32_t *__restrict__ root, const int32_t *__restrict__ minid,
                                                       const uint32_t *__restrict__ perm, const int32_t *__restrict__ id,
                                                       int32_t *__restrict__ labels, unsigned long long *__restrict__ n_roots) {
    if (tree_frozen(info)) return;
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool is_root = r < n && root[r] == (int32_t)r;
    if (r < n && labels) labels[id[perm[r]]] = minid[root[r]];
    const unsigned long long roots = __builtin_amdgcn_ballot_w64(is_root);
    if ((threadIdx.x & 63) == 0 && roots) atomicAdd(n_roots, (unsigned long long)__popcll(roots));
}
// group colours: the speed ramp at a hash of the label for the bodies of a group of at least min_members, grey
// for the others.  Runs behind k_query_restore: a build that did not fit has left its mark in the sticky word.
__global__ __launch_bounds__(kBlock) void k_fof_colors(const TreeInfo *__restrict__ info, int64_t n,
                                                       const int32_t *__restrict__ root, const int32_t *__restrict__ minid,
                                                       const int32_t *__restrict__ cnt, const uint32_t *__restrict__ perm,
                                                       const int32_t *__restrict__ id, int64_t min_members,
                                                       float *__restrict__ colors) {
    if (tree_frozen(info)) return;
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const int32_t f = root[r];
    float cr = 0.25f, cg = 0.25f, cb = 0.25f;
    if ((int64_t)cnt[f] >= min_members)
        color_ramp_t((double)(((uint32_t)minid[f] * 2654435761u) >> 8) / 16777216.0, cr, cg, cb);
    const int64_t o = 3 * (int64_t)id[perm[r]];
    colors[o] = cr; colors[o + 1] = cg; colors[o + 2] = cb;
}

// ---- the catalogue ----------------------------------------------------------------------------------------------
// The ranks are sorted by root (stable: inside a group they stay in key order), so a group is one segment [h, h + cnt)
// of the sorted array.  The array is cut into chunks of kFofChunk entries at fixed positions; a workgroup reduces the
// parts of the segments inside its chunk by a segmented block scan (scan.h's order contract: the tree is fixed), and a
// segment that crosses chunks - a group may hold nearly all the bodies - is put together from its chunks' partials in
// chunk order by one wave (a fixed strided order per lane, then a fixed tree).  No floating-point atomics anywhere:
// two calls on one state give the same bits.
constexpr int kFofChunk = 256;
constexpr int kFofSums = 13;  // M, m x[3], m v[3], x[3], v[3]
constexpr int kFofVals = 19;  // ... then lo[3], hi[3]
struct FofSeg {
    double v;
    int head;  // a segment starts at or in front of this entry (inside the scanned range)
};
__device__ __forceinline__ FofSeg lane_up(const FofSeg &s, int d) { return FofSeg{__shfl_up(s.v, d), __shfl_up(s.head, d)}; }
struct FofMax {
    __device__ double operator()(double a, double b) const { return b > a ? b : a; }
};
template <class Inner>
struct FofSegOp {
    Inner in;
    __device__ FofSeg operator()(const FofSeg &a, const FofSeg &b) const {
        return FofSeg{b.head ? b.v : in(a.v, b.v), a.head | b.head};
    }
};
// what a value of column c is combined by, and its identity
__device__ __forceinline__ double fof_combine(int c, double a, double b) {
    return c < kFofSums ? __dadd_rn(a, b) : c < kFofSums + 3 ? (b < a ? b : a) : (b > a ? b : a);
}
__device__ __forceinline__ double fof_identity(int c) { return c < kFofSums ? 0.0 : c < kFofSums + 3 ? INFINITY : -INFINITY; }

// heads of the segments: where a root's segment begins, and "no catalogue row" until the compaction says otherwise
__global__ __launch_bounds__(kBlock) void k_fof_heads(int64_t n, const uint32_t *__restrict__ key_s, int32_t *__restrict__ hpos,
                                                      int32_t *__restrict__ slot_of) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    const uint32_t k = key_s[e];
    if (e == 0 || key_s[e - 1] != k) {
        hpos[k] = (int32_t)e;
        slot_of[k] = -1;
    }
}
__global__ __launch_bounds__(kBlock) void k_fof_iota(int64_t n, uint32_t *__restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r < n) out[r] = (uint32_t)r;
}
// the qualifying groups in the order of their segments: row `slot` is the group whose segment begins at qhead[slot]
struct FofQualifies {
    const uint32_t *key_s;
    const int32_t *cnt;
    int64_t min_members;
    __device__ unsigned operator()(int64_t first, int64_t n) const {
        return scan::item_mask(first, n, [&](int64_t e) {
            const uint32_t k = key_s[e];
            return (e == 0 || key_s[e - 1] != k) && (int64_t)cnt[k] >= min_members;
        });
    }
};
struct FofEmitHead {
    const uint32_t *key_s;
    int32_t *qhead, *slot_of;
    __device__ void operator()(unsigned m, int64_t first, int64_t slot) const {
        scan::for_each_item(m, first, slot, [&](int64_t e, int64_t row) {
            qhead[row] = (int32_t)e;
            slot_of[key_s[e]] = (int32_t)row;
        });
    }
};
// One workgroup per chunk, one sorted entry per thread.  The scanned value at the LAST entry of a segment's part
// inside the chunk is that part's reduction; it goes
//   to the group's row           if the whole segment lies inside the chunk (and the group has a row),
//   to last_part[chunk]          else if the part ends at the chunk's last entry,
//   to first_part[chunk]         else (the part then begins at the chunk's first entry).
__global__ __launch_bounds__(kFofChunk) void k_fof_chunks(int64_t n, const uint32_t *__restrict__ key_s,
                                                          const uint32_t *__restrict__ rank_s, const uint32_t *__restrict__ perm,
                                                          Bodies cur, const int32_t *__restrict__ hpos,
                                                          const int32_t *__restrict__ cnt, const int32_t *__restrict__ slot_of,
                                                          double *__restrict__ row_vals, double *__restrict__ last_part,
                                                          double *__restrict__ first_part) {
    const int64_t cs = (int64_t)blockIdx.x * kFofChunk, e = cs + threadIdx.x;
    const int64_t ce = cs + kFofChunk - 1 < n - 1 ? cs + kFofChunk - 1 : n - 1;
    const bool in = e < n;
    double val[kFofVals];
#pragma unroll
    for (int c = 0; c < kFofVals; c++) val[c] = fof_identity(c);
    int head = 1;
    int64_t h = 0, end = 0;
    uint32_t k = 0;
    if (in) {
        k = key_s[e];
        h = hpos[k];
        end = h + cnt[k] - 1;
        head = e == h;
        const uint32_t j = perm[rank_s[e]];
        const double m = cur.m[j];
        const double p[3] = {cur.x[j], cur.y[j], cur.z[j]}, v[3] = {cur.vx[j], cur.vy[j], cur.vz[j]};
        val[0] = m;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            val[1 + a] = __dmul_rn(m, p[a]);
            val[4 + a] = __dmul_rn(m, v[a]);
            val[7 + a] = p[a];
            val[10 + a] = v[a];
            val[13 + a] = p[a];
            val[16 + a] = p[a];
        }
    }
#pragma unroll
    for (int c = 0; c < kFofVals; c++) {
        const FofSeg x{val[c], head}, seed{fof_identity(c), 0};
        if (c < kFofSums) val[c] = scan::block_scan<kFofChunk>(x, seed, FofSegOp<scan::Sum>{}).incl.v;
        else if (c < kFofSums + 3) val[c] = scan::block_scan<kFofChunk>(x, seed, FofSegOp<scan::Min>{}).incl.v;
        else val[c] = scan::block_scan<kFofChunk>(x, seed, FofSegOp<FofMax>{}).incl.v;
    }
    if (!in || e != (end < ce ? end : ce)) return;
    double *dst;
    if (h >= cs && end <= ce) {
        const int32_t slot = slot_of[k];
        if (slot < 0) return;
        dst = row_vals + (int64_t)slot * kFofVals;
    } else {
        dst = (e == ce ? last_part : first_part) + (int64_t)blockIdx.x * kFofVals;
    }
#pragma unroll
    for (int c = 0; c < kFofVals; c++) dst[c] = val[c];
}
// One wave per catalogue row: the group's 19 values - its row as k_fof_chunks left it, or its chunks' partials, lane l
// taking the chunks c0 + l, c0 + l + 64, .. in this order, the lanes then combined by the halving tree - and from them
// {M, c[3], v[3], lo[3], hi[3]}, the label and the member count.
__global__ __launch_bounds__(kQueryBlock) void k_fof_rows(int64_t n, int64_t count, const int32_t *__restrict__ qhead,
                                                        const uint32_t *__restrict__ key_s, const int32_t *__restrict__ cnt,
                                                        const int32_t *__restrict__ minid, const double *__restrict__ row_vals,
                                                        const double *__restrict__ last_part,
                                                        const double *__restrict__ first_part, double *__restrict__ out13,
                                                        int32_t *__restrict__ label, int64_t *__restrict__ members) {
    const int64_t slot = blockIdx.x;
    if (slot >= count) return;
    const int lane = threadIdx.x;
    const int64_t e0 = qhead[slot];
    const uint32_t k = key_s[e0];
    const int64_t m = cnt[k], e1 = e0 + m - 1;
    const int64_t c0 = e0 / kFofChunk, c1 = e1 / kFofChunk;
    double val[kFofVals];
    if (c0 == c1) {
#pragma unroll
        for (int c = 0; c < kFofVals; c++) val[c] = row_vals[slot * kFofVals + c];
    } else {
#pragma unroll
        for (int c = 0; c < kFofVals; c++) val[c] = fof_identity(c);
        const int64_t last_of_c1 = c1 * kFofChunk + kFofChunk - 1 < n - 1 ? c1 * kFofChunk + kFofChunk - 1 : n - 1;
        for (int64_t ch = c0 + lane; ch <= c1; ch += kQueryBlock) {
            const double *part = (ch < c1 || e1 == last_of_c1 ? last_part : first_part) + ch * kFofVals;
#pragma unroll
            for (int c = 0; c < kFofVals; c++) val[c] = fof_combine(c, val[c], part[c]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int c = 0; c < kFofVals; c++) val[c] = fof_combine(c, val[c], __shfl_down(val[c], o));
        }
    }
    if (lane != 0) return;
    double *o = out13 + slot * 13;
    const double M = val[0];
    const double div = M != 0.0 ? M : (double)m;  // M == 0: the unweighted means of positions and velocities
    const int from = M != 0.0 ? 1 : 7;
    o[0] = M;
#pragma unroll
    for (int a = 0; a < 6; a++) o[1 + a] = val[from + a] / div;
#pragma unroll
    for (int a = 0; a < 6; a++) o[7 + a] = val[13 + a];
    label[slot] = minid[k];
    members[slot] = m;
}

// ---------------------------------------------------------------------------------------
// K18: exact binned pair counts (nbmi_pair_counts; include/nbmi.h).  On top of the shared part: the
// per-cell body count, an UPPER bound on the computed d2 and with both the cell that is counted whole.
// ---------------------------------------------------------------------------------------
constexpr int kPairMaxBins = 64;  // nb <= 64: nb + 1 edges, nb + 1 counters per lane (`below` and the bins)
struct PairEdges {
    double e2[kPairMaxBins + 1];  // E[k] = edges[k]^2, k <= nb (the rest unused)
};
// cnt[idx] = the number of bodies below node idx: its ranks are [node_ref[idx], node_ref[idx] + cnt[idx]).  The node behind
// the subtree is next_off / kNodeBytes; k_emit_tile gives a subtree that reaches the end of the key order the link
// num_nodes (e = n: nxt = n + pex(n) = total) - the sentinel's row, whose node_ref is -1 and is therefore NOT read: the
// end is recognised by comparing with num_nodes.  A leaf counts 1.
__global__ __launch_bounds__(kBlock) void k_pair_cells(const Node *__restrict__ nodes, const int32_t *__restrict__ node_ref,
                                                       const TreeInfo *__restrict__ info, int64_t n, int64_t capacity,
                                                       int32_t *__restrict__ cnt) {
    if (tree_frozen(info)) return;
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t num_nodes = info->num_nodes;
    if (idx >= num_nodes || idx >= capacity) return;
    const int64_t nx = (int64_t)(nodes[idx].next_off / kNodeBytes);
    const int64_t end = nx >= num_nodes ? n : (int64_t)node_ref[nx];
    cnt[idx] = (int32_t)(end - (int64_t)node_ref[idx]);
}
// query_lower's twin: an upper bound on the COMPUTED d2 between q and every body within `w` per axis of the anchor, so that
// query_lower <= computed d2 <= query_upper for every body of the cell.  u = 2^-53.  Per axis, with T = |q - a| exact and R
// the body's true distance from the anchor on that axis:
//   what the computed |dx| can exceed: nothing beyond (T + R)(1 + u) - it is one rounding of the exact |b - q| <= T + R.
//   t = fl(T) >= T (1 - u), so T <= t (1 + 2 u).  The stored w is NOT below the true reach: that is at most 2 hs + 43
//     half ulps of bounds < 2 hs + 2^-47 bounds (k_query_rows), w is one rounding of 2 hs + 2^-44 bounds (both terms
//     exact), which takes at most u (2 bounds + 2^-44 bounds) < 2^-51 bounds of the 2^-44 bounds.  So R <= w and
//     computed |dx| <= (t + w)(1 + 2 u)(1 + u).
//   s = fl(t + w) >= (t + w)(1 - u);  h = fl(s + s 2^-49) >= s (1 + 16 u)(1 - u) >= (t + w)(1 + 13 u) >= computed |dx|.
//     (The inflation is relative to s, not to t as in query_lower: here the roundings scale with t + w, and w may be the
//     larger part.)
//   five roundings: the computed d2 is <= (sum dx^2)(1 + u)^3 - a product and two sums above each term - with two more
//     (1 + u) from the squared |dx|: <= (sum (T + R)^2)(1 + u)^5 <= (sum (t + w)^2)(1 + 2 u)^2 (1 + u)^5 < (sum (t + w)^2)
//     (1 + 10 u).  The value below is >= (sum h^2)(1 - u)^4 (1 + 2^-48) >= (sum (t + w)^2)(1 + 13 u)^2 (1 - u)^4 (1 + 32 u)
//     > (sum (t + w)^2)(1 + 50 u): a factor five to spare.
//   near the subnormal range: sums and differences are exact there, only products lose their relative bound.  s 2^-49 is
//     inexact only for s < 2^-973; then that axis' |dx| < 2^-971 and its square rounds to 0, which any h^2 >= 0 covers.
//     A value above 2^-960 has a normal largest term, and a subnormal product's absolute error (2^-1075 each, on either
//     side) is below 2^-113 of it: inside the margin.  A value of at most 2^-960 means every h <= 2^-480 (1 + u), every
//     computed |dx| <= h, the computed d2 < 3 x 2^-960 (1 + 4 u) + 3 x 2^-1075 < 2^-958: that is returned instead.
//   An overflow to +inf is harmless: +inf is <= no edge, the cell is never accepted.
//   q may be any finite point, outside the root cube too (nbmi_pair_counts_at: |q| <= 1e18): the statements about w concern
//     the cell alone, those about t, s and h are relative rounding bounds whatever the size of t, and far from the cube t
//     merely dominates w.  Nothing had to be restricted.
__device__ __forceinline__ double query_upper(double4 a, double qx, double qy, double qz) {
    const double sx = __dadd_rn(fabs(__dsub_rn(a.x, qx)), a.w), sy = __dadd_rn(fabs(__dsub_rn(a.y, qy)), a.w),
                 sz = __dadd_rn(fabs(__dsub_rn(a.z, qz)), a.w);
    const double hx = __dadd_rn(sx, __dmul_rn(sx, 0x1p-49)), hy = __dadd_rn(sy, __dmul_rn(sy, 0x1p-49)),
                 hz = __dadd_rn(sz, __dmul_rn(sz, 0x1p-49));
    const double hi = __dmul_rn(__dadd_rn(__dadd_rn(__dmul_rn(hx, hx), __dmul_rn(hy, hy)), __dmul_rn(hz, hz)), 1.0 + 0x1p-48);
    return hi > 0x1p-960 ? hi : 0x1p-958;
}
// the number of E[0 .. nb] that are < v (E strictly increasing, in LDS): 0 = `below`, k + 1 = bin k, nb + 1 = beyond the
// last edge.  An edge that equals v is not below it: the upper edge belongs to the bin.
__device__ __forceinline__ int pair_bin(const double *__restrict__ E, int nb, double v) {
    int pos = 0;
#pragma unroll
    for (int step = 64; step > 0; step >>= 1) {
        const int np = pos + step;
        const bool in = np <= nb + 1;
        if (in && E[in ? np - 1 : 0] < v) pos = np;
    }
    return pos;
}
// The counters of a wave of K18 / K28 and what is done with them.  Dynamic LDS (pair_lds_bytes): E[nb + 1], then nb + 1
// uint32 per lane, [counter][lane] - consecutive lanes, consecutive words, no bank conflicts; a lane counts at most n < 2^31
// bodies.  The E[k] sit in LDS in front of the counters because the search's indices diverge by lane.
struct PairCounters {
    double *E;
    uint32_t *c;  // the lane's column: counter k at c[64 k]
    int nb;
    long long whole;  // bodies this lane counted through whole cells
    __device__ __forceinline__ void init(const PairEdges &edges, int bins, int lane) {
        extern __shared__ double pair_lds[];
        nb = bins;
        whole = 0;
        E = pair_lds;
        c = reinterpret_cast<uint32_t *>(pair_lds + nb + 1) + lane;
        for (int k = 0; k <= nb; k++) {
            E[k] = edges.e2[k];  // (every lane stores the same value)
            c[64 * k] = 0u;
        }
        __syncthreads();
    }
    __device__ __forceinline__ void count(double d2) {
        const int b = pair_bin(E, nb, d2);
        if (b <= nb) c[64 * b]++;
    }
    // An internal cell for an active lane (query_walk_cells' `cell`: true = it stays open), with p = pair_bin(query_lower):
    // pruned if p > nb; counted whole, cnt[idx] bodies into counter p, if accept() and query_upper <= E[p]; else open.
    // accept() is the caller's say on whole cells, asked only about a cell that was not pruned.
    template <class Accept>
    __device__ __forceinline__ bool cell(unsigned idx, const double4 &row, const QueryCtx &C, const int32_t *__restrict__ cnt,
                                         Accept accept) {
        const int p = pair_bin(E, nb, query_lower(row, C.qx, C.qy, C.qz));
        if (p > nb) return false;  // pruned
        if (!accept()) return true;
        if (!(query_upper(row, C.qx, C.qy, C.qz) <= E[p])) return true;
        const uint32_t m = (uint32_t)cnt[idx];
        c[64 * p] += m;
        whole += (long long)m;
        return false;
    }
    // the lane's nb + 1 counters as int32 (K28's row of a point)
    __device__ __forceinline__ void store_row(int32_t *__restrict__ row) const {
        for (int k = 0; k <= nb; k++) row[k] = (int32_t)c[64 * k];
    }
    // every counter summed over the wave in 64 bits and added to out[2 + counter] (nbmi::wave_add); out[0] += distances
    // evaluated, out[1] += bodies counted through whole cells
    __device__ __forceinline__ void flush(unsigned long long *__restrict__ out, long long evals, int lane) const {
        for (int k = 0; k <= nb; k++) nbmi::wave_add(out + 2 + k, (long long)c[64 * k], lane);
        nbmi::wave_add(out, evals, lane);
        nbmi::wave_add(out + 1, whole, lane);
    }
};
constexpr size_t pair_lds_bytes(int nb) { return (size_t)(nb + 1) * (sizeof(double) + kQueryBlock * sizeof(uint32_t)); }
// One wave per 64 key-adjacent bodies, as k_fof_link: pairs inside the wave directly (query_half_search), every other
// pair by the walk that starts at the wave's own first leaf and skips the leaves of the ranks below w0 + 64 - the wave
// sees exactly the bodies of a higher rank, every pair of two waves once.  At an internal cell an active lane, in this order:
//   prunes          if query_lower > E[nb], strictly (a pair AT the last edge is always reached)
//   accepts whole   if query_upper <= E[0] (all of the cell into `below`), or E[k] < query_lower and query_upper <= E[k + 1] (all
//                   of it into bin k): cnt bodies without a distance.  With p = pair_bin(query_lower) both read
//                   query_upper <= E[p], counter p.
//   else keeps the cell open.
// A cell whose ranks reach below w0 + 64 is NEVER accepted whole (it may be pruned): it holds bodies of the wave itself,
// already counted directly, the lane's own among them.  The walk begins behind the leaf of rank w0, so every cell it
// meets starts above w0 and the condition is node_ref < w0 + 64, wave-uniform.  accept = 0 (NBMI_PAIRS_CELLS=0) accepts
// nothing.  Counters and sums: PairCounters.
__global__ __launch_bounds__(kQueryBlock) void k_pair_counts(const Node *__restrict__ nodes, const double4 *__restrict__ rows,
                                                            const int32_t *__restrict__ node_ref,
                                                            const int32_t *__restrict__ cnt, const TreeInfo *__restrict__ info,
                                                            const uint32_t *__restrict__ perm, Bodies cur, int64_t n, int nb,
                                                            PairEdges edges, int accept, const uint32_t *__restrict__ wleaf,
                                                            unsigned long long *__restrict__ out) {
    const QueryCtx C = query_prologue(info, cur, perm, n);
    if (C.frozen) return;
    PairCounters K;
    K.init(edges, nb, C.lane);
    long long evals = 0;
    query_half_search(C, n, evals, [&](double d2, int64_t) { K.count(d2); });
    const unsigned start = __builtin_amdgcn_readfirstlane(wleaf[blockIdx.x]) * kNodeBytes;
    const int64_t own_end = C.w0 + kQueryBlock;
    query_walk_cells(
        nodes, rows, node_ref, start, C, (int64_t)0, own_end, evals,
        [&](unsigned idx, const double4 &row, unsigned) {
            return K.cell(idx, row, C, cnt, [&] { return accept && (int64_t)node_ref[idx] >= own_end; });  // (a cell of the wave's own stays open)
        },
        [&](double d2, const double4 &, int64_t) { K.count(d2); });
    K.flush(out, evals, C.lane);
}

// ---------------------------------------------------------------------------------------
// K28: exact counts of the bodies per distance bin about arbitrary points (nbmi_pair_counts_at; include/nbmi.h, DESIGN.md
// section 4.28).  K18's counting (PairCounters) with K19's lanes: one wave per 64 probes of a chunk, lane `rank` has row
// `rank` of the probe columns (probe_order_chunk), each walking the WHOLE tree from the root - a point is no body, so
// there is no half search, there are no own leaves to skip (ex_lo = ex_hi = 0) and no own-wave condition on a whole
// cell.  At the end a valid lane also stores its nb + 1 counters to row order[rank] of per_point (null: not asked for;
// the stores of a wave are nb + 1 words apart); out accumulates over the chunks of a call.
// ---------------------------------------------------------------------------------------
// a probe in the lane: the query point is row `rank` of the columns, the wave has no bodies of its own
__device__ __forceinline__ QueryCtx query_prologue(const TreeInfo *__restrict__ info, const double *__restrict__ sx,
                                                   const double *__restrict__ sy, const double *__restrict__ sz, int64_t mc) {
    QueryCtx C = query_wave(info, mc);
    C.own = QueryGroup{0.0, 0.0, 0.0, 0.0, C.w0};
    C.qx = C.qy = C.qz = 0.0;
    if (C.valid) { C.qx = sx[C.rank]; C.qy = sy[C.rank]; C.qz = sz[C.rank]; }
    return C;
}
__global__ __launch_bounds__(kQueryBlock) void k_pair_counts_at(const Node *__restrict__ nodes, const double4 *__restrict__ rows,
                                                               const int32_t *__restrict__ node_ref,
                                                               const int32_t *__restrict__ cnt, const TreeInfo *__restrict__ info,
                                                               const double *__restrict__ sx, const double *__restrict__ sy,
                                                               const double *__restrict__ sz, const uint32_t *__restrict__ order,
                                                               int64_t mc, int nb, PairEdges edges, int accept,
                                                               int32_t *__restrict__ per_point,
                                                               unsigned long long *__restrict__ out) {
    if (tree_frozen(info)) return;  // (before the lane loads its point)
    const QueryCtx C = query_prologue(info, sx, sy, sz, mc);
    PairCounters K;
    K.init(edges, nb, C.lane);
    long long evals = 0;
    query_walk_cells(
        nodes, rows, node_ref, 0u, C, (int64_t)0, (int64_t)0, evals,
        [&](unsigned idx, const double4 &row, unsigned) { return K.cell(idx, row, C, cnt, [&] { return accept != 0; }); },
        [&](double d2, const double4 &, int64_t) { K.count(d2); });
    if (per_point && C.valid) K.store_row(per_point + (order ? (int64_t)order[C.rank] : C.rank) * (nb + 1));
    K.flush(out, evals, C.lane);
}

// ---------------------------------------------------------------------------------------
// K29: the exact Euclidean minimum spanning tree (nbmi_mst; include/nbmi.h).  Boruvka rounds on
// top of the shared query part: per round every body finds its least foreign pair under the key (d2, min id, max id) -
// the search, k_mst_search - every component the least of its bodies' pairs (two passes of 64-bit atomic minima), and
// the winning pairs are appended to the edge list and united (unionfind.h).  Components live in key-rank space: comp[r]
// is the root rank of r's set, flattened behind every round.  Everything one kernel reads of what other waves write -
// comp, the cells' tags, the components' minima - was written before a kernel boundary; the only words touched across
// waves INSIDE a kernel are the atomic minima (nobody reads them there) and parent[] in k_mst_emit, through fof_unite's
// relaxed agent-scope atomics as unionfind.h (d) requires.  So no wave sees another's progress and evals is a function of
// the state.
// ---------------------------------------------------------------------------------------
constexpr unsigned long long kMstNone = 0x7fffffffffffffffull;  // above the bits of every finite d2 >= 0 and every packed pair
// the unordered pair of caller indices a, b as one word that orders as (min, max)
__device__ __forceinline__ unsigned long long mst_pack(uint32_t a, uint32_t b) {
    return a < b ? ((unsigned long long)a << 32) | b : ((unsigned long long)b << 32) | a;
}
// dst[c] = min(dst[c], v) for the lanes with `on`.  Key-adjacent bodies mostly share their component: the lanes that share
// the first such lane's go in as one atomic, the others on their own (fof_flatten's pattern, one round of it).
__device__ __forceinline__ void mst_wave_min(unsigned long long *dst, int c, unsigned long long v, bool on) {
    const unsigned long long todo = __builtin_amdgcn_ballot_w64(on);
    if (todo == 0ull) return;
    const int lane = threadIdx.x & 63;
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
    const int c0 = __builtin_amdgcn_readlane(c, leader);
    const bool with = on && c == c0;
    long long least = with ? (long long)v : (long long)kMstNone;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long other = __shfl_xor(least, o);
        least = other < least ? other : least;
    }
    if (lane == leader) (void)__hip_atomic_fetch_min(dst + c0, (unsigned long long)least, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (on && !with) (void)__hip_atomic_fetch_min(dst + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// every rank a component of its own; rid[r] = the caller index of rank r
__global__ __launch_bounds__(kBlock) void k_mst_init(const TreeInfo *__restrict__ info, int64_t n, const uint32_t *__restrict__ perm,
                                                     const int32_t *__restrict__ id, int32_t *__restrict__ parent,
                                                     int32_t *__restrict__ comp, int32_t *__restrict__ rid,
                                                     double *__restrict__ bd2, int32_t *__restrict__ bpart,
                                                     unsigned long long *__restrict__ cmin, unsigned long long *__restrict__ cpair) {
    if (tree_frozen(info)) return;
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    parent[r] = (int32_t)r;
    comp[r] = (int32_t)r;
    rid[r] = id[perm[r]];
    bd2[r] = INFINITY;
    bpart[r] = -1;
    cmin[r] = kMstNone;
    cpair[r] = kMstNone;
}
// diff[r] = rank r + 1 exists and lies in another component; its exclusive scan S tells every run of ranks whether it is
// uniform: [a, a + c) holds one component iff S[a + c - 1] == S[a]
__global__ __launch_bounds__(kBlock) void k_mst_diff(const TreeInfo *__restrict__ info, int64_t n, const int32_t *__restrict__ comp,
                                                     int32_t *__restrict__ diff) {
    if (tree_frozen(info)) return;
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    diff[r] = r + 1 < n && comp[r] != comp[r + 1] ? 1 : 0;
}
// ctag[idx] = the component of node idx if all the bodies below it (k_pair_cells' cnt) share one, else -1; a leaf's tag is
// its body's component.  All nodes at once: no pass per level.
__global__ __launch_bounds__(kBlock) void k_mst_tags(const int32_t *__restrict__ node_ref, const int32_t *__restrict__ cnt,
                                                     const TreeInfo *__restrict__ info, int64_t n, int64_t capacity,
                                                     const int32_t *__restrict__ comp, const int32_t *__restrict__ dscan,
                                                     int32_t *__restrict__ ctag) {
    if (tree_frozen(info)) return;
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= info->num_nodes || idx >= capacity) return;
    const int64_t a = node_ref[idx], c = cnt[idx];
    const bool ok = a >= 0 && c >= 1 && a + c <= n;
    ctag[idx] = ok && dscan[a + c - 1] == dscan[a] ? comp[a] : -1;
}
// The search: one wave per 64 key-adjacent bodies, one body per lane, k_knn's shape.  A lane keeps its least foreign pair
// (best, bpack, bp = the partner's rank) under the full key and `bound`, an upper bound on the d2 of that pair.
//   seed   the wave's own bodies and the 64 ranks on either side, by readlane (knn_seed's pattern), foreign ones only
//   walk   from the root.  A cell is closed for a lane if it is uniform in the lane's own component (nothing foreign in
//          it) or if query_lower EXCEEDS bound - strictly, so a pair that ties the best in d2 is always reached and then
//          decided by the indices.  A cell that stays open is not uniform in the lane's component, so it holds a foreign
//          body, and query_upper of it bounds the least foreign d2 from above before any leaf is seen: bound may drop to
//          it.  That only ever lowers a true upper bound, so the strict pruning stays exact.  A leaf of the own component
//          is skipped, every other compared under the full key.
//   carry  (kCarry: every round but the first) components only grow, so a body's least foreign pair of the last round is
//          still its least if that partner is still foreign: such a lane does not search again, and a wave without a lane
//          left to search goes straight to the minimum.  The lanes that do search first take a bound from their own
//          ancestors (below).
// Then the component minimum's first pass: the bits of best d2 (a finite double >= 0 orders as its bits, as k_mr_keys
// relies on) into cmin[component].
template <bool kCarry>
__global__ __launch_bounds__(kQueryBlock) void k_mst_search(const Node *__restrict__ nodes, const double4 *__restrict__ rows,
                                                            const int32_t *__restrict__ node_ref, const TreeInfo *__restrict__ info,
                                                            const uint32_t *__restrict__ perm, Bodies cur, int64_t n,
                                                            const int32_t *__restrict__ comp, const int32_t *__restrict__ rid,
                                                            const int32_t *__restrict__ ctag, const int32_t *__restrict__ cnt,
                                                            double *__restrict__ bd2, int32_t *__restrict__ bpart,
                                                            unsigned long long *cmin,
                                                            unsigned long long *__restrict__ evals_out) {
    QueryCtx C = query_prologue(info, cur, perm, n);
    if (C.frozen) return;
    const int64_t w0 = C.w0;
    const bool has = C.valid;
    const int mine = has ? comp[C.rank] : -1;
    const uint32_t myid = has ? (uint32_t)rid[C.rank] : 0u;
    double best = INFINITY;
    unsigned long long bpack = kMstNone;
    int bp = -1;
    bool search = has;
    if (kCarry && has) {
        const int last = bpart[C.rank];
        if (last >= 0 && comp[last] != mine) {
            search = false;
            bp = last;
            best = bd2[C.rank];
        }
    }
    long long evals = 0;
    if (__builtin_amdgcn_ballot_w64(search) != 0ull) {
        C.valid = search;  // the lanes that carry their pair over sit the search out
        double bound = INFINITY;
        auto consider = [&](double d2, uint32_t oid, int64_t r) {
            const unsigned long long pack = mst_pack(myid, oid);
            if (d2 < best || (d2 == best && pack < bpack)) {
                best = d2;
                bpack = pack;
                bp = (int)r;
                bound = d2 < bound ? d2 : bound;
            }
        };
        const QueryGroup grp[3] = {C.own, query_group(cur, perm, w0 - 64, n), query_group(cur, perm, w0 + 64, n)};
        const int64_t ex_lo = w0 - 64 > 0 ? w0 - 64 : 0, ex_hi = w0 + 128 < n ? w0 + 128 : n;
#pragma unroll
        for (int g = 0; g < 3; g++) {
            const int64_t gr = grp[g].base + C.lane;
            const bool in = gr >= 0 && gr < n;
            const int gc = in ? comp[gr] : -1, gi = in ? rid[gr] : 0;
            for (int i = 0; i < 64; i++) {
                const int64_t r = grp[g].base + i;
                if (r < 0 || r >= n) continue;
                const double d2 = query_d2(query_bcast(grp[g].x, i), query_bcast(grp[g].y, i), query_bcast(grp[g].z, i), C.qx, C.qy, C.qz);
                const int oc = __builtin_amdgcn_readlane(gc, i), oi = __builtin_amdgcn_readlane(gi, i);
                if (search && oc != mine) {
                    evals++;
                    consider(d2, (uint32_t)oi, r);
                }
            }
        }
        if (kCarry) {
            // Behind the first round the seeds are mostly of the lane's own component and leave no bound, and the walk
            // below meets the cells in key order, not nearest first.  So first down the lane's own ancestors only - the
            // cells whose ranks hold the lane's - as far as they are not uniform: the smallest of them that holds a
            // foreign body bounds the lane's pair by query_upper.  No leaf is looked at (all ranks excluded).
            query_walk_cells(
                nodes, rows, node_ref, 0u, C, (int64_t)0, n, evals,
                [&](unsigned idx, const double4 &row, unsigned) {
                    const int64_t a = node_ref[idx];
                    if (C.rank < a || C.rank >= a + cnt[idx] || ctag[idx] == mine) return false;
                    const double up = query_upper(row, C.qx, C.qy, C.qz);
                    bound = up < bound ? up : bound;
                    return true;
                },
                [&](double, const double4 &, int64_t) {});
        }
        query_walk_cells(
            nodes, rows, node_ref, 0u, C, ex_lo, ex_hi, evals,
            [&](unsigned idx, const double4 &row, unsigned) {
                if (ctag[idx] == mine) return false;
                if (query_lower(row, C.qx, C.qy, C.qz) > bound) return false;
                const double up = query_upper(row, C.qx, C.qy, C.qz);
                bound = up < bound ? up : bound;
                return true;
            },
            [&](double d2, const double4 &, int64_t r) {
                if (comp[r] != mine) consider(d2, (uint32_t)rid[r], r);
            });
        if (search) {
            bd2[C.rank] = best;
            bpart[C.rank] = bp;
        }
    }
    mst_wave_min(cmin, mine, (unsigned long long)__double_as_longlong(best), has && bp >= 0);
    if (evals_out) nbmi::wave_add(evals_out, evals, threadIdx.x);
}
// The component minimum's second pass, behind the kernel boundary that made cmin final: among the bodies that hold their
// component's least d2, the least packed pair into cpair[component].
__global__ __launch_bounds__(kBlock) void k_mst_pick(const TreeInfo *__restrict__ info, int64_t n, const int32_t *__restrict__ comp,
                                                     const int32_t *__restrict__ rid, const double *__restrict__ bd2,
                                                     const int32_t *__restrict__ bpart, const unsigned long long *__restrict__ cmin,
                                                     unsigned long long *cpair) {
    if (tree_frozen(info)) return;
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int c = -1;
    unsigned long long pack = kMstNone;
    bool on = false;
    if (r < n) {
        c = comp[r];
        const int bp = bpart[r];
        if (bp >= 0 && (unsigned long long)__double_as_longlong(bd2[r]) == cmin[c]) {
            on = true;
            pack = mst_pack((uint32_t)rid[r], (uint32_t)rid[bp]);
        }
    }
    mst_wave_min(cpair, c, pack, on);
}
// Emit and unite, behind the boundary that made cpair final.  A component's winning pair {i, j} has exactly one body in
// the component - the other is foreign - so exactly one lane of the grid holds (cmin, cpair) of its component: that
// lane, not the root's, appends the edge and unites the two sets.  Two components that chose each other chose the same
// pair (the order is total and both minimise over a set that holds it), and then both winning lanes are the two ends of
// that pair: only the end with the smaller caller index appends it.  A pair that is the minimum of one component only is
// appended by that component's lane; so every chosen pair is appended once, none twice.  The slot comes from an integer
// counter; the order of the list is settled by the sort behind the rounds.  parent[] is touched through fof_unite alone.
__global__ __launch_bounds__(kBlock) void k_mst_emit(const TreeInfo *__restrict__ info, int64_t n, const int32_t *__restrict__ comp,
                                                     const int32_t *__restrict__ rid, const double *__restrict__ bd2,
                                                     const int32_t *__restrict__ bpart, const unsigned long long *__restrict__ cmin,
                                                     const unsigned long long *__restrict__ cpair, int32_t *parent,
                                                     unsigned long long *__restrict__ e_pack, unsigned long long *__restrict__ e_d2,
                                                     unsigned long long *count) {
    if (tree_frozen(info)) return;
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const int bp = bpart[r];
    if (bp < 0) return;
    const int c = comp[r];
    const unsigned long long bits = (unsigned long long)__double_as_longlong(bd2[r]);
    if (bits != cmin[c]) return;
    const unsigned long long pack = mst_pack((uint32_t)rid[r], (uint32_t)rid[bp]);
    if (pack != cpair[c]) return;
    const int c2 = comp[bp];
    const bool mutual = cmin[c2] == bits && cpair[c2] == pack;
    if (!mutual || rid[r] < rid[bp]) {
        const unsigned long long slot = atomicAdd(count, 1ull);
        if (slot < (unsigned long long)(n - 1)) {  // (a tree has no more edges: nothing is ever written behind the list)
            e_pack[slot] = pack;
            e_d2[slot] = bits;
        }
    }
    (void)fof_unite(parent, (int)r, bp);
}
// Behind the boundary parent[] is final and read plainly: the next round's components, and its minima cleared.
__global__ __launch_bounds__(kBlock) void k_mst_flatten(const TreeInfo *__restrict__ info, int64_t n,
                                                        const int32_t *__restrict__ parent, int32_t *__restrict__ comp,
                                                        unsigned long long *__restrict__ cmin, unsigned long long *__restrict__ cpair) {
    if (tree_frozen(info)) return;
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    int f = (int)r;
    for (int p = parent[f]; p != f; p = parent[f]) f = p;
    comp[r] = f;
    cmin[r] = kMstNone;
    cpair[r] = kMstNone;
}
// the final order's helpers: 0 .. m - 1;  key[k] = d2 of the edge at `order[k]`;  the sorted list in the caller's arrays
__global__ __launch_bounds__(kBlock) void k_mst_gather(int64_t m, const uint32_t *__restrict__ order,
                                                       const unsigned long long *__restrict__ e_d2, uint64_t *__restrict__ key) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < m) key[k] = e_d2[order[k]];
}
__global__ __launch_bounds__(kBlock) void k_mst_out(int64_t m, const uint32_t *__restrict__ order, const uint64_t *__restrict__ key,
                                                    const unsigned long long *__restrict__ e_pack, int32_t *__restrict__ edge_i,
                                                    int32_t *__restrict__ edge_j, double *__restrict__ edge_d2) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= m) return;
    const unsigned long long pack = e_pack[order[k]];
    edge_i[k] = (int32_t)(pack >> 32);
    edge_j[k] = (int32_t)(pack & 0xffffffffull);
    edge_d2[k] = __longlong_as_double((long long)key[k]);
}

// ---------------------------------------------------------------------------------------
// K19: the field at arbitrary points (nbmi_field_at; include/nbmi.h).
// The probe walk of K14 (field_walk) with a probe in the lane instead of a body, the acceleration summed as well.  Which
// probes share a wave - the sort below, the chunks of the call, the other points - decides the speed of a call and never
// a bit of its result.
// ---------------------------------------------------------------------------------------
// A call is cut into chunks of at most this many points: the scratch never holds more.
constexpr int64_t kFieldChunk = 1048576;
constexpr int64_t kFieldMinRows = 1024;  // smallest scratch (rows double from here up to the chunk)
constexpr int kFieldSortBits = 40;       // the sort looks at the top 40 key bits, as the build of a million bodies does

// Sort key of a probe: the digits of k_keys (key_word, the handle's curve) in the tree's root cube, coordinates outside
// the cube clamped to its faces.  pts: the chunk, (m, 3).
template <bool kHilbert>
__global__ __launch_bounds__(kBlock) void k_field_keys(const double *__restrict__ pts, int64_t m, const TreeInfo *__restrict__ info,
                                                       uint64_t *__restrict__ key, uint32_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const double b = info->bounds;
    const double px = fmin(fmax(pts[3 * i], -b), b), py = fmin(fmax(pts[3 * i + 1], -b), b), pz = fmin(fmax(pts[3 * i + 2], -b), b);
    double cx = 0.0, cy = 0.0, cz = 0.0, hs = b;
    unsigned st = 0u;
    key[i] = key_word<kHilbert>(px, py, pz, cx, cy, cz, hs, st, nbmi::kHilDigit, nbmi::kHilNext);
    idx[i] = (uint32_t)i;
}

// The probes of a chunk as columns in walk order: rank r holds point order[r] (order == null: point r).
__global__ __launch_bounds__(kBlock) void k_field_gather(const double *__restrict__ pts, const uint32_t *__restrict__ order, int64_t m,
                                                         double *__restrict__ sx, double *__restrict__ sy, double *__restrict__ sz) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= m) return;
    const int64_t i = order ? (int64_t)order[r] : r;
    sx[r] = pts[3 * i]; sy[r] = pts[3 * i + 1]; sz[r] = pts[3 * i + 2];
}

// One chunk of probes through the probe walk (field_walk, K14): lane `rank` has row `rank` of the probe columns, which
// `tab` names as buffer 0 (probe_alloc); pmax is the call's largest |coordinate|.  Results land at the probe's row of the
// chunk, order[rank].
template <bool kQuad>
__global__ __launch_bounds__(kBlock) void k_field_tree(const Node *__restrict__ nodes, const double4 *__restrict__ pot,
                                                       const WalkTable *tab, const TreeInfo *info,
                                                       const double *__restrict__ sx, const double *__restrict__ sy,
                                                       const double *__restrict__ sz, const uint32_t *__restrict__ order, int64_t m,
                                                       float eps2f, double eps, double pmax, const double *__restrict__ quad,
                                                       double *__restrict__ acc_out, double *__restrict__ phi_out,
                                                       int32_t *__restrict__ cnt_out) {
    if (tree_frozen(info)) return;  // the tree did not fit: the caller reports it
    const int64_t rank = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = rank < m;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (valid) { qx = sx[rank]; qy = sy[rank]; qz = sz[rank]; }
    const FieldSum f = field_walk<kQuad, true, true>(nodes, pot, info, Body64{tab, 0, (uint32_t)(valid ? rank : 0)}, qx, qy, qz, (float)qx,
                                                     (float)qy, (float)qz, valid, eps2f, eps, pmax, quad);
    if (valid) {
        const int64_t o = order ? (int64_t)order[rank] : rank;
        if (acc_out) { acc_out[3 * o] = f.ax; acc_out[3 * o + 1] = f.ay; acc_out[3 * o + 2] = f.az; }
        if (phi_out) phi_out[o] = f.phi;
        if (cnt_out) cnt_out[o] = f.terms;
    }
}

// Direct handle: the sum over all bodies in body order (direct_tiles) with a point in the thread.  The only guard is the
// definition's dist_sq > eps^2.
// The sum itself, shared by k_field_direct and k_tracer_direct; every thread of the block calls it (`tile`: kBlock rows of
// shared memory).
__device__ __forceinline__ FieldSum field_direct_sum(const Bodies &cur, int64_t n, double G, double eps2, double x, double y, double z,
                                                     double4 *tile) {
    double ax = 0.0, ay = 0.0, az = 0.0, phi = 0.0;
    int32_t terms = 0;
    direct_tiles(cur, n, G, tile, [&](const double4 &q, int64_t) {
        const double ex = q.x - x, ey = q.y - y, ez = q.z - z;
        const double d2 = ex * ex + ey * ey + ez * ez + eps2;
        if (d2 > eps2) {
            const double dist = sqrt(d2);
            const double w = q.w / (dist * d2);
            phi -= q.w / dist;
            ax += ex * w; ay += ey * w; az += ez * w;
            terms++;
        }
    });
    return FieldSum{ax, ay, az, phi, terms};
}

__global__ __launch_bounds__(kBlock) void k_field_direct(Bodies cur, int64_t n, double G, double eps2, const double *__restrict__ pts,
                                                         int64_t m, double *__restrict__ acc_out, double *__restrict__ phi_out,
                                                         int32_t *__restrict__ cnt_out) {
    __shared__ double4 tile[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = i < m;
    double x = 0.0, y = 0.0, z = 0.0;
    if (valid) { x = pts[3 * i]; y = pts[3 * i + 1]; z = pts[3 * i + 2]; }
    const FieldSum f = field_direct_sum(cur, n, G, eps2, x, y, z, tile);
    if (valid) {
        if (acc_out) { acc_out[3 * i] = f.ax; acc_out[3 * i + 1] = f.ay; acc_out[3 * i + 2] = f.az; }
        if (phi_out) phi_out[i] = f.phi;
        if (cnt_out) cnt_out[i] = f.terms;
    }
}

// ---------------------------------------------------------------------------------------
// K27: the tidal tensor T_ab = da_a/dx_b at points and at the bodies (nbmi_tidal_at / nbmi_get_tidal_f64; include/nbmi.h,
// DESIGN.md section 4.27).  The probe walk's tidal instantiation (field_walk<.., kTidal>) under K19's and K14's two lane
// setups; rows are {Txx, Tyy, Tzz, Txy, Txz, Tyz}.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void tidal_store(double *__restrict__ out, int64_t o, const TidalSum &f) {
    double *r = out + 6 * o;
    r[0] = f.xx; r[1] = f.yy; r[2] = f.zz; r[3] = f.xy; r[4] = f.xz; r[5] = f.yz;
}
// The Frobenius norm of a row, in the header's association.
__device__ __forceinline__ double tidal_norm(const TidalSum &f) {
    return sqrt(((f.xx * f.xx + f.yy * f.yy) + f.zz * f.zz) + 2.0 * ((f.xy * f.xy + f.xz * f.xz) + f.yz * f.yz));
}

// One chunk of probes, the lane as k_field_tree's; results at the probe's row of the chunk.
template <bool kQuad>
__global__ __launch_bounds__(kBlock) void k_tidal_tree(const Node *__restrict__ nodes, const double4 *__restrict__ pot,
                                                       const WalkTable *tab, const TreeInfo *info,
                                                       const double *__restrict__ sx, const double *__restrict__ sy,
                                                       const double *__restrict__ sz, const uint32_t *__restrict__ order, int64_t m,
                                                       float eps2f, double eps, double pmax, const double *__restrict__ quad,
                                                       double *__restrict__ t6_out, int32_t *__restrict__ cnt_out) {
    if (tree_frozen(info)) return;  // the tree did not fit: the caller reports it
    const int64_t rank = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = rank < m;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (valid) { qx = sx[rank]; qy = sy[rank]; qz = sz[rank]; }
    const TidalSum f = field_walk<kQuad, false, true, true>(nodes, pot, info, Body64{tab, 0, (uint32_t)(valid ? rank : 0)}, qx, qy, qz,
                                                            (float)qx, (float)qy, (float)qz, valid, eps2f, eps, pmax, quad);
    if (valid) {
        const int64_t o = order ? (int64_t)order[rank] : rank;
        if (t6_out) tidal_store(t6_out, o, f);
        if (cnt_out) cnt_out[o] = f.terms;
    }
}

// A body in the lane (lane_prologue, as k_potential_tree), the build's band.  Rows land in the caller's order, id[j] (either output
// may be null).
template <bool kQuad>
__global__ __launch_bounds__(kBlock) void k_tidal_bodies(const Node *__restrict__ nodes, const double4 *__restrict__ pot,
                                                         const WalkTable *tab, const TreeInfo *info,
                                                         const float4 *__restrict__ posm_s, const uint32_t *__restrict__ perm,
                                                         int curbuf, float eps2f, int64_t n, const int32_t *__restrict__ id,
                                                         double *__restrict__ t6_out, double *__restrict__ norm_out,
                                                         const double *__restrict__ quad) {
    if (tree_frozen(info)) return;  // the tree did not fit: the caller reports it
    const int64_t rank = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const WalkCtx C = lane_prologue(nodes, posm_s, perm, rank, n, info, tab, curbuf);
    const Lane64 L = lane_f64(C);
    const TidalSum f = field_walk<kQuad, false, false, true>(nodes, pot, info, C.b64, L.qx, L.qy, L.qz, C.px, C.py, C.pz, C.valid, eps2f,
                                                             0.0, 0.0, quad);
    if (C.valid) {
        const int64_t o = id[C.j];
        if (t6_out) tidal_store(t6_out, o, f);
        if (norm_out) norm_out[o] = tidal_norm(f);
    }
}

// Direct handle: the sum over all bodies in body order (direct_tiles) with the one guard dist_sq > eps^2.
// pts != null: point i of (m, 3) rows, results at row i.  pts == null: state row i of the m = n bodies (its own term
// has d = 0 and is dropped by the guard), results at the caller's row id[i].
__global__ __launch_bounds__(kBlock) void k_tidal_direct(Bodies cur, int64_t n, double G, double eps2, const double *__restrict__ pts,
                                                         int64_t m, double *__restrict__ t6_out, double *__restrict__ norm_out,
                                                         int32_t *__restrict__ cnt_out) {
    __shared__ double4 tile[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = i < m;
    double x = 0.0, y = 0.0, z = 0.0;
    if (valid) {
        if (pts) { x = pts[3 * i]; y = pts[3 * i + 1]; z = pts[3 * i + 2]; }
        else { x = cur.x[i]; y = cur.y[i]; z = cur.z[i]; }
    }
    TidalSum f{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0};
    direct_tiles(cur, n, G, tile, [&](const double4 &q, int64_t) {
        const double ex = q.x - x, ey = q.y - y, ez = q.z - z;
        const double d2 = ex * ex + ey * ey + ez * ez + eps2;
        if (d2 > eps2) {
            const double dist = sqrt(d2);
            const double w = q.w / (dist * d2), w5 = (3.0 * w) / d2;
            f.xx += (ex * ex) * w5 - w; f.yy += (ey * ey) * w5 - w; f.zz += (ez * ez) * w5 - w;
            f.xy += (ex * ey) * w5; f.xz += (ex * ez) * w5; f.yz += (ey * ez) * w5;
            f.terms++;
        }
    });
    if (valid) {
        const int64_t o = pts ? i : (int64_t)cur.id[i];
        if (t6_out) tidal_store(t6_out, o, f);
        if (norm_out) norm_out[o] = tidal_norm(f);
        if (cnt_out) cnt_out[o] = f.terms;
    }
}

// ---------------------------------------------------------------------------------------
// K20: massless tracers carried by the integrator (nbmi_set_tracers; include/nbmi.h).
// The probe walks of K19 with the handle's integrator as their epilogue, on the tree the step has just built.  State:
// p, v (and the leapfrog's a), (m, 3) float64 rows in the caller's order.  kLeap: 0 = kick-drift, kLeapClose = the
// leapfrog's closing half-kick (a is stored), kLeapPrime = a = F(p) stored, state untouched.
// ---------------------------------------------------------------------------------------
constexpr int64_t kTracerMax = (int64_t)1 << 26;  // the largest m nbmi_set_tracers accepts

// A retired tracer's row is left alone: a position beyond 1e18 (nbmi_field_at's limit) or anything that is not finite.
__device__ __forceinline__ bool tracer_live(double px, double py, double pz, double vx, double vy, double vz) {
    return fabs(px) <= 1e18 && fabs(py) <= 1e18 && fabs(pz) <= 1e18 && isfinite(vx) && isfinite(vy) && isfinite(vz);
}

// The largest |coordinate| the tracers have reached since nbmi_set_tracers, as the bit pattern of a non-negative double
// (k_field_tree's pmax, kept on the device: it only ever grows, and a band wider than needed changes no decision).  One
// atomic per wave, and only where it would raise the word.  Positions of tracers that retire with this move do not count.
__device__ __forceinline__ void tracer_raise_pmax(unsigned long long *pmax, bool moved, double px, double py, double pz) {
    double mx = moved ? fmax(fmax(fabs(px), fabs(py)), fabs(pz)) : 0.0;
    mx = mx <= 1e18 ? mx : 0.0;  // (a NaN fails the comparison too)
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(mx);
        if (bits > __atomic_load_n(pmax, __ATOMIC_RELAXED)) atomicMax(pmax, bits);
    }
}

// What the integrator does with a = F(p) of one live tracer, row o.  Returns whether p moved.
template <int kLeap>
__device__ __forceinline__ bool tracer_epilogue(double *__restrict__ p, double *__restrict__ v, double *__restrict__ a, int64_t o,
                                                double &px, double &py, double &pz, double vx, double vy, double vz,
                                                const FieldSum &f, double dt, double damping) {
    if (kLeap != 0) { a[3 * o] = f.ax; a[3 * o + 1] = f.ay; a[3 * o + 2] = f.az; }
    if (kLeap == kLeapPrime) return false;
    const double k = kLeap == kLeapClose ? 0.5 * dt : dt;
    vx = (vx + f.ax * k) * damping; vy = (vy + f.ay * k) * damping; vz = (vz + f.az * k) * damping;
    v[3 * o] = vx; v[3 * o + 1] = vy; v[3 * o + 2] = vz;
    if (kLeap != 0) return false;
    px = px + vx * dt; py = py + vy * dt; pz = pz + vz * dt;
    p[3 * o] = px; p[3 * o + 1] = py; p[3 * o + 2] = pz;
    return true;
}

// One chunk of tracers on the tree that stands: lane `rank` walks the probe of the sorted columns (k_field_gather of the
// chunk's rows of p) and integrates row order[rank] of the chunk (p, v, a: the chunk's first row).  Writing p in place is
// safe: opening()'s float64 re-decision reads the sorted copies.
template <bool kQuad, int kLeap>
__global__ __launch_bounds__(kBlock) void k_tracer_tree(const Node *__restrict__ nodes, const double4 *__restrict__ pot,
                                                        const WalkTable *tab, const TreeInfo *info,
                                                        const double *__restrict__ sx, const double *__restrict__ sy,
                                                        const double *__restrict__ sz, const uint32_t *__restrict__ order, int64_t m,
                                                        float eps2f, double eps, unsigned long long *pmax_word,
                                                        const double *__restrict__ quad, double *__restrict__ p,
                                                        double *__restrict__ v, double *__restrict__ a, double dt, double damping) {
    if (tree_frozen(info)) return;  // the tree did not fit: neither bodies nor tracers advance
    const int64_t rank = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool inside = rank < m;
    double qx = 0.0, qy = 0.0, qz = 0.0, vx = 0.0, vy = 0.0, vz = 0.0;
    int64_t o = 0;
    if (inside) {
        o = order ? (int64_t)order[rank] : rank;
        qx = sx[rank]; qy = sy[rank]; qz = sz[rank];
        vx = v[3 * o]; vy = v[3 * o + 1]; vz = v[3 * o + 2];
    }
    const bool live = inside && tracer_live(qx, qy, qz, vx, vy, vz);
    const double pmax = __longlong_as_double((long long)__atomic_load_n(pmax_word, __ATOMIC_RELAXED));
    const FieldSum f = field_walk<kQuad, true, true>(nodes, pot, info, Body64{tab, 0, (uint32_t)(inside ? rank : 0)}, qx, qy, qz, (float)qx,
                                                     (float)qy, (float)qz, live, eps2f, eps, pmax, quad);
    bool moved = false;
    if (live) moved = tracer_epilogue<kLeap>(p, v, a, o, qx, qy, qz, vx, vy, vz, f, dt, damping);
    if (kLeap == 0) tracer_raise_pmax(pmax_word, moved, qx, qy, qz);
}

// Direct handle (and any handle without bodies: a = 0): all m tracers in the caller's order, k_field_direct's sum.
template <int kLeap>
__global__ __launch_bounds__(kBlock) void k_tracer_direct(Bodies cur, int64_t n, double G, double eps2, int64_t m,
                                                          double *__restrict__ p, double *__restrict__ v, double *__restrict__ a,
                                                          double dt, double damping) {
    __shared__ double4 tile[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool inside = i < m;
    double x = 0.0, y = 0.0, z = 0.0, vx = 0.0, vy = 0.0, vz = 0.0;
    if (inside) {
        x = p[3 * i]; y = p[3 * i + 1]; z = p[3 * i + 2];
        vx = v[3 * i]; vy = v[3 * i + 1]; vz = v[3 * i + 2];
    }
    const FieldSum f = field_direct_sum(cur, n, G, eps2, x, y, z, tile);
    if (inside && tracer_live(x, y, z, vx, vy, vz)) tracer_epilogue<kLeap>(p, v, a, i, x, y, z, vx, vy, vz, f, dt, damping);
}

// [leapfrog] The tracers' opening half-kick and drift, in place: v = v + a dt/2, p = p + v dt.  info (Barnes-Hut): the
// header of the substep's tree - a build that did not fit leaves the tracers where they were, as it leaves the bodies.
// pmax (Barnes-Hut): see tracer_raise_pmax; every thread of the grid takes part in its wave's maximum.
__global__ __launch_bounds__(kBlock) void k_tracer_kick_drift(const TreeInfo *info, int64_t m, double *__restrict__ p,
                                                              double *__restrict__ v, const double *__restrict__ a, double dt,
                                                              unsigned long long *pmax) {
    if (info && tree_frozen(info)) return;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const double h = 0.5 * dt;
    bool moved = false;
    double x = 0.0, y = 0.0, z = 0.0;
    if (i < m) {
        x = p[3 * i]; y = p[3 * i + 1]; z = p[3 * i + 2];
        double vx = v[3 * i], vy = v[3 * i + 1], vz = v[3 * i + 2];
        const double ax = a[3 * i], ay = a[3 * i + 1], az = a[3 * i + 2];
        if (tracer_live(x, y, z, vx, vy, vz) && isfinite(ax) && isfinite(ay) && isfinite(az)) {
            vx = vx + ax * h; vy = vy + ay * h; vz = vz + az * h;
            x = x + vx * dt; y = y + vy * dt; z = z + vz * dt;
            v[3 * i] = vx; v[3 * i + 1] = vy; v[3 * i + 2] = vz;
            p[3 * i] = x; p[3 * i + 1] = y; p[3 * i + 2] = z;
            moved = true;
        }
    }
    if (pmax) tracer_raise_pmax(pmax, moved, x, y, z);
}

// ---------------------------------------------------------------------------------------
// K20: grid deposit (nbmi_deposit; include/nbmi.h).  A scatter of fixed-point integers: every
// (body, cell) contribution is rounded to a multiple of the plane's quantum 2^e and added with 64-bit integer atomics,
// so the sum of a cell is one unique integer whatever the order and however the kernel combines contributions first.
// k_plane_max finds max |q| per plane (exact in any order; the bit pattern of a non-negative double orders as an
// integer, and a NaN lies above +inf), the host turns it into e, k_deposit scatters, k_deposit_out converts in place.
// ---------------------------------------------------------------------------------------
constexpr int kDepPlanes = 6;      // NUMBER, MASS, MOMENTUM x 3, KINETIC
constexpr int kDepRows = 8;        // state rows per thread of k_deposit: a workgroup covers 2 048 consecutive rows
constexpr int kDepSlots = 1024;    // aggregating form: cells the workgroup's LDS table can hold
constexpr int kDepSlotBits = 10;
constexpr int kDepProbes = 4;      // ... linear probes before a contribution goes to memory directly
struct DepositArgs {
    double lo[3], inv[3], dimd[3];
    int dims[3];
    int cic[3];               // the axis splits a body over two cells (scheme CIC and dims >= 2)
    int planes;
    int slot[kDepPlanes];     // plane -> quantity: 0 = 1, 1 = m, 2 .. 4 = m v, 5 = m |v|^2
    int e[kDepPlanes];        // the plane's exponent
    int live[kDepPlanes];     // max |q| != 0
    long long cells;
};

// ---- what every fixed-point sum over the state rows is made of (K20 and K26) ----
// q -> its multiple of the plane's quantum 2^e, and a sum of those back
__host__ __device__ __forceinline__ long long fx_quantise(double q, int e) { return (long long)rint(ldexp(q, -e)); }
__host__ __device__ __forceinline__ double fx_value(unsigned long long K, int e) { return ldexp((double)(long long)K, e); }

// The K quantities of a body, then the one a plane asks for.  A chain of uniform selects: nothing is indexed dynamically.
template <int K>
struct PlaneQ {
    double q[K];
    template <int T = 0>
    __device__ __forceinline__ double select(int slot) const {
        if constexpr (T == K - 1) return q[T];
        else return slot == T ? q[T] : select<T + 1>(slot);
    }
};

// Pass 1 of a sum: out[p] = the largest bit pattern of |q| of plane p.  `src` carries `planes` and `slot[]` and says
// per body whether it takes part and what its quantities are: bool take(cur, i, q, out).
template <int P, class Source>
__global__ __launch_bounds__(kBlock) void k_plane_max(Bodies cur, int64_t n, Source src, unsigned long long *__restrict__ out /* [P] */) {
    __shared__ unsigned long long sh[kBlock];
    unsigned long long mx[P];
#pragma unroll
    for (int p = 0; p < P; p++) mx[p] = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        PlaneQ<P> q;
        if (!src.take(cur, i, q, out)) continue;
#pragma unroll
        for (int p = 0; p < P; p++) {
            if (p < src.planes) {
                const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(q.select(src.slot[p])));
                mx[p] = b > mx[p] ? b : mx[p];
            }
        }
    }
#pragma unroll
    for (int p = 0; p < P; p++) {
        if (p >= src.planes) break;
        sh[threadIdx.x] = mx[p];
        __syncthreads();
        for (int w = kBlock / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) sh[threadIdx.x] = sh[threadIdx.x] > sh[threadIdx.x + w] ? sh[threadIdx.x] : sh[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0 && sh[0] != 0ull) atomicMax(&out[p], sh[0]);
        __syncthreads();
    }
}

// The three counters of a main pass: per thread, then the workgroup's three LDS words (cleared before a barrier), then
// one global atomic per non-zero word.  The barrier inside also ends the pass's LDS adds for the flush that follows.
__device__ __forceinline__ void stats3_clear(unsigned int *sh) {
    if (threadIdx.x < 3) sh[threadIdx.x] = 0u;
}
__device__ __forceinline__ void stats3_add(unsigned int *sh, unsigned long long *__restrict__ stats, unsigned int c0,
                                           unsigned int c1, unsigned int c2) {
    if (c0) atomicAdd(&sh[0], c0);
    if (c1) atomicAdd(&sh[1], c1);
    if (c2) atomicAdd(&sh[2], c2);
    __syncthreads();
    if (threadIdx.x < 3 && sh[threadIdx.x]) atomicAdd(&stats[threadIdx.x], (unsigned long long)sh[threadIdx.x]);
}

// the six quantities of a body, as the header writes them (float64, no FMA)
using DepQ = PlaneQ<kDepPlanes>;
__device__ __forceinline__ DepQ dep_quantities(double m, double vx, double vy, double vz) {
    return DepQ{{1.0, m, __dmul_rn(m, vx), __dmul_rn(m, vy), __dmul_rn(m, vz),
                 __dmul_rn(m, __dadd_rn(__dadd_rn(__dmul_rn(vx, vx), __dmul_rn(vy, vy)), __dmul_rn(vz, vz)))}};
}
// pass 1 of nbmi_deposit: every body takes part
struct DepSource : DepositArgs {
    __device__ __forceinline__ bool take(const Bodies &cur, int64_t i, DepQ &q, unsigned long long *) const {
        q = dep_quantities(cur.m[i], cur.vx[i], cur.vy[i], cur.vz[i]);
        return true;
    }
};

// A body's cells and weights on one axis.  The range test is made on the floored double; an index is converted only
// when it passed.
struct DepAxis {
    int i0, i1;
    double w0, w1;
    bool ok0, ok1;
};
__device__ __forceinline__ DepAxis dep_axis(double x, double lo, double inv, double dimd, bool cic) {
    DepAxis r;
    const double u = __dmul_rn(__dsub_rn(x, lo), inv);
    if (!cic) {
        const double fl = floor(u);
        r.ok0 = fl >= 0.0 && fl < dimd;
        r.i0 = r.ok0 ? (int)fl : 0;
        r.w0 = 1.0;
        r.ok1 = false;
        r.i1 = 0;
        r.w1 = 0.0;
    } else {
        const double s = __dsub_rn(u, 0.5), fl = floor(s), f = __dsub_rn(s, fl), f1 = __dadd_rn(fl, 1.0);
        r.ok0 = fl >= 0.0 && fl < dimd;
        r.i0 = r.ok0 ? (int)fl : 0;
        r.w0 = __dsub_rn(1.0, f);
        r.ok1 = f1 >= 0.0 && f1 < dimd;
        r.i1 = r.ok1 ? (int)f1 : 0;
        r.w1 = f;
    }
    return r;
}

// One pass over the state rows.  AGG = false: one global atomic per (contribution, plane).  AGG = true: the workgroup
// first adds into an LDS table keyed by cell (open addressing, kDepProbes probes; a contribution that finds no slot goes
// to memory directly) and flushes one atomic per (distinct cell, plane) at the end.  Both give the same integers.
// stats = {bodies with a contribution, contributions, bodies skipped as not finite}.  Dynamic LDS (AGG):
// planes * kDepSlots sums, then kDepSlots keys.
template <bool AGG>
__global__ __launch_bounds__(kBlock) void k_deposit(Bodies cur, int64_t n, DepositArgs a, unsigned long long *__restrict__ K,
                                                    unsigned long long *__restrict__ stats) {
    extern __shared__ unsigned long long dep_lds[];
    __shared__ unsigned int sh_stats[3];
    unsigned long long *vals = dep_lds;
    int *keys = (int *)(dep_lds + (size_t)a.planes * kDepSlots);
    stats3_clear(sh_stats);
    if (AGG) {
        for (int t = threadIdx.x; t < kDepSlots; t += kBlock) keys[t] = -1;
        for (int t = threadIdx.x; t < a.planes * kDepSlots; t += kBlock) vals[t] = 0ull;
    }
    __syncthreads();
    unsigned int hit = 0u, contributions = 0u, skipped = 0u;
    const int64_t base = (int64_t)blockIdx.x * (kBlock * kDepRows);
    for (int r = 0; r < kDepRows; r++) {
        const int64_t i = base + (int64_t)r * kBlock + threadIdx.x;
        if (i >= n) continue;
        const double x = cur.x[i], y = cur.y[i], z = cur.z[i];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) {
            skipped++;
            continue;
        }
        const DepAxis ax = dep_axis(x, a.lo[0], a.inv[0], a.dimd[0], a.cic[0] != 0);
        const DepAxis ay = dep_axis(y, a.lo[1], a.inv[1], a.dimd[1], a.cic[1] != 0);
        const DepAxis az = dep_axis(z, a.lo[2], a.inv[2], a.dimd[2], a.cic[2] != 0);
        if (!((ax.ok0 || ax.ok1) && (ay.ok0 || ay.ok1) && (az.ok0 || az.ok1))) continue;
        hit++;
        const DepQ q = dep_quantities(cur.m[i], cur.vx[i], cur.vy[i], cur.vz[i]);
        double qp[kDepPlanes];
#pragma unroll
        for (int p = 0; p < kDepPlanes; p++) qp[p] = p < a.planes ? q.select(a.slot[p]) : 0.0;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const bool ok = ((c & 1) ? ax.ok1 : ax.ok0) && ((c & 2) ? ay.ok1 : ay.ok0) && ((c & 4) ? az.ok1 : az.ok0);
            if (!ok) continue;
            contributions++;
            const double w = __dmul_rn(__dmul_rn((c & 1) ? ax.w1 : ax.w0, (c & 2) ? ay.w1 : ay.w0), (c & 4) ? az.w1 : az.w0);
            const int ix = (c & 1) ? ax.i1 : ax.i0, iy = (c & 2) ? ay.i1 : ay.i0, iz = (c & 4) ? az.i1 : az.i0;
            const int cell = (iz * a.dims[1] + iy) * a.dims[0] + ix;  // < cells <= 2^28
            int slot = -1;
            if (AGG) {
                int h = (int)(((unsigned)cell * 2654435761u) >> (32 - kDepSlotBits));
                for (int t = 0; t < kDepProbes; t++) {
                    const int old = atomicCAS(&keys[h], -1, cell);
                    if (old == -1 || old == cell) {
                        slot = h;
                        break;
                    }
                    h = (h + 1) & (kDepSlots - 1);
                }
            }
#pragma unroll
            for (int p = 0; p < kDepPlanes; p++) {
                if (p >= a.planes || !a.live[p]) continue;
                const long long k = fx_quantise(__dmul_rn(qp[p], w), a.e[p]);
                if (k == 0) continue;
                if (AGG && slot >= 0) atomicAdd(&vals[p * kDepSlots + slot], (unsigned long long)k);
                else atomicAdd(&K[(long long)p * a.cells + cell], (unsigned long long)k);
            }
        }
    }
    stats3_add(sh_stats, stats, hit, contributions, skipped);
    if (AGG) {
        for (int t = threadIdx.x; t < kDepSlots; t += kBlock) {
            const int cell = keys[t];
            if (cell < 0) continue;
            for (int p = 0; p < a.planes; p++) {
                const unsigned long long v = vals[p * kDepSlots + t];
                if (v) atomicAdd(&K[(long long)p * a.cells + cell], v);
            }
        }
    }
}

// K (int64, in place) -> out = ldexp((double) K, e) per plane
__global__ __launch_bounds__(kBlock) void k_deposit_out(unsigned long long *__restrict__ K, DepositArgs a) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.cells) return;
    for (int p = 0; p < a.planes; p++) {
        const long long j = (long long)p * a.cells + i;
        K[j] = (unsigned long long)__double_as_longlong(fx_value(K[j], a.e[p]));
    }
}

// ---------------------------------------------------------------------------------------
// K26: radial profiles and mass radii about a centre (nbmi_radial_profile, nbmi_mass_radii; include/nbmi.h, DESIGN.md
// section 4.26).  The profile is K20's scheme on a tiny dense table: k_plane_max finds max |q| per plane over the
// bodies with a finite r2, the host turns it into e, k_profile adds the fixed-point integers per workgroup in LDS and
// sends one global atomic per non-zero (slot, plane); the host converts the at most 8 x 257 sums.
// ---------------------------------------------------------------------------------------
constexpr int kProfPlanes = 8;       // NUMBER, MASS, RADIAL_MOMENTUM, RADIAL_KINETIC, KINETIC, ANGULAR_MOMENTUM x 3
constexpr int kProfMaxBins = 256;
constexpr int kProfRows = 8;         // state rows per thread of k_profile: a workgroup covers 2 048 consecutive rows
constexpr int kProfEdgePad = 512;    // E in LDS, padded with +inf so that the 9-step search needs no bound test
constexpr int kProfNeedM = 1, kProfNeedVr = 2, kProfNeedW2 = 4, kProfNeedL = 8;  // the mass; vr (sqrt, divide); w2; r x w
struct ProfileArgs {
    double c[3], b[3];
    int bulk;                 // w = v - b (0: w = v, no subtraction)
    int need;                 // kProfNeed*: what the selected planes read beyond the positions
    int nb;
    int planes;
    int slot[kProfPlanes];    // plane -> quantity 0 .. 7 in the order above
    int e[kProfPlanes];
    int live[kProfPlanes];
    double E[kProfMaxBins + 1];
};

// r = x - c and r2 = (rx rx + ry ry) + rz rz, as the header writes them
struct ProfR { double rx, ry, rz, r2; };
__device__ __forceinline__ ProfR prof_r(const Bodies &cur, int64_t i, const double *c) {
    ProfR r;
    r.rx = __dsub_rn(cur.x[i], c[0]);
    r.ry = __dsub_rn(cur.y[i], c[1]);
    r.rz = __dsub_rn(cur.z[i], c[2]);
    r.r2 = __dadd_rn(__dadd_rn(__dmul_rn(r.rx, r.rx), __dmul_rn(r.ry, r.ry)), __dmul_rn(r.rz, r.rz));
    return r;
}
// the eight quantities of a body with a finite r2
using ProfQ = PlaneQ<kProfPlanes>;
__device__ __forceinline__ ProfQ prof_quantities(const Bodies &cur, int64_t i, const ProfR &r, const ProfileArgs &a) {
    ProfQ q = {};
    q.q[0] = 1.0;
    if (a.need == 0) return q;  // NUMBER alone.  (`need` is uniform: what no selected plane asks for is not loaded or computed)
    const double m = cur.m[i];
    q.q[1] = m;
    if (!(a.need & (kProfNeedVr | kProfNeedW2 | kProfNeedL))) return q;
    double wx = cur.vx[i], wy = cur.vy[i], wz = cur.vz[i];
    if (a.bulk) {
        wx = __dsub_rn(wx, a.b[0]); wy = __dsub_rn(wy, a.b[1]); wz = __dsub_rn(wz, a.b[2]);
    }
    if (a.need & kProfNeedVr) {
        const double rho = sqrt(r.r2);
        const double dot = __dadd_rn(__dadd_rn(__dmul_rn(r.rx, wx), __dmul_rn(r.ry, wy)), __dmul_rn(r.rz, wz));
        const double vr = rho == 0.0 ? 0.0 : dot / rho;
        const double mvr = __dmul_rn(m, vr);
        q.q[2] = mvr;
        q.q[3] = __dmul_rn(mvr, vr);
    }
    if (a.need & kProfNeedW2)
        q.q[4] = __dmul_rn(m, __dadd_rn(__dadd_rn(__dmul_rn(wx, wx), __dmul_rn(wy, wy)), __dmul_rn(wz, wz)));
    if (a.need & kProfNeedL) {
        q.q[5] = __dmul_rn(m, __dsub_rn(__dmul_rn(r.ry, wz), __dmul_rn(r.rz, wy)));
        q.q[6] = __dmul_rn(m, __dsub_rn(__dmul_rn(r.rz, wx), __dmul_rn(r.rx, wz)));
        q.q[7] = __dmul_rn(m, __dsub_rn(__dmul_rn(r.rx, wy), __dmul_rn(r.ry, wx)));
    }
    return q;
}
// pass 1 of nbmi_radial_profile: the bodies with a finite r2 take part
struct ProfSource : ProfileArgs {
    __device__ __forceinline__ bool take(const Bodies &cur, int64_t i, ProfQ &q, unsigned long long *) const {
        const ProfR r = prof_r(cur, i, c);
        if (!isfinite(r.r2)) return false;
        q = prof_quantities(cur, i, r, *this);
        return true;
    }
};

// One pass over the state rows.  Dynamic LDS: kProfEdgePad doubles (E, then +inf), then planes x (nb + 1) sums, plane
// major.  The slot is the number of E[k] < r2, found by nine unconditional halvings.  One LDS atomic per (body, plane) -
// also where every body of the workgroup hits one shell: summing a wave's equal slots first measured 1 - 9 % slower
// everywhere (scripts/experiments/profile_wave_sum.patch) - and at the end one global atomic per non-zero (slot, plane).
// stats = {bodies in a slot, bodies beyond, bodies skipped}.
__global__ __launch_bounds__(kBlock) void k_profile(Bodies cur, int64_t n, ProfileArgs a, unsigned long long *__restrict__ K,
                                                    unsigned long long *__restrict__ stats) {
    extern __shared__ unsigned long long prof_lds[];
    __shared__ unsigned int sh_stats[3];
    double *E = (double *)prof_lds;
    unsigned long long *vals = prof_lds + kProfEdgePad;
    const int nslots = a.nb + 1;
    stats3_clear(sh_stats);
    for (int t = threadIdx.x; t < kProfEdgePad; t += kBlock) E[t] = t <= a.nb ? a.E[t] : __longlong_as_double(0x7ff0000000000000ll);
    for (int t = threadIdx.x; t < a.planes * nslots; t += kBlock) vals[t] = 0ull;
    __syncthreads();
    unsigned int inside = 0u, beyond = 0u, skipped = 0u;
    const int64_t base = (int64_t)blockIdx.x * (kBlock * kProfRows);
    for (int r = 0; r < kProfRows; r++) {
        const int64_t i = base + (int64_t)r * kBlock + threadIdx.x;
        int slot = -1;  // -1: nothing to add
        ProfQ q = {};
        if (i < n) {
            const ProfR rr = prof_r(cur, i, a.c);
            if (!isfinite(rr.r2)) {
                skipped++;
            } else {
                int pos = 0;
#pragma unroll
                for (int step = kProfEdgePad / 2; step > 0; step >>= 1) pos += E[pos + step - 1] < rr.r2 ? step : 0;
                if (pos > a.nb) {
                    beyond++;
                } else {
                    inside++;
                    slot = pos;
                    q = prof_quantities(cur, i, rr, a);
                }
            }
        }
        if (slot < 0) continue;
#pragma unroll
        for (int p = 0; p < kProfPlanes; p++) {
            if (p >= a.planes || !a.live[p]) continue;  // (uniform)
            const long long k = fx_quantise(q.select(a.slot[p]), a.e[p]);
            if (k != 0ll) atomicAdd(&vals[p * nslots + slot], (unsigned long long)k);
        }
    }
    stats3_add(sh_stats, stats, inside, beyond, skipped);
    for (int t = threadIdx.x; t < a.planes * nslots; t += kBlock) {
        const unsigned long long v = vals[t];
        if (v) atomicAdd(&K[t], v);
    }
}

// ---- mass radii: sort by the bits of r2, prefix sums of the masses' integers, one crossing test per tie run ----
constexpr uint64_t kMrSkipKey = 0x7fffffffffffffffull;  // above every finite r2's bits: the skipped bodies sort last
constexpr int kMrMaxFractions = 64;
struct MrArgs {
    int nf;
    int e;
    long long T[kMrMaxFractions];
    long long tmin, tmax;
};
// pass 1 of nbmi_mass_radii: every body, one plane, |m|.  res[0] = the largest mass's bits, res[1] = 1 if a mass is negative
struct MrSource {
    static constexpr int planes = 1;
    static constexpr int slot[1] = {0};
    __device__ __forceinline__ bool take(const Bodies &cur, int64_t i, PlaneQ<1> &q, unsigned long long *res) const {
        q.q[0] = cur.m[i];
        if (q.q[0] < 0.0) atomicMax(&res[1], 1ull);
        return true;
    }
};
// key = the bits of r2 (a non-negative finite double orders as its bits), kMrSkipKey for a body that is skipped
__global__ __launch_bounds__(kBlock) void k_mr_keys(Bodies cur, int64_t n, double cx, double cy, double cz,
                                                    uint64_t *__restrict__ key, uint32_t *__restrict__ idx,
                                                    unsigned long long *__restrict__ skipped) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    long long skip = 0;
    if (i < n) {
        const double c[3] = {cx, cy, cz};
        const ProfR r = prof_r(cur, i, c);
        const bool ok = isfinite(r.r2);
        key[i] = ok ? (uint64_t)__double_as_longlong(r.r2) : kMrSkipKey;
        idx[i] = (uint32_t)i;
        skip = ok ? 0 : 1;
    }
    nbmi::wave_add(skipped, skip, threadIdx.x & 63);
}
// Scan element over the sorted bodies: sum = the integers so far, run = those of the tie run that the last entry belongs
// to (as far as it lies inside the scanned range), head = a run starts inside the range.
struct MrSeg {
    long long sum, run;
    int head;
};
__device__ __forceinline__ MrSeg lane_up(const MrSeg &s, int d) { return MrSeg{__shfl_up(s.sum, d), __shfl_up(s.run, d), __shfl_up(s.head, d)}; }
struct MrSegOp {
    __device__ MrSeg operator()(const MrSeg &a, const MrSeg &b) const {
        return MrSeg{a.sum + b.sum, b.head ? b.run : a.run + b.run, a.head | b.head};
    }
};
// the entry of sorted position j: k = fx_quantise(m, e) of its body (0 for a skipped body), head = it starts a tie run
__device__ __forceinline__ MrSeg mr_entry(const uint64_t *__restrict__ key_s, const long long *__restrict__ kk, int64_t j) {
    const long long k = kk[j];
    return MrSeg{k, k, (j == 0 || key_s[j] != key_s[j - 1]) ? 1 : 0};
}
// phase 1: the integers in sorted order (kept in kk) and the fold of every tile of scan::kTile entries
__global__ __launch_bounds__(scan::kBlock) void k_mr_tiles(Bodies cur, int64_t n, const uint64_t *__restrict__ key_s,
                                                           const uint32_t *__restrict__ idx_s, int e, long long *__restrict__ kk,
                                                           MrSeg *__restrict__ tiles) {
    const int64_t first = ((int64_t)blockIdx.x * scan::kBlock + threadIdx.x) * scan::kItems;
    MrSeg acc{0ll, 0ll, 0};
#pragma unroll
    for (int t = 0; t < scan::kItems; t++) {
        const int64_t j = first + t;
        if (j >= n) break;
        const uint64_t key = key_s[j];
        const long long k = key == kMrSkipKey ? 0ll : fx_quantise(cur.m[idx_s[j]], e);
        kk[j] = k;
        acc = MrSegOp()(acc, MrSeg{k, k, (j == 0 || key != key_s[j - 1]) ? 1 : 0});
    }
    const MrSeg total = scan::block_scan<scan::kBlock>(acc, MrSeg{0ll, 0ll, 0}, MrSegOp()).total;
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}
// phase 3: with the scanned tiles in front, every entry that ends a tie run of bodies taking part tests
// C_prev_run < T <= C_run per fraction and writes out[3 f] = {bits of r2, bodies inside, the integer sum}
__global__ __launch_bounds__(scan::kBlock) void k_mr_select(int64_t n, const uint64_t *__restrict__ key_s,
                                                            const long long *__restrict__ kk, const MrSeg *__restrict__ tiles,
                                                            MrArgs a, unsigned long long *__restrict__ out) {
    const int64_t first = ((int64_t)blockIdx.x * scan::kBlock + threadIdx.x) * scan::kItems;
    MrSeg acc{0ll, 0ll, 0};
#pragma unroll
    for (int t = 0; t < scan::kItems; t++)
        if (first + t < n) acc = MrSegOp()(acc, mr_entry(key_s, kk, first + t));
    MrSeg run = scan::block_scan<scan::kBlock>(acc, tiles[blockIdx.x], MrSegOp()).excl;
#pragma unroll
    for (int t = 0; t < scan::kItems; t++) {
        const int64_t j = first + t;
        if (j >= n) break;
        run = MrSegOp()(run, mr_entry(key_s, kk, j));
        const uint64_t key = key_s[j];
        if (key == kMrSkipKey || (j + 1 < n && key_s[j + 1] == key)) continue;
        const long long c_run = run.sum, c_prev = run.sum - run.run;
        if (c_run < a.tmin || c_prev >= a.tmax) continue;
        for (int f = 0; f < a.nf; f++) {
            if (c_prev < a.T[f] && a.T[f] <= c_run) {
                out[3 * f] = key;
                out[3 * f + 1] = (unsigned long long)(j + 1);
                out[3 * f + 2] = (unsigned long long)c_run;
            }
        }
    }
}

}  // namespace

// =========================================================================================
// handle
// =========================================================================================
// Measured (MI355X, theta 0.5, walk ms, middle cut -> cut at the wave's own leaves): galaxy 1 M 1.251 -> 1.251, 2 M
// 2.515 -> 2.409, 4 M 5.13 -> 4.95, 10 M 12.85 -> 12.28; collision 1 M 1.402 -> 1.389, 2 M 2.477 -> 2.386, 4 M
// 4.68 -> 4.40, 10 M 11.50 -> 10.79.  The home cut keeps both cursors busy for 68-81 % of the visits instead of
// ~20 % (scripts/analysis/range_balance.py), but what two cursors overlap is the latency of far-field jumps, and
// that only shows once the node array is far beyond the L2.  (A cut placed by a two-component model of where the
// visits are - 75 % instead of 68 % at 1 M - measured the same or slower.)
constexpr int64_t kHomeSplitBodies = 1500000;

// The walk-order side of a chunk of probes (nbmi_field_at and the tracers, sections 4.18 / 4.19): `rows` probes as
// columns in walk order - 56 bytes each with their sort keys and indices in and out - the sort's temp buffer for that
// many pairs, and the walk table whose buffer 0 names the columns.  probe_alloc / probe_free.
struct ProbeScratch {
    int64_t rows = 0;
    double *sx = nullptr, *sy = nullptr, *sz = nullptr;
    uint64_t *key = nullptr, *key_s = nullptr;
    uint32_t *idx = nullptr, *order = nullptr;
    char *sort_tmp = nullptr;
    size_t sort_bytes = 0;
    WalkTable *wtab = nullptr;
};

struct nbmi_sim {
    int64_t n = 0;
    int method = 0, device = 0;
    double G = 0, softening = 0, damping = 1, theta = 0.5;
    hipStream_t stream = nullptr;
    int curbuf = 0;
    int64_t steps_taken = 0;  // nbmi_step_count()
    Bodies buf[2] = {};
    // scratch
    uint64_t *key_hi = nullptr, *key_lo = nullptr, *hi_s = nullptr, *lo_s = nullptr;
    uint32_t *idx = nullptr, *perm = nullptr;
    int32_t *delta = nullptr, *Pex = nullptr;  // Pex: exclusive prefix of the cell counts INSIDE a sub-tile (PexL)
    int32_t *subPex = nullptr, *sub_cnt = nullptr;  // per sub-tile: exclusive prefix / total of the cell counts
    float4 *posm_s = nullptr;
    double4 *p64_s = nullptr;  // float64 twin of posm_s: owner mode only (bounding boxes)
    double4 *S = nullptr;      // in-sub-tile exclusive prefix of {G m, G m x, G m y, G m z}
    double4 *sub_tot = nullptr;  // per sub-tile totals of the same
    Moment *T = nullptr;         // per sub-tile exclusive prefix, double-double
    Node *nodes = nullptr;
    Node64 *nodes64 = nullptr;  // float64 twin rows of the internal cells (near-tie re-decision)
    NodeD *nodesd = nullptr;    // float64 node records of every node (waves that compute forces in float64)
    int force_prec = 0;         // 0 = per wave by local density, 1 = fp32 everywhere, 2 = float64 everywhere (NBMI_FORCE_PREC)
    int all64_enter_pm = kAll64Enter, all64_leave_pm = kAll64Leave;  // "auto": every wave float64 while most of the system asks (per mille of the waves)
    double prec_tau = 5.0e-5;   // force_prec 0: float64 where G rho dt^2 exceeds this (NBMI_PREC_TAU)
    WalkTable *wtab = nullptr;  // device copies of the walk's per-handle constants: [0] kick-drift, [kLeapClose], [kLeapPrime]
    uint8_t *node_level = nullptr;
    int32_t *node_ref = nullptr;  // first body (sorted rank) of every node; queries only
    int64_t node_capacity = 0;   // rows of the walk array (own tree + received trees)
    int64_t own_node_rows = 0;   // rows the handle's own tree may use
    TreeInfo *info = nullptr;  // device
    void *tmp_sort = nullptr;
    size_t tmp_sort_bytes = 0;
    float *colors = nullptr;  // (N,3) original order
    void *stage = nullptr;    // getter staging, 3N doubles
    bool tree_valid = false;
    int64_t shard_begin = 0, shard_end = 0;
    bool exchange_sync = true;  // export / import block the host (false: the caller orders streams itself)
    // octree inputs in key order: the handle's own sorted arrays (nt == n)
    int64_t nt = 0;
    uint64_t *t_hi = nullptr, *t_lo = nullptr;
    float4 *t_posm = nullptr;
    // owner mode (multi-GPU stage 2): this handle holds the bodies of one octant-key range
    bool owner = false;
    int world = 0, rank = 0;
    int64_t cap = 0;            // body capacity (0: exactly n)
    int64_t let_capacity = 0;   // rows of one locally essential tree in the exchange buffers
    int64_t node_extra = 0;     // node rows reserved behind the own tree for received trees
    uint64_t *let_split = nullptr;
    uint8_t *let_dead = nullptr;   // rows whose body has just been handed to another rank
    int64_t n_leaving = 0;
    uint32_t *let_dest = nullptr;
    int64_t *let_counts = nullptr;
    int32_t *let_diff = nullptr, *let_scan = nullptr, *let_keep = nullptr, *let_tiles = nullptr, *let_ranges = nullptr;
    double *let_supers = nullptr, *let_megas = nullptr, *let_rankbox = nullptr;
    int64_t let_stride = 0, let_tile_stride = 0;  // rows between two destinations' work arrays
    TreeInfo *h_info = nullptr;   // pinned host copy of the tree header, refreshed by every nbmi_owner_adopt
    hipEvent_t ev_info = nullptr;  // ... complete when this event is
    int64_t last_nodes = -1;      // num_nodes of the previous step's own tree (launch bound of this step's tree export)
    int64_t own_base = 0;         // [r3] row of the walk array at which the own tree is built (world > 1: behind the room for the lower ranks' pieces)
    int32_t *chain_r = nullptr;   // nodes of the cells that hold the rank's last body, by level
    OwnLink *own_links = nullptr; // the own piece's links that leave the rank
    const ChainTable *chains = nullptr;  // every rank's table (the caller's gathered buffer of this step)
    // frame codec: previous decoded frame (positions then colours, float32, caller's order) and the int16 payload
    float *frame_prev = nullptr;
    int16_t *frame_q = nullptr;
    bool frame_have_prev = false;
    // asynchronous frames (nbmi_frame_begin): per slot one device and one pinned host buffer of a FrameHeader + 24 bytes
    // per body, filled by k_frame_snapshot on `stream` and copied out on `frame_stream`; allocated by the first begin
    struct FrameSlot {
        char *dev = nullptr, *host = nullptr;
        hipEvent_t ev_snap = nullptr, ev_done = nullptr;  // snapshot written (on stream) / copy complete (on frame_stream)
        bool begun = false, used = false;
        int kind = 0;
        int64_t steps = 0, seq = 0;
    } frame_slot[NBMI_FRAME_SLOTS];
    hipStream_t frame_stream = nullptr;
    int64_t frame_seq = 0;
    // render-side reduction scratch (nbmi_visible_points), allocated on first use
    uint8_t *vis_flag = nullptr;
    uint32_t *vis_slot = nullptr, *vis_tiles = nullptr;
    int xcd_chunk = 0;  // walk block -> XCD mapping, see logical_block()
    int xcd_balance = 1;  // XCD ranges cut by last step's measured wave times (NBMI_XCD_BALANCE=0: equal eighths)
    int *xcd_bounds = nullptr;        // device [9]
    unsigned *wave_cycles = nullptr;  // device [4 per walk block]
    unsigned char *wave_flag = nullptr;  // device [one per wave]
    int32_t *sub_flag = nullptr;         // device [one per tile]: waves of the tile that ask for float64
    double step_dt = 0.0;                // dt of the step whose build is being enqueued (DtScope; 0: a build without a step)
    double uniform_gm = -1.0;            // direct N^2: G m when every body has the same positive mass (the reference's presets: masses = 1), else < 0
    double max_gm = 0.0;                 // largest |G m| of the bodies at creation (guarded())
    int owner_all64 = -1;                // owner mode: the system-wide "every wave float64" verdict for the next walk (-1: this rank's own rule)
    double owner_dt = 0.0;               // owner mode: the dt the next nbmi_owner_step will use (nbmi_owner_set_dt; "auto" needs it at build time)
    int balance_blocks = 0;           // the block count the bounds on the device were made for (0: none yet)
    // the cuts for the NEXT walk are made on a stream of their own, beside the next step's build (one workgroup, 70 us
    // at 10 M bodies: off the critical path)
    hipStream_t side = nullptr;
    hipEvent_t ev_walked = nullptr, ev_cut = nullptr;
    bool cut_pending = false;         // a k_xcd_bounds on `side` that the next balanced walk has to wait for
    int64_t balanced_walks = 0;       // walks of this handle launched in balance mode (nbmi_debug_wave_times reports it)
    int walk_block = kBlock;  // threads per walk block (64, 128 or 256; measurement knob NBMI_WALK_BLOCK)
    bool keys_lean = true;    // the stepping build (a BuildRequest with step_dt > 0 and no aux, plain handle) computes and
                              // stores the upper key word only (key_low_word); NBMI_KEYS_LEAN=0: full keys.  Dropped for good
                              // once a long run shows up (decode_device_error): every member of a run recomputes the others' words
    bool lean_build = false;  // the build being enqueued / the last one built is lean: key_lo and lo_s do not hold it
    bool sort_packed = true;  // sort ONE packed word (prefix << 24 | body index) with the keys-only sort where it fits
                              // (packed_sort_ok); NBMI_SORT_PACKED=0: always (key, index) pairs
    uint64_t *packed = nullptr, *packed_s = nullptr;  // the packed words of k_keys and their sorted order
    nbmi::RadixConfig sort_cfg;   // digit bits / threads per tile of the packed sort's passes; 0 = by size
                                  // (NBMI_SORT_DIGIT_BITS = 8 | 10, NBMI_SORT_THREADS = 256 | 512 | 1024)
    int sort_fused_hist = -1;     // k_keys_hist counts the packed sort's digit histogram instead of k_radix_hist: -1 by size
                                  // (fused_hist_pays), NBMI_SORT_FUSED_HIST=0 never, =1 always
    int sort_bits = 0;   // upper-word bits the radix sort looks at (0: chosen from n; NBMI_SORT_BITS); widened when long runs show up
    bool maxabs_fused = false;  // TreeInfo::maxabs_next holds max |coordinate| of the CURRENT positions (set by a full
                                // integrating walk, dropped by anything else that writes positions); NBMI_FUSE_MAXABS=0: never
    bool fuse_maxabs = true;
    bool hilbert = true;  // sort keys relabelled along the Hilbert curve (k_keys); NBMI_HILBERT=0: plain octant digits
    // conservation diagnostics (nbmi_diagnostics), allocated by the first call that needs them; no step touches them
    double *diag_phi = nullptr;       // [n] phi per state row
    int32_t *diag_cnt = nullptr;      // [n] applied potential terms per state row
    double *diag_part = nullptr;      // [kDiagBlocksMax * kDiagSums + kDiagSums] block partials, then the totals
    long long *diag_partc = nullptr;  // [kDiagBlocksMax + 1] the same for the term counts
    double4 *diag_pot = nullptr;      // [node rows] float64 {cx, cy, cz, G m} of every node of the diagnostic's own build
    TreeInfo *side_info = nullptr;    // the tree header as it stood before a query's own build (SideBuild puts it back)
    // Scratch of the tree queries; no step touches it.  Every group is allocated by the first
    // call that needs it (query_alloc) and holds `ready` from its last allocation on.
    struct QueryScratch {
        struct {  // every query: 32 bytes per node row (k_query_rows), 4 bytes per 64 bodies (the waves' first leaves)
            bool ready = false;
            double4 *rows = nullptr;
            uint32_t *wleaf = nullptr;
            unsigned long long *evals = nullptr;  // distances evaluated by k_knn
        } shared;
        struct {  // nbmi_knn (section 4.14): 16 bytes per body (r2_k and mass_k by state row)
            bool ready = false;
            double *r2 = nullptr, *mass = nullptr;
        } knn;
        struct {  // nbmi_fof (section 4.15): 16 bytes per body (parent, root, smallest caller index and member count by key rank)
            bool ready = false;
            int32_t *parent = nullptr, *root = nullptr, *minid = nullptr, *cnt = nullptr;
            unsigned long long *counters = nullptr;  // [0] distances evaluated, [1] roots
        } fof;
        // nbmi_fof_catalogue: 24 bytes per body (sorted roots, ranks in and out, segment heads, row of a root, head of a
        // row), the sort's temp buffer, 304 bytes per chunk of 256 bodies and - outside `ready` - 268 bytes per catalogue
        // row (a power of two of rows, regrown - the smaller arrays freed - when a call needs more)
        struct {
            bool ready = false;
            uint32_t *key_s = nullptr, *rank = nullptr, *rank_s = nullptr, *tiles = nullptr;
            int32_t *hpos = nullptr, *slot = nullptr, *qhead = nullptr;
            char *sort_tmp = nullptr;
            size_t sort_bytes = 0;
            double *last = nullptr, *first = nullptr;
            int64_t row_cap = 0;
            double *row_vals = nullptr, *out13 = nullptr;
            int32_t *label = nullptr;
            int64_t *members = nullptr;
        } cat;
        struct {  // nbmi_pair_counts (section 4.16): 4 bytes per node row (the cells' body counts), 67 words of results
            bool ready = false;
            int32_t *cnt = nullptr;
            unsigned long long *out = nullptr;  // [0] distances evaluated, [1] pairs counted through whole cells, [2 + c] counter c
        } pairs;
        // nbmi_mst (section 4.29): 64 bytes per body - caller index, last partner and its d2, the components' two minima
        // (after the rounds: the sort's two key arrays), the scan's input and output, the edge list, the sort's two index
        // arrays - 4 bytes per node row (the cells' tags), 4 bytes per 2 048 bodies of scan tiles, the sort's temp buffer
        // and two counters.  It also uses fof's parent / root and pairs' cnt.
        struct {
            bool ready = false;
            int32_t *rid = nullptr, *bpart = nullptr, *diff = nullptr, *dscan = nullptr, *tiles = nullptr, *ctag = nullptr;
            double *bd2 = nullptr;
            unsigned long long *cmin = nullptr, *cpair = nullptr, *e_pack = nullptr, *e_d2 = nullptr;
            uint32_t *va = nullptr, *vb = nullptr;
            char *sort_tmp = nullptr;
            size_t sort_bytes = 0;
            unsigned long long *counters = nullptr;  // [0] distances evaluated, [1] edges appended
            // of the last call, per round (nbmi_mst_rounds; host side): distances evaluated, edges appended, host wall ms
            struct Round {
                int64_t evals, edges;
                double ms;
            };
            std::vector<Round> rounds;
        } mst;
    } q;
    bool pair_cells = true;  // cells inside one bin are counted whole (NBMI_PAIRS_CELLS=0: never; measurement)
    // Scratch of nbmi_deposit (section 4.20): `words` 64-bit sums (planes x cells of the largest call so far, regrown by
    // the call that needs more) and 9 words of results: max |q| per plane, then the three stats.  No step touches it.
    struct {
        int64_t words = 0;
        unsigned long long *K = nullptr, *res = nullptr;
    } dep;
    // Scratch of nbmi_radial_profile (section 4.26): 8 maxima, 3 stats and 8 x 257 sums.  No step touches it.
    struct {
        unsigned long long *res = nullptr;
    } prof;
    // Scratch of nbmi_mass_radii (section 4.26) for `rows` bodies - 32 bytes each: keys and rows in and out of the sort,
    // the masses' integers in sorted order - the sort's temp buffer for that many pairs, 24 bytes per 2 048 bodies of
    // tile folds and 195 words of results: the largest mass, "a mass is negative", bodies skipped, 3 per fraction.
    struct {
        int64_t rows = 0;
        uint64_t *key = nullptr, *key_s = nullptr;
        uint32_t *idx = nullptr, *idx_s = nullptr;
        long long *kk = nullptr;
        MrSeg *tiles = nullptr;
        char *sort_tmp = nullptr;
        size_t sort_bytes = 0;
        unsigned long long *res = nullptr;
    } mr;
    bool deposit_agg = true;  // the workgroup combines contributions per cell in LDS first (NBMI_DEPOSIT_AGG=0: one global
                              // atomic per contribution; same bits, 3.1 - 134 x the time: DESIGN.md section 4.20)
    // Scratch of nbmi_field_at (section 4.18): `rows` points of a chunk - 108 bytes each: the points as they came, acc,
    // phi, terms, and their walk-order side.  Grown by the call that needs more, never beyond kFieldChunk rows; no step
    // touches it.
    struct : ProbeScratch {
        double *pts = nullptr, *acc = nullptr, *phi = nullptr;
        int32_t *cnt = nullptr;
        double *t6 = nullptr;  // nbmi_tidal_at's rows, 48 bytes more per point: null until its first call (section 4.27)
        // nbmi_pair_counts_at's per-point rows (section 4.28), pp_words int32: null until a call asks for per_point, grown
        // by the call that needs more than `rows` x (nb + 1) words hold
        int32_t *pp = nullptr;
        int64_t pp_words = 0;
    } field;
    bool field_sort = true;  // probes walk in key order (NBMI_FIELD_SORT=0: in the caller's order; measurement)
    // Massless tracers (nbmi_set_tracers, section 4.19); all null / 0 on a handle without them.  State: p and v, (m, 3)
    // rows in the caller's order, and the leapfrog's a (allocated by the first leapfrog step; acc_valid as the bodies').
    // pmax: the device word of tracer_raise_pmax.  Scratch (Barnes-Hut): the walk-order side for `rows` = min(m,
    // kFieldChunk) probes.  The steps enqueue work on it without waiting, so it is the tracers' own: nbmi_field_at's
    // regrowth never frees it.
    struct : ProbeScratch {
        int64_t m = 0;
        double *p = nullptr, *v = nullptr, *a = nullptr;
        bool acc_valid = false;
        unsigned long long *pmax = nullptr;
    } tr;
    // what nbmi_compute_colors / nbmi_frame_begin colour by (nbmi_set_color_mode)
    int color_mode = NBMI_COLOR_SPEED, color_k = 32;
    double color_lo = 0.0, color_hi = 1.0;
    // integrator (nbmi_set_integrator).  Leapfrog keeps a = F(x) of the current state beside its
    // rows: acc = 3 columns of n doubles, allocated by the first leapfrog step; acc_valid = false until a step primes it
    int integrator = NBMI_INTEGRATOR_KICK_DRIFT;
    bool acc_valid = false;
    double *acc = nullptr;
    // multipole order of an applied cell term (nbmi_set_multipole).  The three arrays exist from
    // the first switch into quadrupole mode on: the walk's fp32 records, the float64 work rows of the bottom-up pass
    // (kQuadDoubles per node row; the potential reads its moments there) and the float64 {cx, cy, cz, G m} rows of the
    // mode's builds
    int multipole = NBMI_MULTIPOLE_MONOPOLE;
    int multipole_env = NBMI_MULTIPOLE_MONOPOLE;  // NBMI_MULTIPOLE: the initial value where the handle allows it
    NodeQ *nodesq = nullptr;
    double *quad_work = nullptr;
    double4 *quad_pot = nullptr;
    // one-wave walk: cursors per wave and where the array is cut.  -1 = by size: two cursors, cut at the middle of the
    // array, or (from kHomeSplitBodies = 1.5 M bodies on) at the leaf of the wave's middle body; NBMI_WALK_PAIR = 0 / 1 / 2 forces
    // one cursor / the middle cut / the home cut
    int walk_pair = -1;
    int64_t split_max_waves = 9400;  // split walk: K waves per group while groups x K fits; NBMI_SPLIT_WAVES (0 = off)
    // timers
    bool timers = false;
    hipEvent_t ev[6] = {};
    double ms[5] = {0, 0, 0, 0, 0};
    int64_t timed_steps = 0;
    std::vector<void *> allocs;
};

namespace {

template <typename T>
int dev_alloc(nbmi_sim *s, T **p, size_t count) {
    void *q = nullptr;
    NBMI_HIP_CHECK(hipMalloc(&q, (count ? count : 1) * sizeof(T)));
    s->allocs.push_back(q);
    *p = (T *)q;
    return 0;
}

// gives back one array of dev_alloc (the caller knows that nothing enqueued uses it)
template <typename T>
void dev_free(nbmi_sim *s, T **p) {
    if (!*p) return;
    auto it = std::find(s->allocs.begin(), s->allocs.end(), (void *)*p);
    if (it != s->allocs.end()) s->allocs.erase(it);
    (void)hipFree(*p);
    *p = nullptr;
}

// After a launch whose failure gets a message of its own: 0, or - it failed - NBMI_ERR_HIP with the message `fmt`
// (printf-style, at most one %s: `who`).
int launch_failed(const char *fmt, const char *who = "") {
    if (hipGetLastError() == hipSuccess) return 0;
    nbmi::set_error(fmt, who);
    return NBMI_ERR_HIP;
}

int alloc_bodies(nbmi_sim *s, Bodies *b, int64_t n) {
    if (dev_alloc(s, &b->x, n) || dev_alloc(s, &b->y, n) || dev_alloc(s, &b->z, n) || dev_alloc(s, &b->vx, n) ||
        dev_alloc(s, &b->vy, n) || dev_alloc(s, &b->vz, n) || dev_alloc(s, &b->m, n) || dev_alloc(s, &b->id, n))
        return -2;
    return 0;
}

// the walk's per-handle constants as the handle stands
WalkTable walk_table(const nbmi_sim *s) {
    WalkTable t;
    t.buf[0] = s->buf[0];
    t.buf[1] = s->buf[1];
    t.n64 = s->nodes64;
    t.nodesd = s->nodesd;
    t.xcd_bounds = s->xcd_bounds;
    t.wave_cycles = s->wave_cycles;
    t.wave_flag = s->wave_flag;
    t.pex = s->Pex;
    t.subpex = s->subPex;
    t.maxabs_next = &s->info->maxabs_next;
    t.theta = s->theta;
    t.eps2 = s->softening * s->softening;
    t.own_base = s->own_base;
    t.ax = s->acc;
    t.ay = s->acc ? s->acc + s->n : nullptr;
    t.az = s->acc ? s->acc + 2 * s->n : nullptr;
    t.leap = 0;
    return t;
}
// (re)writes the device copy of them
int upload_walk_table(nbmi_sim *s) {
    const WalkTable t = walk_table(s);
    WalkTable tabs[3] = {t, t, t};  // one per epilogue: kick-drift, kLeapClose, kLeapPrime
    tabs[0].leap = 0;
    tabs[kLeapClose].leap = kLeapClose;
    tabs[kLeapPrime].leap = kLeapPrime;
    NBMI_HIP_CHECK(hipMemcpyAsync(s->wtab, tabs, sizeof(tabs), hipMemcpyHostToDevice, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));  // `tabs` is a stack object
    return 0;
}

int check_handle(nbmi_sim *s) {
    if (!s) {
        nbmi::set_error("null nbmi_sim handle");
        return NBMI_ERR_ARG;
    }
    if (hipSetDevice(s->device) != hipSuccess) {
        nbmi::set_error("hipSetDevice(%d) failed", s->device);
        return NBMI_ERR_HIP;
    }
    return 0;
}

// the null check of a getter's output (or, with another `what`, of any pointer argument)
int require_out(const void *p, const char *what = "null output") {
    if (!p) nbmi::set_error("%s", what);
    return p ? 0 : NBMI_ERR_ARG;
}
// The positions changed behind the handle's back, or what a mass or a force means did: the tree no longer describes
// the state, maxabs_next is not its extent, and the leapfrog's stored a = F(x) is not its force.  A site that drops
// fewer than these three says which survive and why.
void state_changed(nbmi_sim *s) { s->tree_valid = s->maxabs_fused = s->acc_valid = s->tr.acc_valid = false; }

// Runtime values as template arguments: f is a generic lambda and gets std::true_type / std::false_type, or the
// std::integral_constant of the one of Vs... that v equals (v is always one of them).
template <class F>
void with_bool(bool b, F &&f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
template <int... Vs, class F>
void with_int(int v, F &&f) {
    (void)((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// s->step_dt is a step's dt exactly while that step's build is being enqueued: force precision "auto" is decided
// during the build and needs it (auto_prec)
struct DtScope {
    nbmi_sim *s;
    DtScope(nbmi_sim *sim, double dt) : s(sim) { s->step_dt = dt; }
    ~DtScope() { s->step_dt = 0.0; }
};
// What enqueue_tree is asked for.  timing: none, all phase events, or all but the first, which the caller has recorded
// (a leapfrog step: its k_kick_drift counts as the bounds phase).  step_dt > 0 makes it the build of a step with that
// dt: "auto" takes its decision, and the lean key form may serve it (nothing reads a step's keys afterwards).
enum class BuildTiming { kNone, kAll, kCaller };
struct BuildRequest {
    BuildTiming timing = BuildTiming::kNone;
    bool aux = true;  // also write node_ref / node_level (cell queries, owner-mode kernels)
    // where the float64 {cx, cy, cz, G m} row of every node goes (nbmi_diagnostics' tree potential; null: none, a step
    // never writes them)
    double4 *diag_rows = nullptr;
    double step_dt = 0.0;
};
// (A handle with tracers also asks for the float64 node rows their walk reads; a quadrupole build writes its own.)
BuildRequest step_build(const nbmi_sim *s, double dt, BuildTiming timed) {
    double4 *rows = s->tr.m && s->multipole != NBMI_MULTIPOLE_QUADRUPOLE ? s->diag_pot : nullptr;
    return BuildRequest{s->timers ? timed : BuildTiming::kNone, false, rows, dt};
}
// What enqueue_local_sort is asked for.  Owner mode: n_sort rows are keyed and sorted (rows of emigrants are still in
// place, flagged `dead`, and sort to the end); the first n_live of the order are gathered for the tree.
struct SortRequest {
    bool timed = false, lean = false;  // record the key and sort phase events / upper key word only (nbmi_sim::keys_lean)
    int64_t n_sort = -1, n_live = -1;  // -1: all of the handle's rows
    const uint8_t *dead = nullptr;
};

// The octree build in three enqueue stages (one after the other for a single-GPU step; the
// multi-GPU run exchange puts its two collectives between them):
//   enqueue_maxabs      reset the tree header, max |coordinate| of the handle's own bodies
//   enqueue_local_sort  keys -> sort -> tie fix -> gather: the handle's bodies in key order
//   enqueue_global_tree delta -> scans -> node emission over the nt bodies of t_hi/t_lo/t_posm
int enqueue_maxabs(nbmi_sim *s) {
    const int64_t n = s->n;
    hipStream_t st = s->stream;
    Bodies cur = s->buf[s->curbuf];
    if (s->maxabs_fused) {  // the last walk left it behind (and nothing has touched the positions since)
        s->maxabs_fused = false;
        k_header<<<1, 64, 0, st>>>(s->info);
        NBMI_HIP_CHECK(hipGetLastError());
        return 0;
    }
    // reset maxabs/num_nodes/max_level/error (keep counters)
    NBMI_HIP_CHECK(hipMemsetAsync(s->info, 0, offsetof(TreeInfo, wave_visits), st));
    if (n == 0) return 0;  // an owner-mode rank may hold no bodies: the cleared header is all there is (a 0-block launch is an error)
    int gb = nblocks(n);
    if (gb > 256) gb = 256;  // one same-address atomic per block: keep them few
    k_maxabs<<<gb, kBlock, 0, st>>>(cur.x, cur.y, cur.z, n, s->info);
    NBMI_HIP_CHECK(hipGetLastError());
    return 0;
}

// force precision "auto" is decided during the build of a step (it needs dt); anything else leaves the flags alone
static inline bool auto_prec(const nbmi_sim *s) { return s->nodesd && s->force_prec == 0 && s->step_dt > 0.0; }

// Whether a local sort can take the packed, keys-only form: the prefix fits above the index (a prefix widened past 40
// bits by long runs does not), every index fits in 24 bits, and there are no dead rows (owner mode: their all-ones key
// needs one bit more than the prefix).  Everything else sorts (key, index) pairs as before.
static inline bool packed_sort_ok(const nbmi_sim *s, int64_t n, const uint8_t *dead) {
    return s->sort_packed && s->packed && s->sort_bits <= kPackMaxSortBits && n <= ((int64_t)1 << kPackIdxBits) && !dead;
}

int enqueue_local_sort(nbmi_sim *s, const SortRequest &req = {}) {
    const bool lean = req.lean;
    const uint8_t *dead = req.dead;
    s->lean_build = lean;
    const uint64_t *key_lo = lean ? nullptr : s->key_lo;  // what the tie-fix and the gather read
    const int hil = s->hilbert ? 1 : 0;
    const int64_t n = req.n_sort < 0 ? s->n : req.n_sort, n_live = req.n_live < 0 ? n : req.n_live;
    hipStream_t st = s->stream;
    Bodies cur = s->buf[s->curbuf];
    // radix sort on the top sort_bits bits of the upper word, then the tie-fix completes the 126-bit order
    if (s->sort_bits == 0) {
        // enough levels that cells of that level hold about one body on average, plus four: 3 (log8 n + 4) bits,
        // rounded up to whole 8-bit digit passes (1 M and 10 M bodies: 40 bits = 5 passes; measured at 1 M: with
        // 32 bits the tie-fix's runs in the galaxy core cost more (sort phase 0.25 ms) than the pass saved (0.15))
        int levels = 4;
        for (int64_t c = 1; c < n; c *= 8) levels++;
        int bits = ((3 * levels + 7) / 8) * 8;
        if (bits < 16) bits = 16;
        s->sort_bits = bits < 63 ? bits : 63;
    }
    const int shift = 63 - s->sort_bits;
    const bool packed = packed_sort_ok(s, n, dead);
    uint64_t *pk = packed ? s->packed : nullptr;
    // the packed sort's histogram is counted by k_keys_hist, which has the prefixes in registers: the sort's clear goes
    // in front of it, and the sort is told the counts are there (otherwise the sort reads `packed` for them)
    const bool fused = packed && n > 0 && (s->sort_fused_hist < 0 ? fused_hist_pays(n) : s->sort_fused_hist != 0);
    nbmi::RadixHist hist;
    if (fused)
        NBMI_HIP_CHECK(nbmi::radix_keys_prepare_u64(s->tmp_sort, s->tmp_sort_bytes, (size_t)n, kPackIdxBits, kPackIdxBits + s->sort_bits,
                                                    s->sort_cfg, st, &hist));
    with_bool(s->hilbert, [&](auto h) {
        with_bool(lean, [&](auto l) {
            if (fused) {
                const int grid = keys_hist_grid(n);
                const int rounds = (int)((n + (int64_t)grid * kKeysHistBlock - 1) / ((int64_t)grid * kKeysHistBlock));
                k_keys_hist<decltype(h)::value, decltype(l)::value><<<grid, kKeysHistBlock, 0, st>>>(
                    cur.x, cur.y, cur.z, n, s->info, s->key_hi, s->key_lo, pk, shift, hist, rounds);
            }
            else
                k_keys<decltype(h)::value, decltype(l)::value><<<nblocks(n), kBlock, 0, st>>>(cur.x, cur.y, cur.z, n, s->info, s->key_hi,
                                                                                             s->key_lo, s->idx, dead, pk, shift);
        });
    });
    if (req.timed) NBMI_HIP_CHECK(hipEventRecord(s->ev[1], st));
    if (packed) {
        // one 8-byte word per body through the passes instead of an 8-byte key and a 4-byte index: the index sits
        // below the prefix, so a stable sort of the pairs and a sort of the words on the prefix bits give the same order
        NBMI_HIP_CHECK(nbmi::radix_sort_keys_u64(s->tmp_sort, s->tmp_sort_bytes, s->packed, s->packed_s, (size_t)n, kPackIdxBits,
                                                 kPackIdxBits + s->sort_bits, st, s->sort_cfg, fused));
        // the tie-fix reads the unsorted key_hi, so it writes where the pair sort would have put its output: `perm` /
        // `hi_s` are final without a swap
        k_tiefix<true><<<nblocks(n), kBlock, 0, st>>>(s->packed_s, s->key_hi, key_lo, nullptr, shift, s->perm, s->hi_s, n, s->info, cur, hil);
    } else {
        NBMI_HIP_CHECK(nbmi::radix_sort_pairs_u64(s->tmp_sort, s->tmp_sort_bytes, s->key_hi, s->hi_s, s->idx, s->perm,
                                                  (size_t)n, shift, 63, st));
        k_tiefix<false><<<nblocks(n), kBlock, 0, st>>>(s->hi_s, nullptr, key_lo, s->perm, shift, s->idx, s->key_hi, n, s->info, cur, hil,
                                                       dead ? s->let_scan : nullptr, n - n_live);
        // the finished permutation / sorted upper words are `perm` / `hi_s` from here on; the old buffers take
        // the next step's indices and keys
        std::swap(s->perm, s->idx);
        std::swap(s->hi_s, s->key_hi);
    }
    s->t_hi = s->hi_s;
    if (req.timed) NBMI_HIP_CHECK(hipEventRecord(s->ev[2], st));
    // ranks 0 .. n_live: entry n_live is the slot of the totals
    with_bool(lean, [&](auto l) {
        k_gather_scan<decltype(l)::value><<<(int)((n_live + 1 + kScanTile - 1) / kScanTile), kBlock, 0, st>>>(
            cur, s->perm, s->hi_s, key_lo, n_live, s->G, s->posm_s, s->p64_s, lean ? nullptr : s->lo_s, s->delta, s->S, s->Pex,
            s->sub_tot, s->sub_cnt, auto_prec(s) ? s->wave_flag : nullptr, s->sub_flag,
            auto_prec(s) ? (float)(s->prec_tau / (s->step_dt * s->step_dt)) : 0.f, (float)s->softening, s->info, hil);
    });
    return 0;
}

// aux, diag: BuildRequest's aux and diag_rows
int enqueue_global_tree(nbmi_sim *s, bool aux = true, double4 *diag = nullptr) {
    const int64_t n = s->nt;
    hipStream_t st = s->stream;
    // (delta, the in-sub-tile prefixes S / PexL and the sub-tile totals: written by k_gather_scan)
    const int64_t nsub = (n + 1 + kScanTile - 1) / kScanTile;  // sub-tiles that hold the entries 0 .. n
    k_scan_subtiles<<<1, kSubScanThreads, 0, st>>>(s->sub_tot, s->sub_cnt, nsub, s->T, s->subPex,
                                                   auto_prec(s) ? s->sub_flag : nullptr, (n + 63) / 64, s->all64_enter_pm, s->all64_leave_pm, s->info);
    // theta = 0 means "never accept an internal node": s2t = +inf
    const double inv_theta2 = s->theta > 0.0 ? 1.0 / (s->theta * s->theta) : INFINITY;
    const int64_t ob = s->own_base;  // (owner mode: the own tree begins at this row of the walk array; node_level / node_ref / diag64 count from the tree's start)
    const bool quad = s->multipole == NBMI_MULTIPOLE_QUADRUPOLE;
    if (quad) {  // the bottom-up pass goes by level and reads the float64 rows
        aux = true;
        if (!diag) diag = s->quad_pot;
    }
    with_int<kEmitTileSmall, kEmitTile>(n <= kEmitSmallBodies ? kEmitTileSmall : kEmitTile, [&](auto tile) {
        constexpr int kTile = decltype(tile)::value;
        k_emit_tile<kTile><<<(int)((n + kTile - 1) / kTile), kBlock, 0, st>>>(
            s->delta, s->Pex, s->subPex, s->S, s->T, s->t_posm, s->t_hi, s->lean_build ? nullptr : s->t_lo, n,
            s->own_node_rows, s->softening, inv_theta2, s->nodes + ob, s->nodes64 + ob, aux ? s->node_level : nullptr,
            aux ? s->node_ref : nullptr, diag, s->force_prec != 1 && s->nodesd ? s->nodesd + ob : nullptr,
            s->buf[s->curbuf], s->perm, s->G, s->info, s->hilbert ? 1 : 0, ob);
    });
    if (quad && n > 0) {
        // second moments, level by level from the deepest cells up (k_quad_level).  The host does not know the depth:
        // every level is launched, and a launch above the deepest one returns at once
        k_max_level<<<64, kBlock, 0, st>>>(s->delta, n, s->info);
        for (int lev = kMaxLevel; lev >= 0; lev--)
            k_quad_level<<<kQuadGrid, kBlock, 0, st>>>(s->nodes, s->node_level, diag, s->info, lev, s->quad_work, s->nodesq);
    }
    NBMI_HIP_CHECK(hipGetLastError());
    return 0;
}

// Single-GPU build: the tree over the handle's own bodies
int enqueue_tree(nbmi_sim *s, const BuildRequest &req = {}) {
    if (s->owner) {
        nbmi::set_error("this handle is in owner mode: use the nbmi_owner_* calls");
        return NBMI_ERR_ARG;
    }
    const DtScope dt_scope(s, req.step_dt);
    const bool timed = req.timing != BuildTiming::kNone;
    if (req.timing == BuildTiming::kAll) NBMI_HIP_CHECK(hipEventRecord(s->ev[0], s->stream));
    if (int rc = enqueue_maxabs(s)) return rc;
    // a step's build (no queries on it: aux = false) needs no stored low key word; the quadrupole build is one with aux
    const bool lean = s->keys_lean && req.step_dt > 0.0 && !req.aux && s->multipole != NBMI_MULTIPOLE_QUADRUPOLE;
    if (int rc = enqueue_local_sort(s, SortRequest{timed, lean})) return rc;
    if (int rc = enqueue_global_tree(s, req.aux, req.diag_rows)) return rc;
    if (timed) NBMI_HIP_CHECK(hipEventRecord(s->ev[3], s->stream));
    s->tree_valid = req.aux || s->multipole == NBMI_MULTIPOLE_QUADRUPOLE;  // (a quadrupole build always writes node_ref / node_level)
    return 0;
}

// largest |G m| of a host mass array (nbmi_sim::max_gm)
double largest_gm(double G, const double *mass, int64_t n) {
    double m = 0.0;
    for (int64_t i = 0; mass && i < n; i++) m = fabs(mass[i]) > m ? fabs(mass[i]) : m;
    return fabs(G) * m;
}

// Whether the force kernels must skip the pairs at dist_sq <= eps^2 (kGuard) instead of relying on d = 0 to zero the
// own leaf's / the j == i term: at eps == 0 that term is 0 * inf, and so it is at an eps small enough that the fp32
// G m eps^-3 overflows (~1e-13 for G m = 1).  Masses are fixed at creation, so the largest G m decides once; the direct
// kernel with equal masses forms eps^-3 alone, hence at least 1.  2^120 leaves 2^8 below FLT_MAX for the roundings.
bool guarded(const nbmi_sim *s) {
    const float eps2 = (float)(s->softening * s->softening);
    if (!(eps2 > 0.f)) return true;
    const double gm = s->max_gm > 1.0 ? s->max_gm : 1.0;
    return gm / ((double)eps2 * sqrt((double)eps2)) > 0x1p120;
}

// what a force walk does with its result (with_int<kWalkForces, kWalkStep, kWalkLeap>)
constexpr int kWalkForces = 0;  // accelerations in the caller's order, work counters (no integration)
constexpr int kWalkStep = 1;    // the fused kick-drift
constexpr int kWalkLeap = 2;    // a leapfrog epilogue (WalkTable::leap)

// leap (integrating walks only): 0 = kick-drift, kLeapClose / kLeapPrime = the leapfrog epilogues (leap_epilogue)
int enqueue_walk(nbmi_sim *s, bool integrate, double dt, double *acc_out, int leap = 0) {
    const int64_t n = s->n;
    hipStream_t st = s->stream;
    if (!s->wtab || !s->nodes64) {  // the kernels dereference both: never launch without them
        nbmi::set_error("internal: walk table not initialised");
        return NBMI_ERR_ARG;
    }
    const WalkTable *tab = s->wtab + (integrate ? leap : 0);
    WalkParams P;
    P.rank_begin = integrate ? s->shard_begin : 0;
    P.rank_end = integrate ? s->shard_end : n;
    P.eps2 = (float)(s->softening * s->softening);
    const bool guard = guarded(s);
    const int what = !integrate ? kWalkForces : (leap ? kWalkLeap : kWalkStep);
    P.dt = dt;
    P.damping = s->damping;
    const int64_t cntr = P.rank_end - P.rank_begin;
    if (cntr <= 0) return 0;
    P.xcd_chunk = s->xcd_chunk;
    P.pair = s->walk_pair >= 0 ? s->walk_pair : (s->nt >= kHomeSplitBodies ? 2 : 1);
    if (s->owner && s->world > 1 && P.pair == 1) P.pair = 2;  // (the middle of the array may lie in the unused rows in front of the pieces)
    P.curbuf = s->curbuf;
    P.balance = 0;
    P.force_prec = s->nodesd ? s->force_prec : 1;
    P.prec_tau = (float)s->prec_tau;

    if (s->multipole == NBMI_MULTIPOLE_QUADRUPOLE) {  // one one-wave walk at every size
        if (s->owner || !s->nodesq) {
            nbmi::set_error("internal: quadrupole walk on a handle that does not support it");
            return NBMI_ERR_ARG;
        }
        const int gq = (int)((cntr + kBlock - 1) / kBlock);
        with_int<kWalkForces, kWalkStep, kWalkLeap>(what, [&](auto w) {
            with_bool(guard, [&](auto g) {
                constexpr int kW = decltype(w)::value;
                k_walk_quad<kW != kWalkForces, decltype(g)::value, kW == kWalkLeap><<<gq, kBlock, 0, st>>>(
                    s->nodes, s->nodesq, P.force_prec != 1 ? s->nodesd : nullptr, tab, s->info, s->posm_s, s->perm, acc_out, P, s->info);
            });
        });
        NBMI_HIP_CHECK(hipGetLastError());
        return 0;
    }
    // few groups: a block of K waves per group, each walking one K-th of the array.  K depends only on
    // the size of the tree (not on the shard), so that every sharding adds up the same partial sums.
    const int64_t tree_groups = (s->nt + 63) / 64, groups = (cntr + 63) / 64;
    // measured (galaxy, 10 k ... 300 k bodies): the largest K <= 16 with groups x K <= ~9 400 waves is the
    // fastest or within 5 % of it; beyond ~280 k bodies the one-wave walk wins
    int parts = 1;
    while (parts < 16 && tree_groups <= 4300 && tree_groups * parts * 2 <= s->split_max_waves) parts *= 2;
    if (integrate && !guard && parts > 1) {
        with_int<2, 4, 8, 16>(parts, [&](auto k) {
            with_bool(leap != 0, [&](auto l) {
                constexpr int K = decltype(k)::value;
                k_walk_split<K, decltype(l)::value><<<(int)groups, 64 * K, 0, st>>>(s->nodes, tab, s->info, s->posm_s, s->perm, P);
            });
        });
        NBMI_HIP_CHECK(hipGetLastError());
        return 0;
    }
    const int wb = s->walk_block;
    const int gb = (int)((cntr + wb - 1) / wb);
    // balance mode: full, unsharded integrating walks of the product kernel with the default block mapping
    // (measured: 10 M collision walk 15.9 -> 14.8 ms, fp32 10.4 -> 9.8; 4 M galaxy 6.96 -> 6.90; at 1 M bodies the eighths are
    // within 1 % of each other already and the half-empty launch costs 2 %: from 8 192 blocks = 2 M bodies on)
    const bool balance = integrate && !guard && s->xcd_balance && s->xcd_chunk == 0 && wb == kBlock && !s->owner &&
                         (gb >= 8192 || s->xcd_balance > 1) && gb >= kXcdMinBlocks &&  // (k_xcd_bounds' precondition)
                         P.rank_begin == 0 && P.rank_end == n && getenv("NBMI_XCD_CHUNK") == nullptr;
    const int jmax = (int)xcd_jmax(gb);  // balance mode: the launch has 8 jmax workgroups
    if (balance) {
        if (s->cut_pending) {  // the cuts made from the last walk's times (on the side stream)
            NBMI_HIP_CHECK(hipStreamWaitEvent(st, s->ev_cut, 0));
            s->cut_pending = false;
        }
        if (s->balance_blocks != gb) {  // first use (or another shard size): no times yet -> equal eighths
            NBMI_HIP_CHECK(hipMemsetAsync(s->wave_cycles, 0, (size_t)gb * 16, st));
            k_xcd_bounds<<<1, 1024, 0, st>>>(s->wave_cycles, gb, jmax, s->xcd_bounds);
            s->balance_blocks = gb;
        }
        P.balance = 1;
        if (!s->side) {
            NBMI_HIP_CHECK(hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking));
            NBMI_HIP_CHECK(hipEventCreateWithFlags(&s->ev_walked, hipEventDisableTiming));
            NBMI_HIP_CHECK(hipEventCreateWithFlags(&s->ev_cut, hipEventDisableTiming));
        }
    }
    const int grid = balance ? 8 * jmax : gb;
    with_int<kWalkForces, kWalkStep, kWalkLeap>(what, [&](auto w) {
        with_bool(guard, [&](auto g) {
            constexpr int kW = decltype(w)::value;
            k_walk<kW != kWalkForces, kW == kWalkForces, decltype(g)::value, kW == kWalkLeap><<<grid, wb, 0, st>>>(
                s->nodes, tab, s->info, s->posm_s, s->perm, acc_out, P, s->info);
        });
    });
    NBMI_HIP_CHECK(hipGetLastError());
    if (balance) {
        s->balanced_walks++;
        // cuts for the next step: beside whatever the main stream does next (the next step's keys, sort and build)
        NBMI_HIP_CHECK(hipEventRecord(s->ev_walked, st));
        NBMI_HIP_CHECK(hipStreamWaitEvent(s->side, s->ev_walked, 0));
        k_xcd_bounds<<<1, 1024, 0, s->side>>>(s->wave_cycles, gb, jmax, s->xcd_bounds);
        NBMI_HIP_CHECK(hipGetLastError());
        NBMI_HIP_CHECK(hipEventRecord(s->ev_cut, s->side));
        s->cut_pending = true;
    }
    return 0;
}

// leap (kIntegrate only): 0 = kick-drift, kLeapClose / kLeapPrime = the leapfrog epilogues (acc_out: the acceleration
// columns); kLeapClose finds posm_s already packed by k_kick_drift
template <bool kIntegrate>
int launch_direct(nbmi_sim *s, double dt, double *acc_out, int leap = 0) {
    const int64_t n = s->n;
    hipStream_t st = s->stream;
    Bodies cur = s->buf[s->curbuf], nxt = s->buf[1 - s->curbuf];
    if (leap != kLeapClose) k_pack_posm<<<nblocks(n), kBlock, 0, st>>>(cur, n, s->G, s->posm_s);
    const float eps2 = (float)(s->softening * s->softening);
    const bool guard = guarded(s);
    // multi-GPU: a sharded handle integrates only the bodies [shard_begin, shard_end) (index order:
    // the direct method never re-orders the state); the force pass always covers everything
    const int64_t ibeg = kIntegrate ? s->shard_begin : 0, iend = kIntegrate ? s->shard_end : n;
    const int64_t cnt = iend - ibeg;
    if (cnt <= 0) return 0;
    // bodies per thread: enough blocks to cover 256 CUs a few times over
    int ib = cnt >= 512 * 1024 ? 4 : (cnt >= 128 * 1024 ? 2 : 1);
    // pair arithmetic: 0 = guarded, 1 = all masses equal (G m is a constant), 2 = the general form
    const int pairs = guard ? 0 : (s->uniform_gm > 0.0 ? 1 : 2);
    with_int<1, 2, 4>(ib, [&](auto ibv) {
        with_int<0, 1, 2>(pairs, [&](auto pv) {
            with_int<0, kLeapClose, kLeapPrime>(leap, [&](auto lv) {
                constexpr int kIB = decltype(ibv)::value, kPairs = decltype(pv)::value;
                constexpr int kLV = kIntegrate ? decltype(lv)::value : 0;  // (the force pass has no epilogue to choose)
                const int gb = (int)((cnt + (int64_t)kBlock * kIB - 1) / ((int64_t)kBlock * kIB));
                k_direct<kIB, kPairs == 0, kIntegrate, kPairs == 1, kLV><<<gb, kBlock, 0, st>>>(
                    s->posm_s, n, ibeg, iend, eps2, cur, nxt, acc_out, dt, s->damping, kPairs == 1 ? s->uniform_gm : 0.0);
            });
        });
    });
    NBMI_HIP_CHECK(hipGetLastError());
    return 0;
}

// [leapfrog] The acceleration columns exist (allocated by the first leapfrog step) and hold a = F(x) of the current state
// (primed once after create / nbmi_set_state / a switch into leapfrog / a reported capacity error, inside the step so that
// force precision "auto" sees its dt).
int leap_prepare_bodies(nbmi_sim *s, double dt) {
    if (!s->acc) {
        if (dev_alloc(s, &s->acc, (size_t)3 * s->n)) return NBMI_ERR_HIP;
        NBMI_HIP_CHECK(hipMemsetAsync(s->acc, 0, (size_t)3 * s->n * sizeof(double), s->stream));
        if (s->method == NBMI_METHOD_BARNES_HUT && upload_walk_table(s)) return NBMI_ERR_HIP;
    }
    if (s->acc_valid) return 0;
    if (s->method == NBMI_METHOD_BARNES_HUT) {
        if (int rc = enqueue_tree(s, step_build(s, dt, BuildTiming::kNone))) return rc;
        if (int rc = enqueue_walk(s, true, dt, nullptr, kLeapPrime)) return rc;
        s->tree_valid = false;
    } else {
        if (int rc = launch_direct<true>(s, dt, s->acc, kLeapPrime)) return rc;
    }
    s->acc_valid = true;
    return 0;
}
int tracer_leap_prepare(nbmi_sim *s);  // (below, beside the other tracer stages)
// the bodies' stored acceleration, then the tracers'
int leap_prepare(nbmi_sim *s, double dt) {
    if (int rc = leap_prepare_bodies(s, dt)) return rc;
    return s->tr.m ? tracer_leap_prepare(s) : 0;
}

// [leapfrog] Opening half-kick + drift of the current buffer into the other one (k_kick_drift), which becomes current
// for the force pass.  The grid is capped: one same-address atomic per block (as k_maxabs).
int enqueue_kick_drift(nbmi_sim *s, double dt) {
    const int64_t n = s->n;
    int gb = nblocks(n);
    if (gb > 2048) gb = 2048;
    const bool bh = s->method == NBMI_METHOD_BARNES_HUT;
    k_kick_drift<<<gb, kBlock, 0, s->stream>>>(s->buf[s->curbuf], s->buf[1 - s->curbuf], s->acc, s->acc + n, s->acc + 2 * n, n,
                                                dt, s->G, bh ? nullptr : s->posm_s, bh ? &s->info->maxabs_next : nullptr);
    NBMI_HIP_CHECK(hipGetLastError());
    s->curbuf ^= 1;
    return 0;
}

// NBMI_ERR_CAPACITY with the message of a build that ran out of node rows; `tail`: what that meant for the bodies
int capacity_error(const nbmi_sim *s, long long nodes, const char *tail) {
    nbmi::set_error("octree needs %lld nodes, more than the %lld rows allocated%s", nodes, (long long)s->node_capacity, tail);
    return NBMI_ERR_CAPACITY;
}

// What the device error words mean, whoever fetched them (check_device_error from the device, nbmi_frame_wait from its
// snapshot's header): the host-side consequences, the message and the code.
int decode_device_error(nbmi_sim *s, const FrameHeader &w) {
    if (w.sort_error) {  // a look-back spin of the radix sort timed out: that pass scattered to wrong offsets
        nbmi::set_error("device radix sort: a look-back spin timed out; the steps since the last synchronisation are invalid");
        return NBMI_ERR_HIP;
    }
    if (w.max_run > 4096) {
        // many bodies agree on the sorted prefix (a dense core inside one level-13 cell): the tie-fix did the rest
        // correctly but at L reads per member - sort on more bits from the next step on.  The run may be one in the whole
        // upper word, where every member recomputes the others' low words: full keys from now on
        if (s->sort_bits < 63) s->sort_bits = s->sort_bits + 8 < 63 ? s->sort_bits + 8 : 63;
        s->keys_lean = false;
    }
    if (w.error || w.sticky_error)
        return capacity_error(s, w.sticky_error ? w.sticky_nodes : w.num_nodes,
                              " (4N, as the reference); the bodies were not advanced from that step on");
    return 0;
}

// Fetches and decodes the error words behind everything on the stream, and puts device and handle in order again
int check_device_error(nbmi_sim *s) {
    if (s->method != NBMI_METHOD_BARNES_HUT) return 0;  // (a direct handle builds and sorts nothing)
    TreeInfo h;
    unsigned sort_err = 0u;
    NBMI_HIP_CHECK(hipMemcpyAsync(&h, s->info, sizeof(h), hipMemcpyDeviceToHost, s->stream));
    if (s->tmp_sort) NBMI_HIP_CHECK(nbmi::radix_error_word(s->tmp_sort, &sort_err, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    const int rc = decode_device_error(s, FrameHeader{h.error, h.sticky_error, h.max_run, sort_err, h.num_nodes, h.sticky_nodes, {}});
    if (sort_err) {
        NBMI_HIP_CHECK(nbmi::radix_init_temp(s->tmp_sort, s->stream));
        NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
        s->tree_valid = false;  // (the positions and the header are as they were: the other two survive)
    } else if (rc) {
        // reported once: clear the sticky word so the handle can go on after nbmi_set_state / a retry.  The
        // bodies stand at the last step that completed (the walk froze them while the word was set).
        NBMI_HIP_CHECK(hipMemsetAsync(&s->info->sticky_error, 0, sizeof(int), s->stream));
        NBMI_HIP_CHECK(hipMemsetAsync(&s->info->error, 0, sizeof(int), s->stream));
        NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
        state_changed(s);  // (leapfrog: a priming walk may have been frozen; the next step primes again)
    }
    return rc;
}

// A query's own octree build between two steps (nbmi_diagnostics' potential, the k-NN query, the group finder).  The build overwrites the
// tree header (maxabs_next, force_all64, the counters) and host fields of the handle; the scope puts both back, so the
// next step finds the handle as it would have without the query.
struct SideBuild {
    nbmi_sim *s;
    // The host fields that a build which is no step's, or the report of its error, changes.  (step_dt is none:
    // enqueue_tree installs its request's 0 itself.)  Left out, after a look at enqueue_tree, enqueue_local_sort and
    // decode_device_error:
    //   lean_build  every enqueue_local_sort writes it before its one reader, the same build's enqueue_global_tree
    //   t_hi, and perm / idx, hi_s / key_hi, which a pair sort swaps: they name the last build's arrays - what a tree
    //               that is valid afterwards is read through - and every build writes them before it reads them
    //   acc_valid   no build touches it, and a reported capacity error is to drop it for good
    struct Saved {
        bool tree_valid, maxabs_fused;
        int sort_bits;   // chosen by the first build; widened, and ...
        bool keys_lean;  // ... dropped, where the query's own error check sees a long run: the next step's build shows it again
    } saved;
    int rc;  // of the construction: nothing to finish if set
    explicit SideBuild(nbmi_sim *sim)
        : s(sim), saved{s->tree_valid, s->maxabs_fused, s->sort_bits, s->keys_lean}, rc(save_header()) {}
    int save_header() {
        if (!s->side_info && dev_alloc(s, &s->side_info, 1)) return NBMI_ERR_HIP;
        NBMI_HIP_CHECK(hipMemcpyAsync(s->side_info, s->info, sizeof(TreeInfo), hipMemcpyDeviceToDevice, s->stream));
        return 0;
    }
    // r: of the build and the query's kernels.  wait (the diagnostic): the query is waited for and a capacity error of
    // its build reported at once - check_device_error clears the words, so k_query_restore then writes the saved header
    // as it is.  Otherwise (k-NN) nothing waits, and k_query_restore keeps the build's error in the sticky words for the
    // next call that looks.
    int finish(int r, bool wait) {
        if (wait && r == 0) r = check_device_error(s);  // NBMI_ERR_CAPACITY: the message of a step
        k_query_restore<<<1, 64, 0, s->stream>>>(s->info, s->side_info);
        if (hipGetLastError() != hipSuccess && r == 0) {
            nbmi::set_error("k_query_restore launch failed");
            r = NBMI_ERR_HIP;
        }
        // the same positions give the same tree: what the queries read is still that tree if it was before
        s->tree_valid = saved.tree_valid && r == 0;
        s->maxabs_fused = saved.maxabs_fused;
        s->sort_bits = saved.sort_bits;
        s->keys_lean = saved.keys_lean;
        return r;
    }
};

// ---- the float64 probe family (potentials, nbmi_field_at, tracers: sections 4.9, 4.18, 4.19) ----
// The octree of the current positions with the float64 node rows {cx, cy, cz, G M}, inside a SideBuild, and on it what
// `walk` enqueues (its result is the call's).  What the callers differ in:
//   report_first  a capacity error of an earlier step is waited for and reported first, as a getter does (the tracers'
//                 priming is part of a step and never waits)
//   check_build   the build's own capacity error is reported before `walk` runs: nothing is copied out of a walk that
//                 did not run
//   wait          SideBuild::finish's
//   step_rows     the rows go where a step's build puts them (step_build).  A quadrupole build writes them to the rows it
//                 is given or, given none, to quad_pot: the tracers' walk reads quad_pot in that mode, on this tree as
//                 on a step's, so their build is given none there; the other two read diag_pot in either mode.
template <class Walk>
int side_tree(nbmi_sim *s, bool report_first, bool check_build, bool wait, bool step_rows, Walk walk) {
    if (!s->diag_pot && dev_alloc(s, &s->diag_pot, s->node_capacity + 2)) return NBMI_ERR_HIP;
    if (report_first) {
        NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
        if (int rc = check_device_error(s)) return rc;
    }
    SideBuild side(s);  // (no "auto" decision in its build: the wave flags and force_all64 stay the last step's)
    if (side.rc) return side.rc;
    BuildRequest build;
    build.aux = false;
    build.diag_rows = step_rows && s->multipole == NBMI_MULTIPOLE_QUADRUPOLE ? nullptr : s->diag_pot;
    int rc = enqueue_tree(s, build);
    if (rc == 0 && check_build) rc = check_device_error(s);
    if (rc == 0) rc = walk();
    return side.finish(rc, wait);
}

void probe_free(nbmi_sim *s, ProbeScratch &g) {
    dev_free(s, &g.sx); dev_free(s, &g.sy); dev_free(s, &g.sz); dev_free(s, &g.key); dev_free(s, &g.key_s);
    dev_free(s, &g.idx); dev_free(s, &g.order); dev_free(s, &g.sort_tmp); dev_free(s, &g.wtab);
    g.rows = 0;
    g.sort_bytes = 0;
}
// An empty scratch for chunks of `rows` probes, its sort buffer initialised and its walk table on the device; on failure
// nothing is left allocated.  Of the table the probe walk reads n64, theta, eps2 (exact_take_idx, field_walk) and
// buf[0].x / y / z, the columns.  None of them changes after create_impl - the later uploads of the handle's own table
// (upload_walk_table) bring the acceleration columns and nodesd - so one upload per allocation serves.  Waits for the
// stream: the table is a stack object.
int probe_alloc(nbmi_sim *s, ProbeScratch &g, int64_t rows) {
    const size_t r = (size_t)rows;
    g.sort_bytes = nbmi::radix_temp_bytes_u64(r, kFieldSortBits);
    auto fill = [&]() -> int {
        if (dev_alloc(s, &g.sx, r) || dev_alloc(s, &g.sy, r) || dev_alloc(s, &g.sz, r) || dev_alloc(s, &g.key, r) ||
            dev_alloc(s, &g.key_s, r) || dev_alloc(s, &g.idx, r) || dev_alloc(s, &g.order, r) ||
            dev_alloc(s, &g.sort_tmp, g.sort_bytes + 256) || dev_alloc(s, &g.wtab, 1))
            return NBMI_ERR_HIP;
        WalkTable t = walk_table(s);
        t.buf[0].x = g.sx; t.buf[0].y = g.sy; t.buf[0].z = g.sz;
        NBMI_HIP_CHECK(nbmi::radix_init_temp(g.sort_tmp, s->stream));
        NBMI_HIP_CHECK(hipMemcpyAsync(g.wtab, &t, sizeof(t), hipMemcpyHostToDevice, s->stream));
        NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
        return 0;
    };
    if (int rc = fill()) {
        probe_free(s, g);
        return rc;
    }
    g.rows = rows;
    return 0;
}
// One chunk of mc <= g.rows probes, pts (mc, 3), into the columns in walk order: keys in the tree's root cube, sort,
// gather.  *order: the probe at each rank, or null where the chunk is walked as it came (NBMI_FIELD_SORT=0, or a chunk
// of one wave: there is no neighbour to choose).
int probe_order_chunk(nbmi_sim *s, ProbeScratch &g, const double *pts, int64_t mc, const uint32_t **order) {
    hipStream_t st = s->stream;
    *order = nullptr;
    if (s->field_sort && mc > 64) {
        if (s->hilbert) k_field_keys<true><<<nblocks(mc), kBlock, 0, st>>>(pts, mc, s->info, g.key, g.idx);
        else k_field_keys<false><<<nblocks(mc), kBlock, 0, st>>>(pts, mc, s->info, g.key, g.idx);
        NBMI_HIP_CHECK(nbmi::radix_sort_pairs_u64(g.sort_tmp, g.sort_bytes, g.key, g.key_s, g.idx, g.order, (size_t)mc,
                                                  63 - kFieldSortBits, 63, st));
        *order = g.order;
    }
    k_field_gather<<<nblocks(mc), kBlock, 0, st>>>(pts, *order, mc, g.sx, g.sy, g.sz);
    return 0;
}
// Waits for the stream and looks at the sort's error word: set, the temp buffer is made ready again and `what` reported.
int probe_sort_error(nbmi_sim *s, ProbeScratch &g, const char *what) {
    unsigned sort_err = 0u;
    if (g.sort_tmp) NBMI_HIP_CHECK(nbmi::radix_error_word(g.sort_tmp, &sort_err, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    if (!sort_err) return 0;
    NBMI_HIP_CHECK(nbmi::radix_init_temp(g.sort_tmp, s->stream));
    nbmi::set_error("%s", what);
    return NBMI_ERR_HIP;
}

// The chunks of one call of `who` through nbmi_field_at's scratch, one after the other: a chunk's points are uploaded
// and - `tree`: a tree stands - put in walk order (probe_order_chunk; `order` stays null otherwise), walk(b, mc, order)
// enqueues the kernel of the chunk of mc points that starts at point b, `copy_out(b, mc)` the copies of its results, and
// the stream is waited for, since the next chunk overwrites the scratch.  At the end the sort's error word.
template <class Walk, class CopyOut>
int probe_chunks(nbmi_sim *s, const char *who, bool tree, int64_t m, const double *pts, Walk walk, CopyOut copy_out) {
    auto &f = s->field;
    hipStream_t st = s->stream;
    for (int64_t b = 0; b < m; b += f.rows) {
        const int64_t mc = m - b < f.rows ? m - b : f.rows;
        NBMI_HIP_CHECK(hipMemcpyAsync(f.pts, pts + 3 * b, (size_t)mc * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        const uint32_t *order = nullptr;
        if (tree) {
            if (int rc = probe_order_chunk(s, f, f.pts, mc, &order)) return rc;
        }
        walk(b, mc, order);
        if (int rc = launch_failed("%s: a kernel launch failed", who)) return rc;
        if (int rc = copy_out(b, mc)) return rc;
        NBMI_HIP_CHECK(hipStreamSynchronize(st));
    }
    char what[64];
    snprintf(what, sizeof(what), "%s: the sort of the points failed", who);
    return tree ? probe_sort_error(s, f, what) : 0;
}

// ---- tracers (section 4.19): what a step enqueues for them; nothing here waits for the device ----
// Whether the tracers' field comes from k_field_direct's sum: a direct handle, or no bodies at all (a = 0).
bool tracers_direct(const nbmi_sim *s) { return s->method != NBMI_METHOD_BARNES_HUT || s->n == 0; }

// All tracers through one walk with epilogue `leap` (0 / kLeapClose / kLeapPrime).  Barnes-Hut: on the tree that stands,
// built with the float64 node rows (step_build); chunk by chunk through the tracers' scratch (probe_order_chunk, walk) as
// nbmi_field_at's chunks go.
int enqueue_tracers(nbmi_sim *s, int leap, double dt) {
    auto &t = s->tr;
    hipStream_t st = s->stream;
    const double eps2 = s->softening * s->softening;
    if (tracers_direct(s)) {  // (one launch per chunk too: m x N pair terms in one kernel would hold the device for long)
        for (int64_t b = 0; b < t.m; b += kFieldChunk) {
            const int64_t mc = t.m - b < kFieldChunk ? t.m - b : kFieldChunk;
            with_int<0, kLeapClose, kLeapPrime>(leap, [&](auto lv) {
                k_tracer_direct<decltype(lv)::value><<<nblocks(mc), kBlock, 0, st>>>(
                    s->buf[s->curbuf], s->n, s->G, eps2, mc, t.p + 3 * b, t.v + 3 * b, t.a ? t.a + 3 * b : nullptr, dt, s->damping);
            });
            NBMI_HIP_CHECK(hipGetLastError());
        }
        return 0;
    }
    const bool quad = s->multipole == NBMI_MULTIPOLE_QUADRUPOLE;
    for (int64_t b = 0; b < t.m; b += t.rows) {
        const int64_t mc = t.m - b < t.rows ? t.m - b : t.rows;
        double *p = t.p + 3 * b, *v = t.v + 3 * b, *a = t.a ? t.a + 3 * b : nullptr;
        const uint32_t *order;
        if (int rc = probe_order_chunk(s, t, p, mc, &order)) return rc;
        with_bool(quad, [&](auto q) {
            with_int<0, kLeapClose, kLeapPrime>(leap, [&](auto lv) {
                k_tracer_tree<decltype(q)::value, decltype(lv)::value><<<nblocks(mc), kBlock, 0, st>>>(
                    s->nodes, quad ? s->quad_pot : s->diag_pot, t.wtab, s->info, t.sx, t.sy, t.sz, order, mc, (float)eps2,
                    s->softening, t.pmax, quad ? s->quad_work : nullptr, p, v, a, dt, s->damping);
            });
        });
        NBMI_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

// [leapfrog] the tracers' opening half-kick and drift.  Barnes-Hut: after the substep's build, whose error words it reads.
int enqueue_tracer_kick_drift(nbmi_sim *s, double dt) {
    auto &t = s->tr;
    const bool direct = tracers_direct(s);
    k_tracer_kick_drift<<<nblocks(t.m), kBlock, 0, s->stream>>>(direct ? nullptr : s->info, t.m, t.p, t.v, t.a, dt,
                                                                 direct ? nullptr : t.pmax);
    NBMI_HIP_CHECK(hipGetLastError());
    return 0;
}

// [leapfrog] The tracers' acceleration rows exist and hold a = F(p) for the current bodies and tracers.  Barnes-Hut: the
// priming walk needs a tree of the current positions with the float64 rows, and the step has none at this point (the
// bodies may not need priming): a side_tree of its own, as a query's, so the bodies' next step finds the handle as it
// would without tracers.
int tracer_leap_prepare(nbmi_sim *s) {
    auto &t = s->tr;
    if (!t.a) {
        if (dev_alloc(s, &t.a, (size_t)3 * t.m)) return NBMI_ERR_HIP;
        NBMI_HIP_CHECK(hipMemsetAsync(t.a, 0, (size_t)3 * t.m * sizeof(double), s->stream));
        t.acc_valid = false;
    }
    if (t.acc_valid) return 0;
    auto prime = [&] { return enqueue_tracers(s, kLeapPrime, 0.0); };
    const int rc = tracers_direct(s) ? prime() : side_tree(s, false, false, false, true, prime);
    if (rc == 0) t.acc_valid = true;  // (only once everything is enqueued, as the bodies')
    return rc;
}

// One group of the queries' scratch (nbmi_sim::q), once: `alloc` makes its dev_allocs and returns nonzero if one failed.
template <class Group, class Alloc>
int query_alloc(Group &g, Alloc alloc) {
    if (!g.ready && alloc()) return NBMI_ERR_HIP;
    g.ready = true;
    return 0;
}
// What every query of this family enqueues on the compute stream without ever waiting: inside a SideBuild the octree of
// the current positions is built with the query rows (node_ref), the rows and the waves' first leaves are written
// (query_buffers first), then `launch` adds the query's own kernels.  A capacity error of the build stays in the sticky
// words for the next call that looks.
int query_buffers(nbmi_sim *s) {
    auto &g = s->q.shared;
    return query_alloc(g, [&] {
        return dev_alloc(s, &g.rows, s->node_capacity + 2) || dev_alloc(s, &g.wleaf, (s->n + 63) / 64) || dev_alloc(s, &g.evals, 1);
    });
}
// The scope itself: `work` (its result is the call's) runs with the tree and the rows enqueued, and may wait.
template <class Work>
int query_tree(nbmi_sim *s, Work work) {
    SideBuild side(s);
    if (side.rc) return side.rc;
    int rc = enqueue_tree(s);
    if (rc == 0) {
        k_query_rows<<<nblocks(s->own_node_rows), kBlock, 0, s->stream>>>(s->nodes, s->nodes64, s->node_ref, s->perm,
                                                                           s->buf[s->curbuf], s->info, s->own_node_rows,
                                                                           s->q.shared.rows, s->q.shared.wleaf);
        rc = work();
    }
    return side.finish(rc, false);
}
template <class Launch>
int query_enqueue(nbmi_sim *s, const char *what, Launch launch) {
    return query_tree(s, [&]() -> int {
        launch();
        return launch_failed("%s launch failed", what);
    });
}
// The synchronous form of a query: errors of earlier steps first, as a getter reports them, then the query (`enqueue`,
// one of the *_enqueue forms, which never wait) and its own.
template <class Enqueue>
int query_sync(nbmi_sim *s, Enqueue enqueue) {
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    if (int rc = check_device_error(s)) return rc;
    if (int rc = enqueue()) return rc;
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    return check_device_error(s);
}
// Which handles have the tree the queries walk: every other is refused as `what`.
int query_refuse(const nbmi_sim *s, const char *what) {
    const char *why = s->method != NBMI_METHOD_BARNES_HUT ? "direct N^2 handles have no tree"
                      : s->owner ? "owner-mode handles are not supported (the neighbours may live on other ranks)"
                      : s->shard_begin != 0 || s->shard_end != s->n ? "sharded handles are not supported"
                                                                    : nullptr;
    if (!why) return 0;
    nbmi::set_error("%s: %s", what, why);
    return NBMI_ERR_ARG;
}

// ---- the host side of the fixed-point sums over the state rows (nbmi_deposit, nbmi_radial_profile, nbmi_mass_radii) ----
// Which handles hold every body: every other is refused as `who`.
int sums_refuse(nbmi_sim *s, const char *who) {
    if (int rc = check_handle(s)) return rc;
    const char *why = s->owner ? "owner-mode handles are not supported (the other ranks hold the rest of the bodies)"
                      : s->shard_begin != 0 || s->shard_end != s->n ? "sharded handles are not supported"
                                                                    : nullptr;
    if (!why) return 0;
    nbmi::set_error("%s: %s", who, why);
    return NBMI_ERR_ARG;
}
// The exponent rule ("The quantum and its bound").  With max |q| in [2^(E-1), 2^E) and L the bit
// length of N, the quantum 2^(E + L - headroom) keeps every |k| below 2^(headroom - L) and so any sum of N of them
// below 2^headroom: 62 where a sum only has to fit a signed 64-bit word, 53 where (nbmi_mass_radii) every prefix sum
// also has to be an exact double.  mx_bits = what k_plane_max wrote; a plane that is all zero gets e = 0 and live = 0.
constexpr int kSumHeadroom = 62, kExactSumHeadroom = 53;
int plane_exponents(const char *who, const unsigned long long *mx_bits, int64_t n, int headroom, int planes, const int *slot,
                    const char *const *plane_name, int *e, int *live) {
    const int L = 64 - __builtin_clzll((unsigned long long)n);  // the bit length of N
    for (int p = 0; p < planes; p++) {
        double mx;
        memcpy(&mx, &mx_bits[p], sizeof(mx));
        if (!isfinite(mx)) {
            nbmi::set_error("%s: the largest |q| of plane %d (%s) is not finite", who, p, plane_name[slot[p]]);
            return NBMI_ERR_ARG;
        }
        int E = 0;
        if (mx != 0.0) (void)frexp(mx, &E);
        live[p] = mx != 0.0;
        e[p] = mx != 0.0 ? E + L - headroom : 0;
    }
    return 0;
}
// grid of k_plane_max
int plane_max_blocks(int64_t n) { return (int)(nblocks(n) < 1024 ? nblocks(n) : 1024); }
// The device time of a call's kernel groups, without its copies: begin() and end() bracket a group on the stream while
// the timers are on (at most three per call), and add(), once the stream has been waited for, sums them into "other".
struct TimedSpans {
    nbmi_sim *s;
    int spans = 0;
    hipError_t begin() { return s->timers ? hipEventRecord(s->ev[2 * spans], s->stream) : hipSuccess; }
    hipError_t end() { return s->timers ? hipEventRecord(s->ev[2 * spans++ + 1], s->stream) : hipSuccess; }
    hipError_t add() {
        double total = 0.0;
        for (int k = 0; s->timers && k < spans; k++) {
            float ms = 0.0f;
            if (hipError_t err = hipEventElapsedTime(&ms, s->ev[2 * k], s->ev[2 * k + 1])) return err;
            total += (double)ms;
        }
        s->ms[4] += total;
        return hipSuccess;
    }
};

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================
extern "C" {

int nbmi_device_count(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

const char *nbmi_last_error(void) { return nbmi::get_error(); }

void nbmi_destroy(nbmi_sim *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->side) {
        (void)hipStreamSynchronize(s->side);
        (void)hipStreamDestroy(s->side);
        (void)hipEventDestroy(s->ev_walked);
        (void)hipEventDestroy(s->ev_cut);
    }
    if (s->frame_stream) {
        (void)hipStreamSynchronize(s->frame_stream);
        (void)hipStreamDestroy(s->frame_stream);
    }
    for (auto &f : s->frame_slot) {
        if (f.ev_snap) (void)hipEventDestroy(f.ev_snap);
        if (f.ev_done) (void)hipEventDestroy(f.ev_done);
        if (f.host) (void)hipHostFree(f.host);
    }
    for (void *p : s->allocs) (void)hipFree(p);
    for (auto &e : s->ev)
        if (e) (void)hipEventDestroy(e);
    if (s->ev_info) (void)hipEventDestroy(s->ev_info);
    if (s->h_info) (void)hipHostFree(s->h_info);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

// why this handle cannot run in quadrupole mode (nullptr: it can)
static const char *multipole_refusal(const nbmi_sim *s) {
    if (s->method != NBMI_METHOD_BARNES_HUT) return "direct N^2 handles have no cells";
    if (s->owner) return "owner-mode handles are not supported (the exchanged tree rows carry no second moments)";
    if (s->shard_begin != 0 || s->shard_end != s->n) return "sharded handles are not supported (the exchange rows carry no second moments)";
    return nullptr;
}

// measurement / tuning knobs, read once per handle by both constructors
static void read_env_knobs(nbmi_sim *s) {
    if (const char *e = getenv("NBMI_XCD_CHUNK")) s->xcd_chunk = atoi(e);
    if (const char *e = getenv("NBMI_XCD_BALANCE")) s->xcd_balance = atoi(e);
    if (const char *e = getenv("NBMI_SPLIT_WAVES")) s->split_max_waves = atoll(e);
    if (const char *e = getenv("NBMI_WALK_PAIR")) s->walk_pair = atoi(e);
    if (const char *e = getenv("NBMI_FUSE_MAXABS")) s->fuse_maxabs = atoi(e) != 0;
    if (const char *e = getenv("NBMI_HILBERT")) s->hilbert = atoi(e) != 0;
    if (const char *e = getenv("NBMI_SORT_PACKED")) s->sort_packed = atoi(e) != 0;
    if (const char *e = getenv("NBMI_SORT_DIGIT_BITS")) s->sort_cfg.digit_bits = atoi(e);
    if (const char *e = getenv("NBMI_SORT_THREADS")) s->sort_cfg.threads = atoi(e);
    if (const char *e = getenv("NBMI_SORT_FUSED_HIST")) s->sort_fused_hist = atoi(e) != 0 ? 1 : 0;
    if (const char *e = getenv("NBMI_KEYS_LEAN")) s->keys_lean = atoi(e) != 0;
    if (const char *e = getenv("NBMI_PAIRS_CELLS")) s->pair_cells = atoi(e) != 0;
    if (const char *e = getenv("NBMI_FIELD_SORT")) s->field_sort = atoi(e) != 0;
    if (const char *e = getenv("NBMI_DEPOSIT_AGG")) s->deposit_agg = atoi(e) != 0;
    if (const char *e = getenv("NBMI_FORCE_PREC")) {
        const int v = atoi(e);
        if (v >= 0 && v <= 2) s->force_prec = v;
    }
    if (const char *e = getenv("NBMI_PREC_TAU")) s->prec_tau = atof(e);
    if (const char *e = getenv("NBMI_MULTIPOLE")) {
        if (!strcmp(e, "quadrupole") || !strcmp(e, "1")) s->multipole_env = NBMI_MULTIPOLE_QUADRUPOLE;
    }
    if (const char *e = getenv("NBMI_ALL64_ENTER")) s->all64_enter_pm = (int)(1000.0 * atof(e) + 0.5);
    if (const char *e = getenv("NBMI_ALL64_LEAVE")) s->all64_leave_pm = (int)(1000.0 * atof(e) + 0.5);
    if (const char *e = getenv("NBMI_SORT_BITS")) {
        const int b = atoi(e);
        if (b >= 8 && b <= 63) s->sort_bits = b;
    }
    if (const char *e = getenv("NBMI_WALK_BLOCK")) {
        const int b = atoi(e);
        if (b == 64 || b == 128 || b == 256) s->walk_block = b;
    }
}

// a create that failed: the handle goes, the message stays
static nbmi_sim *create_failed(nbmi_sim *s) {
    std::string keep = nbmi::get_error();
    nbmi_destroy(s);
    nbmi::set_error("%s", keep.c_str());
    return nullptr;
}

static int create_impl(nbmi_sim *s, const double *pos, const double *vel, const double *mass) {
    const int64_t n = s->n;
    const int64_t c = s->cap > n ? s->cap : n;  // rows allocated (owner mode keeps head room for immigrants)
    if (!nbmi::radix_config_ok(s->sort_cfg)) {
        nbmi::set_error("NBMI_SORT_DIGIT_BITS must be 8 or 10 and NBMI_SORT_THREADS 256, 512 or 1024 (got %d, %d)", s->sort_cfg.digit_bits,
                        s->sort_cfg.threads);
        return NBMI_ERR_ARG;
    }
    NBMI_HIP_CHECK(hipSetDevice(s->device));
    NBMI_HIP_CHECK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    for (auto &e : s->ev) NBMI_HIP_CHECK(hipEventCreate(&e));
    if (alloc_bodies(s, &s->buf[0], c) || alloc_bodies(s, &s->buf[1], c)) return -2;
    if (dev_alloc(s, &s->posm_s, c) || dev_alloc(s, &s->colors, 3 * (c ? c : 1)) || dev_alloc(s, &s->info, 1)) return -2;
    void *stage = nullptr;
    NBMI_HIP_CHECK(hipMalloc(&stage, (size_t)(c ? c : 1) * 7 * sizeof(double)));
    s->allocs.push_back(stage);
    s->stage = stage;
    NBMI_HIP_CHECK(hipMemsetAsync(s->info, 0, sizeof(TreeInfo), s->stream));
    NBMI_HIP_CHECK(hipMemsetAsync(s->colors, 0, (size_t)(c ? c : 1) * 3 * sizeof(float), s->stream));
    if (s->method == NBMI_METHOD_BARNES_HUT) {
        // reference: max_nodes = min(8M, 4N) (simulation.py:477), + slack for tiny N; owner mode: + received trees
        s->node_capacity = node_rows_for(c) + s->node_extra;
        const int64_t own_rows = node_rows_for(c);
        if (dev_alloc(s, &s->key_hi, c) || dev_alloc(s, &s->key_lo, c) || dev_alloc(s, &s->hi_s, c) ||
            dev_alloc(s, &s->lo_s, c) ||
            (s->sort_packed && !s->owner && (dev_alloc(s, &s->packed, c) || dev_alloc(s, &s->packed_s, c))) || (s->owner && dev_alloc(s, &s->p64_s, c)) || dev_alloc(s, &s->idx, c) ||
            dev_alloc(s, &s->perm, c) || dev_alloc(s, &s->delta, c) || dev_alloc(s, &s->Pex, c + 1) ||
            dev_alloc(s, &s->S, c + 1) || dev_alloc(s, &s->sub_tot, (c + 1) / kScanTile + 2) ||
            dev_alloc(s, &s->sub_cnt, (c + 1) / kScanTile + 2) || dev_alloc(s, &s->subPex, (c + 1) / kScanTile + 2) ||
            dev_alloc(s, &s->T, (c + 1) / kScanTile + 2) ||
            dev_alloc(s, &s->nodes, s->node_capacity + 2) || dev_alloc(s, &s->nodes64, s->node_capacity + 2) ||
            dev_alloc(s, &s->node_level, own_rows) || dev_alloc(s, &s->node_ref, own_rows) ||
            dev_alloc(s, &s->xcd_bounds, 16) || dev_alloc(s, &s->wave_cycles, (size_t)4 * ((c + 63) / 64 + 8)) ||
            dev_alloc(s, &s->wave_flag, (size_t)(c + 63) / 64 + 64) || dev_alloc(s, &s->sub_flag, (c + 1) / kScanTile + 2) ||
            (s->force_prec != 1 && s->node_capacity + 2 <= kMaxNodeDRows &&
             dev_alloc(s, &s->nodesd, s->node_capacity + 2)) ||
            false)
            return -2;
        // no step yet: no wave has asked for float64 (the flags are written only by the build of a step with a dt, and
        // read before that by nbmi_force_precision_share and by the walk of an owner handle whose dt was never set)
        NBMI_HIP_CHECK(hipMemsetAsync(s->wave_flag, 0, (size_t)(c + 63) / 64 + 64, s->stream));
        NBMI_HIP_CHECK(hipMemsetAsync(s->sub_flag, 0, ((size_t)(c + 1) / kScanTile + 2) * sizeof(int32_t), s->stream));
        s->own_node_rows = own_rows;
        s->tmp_sort_bytes = nbmi::radix_temp_bytes_u64((size_t)c, 63);
        char *t = nullptr;
        if (dev_alloc(s, &t, s->tmp_sort_bytes + 256)) return -2;
        s->tmp_sort = t;
        NBMI_HIP_CHECK(nbmi::radix_init_temp(t, s->stream));
        if (dev_alloc(s, &s->wtab, 3) || upload_walk_table(s)) return -2;
    }
    // upload AoS host arrays through the staging buffer and split to SoA
    double *dpos = (double *)s->stage, *dvel = dpos + 3 * n, *dm = dvel + 3 * n;
    if (n > 0 && pos) {  // pos == NULL: the caller fills buf[0] on the device (nbmi_create_generated)
        NBMI_HIP_CHECK(hipMemcpyAsync(dpos, pos, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, s->stream));
        NBMI_HIP_CHECK(hipMemcpyAsync(dvel, vel, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, s->stream));
        NBMI_HIP_CHECK(hipMemcpyAsync(dm, mass, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s->stream));
        k_split_state<<<nblocks(n), kBlock, 0, s->stream>>>(dpos, dvel, dm, s->buf[0], n);
        NBMI_HIP_CHECK(hipGetLastError());
    }
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    s->shard_begin = 0;
    s->shard_end = n;
    s->nt = n;
    s->t_hi = s->hi_s;
    s->t_lo = s->lo_s;
    s->t_posm = s->posm_s;
    return 0;
}

nbmi_sim *nbmi_create(int64_t n, const double *pos, const double *vel, const double *mass, double G,
                      double softening, double damping, double theta, int method, int device) {
    nbmi::clear_error();
    if (n < 0 || n > kMaxBodies || (n > 0 && (!pos || !vel || !mass))) {
        nbmi::set_error("nbmi_create: bad arguments (n=%lld)", (long long)n);
        return nullptr;
    }
    if (method != NBMI_METHOD_BARNES_HUT && method != NBMI_METHOD_DIRECT) {
        nbmi::set_error("nbmi_create: unknown method %d", method);
        return nullptr;
    }
    if (!(softening >= 0.0) || !(theta >= 0.0)) {
        nbmi::set_error("nbmi_create: softening and theta must be >= 0");
        return nullptr;
    }
    int count = nbmi_device_count();
    if (count <= 0) {
        nbmi::set_error("nbmi_create: no HIP device available");
        return nullptr;
    }
    if (device < 0 || device >= count) {
        nbmi::set_error("nbmi_create: device %d out of range (have %d)", device, count);
        return nullptr;
    }
    nbmi_sim *s = new nbmi_sim();
    s->n = n; s->method = method; s->device = device;
    s->G = G; s->softening = softening; s->damping = damping; s->theta = theta;
    s->max_gm = largest_gm(G, mass, n);
    read_env_knobs(s);
    if (create_impl(s, pos, vel, mass) != 0) return create_failed(s);
    if (s->multipole_env == NBMI_MULTIPOLE_QUADRUPOLE && !multipole_refusal(s)) (void)nbmi_set_multipole(s, s->multipole_env);
    if (method == NBMI_METHOD_DIRECT && n > 0 && mass[0] > 0.0) {
        bool same = true;
        for (int64_t i = 1; i < n && same; i++) same = mass[i] == mass[0];
        if (same) s->uniform_gm = G * mass[0];
    }
    return s;
}

nbmi_sim *nbmi_create_generated(int distribution, int64_t n, double spawn_radius, uint64_t seed, double G,
                                double softening, double damping, double theta, int method, int device) {
    nbmi::clear_error();
    if (n < 0 || n > kMaxBodies || distribution < NBMI_IC_GALAXY || distribution > NBMI_IC_FILAMENT ||
        (method != NBMI_METHOD_BARNES_HUT && method != NBMI_METHOD_DIRECT) || !(softening >= 0.0) || !(theta >= 0.0) ||
        !(spawn_radius > 0.0)) {
        nbmi::set_error("nbmi_create_generated: bad arguments (n=%lld, distribution=%d)", (long long)n, distribution);
        return nullptr;
    }
    const int count = nbmi_device_count();
    if (count <= 0 || device < 0 || device >= count) {
        nbmi::set_error("nbmi_create_generated: no HIP device %d (have %d)", device, count);
        return nullptr;
    }
    nbmi_sim *s = new nbmi_sim();
    s->n = n; s->method = method; s->device = device;
    s->G = G; s->softening = softening; s->damping = damping; s->theta = theta;
    s->max_gm = fabs(G);  // the generators' masses are 1 (filament: 0.1)
    read_env_knobs(s);
    int rc = create_impl(s, nullptr, nullptr, nullptr);
    if (rc == 0) {
        Bodies &b = s->buf[0];
        rc = nbmi::ic_generate(distribution, n, spawn_radius, G, seed, nbmi::IcArrays{b.x, b.y, b.z, b.vx, b.vy, b.vz, b.m, b.id},
                               s->stream);
    }
    if (rc != 0) return create_failed(s);
    if (s->multipole_env == NBMI_MULTIPOLE_QUADRUPOLE && !multipole_refusal(s)) (void)nbmi_set_multipole(s, s->multipole_env);
    return s;
}

void nbmi_philox4x32_10(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
    nbmi::philox4x32_10(counter, key, out);
}

int nbmi_get_masses_f64(nbmi_sim *s, double *out) {
    if (int rc = check_handle(s)) return rc;
    const int64_t n = s->n;
    if (n == 0) return 0;
    if (int rc = require_out(out)) return rc;
    const double *m = s->buf[s->curbuf].m;  // (owner mode: the rows are the caller's order)
    if (!s->owner) {
        k_unperm1_f64<<<nblocks(n), kBlock, 0, s->stream>>>(m, s->buf[s->curbuf].id, n, (double *)s->stage);
        NBMI_HIP_CHECK(hipGetLastError());
        m = (const double *)s->stage;
    }
    NBMI_HIP_CHECK(hipMemcpyAsync(out, m, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    return 0;
}

int nbmi_step(nbmi_sim *s, double dt, int substeps) {
    if (int rc = check_handle(s)) return rc;
    if (substeps < 0) {
        nbmi::set_error("nbmi_step: substeps < 0");
        return NBMI_ERR_ARG;
    }
    if (s->n == 0) {  // nothing to step but tracers, and those on straight lines (a = 0)
        const bool leap0 = s->integrator == NBMI_INTEGRATOR_LEAPFROG;
        if (s->tr.m == 0 || substeps == 0) return 0;
        if (leap0) {
            if (int rc = tracer_leap_prepare(s)) return rc;
        }
        for (int k = 0; k < substeps; k++) {
            if (leap0) {
                if (int rc = enqueue_tracer_kick_drift(s, dt)) return rc;
            }
            if (int rc = enqueue_tracers(s, leap0 ? kLeapClose : 0, dt)) return rc;
        }
        return 0;
    }
    if (s->owner) {
        nbmi::set_error("nbmi_step: this handle is in owner mode, use the nbmi_owner_* calls");
        return NBMI_ERR_ARG;
    }
    if (substeps > 1 && (s->shard_begin != 0 || s->shard_end != s->n)) {
        nbmi::set_error("nbmi_step: a sharded handle needs nbmi_import_ranks between steps (substeps must be 1)");
        return NBMI_ERR_ARG;
    }
    const bool leap = s->integrator == NBMI_INTEGRATOR_LEAPFROG;
    if (leap && substeps > 0) {
        if (int rc = leap_prepare(s, dt)) return rc;
    }
    for (int k = 0; k < substeps; k++) {
        if (s->method == NBMI_METHOD_BARNES_HUT) {
            if (leap) {
                // kick-drift into the other buffer, build + walk there, the closing kick writes back: one step leaves the
                // current buffer where it was
                if (s->timers) NBMI_HIP_CHECK(hipEventRecord(s->ev[0], s->stream));
                if (int rc = enqueue_kick_drift(s, dt)) return rc;
                s->maxabs_fused = true;  // k_kick_drift has published max |x'|
                int rc = enqueue_tree(s, step_build(s, dt, BuildTiming::kCaller));
                if (rc == 0 && s->tr.m) {  // the tracers' whole substep on the tree of the drifted bodies
                    rc = enqueue_tracer_kick_drift(s, dt);
                    if (rc == 0) rc = enqueue_tracers(s, kLeapClose, dt);
                }
                if (rc == 0) rc = enqueue_walk(s, true, dt, nullptr, kLeapClose);
                s->curbuf ^= 1;
                if (rc) {
                    s->maxabs_fused = false;
                    return rc;
                }
            } else {
                if (int rc = enqueue_tree(s, step_build(s, dt, BuildTiming::kAll))) return rc;
                if (s->tr.m) {
                    if (int rc = enqueue_tracers(s, 0, dt)) return rc;
                }
                if (int rc = enqueue_walk(s, true, dt, nullptr)) return rc;
            }
            if (s->timers) {
                NBMI_HIP_CHECK(hipEventRecord(s->ev[4], s->stream));
                NBMI_HIP_CHECK(hipEventSynchronize(s->ev[4]));
                for (int p = 0; p < 4; p++) {
                    float ms = 0.f;
                    NBMI_HIP_CHECK(hipEventElapsedTime(&ms, s->ev[p], s->ev[p + 1]));
                    s->ms[p] += ms;
                }
                s->timed_steps++;
            }
            // a full (unsharded) step leaves every rank of the other buffer written
            // (sharded handles: the ranks outside [shard_begin, shard_end) arrive via nbmi_import_ranks)
            if (!leap) s->curbuf ^= 1;
            s->steps_taken++;
            s->tree_valid = false;
            // (leapfrog: the walk publishes nothing, the next k_kick_drift does)
            s->maxabs_fused = !leap && s->fuse_maxabs && s->shard_begin == 0 && s->shard_end == s->n;
        } else {
            if (s->timers) NBMI_HIP_CHECK(hipEventRecord(s->ev[0], s->stream));
            if (leap) {
                if (int rc = enqueue_kick_drift(s, dt)) return rc;
                int rc = 0;
                if (s->tr.m) {  // (the current buffer holds the drifted bodies)
                    rc = enqueue_tracer_kick_drift(s, dt);
                    if (rc == 0) rc = enqueue_tracers(s, kLeapClose, dt);
                }
                if (rc == 0) rc = launch_direct<true>(s, dt, s->acc, kLeapClose);
                s->curbuf ^= 1;
                if (rc) return rc;
            } else {
                if (s->tr.m) {
                    if (int rc = enqueue_tracers(s, 0, dt)) return rc;
                }
                if (int rc = launch_direct<true>(s, dt, nullptr)) return rc;
            }
            if (s->timers) {
                NBMI_HIP_CHECK(hipEventRecord(s->ev[1], s->stream));
                NBMI_HIP_CHECK(hipEventSynchronize(s->ev[1]));
                float ms = 0.f;
                NBMI_HIP_CHECK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
                s->ms[3] += ms;
                s->timed_steps++;
            }
            if (!leap) s->curbuf ^= 1;
            s->steps_taken++;
        }
    }
    return 0;
}

int64_t nbmi_step_count(nbmi_sim *s) { return s ? s->steps_taken : -1; }

namespace {
int knn_check(nbmi_sim *s, int k, const char *what);
int knn_enqueue(nbmi_sim *s, int k, bool count);
}  // namespace

int nbmi_compute_colors(nbmi_sim *s, double max_speed) {
    if (int rc = check_handle(s)) return rc;
    if (s->n == 0) return 0;
    if (s->color_mode == NBMI_COLOR_DENSITY) {  // (only handles the query accepts get into this mode; nothing waits)
        if (int rc = knn_check(s, s->color_k, "nbmi_compute_colors")) return rc;
        if (int rc = knn_enqueue(s, s->color_k, false)) return rc;
        k_colors_density<<<nblocks(s->n), kBlock, 0, s->stream>>>(s->buf[s->curbuf], s->n, s->q.knn.r2, s->q.knn.mass, s->color_lo,
                                                                  s->color_hi, s->colors);
        NBMI_HIP_CHECK(hipGetLastError());
        return 0;
    }
    k_colors<<<nblocks(s->n), kBlock, 0, s->stream>>>(s->buf[s->curbuf], s->n, max_speed, s->owner, s->colors);
    NBMI_HIP_CHECK(hipGetLastError());
    return 0;
}

int nbmi_sync(nbmi_sim *s) {
    if (int rc = check_handle(s)) return rc;
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    return check_device_error(s);
}

// positions or velocities (N,3) in the caller's order
static int get3(nbmi_sim *s, bool vel, void *out, bool f32) {
    if (int rc = check_handle(s)) return rc;
    const int64_t n = s->n;
    if (n == 0) return 0;
    if (int rc = require_out(out)) return rc;
    Bodies cur = s->buf[s->curbuf];
    const double *a = vel ? cur.vx : cur.x, *b = vel ? cur.vy : cur.y, *c = vel ? cur.vz : cur.z;
    const int32_t *id = s->owner ? nullptr : cur.id;
    if (f32) k_unperm3_f32<<<nblocks(n), kBlock, 0, s->stream>>>(a, b, c, id, n, (float *)s->stage);
    else k_unperm3_f64<<<nblocks(n), kBlock, 0, s->stream>>>(a, b, c, id, n, (double *)s->stage);
    NBMI_HIP_CHECK(hipGetLastError());
    NBMI_HIP_CHECK(hipMemcpyAsync(out, s->stage, (size_t)n * 3 * (f32 ? sizeof(float) : sizeof(double)),
                                  hipMemcpyDeviceToHost, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    return check_device_error(s);
}
int nbmi_get_positions_f32(nbmi_sim *s, float *out) { return get3(s, false, out, true); }
int nbmi_get_positions_f64(nbmi_sim *s, double *out) { return get3(s, false, out, false); }
int nbmi_get_velocities_f64(nbmi_sim *s, double *out) { return get3(s, true, out, false); }
int nbmi_get_colors_f32(nbmi_sim *s, float *out) {
    if (int rc = check_handle(s)) return rc;
    if (s->n == 0) return 0;
    if (int rc = require_out(out)) return rc;
    NBMI_HIP_CHECK(hipMemcpyAsync(out, s->colors, (size_t)s->n * 3 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    return 0;
}

int nbmi_set_state(nbmi_sim *s, const double *pos, const double *vel) {
    if (int rc = check_handle(s)) return rc;
    const int64_t n = s->n;
    if (n == 0) return 0;
    if (!pos || !vel) { nbmi::set_error("null input"); return NBMI_ERR_ARG; }
    double *dpos = (double *)s->stage, *dvel = dpos + 3 * n;
    NBMI_HIP_CHECK(hipMemcpyAsync(dpos, pos, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, s->stream));
    NBMI_HIP_CHECK(hipMemcpyAsync(dvel, vel, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, s->stream));
    k_set_state_perm<<<nblocks(n), kBlock, 0, s->stream>>>(dpos, dvel, s->buf[s->curbuf], n);
    NBMI_HIP_CHECK(hipGetLastError());
    NBMI_HIP_CHECK(hipMemsetAsync(&s->info->sticky_error, 0, sizeof(int), s->stream));  // a fresh state: drop a pending capacity error
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    k_set_all64<<<1, 1, 0, s->stream>>>(s->info, 0);  // a new state: the "most of the system asks" history is the old system's
    NBMI_HIP_CHECK(hipGetLastError());
    state_changed(s);
    return 0;
}

int nbmi_set_integrator(nbmi_sim *s, int integrator) {
    if (int rc = check_handle(s)) return rc;
    if (integrator != NBMI_INTEGRATOR_KICK_DRIFT && integrator != NBMI_INTEGRATOR_LEAPFROG) {
        nbmi::set_error("nbmi_set_integrator: unknown integrator %d", integrator);
        return NBMI_ERR_ARG;
    }
    if (integrator == NBMI_INTEGRATOR_LEAPFROG) {
        if (s->owner) {
            nbmi::set_error("nbmi_set_integrator: owner-mode handles are not supported (leapfrog needs acceleration columns "
                            "that the exchange rows do not carry)");
            return NBMI_ERR_ARG;
        }
        if (s->shard_begin != 0 || s->shard_end != s->n) {
            nbmi::set_error("nbmi_set_integrator: sharded handles are not supported (leapfrog needs acceleration columns "
                            "that the exchange rows do not carry)");
            return NBMI_ERR_ARG;
        }
        if (s->integrator != NBMI_INTEGRATOR_LEAPFROG) s->acc_valid = s->tr.acc_valid = false;  // the next step primes a = F(x)
    }
    s->integrator = integrator;
    return 0;
}

int nbmi_get_integrator(nbmi_sim *s, int *out) {
    if (int rc = check_handle(s)) return rc;
    if (int rc = require_out(out)) return rc;
    *out = s->integrator;
    return 0;
}

int nbmi_set_multipole(nbmi_sim *s, int multipole) {
    if (int rc = check_handle(s)) return rc;
    if (multipole != NBMI_MULTIPOLE_MONOPOLE && multipole != NBMI_MULTIPOLE_QUADRUPOLE) {
        nbmi::set_error("nbmi_set_multipole: unknown multipole order %d", multipole);
        return NBMI_ERR_ARG;
    }
    if (multipole == NBMI_MULTIPOLE_QUADRUPOLE) {
        if (const char *why = multipole_refusal(s)) {
            nbmi::set_error("nbmi_set_multipole: %s", why);
            return NBMI_ERR_ARG;
        }
        if (!s->nodesq && (dev_alloc(s, &s->nodesq, s->node_capacity + 2) ||
                           dev_alloc(s, &s->quad_work, (size_t)kQuadDoubles * (s->node_capacity + 2)) ||
                           dev_alloc(s, &s->quad_pot, s->node_capacity + 2)))
            return NBMI_ERR_HIP;
    }
    if (multipole != s->multipole) {  // (the positions are the same: maxabs_fused survives)
        s->tree_valid = false;  // the records the queries describe belong to the other mode's build
        s->acc_valid = s->tr.acc_valid = false;  // leapfrog: the stored a = F(x) is the other mode's force
    }
    s->multipole = multipole;
    return 0;
}

int nbmi_get_multipole(nbmi_sim *s, int *out) {
    if (int rc = check_handle(s)) return rc;
    if (int rc = require_out(out)) return rc;
    *out = s->multipole;
    return 0;
}

int nbmi_build_tree(nbmi_sim *s) {
    if (int rc = check_handle(s)) return rc;
    if (s->method != NBMI_METHOD_BARNES_HUT) { nbmi::set_error("not a Barnes-Hut handle"); return NBMI_ERR_ARG; }
    if (s->n == 0) return 0;
    if (int rc = enqueue_tree(s)) return rc;
    return check_device_error(s);
}

int nbmi_get_accelerations_f64(nbmi_sim *s, double *out) {
    if (int rc = check_handle(s)) return rc;
    const int64_t n = s->n;
    if (n == 0) return 0;
    if (int rc = require_out(out)) return rc;
    double *acc = (double *)s->stage;
    if (s->method == NBMI_METHOD_BARNES_HUT) {
        if (int rc = enqueue_tree(s)) return rc;
        NBMI_HIP_CHECK(hipMemsetAsync(&s->info->wave_visits, 0, 17 * sizeof(unsigned long long), s->stream));
        if (int rc = enqueue_walk(s, false, 0.0, acc)) return rc;
    } else {
        if (int rc = launch_direct<false>(s, 0.0, acc)) return rc;
    }
    NBMI_HIP_CHECK(hipMemcpyAsync(out, acc, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    return check_device_error(s);
}

namespace {
// phi and the applied-term counts per state row (diag_phi / diag_cnt).  Barnes-Hut: the octree of the current positions
// as nbmi_get_accelerations_f64 builds it, with the float64 node rows, then the potential walk, all inside a SideBuild.
int diag_potential(nbmi_sim *s) {
    const int64_t n = s->n;
    if (!s->diag_phi && (dev_alloc(s, &s->diag_phi, n) || dev_alloc(s, &s->diag_cnt, n))) return NBMI_ERR_HIP;
    hipStream_t st = s->stream;
    if (s->method != NBMI_METHOD_BARNES_HUT) {
        k_potential_direct<<<nblocks(n), kBlock, 0, st>>>(s->buf[s->curbuf], n, s->G, s->softening * s->softening, s->diag_phi,
                                                           s->diag_cnt);
        NBMI_HIP_CHECK(hipGetLastError());
        return 0;
    }
    return side_tree(s, true, false, true, false, [&] {
        with_bool(s->multipole == NBMI_MULTIPOLE_QUADRUPOLE, [&](auto q) {
            k_potential_tree<decltype(q)::value><<<nblocks(n), kBlock, 0, st>>>(
                s->nodes, s->diag_pot, s->wtab, s->info, s->posm_s, s->perm, s->curbuf, (float)(s->softening * s->softening), n,
                s->diag_phi, s->diag_cnt, decltype(q)::value ? s->quad_work : nullptr);
        });
        return launch_failed("k_potential_tree launch failed");
    });
}

int diag_refuse(nbmi_sim *s, const char *what) {
    if (s->owner) {
        nbmi::set_error("%s: owner-mode handles are not supported (the potential needs the other ranks' trees)", what);
        return NBMI_ERR_ARG;
    }
    if (s->shard_begin != 0 || s->shard_end != s->n) {
        nbmi::set_error("%s: sharded handles are not supported", what);
        return NBMI_ERR_ARG;
    }
    return 0;
}
}  // namespace

int nbmi_diagnostics(nbmi_sim *s, int with_potential, double *out12, int64_t *terms) {
    if (int rc = check_handle(s)) return rc;
    if (int rc = diag_refuse(s, "nbmi_diagnostics")) return rc;
    if (int rc = require_out(out12)) return rc;
    const int64_t n = s->n;
    if (n == 0) {
        for (int k = 0; k < 12; k++) out12[k] = 0.0;
        if (!with_potential) out12[11] = NAN;
        if (terms) *terms = 0;
        return 0;
    }
    if (with_potential) {
        if (int rc = diag_potential(s)) return rc;
    }
    if (!s->diag_part && (dev_alloc(s, &s->diag_part, (size_t)(kDiagBlocksMax + 1) * kDiagSums) ||
                          dev_alloc(s, &s->diag_partc, kDiagBlocksMax + 1)))
        return NBMI_ERR_HIP;
    hipStream_t st = s->stream;
    const int64_t want = (n + 4 * kBlock - 1) / (4 * kBlock);  // at least 1 024 rows per block
    const int nb = (int)(want < kDiagBlocksMax ? want : kDiagBlocksMax);
    const int64_t per_block = (n + nb - 1) / nb;
    double *tot = s->diag_part + (size_t)kDiagBlocksMax * kDiagSums;
    long long *totc = s->diag_partc + kDiagBlocksMax;
    k_diag_partial<<<nb, kBlock, 0, st>>>(s->buf[s->curbuf], with_potential ? s->diag_phi : nullptr, s->diag_cnt, n, per_block,
                                          s->diag_part, s->diag_partc);
    k_diag_final<<<1, kBlock, 0, st>>>(s->diag_part, s->diag_partc, nb, tot, totc);
    NBMI_HIP_CHECK(hipGetLastError());
    double h[kDiagSums];
    long long hc = 0;
    NBMI_HIP_CHECK(hipMemcpyAsync(h, tot, sizeof(h), hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipMemcpyAsync(&hc, totc, sizeof(hc), hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    const double M = h[0];
    out12[0] = M;
    for (int k = 0; k < 3; k++) out12[1 + k] = M != 0.0 ? h[1 + k] / M : 0.0;
    for (int k = 0; k < 6; k++) out12[4 + k] = h[4 + k];
    out12[10] = 0.5 * h[10];
    out12[11] = with_potential ? 0.5 * h[11] : NAN;
    if (terms) *terms = with_potential ? (int64_t)hc : 0;
    return 0;
}

int nbmi_get_potentials_f64(nbmi_sim *s, double *out) {
    if (int rc = check_handle(s)) return rc;
    if (int rc = diag_refuse(s, "nbmi_get_potentials_f64")) return rc;
    const int64_t n = s->n;
    if (n == 0) return 0;
    if (int rc = require_out(out)) return rc;
    if (int rc = diag_potential(s)) return rc;
    k_unperm1_f64<<<nblocks(n), kBlock, 0, s->stream>>>(s->diag_phi, s->buf[s->curbuf].id, n, (double *)s->stage);
    NBMI_HIP_CHECK(hipGetLastError());
    NBMI_HIP_CHECK(hipMemcpyAsync(out, s->stage, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    return 0;
}

namespace {
int knn_check(nbmi_sim *s, int k, const char *what) {
    if (int rc = query_refuse(s, what)) return rc;
    if (k < 1 || k > kKnnMaxK || (int64_t)k > s->n - 1) {
        nbmi::set_error("%s: k = %d is outside 1 .. min(%d, N - 1) (N = %lld)", what, k, kKnnMaxK, (long long)s->n);
        return NBMI_ERR_ARG;
    }
    return 0;
}
// The k-NN query: r2_k and mass_k are in q.knn.r2 / q.knn.mass by state row afterwards.  `count`: also sum the evaluated
// distances into q.shared.evals.
int knn_enqueue(nbmi_sim *s, int k, bool count) {
    const int64_t n = s->n;
    auto &g = s->q.knn;
    if (query_buffers(s) || query_alloc(g, [&] { return dev_alloc(s, &g.r2, n) || dev_alloc(s, &g.mass, n); })) return NBMI_ERR_HIP;
    hipStream_t st = s->stream;
    if (count) NBMI_HIP_CHECK(hipMemsetAsync(s->q.shared.evals, 0, sizeof(unsigned long long), st));
    return query_enqueue(s, "k_knn", [&] {
        k_knn<<<(int)((n + kQueryBlock - 1) / kQueryBlock), kQueryBlock, (size_t)k * kQueryBlock * sizeof(double), st>>>(
            s->nodes, s->q.shared.rows, s->node_ref, s->info, s->perm, s->buf[s->curbuf], n, k, g.r2, g.mass,
            count ? s->q.shared.evals : nullptr);
    });
}
}  // namespace

int nbmi_knn(nbmi_sim *s, int k, double *r2_k, double *mass_k, int64_t *evals) {
    if (int rc = check_handle(s)) return rc;
    if (int rc = knn_check(s, k, "nbmi_knn")) return rc;
    if (int rc = query_sync(s, [&] { return knn_enqueue(s, k, evals != nullptr); })) return rc;
    const int64_t n = s->n;
    double *o_r2 = (double *)s->stage, *o_mass = o_r2 + n;
    k_knn_out<<<nblocks(n), kBlock, 0, s->stream>>>(s->q.knn.r2, s->q.knn.mass, s->buf[s->curbuf].id, n, r2_k ? o_r2 : nullptr,
                                                    mass_k ? o_mass : nullptr, nullptr);
    NBMI_HIP_CHECK(hipGetLastError());
    if (r2_k) NBMI_HIP_CHECK(hipMemcpyAsync(r2_k, o_r2, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    if (mass_k) NBMI_HIP_CHECK(hipMemcpyAsync(mass_k, o_mass, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    unsigned long long ev = 0;
    if (evals) NBMI_HIP_CHECK(hipMemcpyAsync(&ev, s->q.shared.evals, sizeof(ev), hipMemcpyDeviceToHost, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    if (evals) *evals = (int64_t)ev;
    return 0;
}

int nbmi_get_densities_f64(nbmi_sim *s, int k, double *rho) {
    if (int rc = check_handle(s)) return rc;
    if (int rc = knn_check(s, k, "nbmi_get_densities_f64")) return rc;
    if (int rc = require_out(rho)) return rc;
    if (int rc = query_sync(s, [&] { return knn_enqueue(s, k, false); })) return rc;
    const int64_t n = s->n;
    k_knn_out<<<nblocks(n), kBlock, 0, s->stream>>>(s->q.knn.r2, s->q.knn.mass, s->buf[s->curbuf].id, n, nullptr, nullptr,
                                                    (double *)s->stage);
    NBMI_HIP_CHECK(hipGetLastError());
    NBMI_HIP_CHECK(hipMemcpyAsync(rho, s->stage, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    return 0;
}

namespace {
// nbmi_fof and everything built on it: the handles the k-NN query accepts, a positive finite linking length
int fof_check(nbmi_sim *s, double link, int64_t min_members, int64_t capacity, const char *what) {
    if (int rc = query_refuse(s, what)) return rc;
    if (!isfinite(link) || !(link > 0.0)) {
        nbmi::set_error("%s: the linking length %g is not finite and > 0", what, link);
        return NBMI_ERR_ARG;
    }
    if (min_members < 1) {
        nbmi::set_error("%s: min_members = %lld is < 1", what, (long long)min_members);
        return NBMI_ERR_ARG;
    }
    if (capacity < 0) {
        nbmi::set_error("%s: capacity = %lld is < 0", what, (long long)capacity);
        return NBMI_ERR_ARG;
    }
    return 0;
}
// the union-find's arrays by key rank (nbmi_mst borrows parent and root)
int fof_buffers(nbmi_sim *s) {
    const int64_t n = s->n;
    auto &g = s->q.fof;
    return query_alloc(g, [&] {
        return dev_alloc(s, &g.parent, n) || dev_alloc(s, &g.root, n) || dev_alloc(s, &g.minid, n) || dev_alloc(s, &g.cnt, n) ||
               dev_alloc(s, &g.counters, 2);
    });
}
// Enqueues build, pair search and flattening and never waits.  Afterwards, by key rank: q.fof.root, minid[root] (the
// label), cnt[root]; counters = {distances evaluated (if `count`), roots}; `labels` (device, may be null) in the caller's
// order.
int fof_enqueue(nbmi_sim *s, double b2, bool count, int32_t *labels) {
    const int64_t n = s->n;
    auto &g = s->q.fof;
    if (query_buffers(s) || fof_buffers(s)) return NBMI_ERR_HIP;
    hipStream_t st = s->stream;
    NBMI_HIP_CHECK(hipMemsetAsync(g.counters, 0, 2 * sizeof(unsigned long long), st));
    return query_enqueue(s, "k_fof_link", [&] {
        const Bodies cur = s->buf[s->curbuf];
        k_fof_init<<<nblocks(n), kBlock, 0, st>>>(n, g.parent, g.minid, g.cnt);
        k_fof_link<<<(int)((n + kQueryBlock - 1) / kQueryBlock), kQueryBlock, 0, st>>>(
            s->nodes, s->q.shared.rows, s->node_ref, s->info, s->perm, cur, n, b2, s->q.shared.wleaf, g.parent,
            count ? g.counters : nullptr);
        k_fof_flatten<<<nblocks(n), kBlock, 0, st>>>(s->info, n, g.parent, s->perm, cur.id, g.root, g.minid, g.cnt);
        k_fof_labels<<<nblocks(n), kBlock, 0, st>>>(s->info, n, g.root, g.minid, s->perm, cur.id, labels, g.counters + 1);
    });
}
int fof_catalogue_buffers(nbmi_sim *s) {
    auto &g = s->q.cat;
    const int64_t n = s->n, chunks = (n + kFofChunk - 1) / kFofChunk;
    return query_alloc(g, [&]() -> int {
        g.sort_bytes = nbmi::radix_temp_bytes_u32((size_t)n, 32);
        if (dev_alloc(s, &g.key_s, n) || dev_alloc(s, &g.rank, n) || dev_alloc(s, &g.rank_s, n) || dev_alloc(s, &g.hpos, n) ||
            dev_alloc(s, &g.slot, n) || dev_alloc(s, &g.qhead, n) || dev_alloc(s, &g.tiles, scan::tiles_for(n) + 1) ||
            dev_alloc(s, &g.last, chunks * kFofVals) || dev_alloc(s, &g.first, chunks * kFofVals) ||
            dev_alloc(s, &g.sort_tmp, g.sort_bytes + 256))
            return NBMI_ERR_HIP;
        NBMI_HIP_CHECK(nbmi::radix_init_temp(g.sort_tmp, s->stream));
        return 0;
    });
}
// The catalogue's row arrays for at least `rows` rows, in powers of two.  Arrays that are too small are freed: the
// caller has just waited for the stream, and nothing enqueued reads them.
int fof_row_buffers(nbmi_sim *s, int64_t rows) {
    auto &g = s->q.cat;
    if (rows <= g.row_cap) return 0;
    g.row_cap = 0;
    dev_free(s, &g.row_vals);
    dev_free(s, &g.out13);
    dev_free(s, &g.label);
    dev_free(s, &g.members);
    int64_t cap = 1024;
    while (cap < rows) cap *= 2;
    if (dev_alloc(s, &g.row_vals, cap * kFofVals) || dev_alloc(s, &g.out13, cap * 13) || dev_alloc(s, &g.label, cap) ||
        dev_alloc(s, &g.members, cap))
        return NBMI_ERR_HIP;
    g.row_cap = cap;
    return 0;
}
}  // namespace

int nbmi_fof(nbmi_sim *s, double link, int32_t *labels, int64_t *n_groups, int64_t *evals) {
    if (int rc = check_handle(s)) return rc;
    if (int rc = fof_check(s, link, 1, 0, "nbmi_fof")) return rc;
    if (n_groups) *n_groups = 0;
    if (evals) *evals = 0;
    const int64_t n = s->n;
    if (n == 0) return 0;
    int32_t *dev_labels = labels ? (int32_t *)s->stage : nullptr;
    if (int rc = query_sync(s, [&] { return fof_enqueue(s, link * link, evals != nullptr, dev_labels); })) return rc;
    unsigned long long c[2] = {0, 0};
    if (labels) NBMI_HIP_CHECK(hipMemcpyAsync(labels, s->stage, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    NBMI_HIP_CHECK(hipMemcpyAsync(c, s->q.fof.counters, sizeof(c), hipMemcpyDeviceToHost, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    if (evals) *evals = (int64_t)c[0];
    if (n_groups) *n_groups = (int64_t)c[1];
    return 0;
}

int nbmi_fof_catalogue(nbmi_sim *s, double link, int64_t min_members, int64_t capacity, int32_t *label, int64_t *members,
                       double *out13, int64_t *count) {
    if (int rc = check_handle(s)) return rc;
    if (int rc = fof_check(s, link, min_members, capacity, "nbmi_fof_catalogue")) return rc;
    if (int rc = require_out(count, "nbmi_fof_catalogue: null count")) return rc;
    if (capacity > 0 && (!label || !members || !out13)) {
        nbmi::set_error("nbmi_fof_catalogue: null output with capacity > 0");
        return NBMI_ERR_ARG;
    }
    *count = 0;
    const int64_t n = s->n;
    if (n == 0) return 0;
    if (int rc = query_sync(s, [&] { return fof_enqueue(s, link * link, false, nullptr); })) return rc;
    if (int rc = fof_catalogue_buffers(s)) return rc;
    hipStream_t st = s->stream;
    // the ranks by root, stable; the heads of the segments; the rows of the qualifying groups in segment order
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < n) bits++;
    k_fof_iota<<<nblocks(n), kBlock, 0, st>>>(n, s->q.cat.rank);
    NBMI_HIP_CHECK(nbmi::radix_sort_pairs_u32(s->q.cat.sort_tmp, s->q.cat.sort_bytes, (const uint32_t *)s->q.fof.root, s->q.cat.key_s,
                                              s->q.cat.rank, s->q.cat.rank_s, (size_t)n, 0, bits, st));
    k_fof_heads<<<nblocks(n), kBlock, 0, st>>>(n, s->q.cat.key_s, s->q.cat.hpos, s->q.cat.slot);
    scan::enqueue_compact(FofQualifies{s->q.cat.key_s, s->q.fof.cnt, min_members}, n, s->q.cat.tiles,
                          FofEmitHead{s->q.cat.key_s, s->q.cat.qhead, s->q.cat.slot}, st);
    NBMI_HIP_CHECK(hipGetLastError());
    uint32_t rows = 0;
    unsigned sort_err = 0u;
    NBMI_HIP_CHECK(hipMemcpyAsync(&rows, s->q.cat.tiles + scan::tiles_for(n), sizeof(rows), hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(nbmi::radix_error_word(s->q.cat.sort_tmp, &sort_err, st));
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    if (sort_err) {
        NBMI_HIP_CHECK(nbmi::radix_init_temp(s->q.cat.sort_tmp, st));
        nbmi::set_error("nbmi_fof_catalogue: device radix sort: a look-back spin timed out");
        return NBMI_ERR_HIP;
    }
    *count = (int64_t)rows;
    if (rows == 0) return 0;
    if (int rc = fof_row_buffers(s, (int64_t)rows)) return rc;
    k_fof_chunks<<<(int)((n + kFofChunk - 1) / kFofChunk), kFofChunk, 0, st>>>(n, s->q.cat.key_s, s->q.cat.rank_s, s->perm,
                                                                               s->buf[s->curbuf], s->q.cat.hpos, s->q.fof.cnt,
                                                                               s->q.cat.slot, s->q.cat.row_vals, s->q.cat.last,
                                                                               s->q.cat.first);
    k_fof_rows<<<(int)rows, kQueryBlock, 0, st>>>(n, (int64_t)rows, s->q.cat.qhead, s->q.cat.key_s, s->q.fof.cnt, s->q.fof.minid,
                                                s->q.cat.row_vals, s->q.cat.last, s->q.cat.first, s->q.cat.out13, s->q.cat.label,
                                                s->q.cat.members);
    NBMI_HIP_CHECK(hipGetLastError());
    std::vector<double> h13((size_t)rows * 13);
    std::vector<int32_t> hlabel(rows);
    std::vector<int64_t> hmembers(rows);
    NBMI_HIP_CHECK(hipMemcpyAsync(h13.data(), s->q.cat.out13, h13.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipMemcpyAsync(hlabel.data(), s->q.cat.label, hlabel.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipMemcpyAsync(hmembers.data(), s->q.cat.members, hmembers.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    // the catalogue's order: members descending, ties by label ascending (labels are distinct)
    std::vector<uint32_t> order(rows);
    for (uint32_t i = 0; i < rows; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return hmembers[a] != hmembers[b] ? hmembers[a] > hmembers[b] : hlabel[a] < hlabel[b];
    });
    const int64_t out_rows = (int64_t)rows < capacity ? (int64_t)rows : capacity;
    for (int64_t i = 0; i < out_rows; i++) {
        const uint32_t r = order[i];
        label[i] = hlabel[r];
        members[i] = hmembers[r];
        for (int c = 0; c < 13; c++) out13[i * 13 + c] = h13[(size_t)r * 13 + c];
    }
    return 0;
}

int nbmi_compute_group_colors(nbmi_sim *s, double link, int64_t min_members) {
    if (int rc = check_handle(s)) return rc;
    if (int rc = fof_check(s, link, min_members, 0, "nbmi_compute_group_colors")) return rc;
    const int64_t n = s->n;
    if (n == 0) return 0;
    if (int rc = fof_enqueue(s, link * link, false, nullptr)) return rc;
    k_fof_colors<<<nblocks(n), kBlock, 0, s->stream>>>(s->info, n, s->q.fof.root, s->q.fof.minid, s->q.fof.cnt, s->perm,
                                                       s->buf[s->curbuf].id, min_members, s->colors);
    NBMI_HIP_CHECK(hipGetLastError());
    return 0;
}

namespace {
// The scratch of a pair call, with the sums cleared: q.pairs.cnt, the cells' body counts, and q.pairs.out = {distances
// evaluated, counted through whole cells, below, counts[0 .. nb)}, to which the kernels add.
int pairs_prepare(nbmi_sim *s) {
    auto &g = s->q.pairs;
    if (query_buffers(s) || query_alloc(g, [&] {
            return dev_alloc(s, &g.cnt, s->node_capacity + 2) || dev_alloc(s, &g.out, kPairMaxBins + 3);
        }))
        return NBMI_ERR_HIP;
    NBMI_HIP_CHECK(hipMemsetAsync(g.out, 0, (kPairMaxBins + 3) * sizeof(unsigned long long), s->stream));
    return 0;
}
// The caller's side of q.pairs.out: where nbmi_pair_counts and nbmi_pair_counts_at put the sums (any may be null).
struct PairSums {
    int nb;
    int64_t *counts, *below, *evals, *cell_pairs;
    void set(const unsigned long long *h) const {
        if (evals) *evals = (int64_t)h[0];
        if (cell_pairs) *cell_pairs = (int64_t)h[1];
        if (below) *below = (int64_t)h[2];
        for (int k = 0; counts && k < nb; k++) counts[k] = (int64_t)h[3 + k];
    }
    void zero() const {
        const unsigned long long h[kPairMaxBins + 3] = {};
        set(h);
    }
    int read(nbmi_sim *s) const {  // waits for the stream
        unsigned long long h[kPairMaxBins + 3];
        NBMI_HIP_CHECK(hipMemcpyAsync(h, s->q.pairs.out, (size_t)(nb + 3) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
        NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
        set(h);
        return 0;
    }
};
// Enqueues build, cell counts and the pair search and never waits.
int pairs_enqueue(nbmi_sim *s, int nb, const PairEdges &e2) {
    const int64_t n = s->n;
    auto &g = s->q.pairs;
    if (int rc = pairs_prepare(s)) return rc;
    hipStream_t st = s->stream;
    return query_enqueue(s, "k_pair_counts", [&] {
        k_pair_cells<<<nblocks(s->own_node_rows), kBlock, 0, st>>>(s->nodes, s->node_ref, s->info, n, s->own_node_rows, g.cnt);
        k_pair_counts<<<(int)((n + kQueryBlock - 1) / kQueryBlock), kQueryBlock, pair_lds_bytes(nb), st>>>(
            s->nodes, s->q.shared.rows, s->node_ref, g.cnt, s->info, s->perm, s->buf[s->curbuf], n, nb, e2,
            s->pair_cells ? 1 : 0, s->q.shared.wleaf, g.out);
    });
}
// The header's rules for nb and edges, for nbmi_pair_counts and nbmi_pair_counts_at (`who`); *e2 = the E[k].
int pair_edges_check(const char *who, int nb, const double *edges, PairEdges *e2) {
    if (nb < 1 || nb > kPairMaxBins) {
        nbmi::set_error("%s: nb = %d is outside 1 .. %d", who, nb, kPairMaxBins);
        return NBMI_ERR_ARG;
    }
    if (!edges) {
        nbmi::set_error("%s: null edges", who);
        return NBMI_ERR_ARG;
    }
    for (int k = 0; k <= nb; k++) {
        if (!isfinite(edges[k]) || edges[k] < 0.0 || (k > 0 && !(edges[k] > edges[k - 1]))) {
            nbmi::set_error("%s: edges[%d] = %g: the edges must be finite, >= 0 and strictly increasing", who, k, edges[k]);
            return NBMI_ERR_ARG;
        }
        e2->e2[k] = edges[k] * edges[k];
        if (!isfinite(e2->e2[k]) || (k > 0 && !(e2->e2[k] > e2->e2[k - 1]))) {
            nbmi::set_error("%s: the square of edges[%d] = %g is not finite or not above the one before it", who, k, edges[k]);
            return NBMI_ERR_ARG;
        }
    }
    return 0;
}
}  // namespace

int nbmi_pair_counts(nbmi_sim *s, int nb, const double *edges, int64_t *counts, int64_t *below, int64_t *evals,
                     int64_t *cell_pairs) {
    if (int rc = check_handle(s)) return rc;
    if (int rc = query_refuse(s, "nbmi_pair_counts")) return rc;
    PairEdges e2{};
    if (int rc = pair_edges_check("nbmi_pair_counts", nb, edges, &e2)) return rc;
    const PairSums sums{nb, counts, below, evals, cell_pairs};
    sums.zero();
    if (s->n < 2) return 0;
    if (int rc = query_sync(s, [&] { return pairs_enqueue(s, nb, e2); })) return rc;
    return sums.read(s);
}

namespace {
int mst_buffers(nbmi_sim *s) {
    auto &g = s->q.mst;
    const int64_t n = s->n;
    return query_alloc(g, [&]() -> int {
        g.sort_bytes = nbmi::radix_temp_bytes_u64((size_t)n, 64);
        if (dev_alloc(s, &g.rid, n) || dev_alloc(s, &g.bpart, n) || dev_alloc(s, &g.diff, n) || dev_alloc(s, &g.dscan, n + 1) ||
            dev_alloc(s, &g.tiles, (n + 1 + kScanTile - 1) / kScanTile + 1) || dev_alloc(s, &g.ctag, s->node_capacity + 2) ||
            dev_alloc(s, &g.bd2, n) || dev_alloc(s, &g.cmin, n) || dev_alloc(s, &g.cpair, n) || dev_alloc(s, &g.e_pack, n) ||
            dev_alloc(s, &g.e_d2, n) || dev_alloc(s, &g.va, n) || dev_alloc(s, &g.vb, n) ||
            dev_alloc(s, &g.sort_tmp, g.sort_bytes + 256) || dev_alloc(s, &g.counters, 2))
            return NBMI_ERR_HIP;
        NBMI_HIP_CHECK(nbmi::radix_init_temp(g.sort_tmp, s->stream));
        return 0;
    });
}
}  // namespace

int nbmi_mst(nbmi_sim *s, int32_t *edge_i, int32_t *edge_j, double *edge_d2, int64_t *rounds, int64_t *evals) {
    static const char *const who = "nbmi_mst";
    if (int rc = check_handle(s)) return rc;
    if (int rc = query_refuse(s, who)) return rc;
    if (rounds) *rounds = 0;
    if (evals) *evals = 0;
    const int64_t n = s->n;
    if (n < 2) return 0;
    hipStream_t st = s->stream;
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    if (int rc = check_device_error(s)) return rc;  // of earlier steps, as a getter reports them
    if (query_buffers(s) || fof_buffers(s)) return NBMI_ERR_HIP;
    if (int rc = pairs_prepare(s)) return rc;
    if (int rc = mst_buffers(s)) return rc;
    auto &g = s->q.mst;
    int32_t *parent = s->q.fof.parent, *comp = s->q.fof.root;
    const int64_t m = n - 1;  // the edges of the tree
    int max_rounds = 0;       // ceil(log2 n): every round at least halves the number of components
    while (((int64_t)1 << max_rounds) < n) max_rounds++;
    int64_t done = 0;
    unsigned long long c[2] = {0, 0};
    unsigned sort_err = 0u;
    // the staging holds 7 N doubles: the edges' two index arrays, then their d2
    int32_t *o_i = (int32_t *)s->stage, *o_j = o_i + n;
    double *o_d2 = (double *)s->stage + n;
    TimedSpans timed{s};
    g.rounds.clear();
    NBMI_HIP_CHECK(hipMemsetAsync(g.counters, 0, 2 * sizeof(unsigned long long), st));
    NBMI_HIP_CHECK(timed.begin());
    int rc = query_tree(s, [&]() -> int {
        const Bodies cur = s->buf[s->curbuf];
        const int grid = nblocks(n), waves = (int)((n + kQueryBlock - 1) / kQueryBlock), node_grid = nblocks(s->own_node_rows);
        const int64_t ntiles = (n + 1 + kScanTile - 1) / kScanTile;
        k_pair_cells<<<node_grid, kBlock, 0, st>>>(s->nodes, s->node_ref, s->info, n, s->own_node_rows, s->q.pairs.cnt);
        k_mst_init<<<grid, kBlock, 0, st>>>(s->info, n, s->perm, cur.id, parent, comp, g.rid, g.bd2, g.bpart, g.cmin, g.cpair);
        if (int r = launch_failed("%s: a kernel launch failed", who)) return r;
        // The loop ends when the tree is complete, after ceil(log2 n) rounds whatever the device says, and when a round
        // appended nothing: the build did not fit (every kernel returned at once), which the caller's check reports.
        while (c[1] < (unsigned long long)m && done < max_rounds) {
            const unsigned long long before = c[1], evals_before = c[0];
            const auto t0 = std::chrono::steady_clock::now();
            k_mst_diff<<<grid, kBlock, 0, st>>>(s->info, n, comp, g.diff);
            k_iscan_reduce<<<(unsigned)ntiles, kBlock, 0, st>>>(g.diff, n, 0, g.tiles, 0);
            scan::k_scan_values<<<1, scan::kScanThreads, 0, st>>>(g.tiles, g.tiles, ntiles, (int64_t)0, 0, scan::Sum());
            k_iscan_apply<<<(unsigned)ntiles, kBlock, 0, st>>>(g.diff, n, 0, g.tiles, 0, g.dscan);
            k_mst_tags<<<node_grid, kBlock, 0, st>>>(s->node_ref, s->q.pairs.cnt, s->info, n, s->own_node_rows, comp, g.dscan, g.ctag);
            with_bool(done > 0, [&](auto carry) {
                k_mst_search<decltype(carry)::value><<<waves, kQueryBlock, 0, st>>>(
                    s->nodes, s->q.shared.rows, s->node_ref, s->info, s->perm, cur, n, comp, g.rid, g.ctag, s->q.pairs.cnt, g.bd2, g.bpart,
                    g.cmin, evals ? g.counters : nullptr);
            });
            k_mst_pick<<<grid, kBlock, 0, st>>>(s->info, n, comp, g.rid, g.bd2, g.bpart, g.cmin, g.cpair);
            k_mst_emit<<<grid, kBlock, 0, st>>>(s->info, n, comp, g.rid, g.bd2, g.bpart, g.cmin, g.cpair, parent, g.e_pack, g.e_d2,
                                                g.counters + 1);
            k_mst_flatten<<<grid, kBlock, 0, st>>>(s->info, n, parent, comp, g.cmin, g.cpair);
            if (int r = launch_failed("%s: a kernel launch failed", who)) return r;
            NBMI_HIP_CHECK(hipMemcpyAsync(c, g.counters, sizeof(c), hipMemcpyDeviceToHost, st));
            NBMI_HIP_CHECK(hipStreamSynchronize(st));
            if (c[1] == before) break;
            done++;
            g.rounds.push_back({(int64_t)(c[0] - evals_before), (int64_t)(c[1] - before),
                                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()});
        }
        if (c[1] != (unsigned long long)m) return 0;
        // the final order: two stable passes, by the packed indices, then by the bits of d2 (cmin / cpair are free now)
        uint64_t *ka = (uint64_t *)g.cmin, *kb = (uint64_t *)g.cpair;
        int idbits = 1;
        while (idbits < 31 && ((int64_t)1 << idbits) < n) idbits++;
        k_fof_iota<<<nblocks(m), kBlock, 0, st>>>(m, g.va);
        NBMI_HIP_CHECK(nbmi::radix_sort_pairs_u64(g.sort_tmp, g.sort_bytes, (const uint64_t *)g.e_pack, ka, g.va, g.vb, (size_t)m, 0,
                                                  32 + idbits, st));
        k_mst_gather<<<nblocks(m), kBlock, 0, st>>>(m, g.vb, g.e_d2, kb);
        NBMI_HIP_CHECK(nbmi::radix_sort_pairs_u64(g.sort_tmp, g.sort_bytes, kb, ka, g.vb, g.va, (size_t)m, 0, 63, st));
        k_mst_out<<<nblocks(m), kBlock, 0, st>>>(m, g.va, ka, g.e_pack, o_i, o_j, o_d2);
        if (int r = launch_failed("%s: a kernel launch failed", who)) return r;
        return nbmi::radix_error_word(g.sort_tmp, &sort_err, st) == hipSuccess ? 0 : NBMI_ERR_HIP;
    });
    if (rc) return rc;
    NBMI_HIP_CHECK(timed.end());
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    NBMI_HIP_CHECK(timed.add());
    if (int r = check_device_error(s)) return r;  // the build's own capacity error, with a step's message
    if (sort_err) {
        NBMI_HIP_CHECK(nbmi::radix_init_temp(g.sort_tmp, st));
        nbmi::set_error("%s: device radix sort: a look-back spin timed out", who);
        return NBMI_ERR_HIP;
    }
    if (c[1] != (unsigned long long)m) {
        nbmi::set_error("%s: %lld rounds left %llu of %lld edges", who, (long long)done, c[1], (long long)m);
        return NBMI_ERR_HIP;
    }
    if (edge_i) NBMI_HIP_CHECK(hipMemcpyAsync(edge_i, o_i, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (edge_j) NBMI_HIP_CHECK(hipMemcpyAsync(edge_j, o_j, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (edge_d2) NBMI_HIP_CHECK(hipMemcpyAsync(edge_d2, o_d2, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    if (rounds) *rounds = done;
    if (evals) *evals = (int64_t)c[0];
    return 0;
}

int nbmi_mst_rounds(nbmi_sim *s, int capacity, int64_t *evals, int64_t *edges, double *ms) {
    if (int rc = check_handle(s)) return rc;
    const auto &r = s->q.mst.rounds;
    for (int k = 0; k < capacity && k < (int)r.size(); k++) {
        if (evals) evals[k] = r[k].evals;
        if (edges) edges[k] = r[k].edges;
        if (ms) ms[k] = r[k].ms;
    }
    return (int)r.size();
}

int nbmi_deposit(nbmi_sim *s, const double *lo, const double *hi, const int32_t *dims, int scheme, int quantities,
                 double *out, int64_t *stats3, int32_t *exponents) {
    static const char *const kPlaneName[kDepPlanes] = {"NUMBER", "MASS", "MOMENTUM x", "MOMENTUM y", "MOMENTUM z", "KINETIC"};
    constexpr int64_t kDepMaxWords = (int64_t)1 << 28;
    if (int rc = sums_refuse(s, "nbmi_deposit")) return rc;
    if (!lo || !hi || !dims || !out) {
        nbmi::set_error("nbmi_deposit: null %s", !lo ? "lo" : !hi ? "hi" : !dims ? "dims" : "out");
        return NBMI_ERR_ARG;
    }
    if (scheme != NBMI_DEPOSIT_NGP && scheme != NBMI_DEPOSIT_CIC) {
        nbmi::set_error("nbmi_deposit: scheme = %d is neither NBMI_DEPOSIT_NGP (0) nor NBMI_DEPOSIT_CIC (1)", scheme);
        return NBMI_ERR_ARG;
    }
    if (quantities == 0 || (quantities & ~15) != 0) {
        nbmi::set_error("nbmi_deposit: quantities = %d selects nothing or has unknown bits", quantities);
        return NBMI_ERR_ARG;
    }
    DepSource a{};
    a.cells = 1;
    for (int k = 0; k < 3; k++) {
        if (!isfinite(lo[k]) || !isfinite(hi[k]) || !(hi[k] > lo[k])) {
            nbmi::set_error("nbmi_deposit: axis %d: the bounds [%g, %g] must be finite with hi > lo", k, lo[k], hi[k]);
            return NBMI_ERR_ARG;
        }
        if (dims[k] < 1) {
            nbmi::set_error("nbmi_deposit: dims[%d] = %d is < 1", k, (int)dims[k]);
            return NBMI_ERR_ARG;
        }
        const double width = hi[k] - lo[k], inv = (double)dims[k] / width;
        if (!isfinite(width) || !isfinite(inv)) {
            nbmi::set_error("nbmi_deposit: axis %d: the width %g or dims / width = %g is not finite", k, width, inv);
            return NBMI_ERR_ARG;
        }
        a.lo[k] = lo[k];
        a.inv[k] = inv;
        a.dims[k] = dims[k];
        a.dimd[k] = (double)dims[k];
        a.cic[k] = scheme == NBMI_DEPOSIT_CIC && dims[k] >= 2;
        a.cells = a.cells <= kDepMaxWords ? a.cells * dims[k] : a.cells;  // (stays above the limit once it is)
    }
    if (quantities & NBMI_DEPOSIT_NUMBER) a.slot[a.planes++] = 0;
    if (quantities & NBMI_DEPOSIT_MASS) a.slot[a.planes++] = 1;
    if (quantities & NBMI_DEPOSIT_MOMENTUM)
        for (int c = 0; c < 3; c++) a.slot[a.planes++] = 2 + c;
    if (quantities & NBMI_DEPOSIT_KINETIC) a.slot[a.planes++] = 5;
    if (a.cells > kDepMaxWords || a.planes * a.cells > kDepMaxWords) {
        nbmi::set_error("nbmi_deposit: %d planes of %d x %d x %d cells are more than 2^28 values", a.planes, (int)dims[0],
                        (int)dims[1], (int)dims[2]);
        return NBMI_ERR_ARG;
    }
    const int64_t n = s->n, words = a.planes * a.cells;
    hipStream_t st = s->stream;
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    if (int rc = check_device_error(s)) return rc;
    unsigned long long h[kDepPlanes + 3] = {};
    if (n > 0) {
        if (!s->dep.res && dev_alloc(s, &s->dep.res, kDepPlanes + 3)) return NBMI_ERR_HIP;
        if (words > s->dep.words) {  // (nothing enqueued uses the old array: every call waits for its copies)
            dev_free(s, &s->dep.K);
            s->dep.words = 0;
            if (dev_alloc(s, &s->dep.K, (size_t)words)) return NBMI_ERR_HIP;
            s->dep.words = words;
        }
        const Bodies cur = s->buf[s->curbuf];
        TimedSpans timed{s};
        NBMI_HIP_CHECK(hipMemsetAsync(s->dep.res, 0, sizeof(h), st));
        NBMI_HIP_CHECK(timed.begin());
        k_plane_max<kDepPlanes><<<plane_max_blocks(n), kBlock, 0, st>>>(cur, n, a, s->dep.res);
        NBMI_HIP_CHECK(hipGetLastError());
        NBMI_HIP_CHECK(timed.end());
        NBMI_HIP_CHECK(hipMemcpyAsync(h, s->dep.res, kDepPlanes * sizeof(h[0]), hipMemcpyDeviceToHost, st));
        NBMI_HIP_CHECK(hipStreamSynchronize(st));
        if (int rc = plane_exponents("nbmi_deposit", h, n, kSumHeadroom, a.planes, a.slot, kPlaneName, a.e, a.live)) return rc;
        NBMI_HIP_CHECK(hipMemsetAsync(s->dep.K, 0, (size_t)words * sizeof(unsigned long long), st));
        NBMI_HIP_CHECK(timed.begin());
        const int blocks = (int)((n + kBlock * kDepRows - 1) / (kBlock * kDepRows));
        if (s->deposit_agg) {
            const size_t lds = (size_t)kDepSlots * (a.planes * sizeof(unsigned long long) + sizeof(int));
            k_deposit<true><<<blocks, kBlock, lds, st>>>(cur, n, a, s->dep.K, s->dep.res + kDepPlanes);
        } else {
            k_deposit<false><<<blocks, kBlock, 0, st>>>(cur, n, a, s->dep.K, s->dep.res + kDepPlanes);
        }
        k_deposit_out<<<nblocks(a.cells), kBlock, 0, st>>>(s->dep.K, a);
        NBMI_HIP_CHECK(hipGetLastError());
        NBMI_HIP_CHECK(timed.end());
        NBMI_HIP_CHECK(hipMemcpyAsync(h + kDepPlanes, s->dep.res + kDepPlanes, 3 * sizeof(h[0]), hipMemcpyDeviceToHost, st));
        NBMI_HIP_CHECK(hipMemcpyAsync(out, s->dep.K, (size_t)words * sizeof(double), hipMemcpyDeviceToHost, st));
        NBMI_HIP_CHECK(hipStreamSynchronize(st));
        NBMI_HIP_CHECK(timed.add());  // the two passes
    } else {
        for (int64_t i = 0; i < words; i++) out[i] = 0.0;
    }
    for (int p = 0; exponents && p < a.planes; p++) exponents[p] = a.e[p];
    for (int k = 0; stats3 && k < 3; k++) stats3[k] = (int64_t)h[kDepPlanes + k];
    return 0;
}

namespace {
// what both calls of section 4.26 refuse: the handles that nbmi_deposit refuses, and a centre that is none
int profile_refuse(nbmi_sim *s, const char *who, const double *center) {
    if (int rc = sums_refuse(s, who)) return rc;
    if (!center) {
        nbmi::set_error("%s: null center", who);
        return NBMI_ERR_ARG;
    }
    for (int k = 0; k < 3; k++) {
        if (!isfinite(center[k])) {
            nbmi::set_error("%s: center[%d] = %g is not finite", who, k, center[k]);
            return NBMI_ERR_ARG;
        }
    }
    return 0;
}
}  // namespace

int nbmi_radial_profile(nbmi_sim *s, const double *center, const double *bulk_velocity, int nb, const double *edges,
                        int quantities, double *out, int64_t *stats3, int32_t *exponents) {
    static const char *const kWho = "nbmi_radial_profile";
    static const char *const kPlaneName[kProfPlanes] = {"NUMBER", "MASS", "RADIAL_MOMENTUM", "RADIAL_KINETIC", "KINETIC",
                                                        "ANGULAR_MOMENTUM x", "ANGULAR_MOMENTUM y", "ANGULAR_MOMENTUM z"};
    if (int rc = profile_refuse(s, kWho, center)) return rc;
    if (!edges || !out) {
        nbmi::set_error("%s: null %s", kWho, !edges ? "edges" : "out");
        return NBMI_ERR_ARG;
    }
    for (int k = 0; bulk_velocity && k < 3; k++) {
        if (!isfinite(bulk_velocity[k])) {
            nbmi::set_error("%s: bulk_velocity[%d] = %g is not finite", kWho, k, bulk_velocity[k]);
            return NBMI_ERR_ARG;
        }
    }
    if (nb < 1 || nb > kProfMaxBins) {
        nbmi::set_error("%s: nb = %d is outside 1 .. %d", kWho, nb, kProfMaxBins);
        return NBMI_ERR_ARG;
    }
    if (quantities == 0 || (quantities & ~63) != 0) {
        nbmi::set_error("%s: quantities = %d selects nothing or has unknown bits", kWho, quantities);
        return NBMI_ERR_ARG;
    }
    ProfSource a{};
    for (int k = 0; k <= nb; k++) {
        if (!isfinite(edges[k]) || edges[k] < 0.0 || (k > 0 && !(edges[k] > edges[k - 1]))) {
            nbmi::set_error("%s: edges[%d] = %g: the edges must be finite, >= 0 and strictly increasing", kWho, k, edges[k]);
            return NBMI_ERR_ARG;
        }
        a.E[k] = edges[k] * edges[k];
        if (!isfinite(a.E[k]) || (k > 0 && !(a.E[k] > a.E[k - 1]))) {
            nbmi::set_error("%s: the square of edges[%d] = %g is not finite or not above the one before it", kWho, k, edges[k]);
            return NBMI_ERR_ARG;
        }
    }
    for (int k = 0; k < 3; k++) {
        a.c[k] = center[k];
        a.b[k] = bulk_velocity ? bulk_velocity[k] : 0.0;
    }
    a.bulk = bulk_velocity ? 1 : 0;
    a.nb = nb;
    for (int b = 0; b < 5; b++)
        if (quantities & (1 << b)) a.slot[a.planes++] = b;
    if (quantities & NBMI_PROFILE_ANGULAR_MOMENTUM)
        for (int c = 0; c < 3; c++) a.slot[a.planes++] = 5 + c;
    a.need = (quantities & ~NBMI_PROFILE_NUMBER ? kProfNeedM : 0) |
             (quantities & (NBMI_PROFILE_RADIAL_MOMENTUM | NBMI_PROFILE_RADIAL_KINETIC) ? kProfNeedVr : 0) |
             (quantities & NBMI_PROFILE_KINETIC ? kProfNeedW2 : 0) | (quantities & NBMI_PROFILE_ANGULAR_MOMENTUM ? kProfNeedL : 0);
    const int64_t n = s->n;
    const int nslots = nb + 1, words = a.planes * nslots;
    hipStream_t st = s->stream;
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    if (int rc = check_device_error(s)) return rc;
    constexpr int kRes = kProfPlanes + 3;
    unsigned long long h[kRes] = {};
    std::vector<unsigned long long> K((size_t)words, 0ull);
    if (n > 0) {
        if (!s->prof.res && dev_alloc(s, &s->prof.res, kRes + kProfPlanes * (kProfMaxBins + 1))) return NBMI_ERR_HIP;
        const Bodies cur = s->buf[s->curbuf];
        TimedSpans timed{s};
        NBMI_HIP_CHECK(hipMemsetAsync(s->prof.res, 0, (size_t)(kRes + words) * sizeof(h[0]), st));
        NBMI_HIP_CHECK(timed.begin());
        k_plane_max<kProfPlanes><<<plane_max_blocks(n), kBlock, 0, st>>>(cur, n, a, s->prof.res);
        NBMI_HIP_CHECK(hipGetLastError());
        NBMI_HIP_CHECK(timed.end());
        NBMI_HIP_CHECK(hipMemcpyAsync(h, s->prof.res, kProfPlanes * sizeof(h[0]), hipMemcpyDeviceToHost, st));
        NBMI_HIP_CHECK(hipStreamSynchronize(st));
        if (int rc = plane_exponents(kWho, h, n, kSumHeadroom, a.planes, a.slot, kPlaneName, a.e, a.live)) return rc;
        NBMI_HIP_CHECK(timed.begin());
        const int blocks = (int)((n + kBlock * kProfRows - 1) / (kBlock * kProfRows));
        const size_t lds = (size_t)(kProfEdgePad + words) * sizeof(unsigned long long);
        k_profile<<<blocks, kBlock, lds, st>>>(cur, n, a, s->prof.res + kRes, s->prof.res + kProfPlanes);
        NBMI_HIP_CHECK(hipGetLastError());
        NBMI_HIP_CHECK(timed.end());
        NBMI_HIP_CHECK(hipMemcpyAsync(h + kProfPlanes, s->prof.res + kProfPlanes, 3 * sizeof(h[0]), hipMemcpyDeviceToHost, st));
        NBMI_HIP_CHECK(hipMemcpyAsync(K.data(), s->prof.res + kRes, (size_t)words * sizeof(h[0]), hipMemcpyDeviceToHost, st));
        NBMI_HIP_CHECK(hipStreamSynchronize(st));
        NBMI_HIP_CHECK(timed.add());  // the two passes
    }
    for (int p = 0; p < a.planes; p++)
        for (int k = 0; k < nslots; k++) out[p * nslots + k] = fx_value(K[(size_t)p * nslots + k], a.e[p]);
    for (int p = 0; exponents && p < a.planes; p++) exponents[p] = a.e[p];
    for (int k = 0; stats3 && k < 3; k++) stats3[k] = (int64_t)h[kProfPlanes + k];
    return 0;
}

int nbmi_mass_radii(nbmi_sim *s, const double *center, int nf, const double *fractions, double *radius2, int64_t *inside,
                    double *mass_inside, double *total_mass, int64_t *stats2, int32_t *exponent) {
    static const char *const kWho = "nbmi_mass_radii";
    if (int rc = profile_refuse(s, kWho, center)) return rc;
    if (!fractions || !radius2) {
        nbmi::set_error("%s: null %s", kWho, !fractions ? "fractions" : "radius2");
        return NBMI_ERR_ARG;
    }
    if (nf < 1 || nf > kMrMaxFractions) {
        nbmi::set_error("%s: nf = %d is outside 1 .. %d", kWho, nf, kMrMaxFractions);
        return NBMI_ERR_ARG;
    }
    for (int f = 0; f < nf; f++) {
        if (!isfinite(fractions[f]) || !(fractions[f] > 0.0) || fractions[f] > 1.0) {
            nbmi::set_error("%s: fractions[%d] = %g is not in (0, 1]", kWho, f, fractions[f]);
            return NBMI_ERR_ARG;
        }
    }
    const int64_t n = s->n;
    hipStream_t st = s->stream;
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    if (int rc = check_device_error(s)) return rc;
    constexpr int kRes = 3;  // the largest mass, a mass is negative, bodies skipped; then 3 words per fraction
    unsigned long long h[kRes + 3 * kMrMaxFractions] = {};
    long long k_total = 0;
    int e = 0;
    auto &g = s->mr;
    if (n > 0) {
        if (n > g.rows) {  // (nothing enqueued uses the old arrays: every call waits for its copies)
            dev_free(s, &g.key); dev_free(s, &g.key_s); dev_free(s, &g.idx); dev_free(s, &g.idx_s); dev_free(s, &g.kk);
            dev_free(s, &g.tiles); dev_free(s, &g.sort_tmp);
            g.rows = 0;
            g.sort_bytes = nbmi::radix_temp_bytes_u64((size_t)n, 63);
            if ((!g.res && dev_alloc(s, &g.res, kRes + 3 * kMrMaxFractions)) || dev_alloc(s, &g.key, (size_t)n) ||
                dev_alloc(s, &g.key_s, (size_t)n) || dev_alloc(s, &g.idx, (size_t)n) || dev_alloc(s, &g.idx_s, (size_t)n) ||
                dev_alloc(s, &g.kk, (size_t)n) || dev_alloc(s, &g.tiles, (size_t)scan::tiles_for(n) + 1) ||
                dev_alloc(s, &g.sort_tmp, g.sort_bytes + 256))
                return NBMI_ERR_HIP;
            NBMI_HIP_CHECK(nbmi::radix_init_temp(g.sort_tmp, st));
            g.rows = n;
        }
        const Bodies cur = s->buf[s->curbuf];
        TimedSpans timed{s};
        NBMI_HIP_CHECK(hipMemsetAsync(g.res, 0, sizeof(h), st));
        NBMI_HIP_CHECK(timed.begin());
        k_plane_max<1><<<plane_max_blocks(n), kBlock, 0, st>>>(cur, n, MrSource{}, g.res);
        k_mr_keys<<<nblocks(n), kBlock, 0, st>>>(cur, n, center[0], center[1], center[2], g.key, g.idx, g.res + 2);
        NBMI_HIP_CHECK(hipGetLastError());
        NBMI_HIP_CHECK(timed.end());
        NBMI_HIP_CHECK(hipMemcpyAsync(h, g.res, kRes * sizeof(h[0]), hipMemcpyDeviceToHost, st));
        NBMI_HIP_CHECK(hipStreamSynchronize(st));
        static const char *const kPlaneName[1] = {"MASS"};
        int live = 0;
        const int not_finite = plane_exponents(kWho, h, n, kExactSumHeadroom, 1, MrSource::slot, kPlaneName, &e, &live);
        if (not_finite || h[1]) {
            nbmi::set_error("%s: a mass is %s", kWho, not_finite ? "not finite" : "negative");
            return NBMI_ERR_ARG;
        }
        if (live) {
            const int64_t ntiles = scan::tiles_for(n);
            MrSeg total{};
            NBMI_HIP_CHECK(timed.begin());
            NBMI_HIP_CHECK(nbmi::radix_sort_pairs_u64(g.sort_tmp, g.sort_bytes, g.key, g.key_s, g.idx, g.idx_s, (size_t)n, 0, 63, st));
            k_mr_tiles<<<(int)ntiles, scan::kBlock, 0, st>>>(cur, n, g.key_s, g.idx_s, e, g.kk, g.tiles);
            scan::k_scan_values<<<1, scan::kScanThreads, 0, st>>>(g.tiles, g.tiles, ntiles, (int64_t)0, MrSeg{0ll, 0ll, 0}, MrSegOp());
            NBMI_HIP_CHECK(hipGetLastError());
            NBMI_HIP_CHECK(timed.end());
            NBMI_HIP_CHECK(hipMemcpyAsync(&total, g.tiles + ntiles, sizeof(total), hipMemcpyDeviceToHost, st));
            NBMI_HIP_CHECK(hipStreamSynchronize(st));
            k_total = total.sum;
            if (k_total > 0) {
                MrArgs a{};
                a.nf = nf;
                a.e = e;
                for (int f = 0; f < nf; f++) {
                    const long long t = (long long)ceil(fractions[f] * (double)k_total);
                    a.T[f] = t < 1 ? 1 : t;
                    a.tmin = f == 0 || a.T[f] < a.tmin ? a.T[f] : a.tmin;
                    a.tmax = f == 0 || a.T[f] > a.tmax ? a.T[f] : a.tmax;
                }
                NBMI_HIP_CHECK(timed.begin());
                k_mr_select<<<(int)ntiles, scan::kBlock, 0, st>>>(n, g.key_s, g.kk, g.tiles, a, g.res + kRes);
                NBMI_HIP_CHECK(hipGetLastError());
                NBMI_HIP_CHECK(timed.end());
                NBMI_HIP_CHECK(hipMemcpyAsync(h + kRes, g.res + kRes, (size_t)3 * nf * sizeof(h[0]), hipMemcpyDeviceToHost, st));
            }
            unsigned sort_err = 0u;
            NBMI_HIP_CHECK(nbmi::radix_error_word(g.sort_tmp, &sort_err, st));
            NBMI_HIP_CHECK(hipStreamSynchronize(st));
            if (sort_err) {
                NBMI_HIP_CHECK(nbmi::radix_init_temp(g.sort_tmp, st));
                NBMI_HIP_CHECK(hipStreamSynchronize(st));
                nbmi::set_error("%s: the sort of the squared radii failed", kWho);
                return NBMI_ERR_HIP;
            }
        }
        NBMI_HIP_CHECK(timed.add());  // the call's kernels
    }
    for (int f = 0; f < nf; f++) {
        if (k_total > 0) {
            memcpy(&radius2[f], &h[kRes + 3 * f], sizeof(double));
        } else {
            radius2[f] = NAN;
        }
        if (inside) inside[f] = k_total > 0 ? (int64_t)h[kRes + 3 * f + 1] : 0;
        if (mass_inside) mass_inside[f] = k_total > 0 ? fx_value(h[kRes + 3 * f + 2], e) : 0.0;
    }
    if (total_mass) *total_mass = fx_value((unsigned long long)k_total, e);
    if (stats2) {
        stats2[0] = n - (int64_t)h[2];
        stats2[1] = (int64_t)h[2];
    }
    if (exponent) *exponent = e;
    return 0;
}

namespace {
// the first row of an (m, 3) array with a value that is not finite or above `limit` in magnitude; -1: none, and *pmax
// (if asked for) is raised to the largest magnitude.  (The maximum stays in a register: nbmi_field_at scans 3 m values
// on every call.)
int64_t first_bad_row(const double *a, int64_t m, double limit, double *pmax) {
    double mx = 0.0;
    for (int64_t i = 0; i < 3 * m; i++) {
        const double v = fabs(a[i]);
        if (!(v <= limit)) return i / 3;  // (a NaN fails the comparison too)
        mx = v > mx ? v : mx;
    }
    if (pmax && mx > *pmax) *pmax = mx;
    return -1;
}

// nbmi_field_at's scratch for chunks of `need` points (nbmi_sim::field): rows double up to the chunk.  Nothing enqueued
// uses the old arrays - the call that filled them has waited for its copies.
int field_alloc(nbmi_sim *s, int64_t need) {
    auto &f = s->field;
    if (need <= f.rows) return 0;
    int64_t rows = f.rows ? f.rows : kFieldMinRows;
    while (rows < need) rows *= 2;
    if (rows > kFieldChunk) rows = kFieldChunk;
    probe_free(s, f);
    dev_free(s, &f.pts); dev_free(s, &f.acc); dev_free(s, &f.phi); dev_free(s, &f.cnt); dev_free(s, &f.t6);
    dev_free(s, &f.pp);
    f.pp_words = 0;
    const size_t r = (size_t)rows;
    if (dev_alloc(s, &f.pts, 3 * r) || dev_alloc(s, &f.acc, 3 * r) || dev_alloc(s, &f.phi, r) || dev_alloc(s, &f.cnt, r))
        return NBMI_ERR_HIP;
    if (s->method == NBMI_METHOD_BARNES_HUT) return probe_alloc(s, f, rows);
    f.rows = rows;  // (a direct handle walks nothing)
    return 0;
}

// What a point call writes, per point and each only if asked for (not null): nbmi_field_at's acc and phi, or - `tidal` -
// nbmi_tidal_at's t6; terms for either.
struct FieldOut {
    bool tidal;
    double *acc, *phi, *t6;
    int32_t *terms;
    bool any() const { return acc || phi || t6 || terms; }
    void zero(int64_t m) const {  // no bodies: no field
        for (int64_t i = 0; i < m; i++) {
            if (acc) acc[3 * i] = acc[3 * i + 1] = acc[3 * i + 2] = 0.0;
            if (phi) phi[i] = 0.0;
            for (int k = 0; t6 && k < 6; k++) t6[6 * i + k] = 0.0;
            if (terms) terms[i] = 0;
        }
    }
};
// The chunks of one call of `who`, enqueued and copied out one after the other; the tree (Barnes-Hut) stands.  pmax: the
// call's largest |coordinate|.
int field_chunks(nbmi_sim *s, const char *who, int64_t m, const double *pts, double pmax, const FieldOut &o) {
    auto &f = s->field;
    hipStream_t st = s->stream;
    const bool tree = s->method == NBMI_METHOD_BARNES_HUT;
    const double eps2 = s->softening * s->softening;
    auto walk = [&](int64_t, int64_t mc, const uint32_t *order) {
        if (!tree) {
            if (o.tidal)
                k_tidal_direct<<<nblocks(mc), kBlock, 0, st>>>(s->buf[s->curbuf], s->n, s->G, eps2, f.pts, mc, o.t6 ? f.t6 : nullptr,
                                                               nullptr, o.terms ? f.cnt : nullptr);
            else
                k_field_direct<<<nblocks(mc), kBlock, 0, st>>>(s->buf[s->curbuf], s->n, s->G, eps2, f.pts, mc, o.acc ? f.acc : nullptr,
                                                               o.phi ? f.phi : nullptr, o.terms ? f.cnt : nullptr);
        } else {
            with_bool(s->multipole == NBMI_MULTIPOLE_QUADRUPOLE, [&](auto q) {
                const double *quad = decltype(q)::value ? s->quad_work : nullptr;
                if (o.tidal)
                    k_tidal_tree<decltype(q)::value><<<nblocks(mc), kBlock, 0, st>>>(
                        s->nodes, s->diag_pot, f.wtab, s->info, f.sx, f.sy, f.sz, order, mc, (float)eps2, s->softening, pmax, quad,
                        o.t6 ? f.t6 : nullptr, o.terms ? f.cnt : nullptr);
                else
                    k_field_tree<decltype(q)::value><<<nblocks(mc), kBlock, 0, st>>>(
                        s->nodes, s->diag_pot, f.wtab, s->info, f.sx, f.sy, f.sz, order, mc, (float)eps2, s->softening, pmax, quad,
                        o.acc ? f.acc : nullptr, o.phi ? f.phi : nullptr, o.terms ? f.cnt : nullptr);
            });
        }
    };
    auto copy_out = [&](int64_t b, int64_t mc) -> int {
        if (o.acc) NBMI_HIP_CHECK(hipMemcpyAsync(o.acc + 3 * b, f.acc, (size_t)mc * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        if (o.phi) NBMI_HIP_CHECK(hipMemcpyAsync(o.phi + b, f.phi, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, st));
        if (o.t6) NBMI_HIP_CHECK(hipMemcpyAsync(o.t6 + 6 * b, f.t6, (size_t)mc * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
        if (o.terms) NBMI_HIP_CHECK(hipMemcpyAsync(o.terms + b, f.cnt, (size_t)mc * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        return 0;
    };
    return probe_chunks(s, who, tree, m, pts, walk, copy_out);
}

// What nbmi_field_at and nbmi_tidal_at (`who`) check before anything is enqueued: the handle's kind, m and the points.
// *pmax: the largest |coordinate|.
int field_points_check(nbmi_sim *s, const char *who, int64_t m, const double *points_xyz, double *pmax) {
    if (int rc = diag_refuse(s, who)) return rc;
    if (m < 0) {
        nbmi::set_error("%s: m = %lld is negative", who, (long long)m);
        return NBMI_ERR_ARG;
    }
    if (m == 0) return 0;
    if (!points_xyz) {
        nbmi::set_error("%s: null points_xyz", who);
        return NBMI_ERR_ARG;
    }
    const int64_t bad = first_bad_row(points_xyz, m, 1e18, pmax);
    if (bad >= 0) {
        const double *r = points_xyz + 3 * bad;
        nbmi::set_error("%s: points_xyz row %lld holds %g: coordinates must be finite and at most 1e18 in magnitude", who,
                        (long long)bad, !(fabs(r[0]) <= 1e18) ? r[0] : !(fabs(r[1]) <= 1e18) ? r[1] : r[2]);
        return NBMI_ERR_ARG;
    }
    return 0;
}
// A point call (`who`) from its checks to its chunks: the points, m == 0, zeros where there are no bodies, nothing asked
// for, the scratch, then the chunks - Barnes-Hut: on a side tree of the current positions with the float64 rows.
int field_call(nbmi_sim *s, const char *who, int64_t m, const double *points_xyz, const FieldOut &o) {
    if (int rc = check_handle(s)) return rc;
    double pmax = 0.0;
    if (int rc = field_points_check(s, who, m, points_xyz, &pmax)) return rc;
    if (m == 0) return 0;
    if (s->n == 0) {
        o.zero(m);
        return 0;
    }
    if (!o.any()) return 0;
    if (int rc = field_alloc(s, m)) return rc;
    auto &f = s->field;
    if (o.tidal && !f.t6 && dev_alloc(s, &f.t6, 6 * (size_t)f.rows)) return NBMI_ERR_HIP;  // 48 bytes per scratch row, from the first tidal call on
    auto chunks = [&] { return field_chunks(s, who, m, points_xyz, pmax, o); };
    return s->method != NBMI_METHOD_BARNES_HUT ? chunks() : side_tree(s, true, true, false, false, chunks);
}
}  // namespace

int nbmi_field_at(nbmi_sim *s, int64_t m, const double *points_xyz, double *acc_xyz, double *phi, int32_t *terms) {
    return field_call(s, "nbmi_field_at", m, points_xyz, FieldOut{false, acc_xyz, phi, nullptr, terms});
}

int nbmi_tidal_at(nbmi_sim *s, int64_t m, const double *points_xyz, double *tidal6, int32_t *terms) {
    return field_call(s, "nbmi_tidal_at", m, points_xyz, FieldOut{true, nullptr, nullptr, tidal6, terms});
}

// The bodies per distance bin about m points (section 4.28): nbmi_pair_counts' tree, rows and cell counts, and on them
// nbmi_field_at's chunks with k_pair_counts_at as their kernel.  Synchronous.
int nbmi_pair_counts_at(nbmi_sim *s, int64_t m, const double *points_xyz, int nb, const double *edges, int64_t *counts,
                        int64_t *below, int32_t *per_point, int64_t *evals, int64_t *cell_pairs) {
    static const char *const who = "nbmi_pair_counts_at";
    if (int rc = check_handle(s)) return rc;
    if (int rc = query_refuse(s, who)) return rc;
    if (int rc = field_points_check(s, who, m, points_xyz, nullptr)) return rc;
    PairEdges e2{};
    if (int rc = pair_edges_check(who, nb, edges, &e2)) return rc;
    const PairSums sums{nb, counts, below, evals, cell_pairs};
    sums.zero();
    if (m == 0) return 0;
    const int64_t n = s->n;
    const int64_t cols = nb + 1;
    if (n == 0) {
        for (int64_t i = 0; per_point && i < m * cols; i++) per_point[i] = 0;
        return 0;
    }
    if (int rc = field_alloc(s, m)) return rc;
    auto &f = s->field;
    auto &g = s->q.pairs;
    if (per_point && f.pp_words < f.rows * cols) {  // (nothing enqueued uses the old rows: every call waits for its copies)
        dev_free(s, &f.pp);
        f.pp_words = 0;
        if (dev_alloc(s, &f.pp, (size_t)(f.rows * cols))) return NBMI_ERR_HIP;
        f.pp_words = f.rows * cols;
    }
    hipStream_t st = s->stream;
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    if (int rc = check_device_error(s)) return rc;  // of earlier steps, as a getter reports them
    if (int rc = pairs_prepare(s)) return rc;
    const int rc = query_tree(s, [&]() -> int {
        k_pair_cells<<<nblocks(s->own_node_rows), kBlock, 0, st>>>(s->nodes, s->node_ref, s->info, n, s->own_node_rows, g.cnt);
        if (int r = launch_failed("%s: a kernel launch failed", who)) return r;
        if (int r = check_device_error(s)) return r;  // the build's own capacity error, before anything walks
        return probe_chunks(
            s, who, true, m, points_xyz,
            [&](int64_t, int64_t mc, const uint32_t *order) {
                k_pair_counts_at<<<(int)((mc + kQueryBlock - 1) / kQueryBlock), kQueryBlock, pair_lds_bytes(nb), st>>>(
                    s->nodes, s->q.shared.rows, s->node_ref, g.cnt, s->info, f.sx, f.sy, f.sz, order, mc, nb, e2,
                    s->pair_cells ? 1 : 0, per_point ? f.pp : nullptr, g.out);
            },
            [&](int64_t b, int64_t mc) -> int {
                if (per_point)
                    NBMI_HIP_CHECK(hipMemcpyAsync(per_point + b * cols, f.pp, (size_t)(mc * cols) * sizeof(int32_t),
                                                  hipMemcpyDeviceToHost, st));
                return 0;
            });
    });
    return rc ? rc : sums.read(s);
}

// The tidal tensor at every body's own position: nbmi_get_potentials_f64's build and lane setup, the rows written in the
// caller's order straight into the getter staging (6 N doubles, then the N norms: it holds 7 N), so nothing is allocated.
int nbmi_get_tidal_f64(nbmi_sim *s, double *tidal6, double *norm) {
    if (int rc = check_handle(s)) return rc;
    if (int rc = diag_refuse(s, "nbmi_get_tidal_f64")) return rc;
    const int64_t n = s->n;
    if (n == 0 || (!tidal6 && !norm)) return 0;
    hipStream_t st = s->stream;
    double *d_t6 = (double *)s->stage, *d_norm = d_t6 + 6 * n;
    const double eps2 = s->softening * s->softening;
    if (s->method != NBMI_METHOD_BARNES_HUT) {
        k_tidal_direct<<<nblocks(n), kBlock, 0, st>>>(s->buf[s->curbuf], n, s->G, eps2, nullptr, n, tidal6 ? d_t6 : nullptr,
                                                       norm ? d_norm : nullptr, nullptr);
        if (int rc = launch_failed("nbmi_get_tidal_f64: a kernel launch failed")) return rc;
    } else {
        const int rc = side_tree(s, true, false, true, false, [&] {
            with_bool(s->multipole == NBMI_MULTIPOLE_QUADRUPOLE, [&](auto q) {
                k_tidal_bodies<decltype(q)::value><<<nblocks(n), kBlock, 0, st>>>(
                    s->nodes, s->diag_pot, s->wtab, s->info, s->posm_s, s->perm, s->curbuf, (float)eps2, n, s->buf[s->curbuf].id,
                    tidal6 ? d_t6 : nullptr, norm ? d_norm : nullptr, decltype(q)::value ? s->quad_work : nullptr);
            });
            return launch_failed("nbmi_get_tidal_f64: a kernel launch failed");
        });
        if (rc) return rc;
    }
    if (tidal6) NBMI_HIP_CHECK(hipMemcpyAsync(tidal6, d_t6, (size_t)n * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (norm) NBMI_HIP_CHECK(hipMemcpyAsync(norm, d_norm, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

namespace {
// Gives back every array of the tracers.  The steps enqueue work on them without waiting: the device is waited for first.
int tracers_release(nbmi_sim *s) {
    auto &t = s->tr;
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    dev_free(s, &t.p); dev_free(s, &t.v); dev_free(s, &t.a); dev_free(s, &t.pmax);
    probe_free(s, t);
    t.m = 0;
    t.acc_valid = false;
    return 0;
}
}  // namespace

int nbmi_set_tracers(nbmi_sim *s, int64_t m, const double *positions_xyz, const double *velocities_xyz) {
    if (int rc = check_handle(s)) return rc;
    if (int rc = diag_refuse(s, "nbmi_set_tracers")) return rc;
    if (m < 0 || m > kTracerMax) {
        nbmi::set_error(m < 0 ? "nbmi_set_tracers: m = %lld is negative" : "nbmi_set_tracers: m = %lld is above the largest accepted, %lld",
                        (long long)m, (long long)kTracerMax);
        return NBMI_ERR_ARG;
    }
    double pmax = 0.0;
    if (m > 0) {
        if (int rc = require_out(positions_xyz, "nbmi_set_tracers: null positions_xyz")) return rc;
        const int64_t bp = first_bad_row(positions_xyz, m, 1e18, &pmax);
        if (bp >= 0) {
            nbmi::set_error("nbmi_set_tracers: positions_xyz row %lld holds (%g, %g, %g): coordinates must be finite and at most 1e18 "
                            "in magnitude", (long long)bp, positions_xyz[3 * bp], positions_xyz[3 * bp + 1], positions_xyz[3 * bp + 2]);
            return NBMI_ERR_ARG;
        }
        const int64_t bv = velocities_xyz ? first_bad_row(velocities_xyz, m, 1.7976931348623157e308, nullptr) : -1;
        if (bv >= 0) {
            nbmi::set_error("nbmi_set_tracers: velocities_xyz row %lld holds (%g, %g, %g): velocities must be finite", (long long)bv,
                            velocities_xyz[3 * bv], velocities_xyz[3 * bv + 1], velocities_xyz[3 * bv + 2]);
            return NBMI_ERR_ARG;
        }
    }
    if (int rc = tracers_release(s)) return rc;
    if (m == 0) return 0;
    auto &t = s->tr;
    hipStream_t st = s->stream;
    const size_t bytes = (size_t)m * 3 * sizeof(double);
    const bool tree = !tracers_direct(s);
    int rc = dev_alloc(s, &t.p, 3 * (size_t)m) || dev_alloc(s, &t.v, 3 * (size_t)m) || dev_alloc(s, &t.pmax, 1) ||
                     (tree && !s->diag_pot && dev_alloc(s, &s->diag_pot, s->node_capacity + 2))  // (the steps' builds write it)
                 ? NBMI_ERR_HIP
                 : 0;
    if (rc == 0 && tree) rc = probe_alloc(s, t, m < kFieldChunk ? m : kFieldChunk);
    auto ok = [&](hipError_t e) { if (e != hipSuccess && rc == 0) { nbmi::set_error("nbmi_set_tracers: %s", hipGetErrorString(e)); rc = NBMI_ERR_HIP; } };
    if (rc == 0) {
        ok(hipMemcpyAsync(t.p, positions_xyz, bytes, hipMemcpyHostToDevice, st));
        if (velocities_xyz) ok(hipMemcpyAsync(t.v, velocities_xyz, bytes, hipMemcpyHostToDevice, st));
        else ok(hipMemsetAsync(t.v, 0, bytes, st));
        ok(hipMemcpyAsync(t.pmax, &pmax, sizeof(double), hipMemcpyHostToDevice, st));  // (the bit pattern of the non-negative double)
        ok(hipStreamSynchronize(st));  // the sources are the caller's arrays and a stack object
    }
    if (rc) {
        tracers_release(s);
        return rc;
    }
    t.m = m;
    return 0;
}

int64_t nbmi_tracer_count(nbmi_sim *s) { return s ? s->tr.m : -1; }

int nbmi_get_tracers_f64(nbmi_sim *s, double *positions_xyz, double *velocities_xyz) {
    if (int rc = check_handle(s)) return rc;
    auto &t = s->tr;
    if (t.m == 0) return 0;
    hipStream_t st = s->stream;
    const size_t bytes = (size_t)t.m * 3 * sizeof(double);
    if (positions_xyz) NBMI_HIP_CHECK(hipMemcpyAsync(positions_xyz, t.p, bytes, hipMemcpyDeviceToHost, st));
    if (velocities_xyz) NBMI_HIP_CHECK(hipMemcpyAsync(velocities_xyz, t.v, bytes, hipMemcpyDeviceToHost, st));
    if (int rc = probe_sort_error(s, t, "nbmi_get_tracers_f64: the sort of the tracers failed; the steps since the last synchronisation are invalid"))
        return rc;
    return check_device_error(s);
}

int nbmi_get_tracer_positions_f32(nbmi_sim *s, float *positions_xyz) {
    if (int rc = check_handle(s)) return rc;
    const int64_t m = s->tr.m;
    if (m == 0) return 0;
    if (int rc = require_out(positions_xyz)) return rc;
    // errors of the steps first (and the wait for them), then the rows chunk by chunk through a bounded host buffer
    if (int rc = nbmi_get_tracers_f64(s, nullptr, nullptr)) return rc;
    const int64_t rows = m < kFieldChunk ? m : kFieldChunk;
    std::vector<double> p;
    try {
        p.resize((size_t)rows * 3);
    } catch (const std::exception &) {  // (no exception crosses the C ABI)
        nbmi::set_error("nbmi_get_tracer_positions_f32: no host memory for a buffer of %lld rows", (long long)rows);
        return NBMI_ERR_HIP;
    }
    for (int64_t b = 0; b < m; b += rows) {
        const int64_t mc = m - b < rows ? m - b : rows;
        NBMI_HIP_CHECK(hipMemcpyAsync(p.data(), s->tr.p + 3 * b, (size_t)mc * 3 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
        for (int64_t i = 0; i < 3 * mc; i++) positions_xyz[3 * b + i] = (float)p[(size_t)i];
    }
    return 0;
}

int nbmi_set_color_mode(nbmi_sim *s, int mode, int k, double log10_lo, double log10_hi) {
    if (int rc = check_handle(s)) return rc;
    if (mode != NBMI_COLOR_SPEED && mode != NBMI_COLOR_DENSITY) {
        nbmi::set_error("nbmi_set_color_mode: unknown colour mode %d", mode);
        return NBMI_ERR_ARG;
    }
    if (mode == NBMI_COLOR_DENSITY) {  // (speed mode takes no parameters: k and the range keep their values)
        if (int rc = knn_check(s, k, "nbmi_set_color_mode")) return rc;
        if (!isfinite(log10_lo) || !isfinite(log10_hi) || !(log10_hi > log10_lo)) {
            nbmi::set_error("nbmi_set_color_mode: the log10(rho) range [%g, %g] is not finite with hi > lo", log10_lo, log10_hi);
            return NBMI_ERR_ARG;
        }
        s->color_k = k;
        s->color_lo = log10_lo;
        s->color_hi = log10_hi;
    }
    s->color_mode = mode;
    return 0;
}

int nbmi_get_color_mode(nbmi_sim *s, int *mode, int *k, double *log10_lo, double *log10_hi) {
    if (int rc = check_handle(s)) return rc;
    if (mode) *mode = s->color_mode;
    if (k) *k = s->color_k;
    if (log10_lo) *log10_lo = s->color_lo;
    if (log10_hi) *log10_hi = s->color_hi;
    return 0;
}

int nbmi_tree_stats(nbmi_sim *s, int64_t *num_nodes, int32_t *max_depth, double *bounds) {
    if (int rc = check_handle(s)) return rc;
    if (s->method != NBMI_METHOD_BARNES_HUT) { nbmi::set_error("not a Barnes-Hut handle"); return NBMI_ERR_ARG; }
    if (s->n == 0) {  // reference: empty root leaf, bounds = 0*1.1+10
        if (num_nodes) *num_nodes = 1;
        if (max_depth) *max_depth = 0;
        if (bounds) *bounds = 10.0;
        return 0;
    }
    if (max_depth) {
        int gb = nblocks(s->nt);
        if (gb > 64) gb = 64;
        k_max_level<<<gb, kBlock, 0, s->stream>>>(s->delta, s->nt, s->info);
        NBMI_HIP_CHECK(hipGetLastError());
    }
    TreeInfo h;
    NBMI_HIP_CHECK(hipMemcpyAsync(&h, s->info, sizeof(h), hipMemcpyDeviceToHost, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    if (num_nodes) *num_nodes = h.num_nodes;
    if (max_depth) *max_depth = h.max_level;
    if (bounds) *bounds = h.bounds;
    if (h.error) return capacity_error(s, h.num_nodes, "");
    return 0;
}

// both key getters; `decode`: back to the reference's octant digits where the handle sorts by Hilbert digits
static int get_keys(nbmi_sim *s, uint64_t *key_hi, uint64_t *key_lo, bool decode, const char *what) {
    if (int rc = check_handle(s)) return rc;
    if (s->method != NBMI_METHOD_BARNES_HUT || !s->tree_valid) {
        nbmi::set_error("%s: call nbmi_build_tree first", what);
        return NBMI_ERR_ARG;
    }
    const int64_t n = s->n;
    if (n == 0) return 0;
    uint64_t *o_hi = (uint64_t *)s->stage, *o_lo = o_hi + n;
    k_keys_to_orig<<<nblocks(n), kBlock, 0, s->stream>>>(s->hi_s, s->lo_s, s->perm, s->buf[s->curbuf].id, n, decode && s->hilbert ? 1 : 0, o_hi, o_lo);
    NBMI_HIP_CHECK(hipGetLastError());
    if (key_hi) NBMI_HIP_CHECK(hipMemcpyAsync(key_hi, o_hi, (size_t)n * 8, hipMemcpyDeviceToHost, s->stream));
    if (key_lo) NBMI_HIP_CHECK(hipMemcpyAsync(key_lo, o_lo, (size_t)n * 8, hipMemcpyDeviceToHost, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    return 0;
}
int nbmi_get_keys(nbmi_sim *s, uint64_t *key_hi, uint64_t *key_lo) { return get_keys(s, key_hi, key_lo, true, "nbmi_get_keys"); }
int nbmi_get_sort_keys(nbmi_sim *s, uint64_t *key_hi, uint64_t *key_lo) { return get_keys(s, key_hi, key_lo, false, "nbmi_get_sort_keys"); }

int nbmi_get_order(nbmi_sim *s, int32_t *order) {
    if (int rc = check_handle(s)) return rc;
    if (s->method != NBMI_METHOD_BARNES_HUT || !s->tree_valid) {
        nbmi::set_error("nbmi_get_order: call nbmi_build_tree first");
        return NBMI_ERR_ARG;
    }
    const int64_t n = s->n;
    if (n == 0) return 0;
    if (int rc = require_out(order)) return rc;
    k_order<<<nblocks(n), kBlock, 0, s->stream>>>(s->perm, s->buf[s->curbuf].id, n, (int32_t *)s->stage);
    NBMI_HIP_CHECK(hipGetLastError());
    NBMI_HIP_CHECK(hipMemcpyAsync(order, s->stage, (size_t)n * 4, hipMemcpyDeviceToHost, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    return 0;
}

int nbmi_get_cells(nbmi_sim *s, int32_t *level, uint64_t *key, int64_t capacity) {
    if (int rc = check_handle(s)) return rc;
    if (s->method != NBMI_METHOD_BARNES_HUT || !s->tree_valid) {
        nbmi::set_error("nbmi_get_cells: call nbmi_build_tree first");
        return NBMI_ERR_ARG;
    }
    int64_t nn = 0;
    if (int rc = nbmi_tree_stats(s, &nn, nullptr, nullptr)) return rc;
    if (nn > capacity || !level || !key) {
        nbmi::set_error("nbmi_get_cells: need room for %lld cells", (long long)nn);
        return NBMI_ERR_ARG;
    }
    if (s->n == 0) { level[0] = 0; key[0] = 0; return 0; }
    int32_t *dl = nullptr;
    uint64_t *dk = nullptr;
    NBMI_HIP_CHECK(hipMalloc((void **)&dl, (size_t)nn * 4));
    NBMI_HIP_CHECK(hipMalloc((void **)&dk, (size_t)nn * 8));
    k_cells<<<nblocks(nn), kBlock, 0, s->stream>>>(s->node_ref, s->node_level, s->t_hi, nn, s->hilbert ? 1 : 0, dl, dk);
    hipError_t e1 = hipMemcpyAsync(level, dl, (size_t)nn * 4, hipMemcpyDeviceToHost, s->stream);
    hipError_t e2 = hipMemcpyAsync(key, dk, (size_t)nn * 8, hipMemcpyDeviceToHost, s->stream);
    hipError_t e3 = hipStreamSynchronize(s->stream);
    (void)hipFree(dl);
    (void)hipFree(dk);
    NBMI_HIP_CHECK(e1);
    NBMI_HIP_CHECK(e2);
    NBMI_HIP_CHECK(e3);
    return 0;
}

int nbmi_get_cell_moments(nbmi_sim *s, int32_t *level, uint64_t *key, double *moments6, int64_t capacity) {
    if (int rc = check_handle(s)) return rc;
    if (s->method != NBMI_METHOD_BARNES_HUT || !s->tree_valid || s->multipole != NBMI_MULTIPOLE_QUADRUPOLE) {
        nbmi::set_error("nbmi_get_cell_moments: call nbmi_build_tree in quadrupole mode first");
        return NBMI_ERR_ARG;
    }
    if (int rc = require_out(moments6)) return rc;
    if (int rc = nbmi_get_cells(s, level, key, capacity)) return rc;
    if (s->n == 0) { for (int k = 0; k < 6; k++) moments6[k] = 0.0; return 0; }
    int64_t nn = 0;
    if (int rc = nbmi_tree_stats(s, &nn, nullptr, nullptr)) return rc;
    double *dq = nullptr;
    NBMI_HIP_CHECK(hipMalloc((void **)&dq, (size_t)nn * 48));
    k_quad_export<<<nblocks(nn), kBlock, 0, s->stream>>>(s->nodes, s->nodesq, nn, dq);
    hipError_t e1 = hipMemcpyAsync(moments6, dq, (size_t)nn * 48, hipMemcpyDeviceToHost, s->stream);
    hipError_t e2 = hipStreamSynchronize(s->stream);
    (void)hipFree(dq);
    NBMI_HIP_CHECK(e1);
    NBMI_HIP_CHECK(e2);
    return 0;
}

int nbmi_enable_timers(nbmi_sim *s, int enable) {
    if (int rc = check_handle(s)) return rc;
    s->timers = enable != 0;
    return 0;
}

int nbmi_get_timers(nbmi_sim *s, double *ms5, int64_t *count, int reset) {
    if (int rc = check_handle(s)) return rc;
    if (ms5) memcpy(ms5, s->ms, sizeof(s->ms));
    if (count) *count = s->timed_steps;
    if (reset) {
        memset(s->ms, 0, sizeof(s->ms));
        s->timed_steps = 0;
    }
    return 0;
}

int nbmi_walk_counters(nbmi_sim *s, int64_t *out8 /* 17 entries */) {
    if (int rc = check_handle(s)) return rc;
    int64_t *out3 = out8;
    if (int rc = require_out(out3)) return rc;
    TreeInfo h;
    NBMI_HIP_CHECK(hipMemcpyAsync(&h, s->info, sizeof(h), hipMemcpyDeviceToHost, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    out3[0] = (int64_t)h.wave_visits; out3[1] = (int64_t)h.lane_visits; out3[2] = (int64_t)h.lane_accepts;
    for (int w = 0; w < 4; w++) out8[3 + w] = (int64_t)h.win_miss[w];
    out8[7] = (int64_t)h.jumps;
    for (int x = 0; x < 8; x++) out8[8 + x] = (int64_t)h.xcd_visits[x];
    out8[16] = (int64_t)h.band_visits;
    return 0;
}

// Test hook: the product's k_xcd_bounds with the product's jmax on a caller's table of wave times; no handle, the
// current device.  Refused before anything is allocated or launched, outputs untouched: what the kernel's precondition
// excludes, a launch of 8 jmax workgroups that no int holds, null pointers.
int nbmi_debug_xcd_bounds(int nb, const uint32_t *wave_cycles, int32_t *bounds9, int32_t *jmax_out) {
    if (nb < kXcdMinBlocks || 8 * xcd_jmax(nb) > (int64_t)INT_MAX || !wave_cycles || !bounds9 || !jmax_out) {
        nbmi::set_error("nbmi_debug_xcd_bounds: bad arguments (nb = %d: from %d blocks on, 8 jmax within an int; no null pointer)", nb,
                        kXcdMinBlocks);
        return NBMI_ERR_ARG;
    }
    const int jmax = (int)xcd_jmax(nb);
    unsigned *d_times = nullptr;
    int *d_bounds = nullptr;
    hipStream_t st = nullptr;
    int32_t got[9];
    const int rc = [&]() -> int {
        NBMI_HIP_CHECK(hipMalloc(&d_times, (size_t)nb * 16));
        NBMI_HIP_CHECK(hipMalloc(&d_bounds, 16 * sizeof(int)));
        NBMI_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        NBMI_HIP_CHECK(hipMemcpyAsync(d_times, wave_cycles, (size_t)nb * 16, hipMemcpyHostToDevice, st));
        k_xcd_bounds<<<1, 1024, 0, st>>>(d_times, nb, jmax, d_bounds);
        NBMI_HIP_CHECK(hipGetLastError());
        NBMI_HIP_CHECK(hipMemcpyAsync(got, d_bounds, sizeof(got), hipMemcpyDeviceToHost, st));
        NBMI_HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }();
    if (st) (void)hipStreamDestroy(st);
    if (d_times) (void)hipFree(d_times);
    if (d_bounds) (void)hipFree(d_bounds);
    if (rc) return rc;
    memcpy(bounds9, got, sizeof(got));
    *jmax_out = jmax;
    return 0;
}

// Test hook: what the next balanced walk of this handle will find, and - with a table - the times it is cut from.
int nbmi_debug_wave_times(nbmi_sim *s, const uint32_t *wave_cycles, int64_t count, int32_t *bounds9, int32_t *nb_out,
                          int32_t *jmax_out, int64_t *balanced_walks) {
    if (int rc = check_handle(s)) return rc;
    const char *why = nullptr;
    const int64_t gb64 = (s->n + s->walk_block - 1) / s->walk_block;  // enqueue_walk's gb of a full walk
    if (!bounds9 || !nb_out || !jmax_out || !balanced_walks) why = "null output";
    else if (s->method != NBMI_METHOD_BARNES_HUT) why = "direct N^2 handles have no tree walk";
    else if (s->owner) why = "owner-mode handles are not supported (their walks never run balanced)";
    else if (s->shard_begin != 0 || s->shard_end != s->n) why = "sharded handles are not supported (their walks never run balanced)";
    else if (wave_cycles && s->walk_block != kBlock) why = "the handle's walk block is not 256 threads (its walks never run balanced)";
    else if (wave_cycles && gb64 < kXcdMinBlocks) why = "fewer than 8 walk blocks (balance mode is not used below that)";
    else if (wave_cycles && count != 4 * gb64) why = "count is not 4 times the handle's walk blocks";
    if (why) {
        nbmi::set_error("nbmi_debug_wave_times: %s", why);
        return NBMI_ERR_ARG;
    }
    const int gb = (int)gb64, jmax = (int)xcd_jmax(gb64);
    hipStream_t st = s->stream;
    if (wave_cycles) {
        // as enqueue_walk's first use, with the caller's times for the zeros: behind a cut that is still on the side
        // stream, and the next balanced walk finds nothing pending and bounds made for its gb
        if (s->cut_pending) {
            NBMI_HIP_CHECK(hipStreamWaitEvent(st, s->ev_cut, 0));
            s->cut_pending = false;
        }
        NBMI_HIP_CHECK(hipMemcpyAsync(s->wave_cycles, wave_cycles, (size_t)gb * 16, hipMemcpyHostToDevice, st));
        k_xcd_bounds<<<1, 1024, 0, st>>>(s->wave_cycles, gb, jmax, s->xcd_bounds);
        NBMI_HIP_CHECK(hipGetLastError());
        s->balance_blocks = gb;
    } else if (s->cut_pending) {
        NBMI_HIP_CHECK(hipEventSynchronize(s->ev_cut));  // (stays pending: the next walk's wait finds it complete)
    }
    int32_t got[9];
    for (int k = 0; k < 9; k++) got[k] = -1;  // no cut for this grid yet: the first balanced walk makes one from zeroed times
    if (s->balance_blocks == gb && gb > 0)
        NBMI_HIP_CHECK(hipMemcpyAsync(got, s->xcd_bounds, sizeof(got), hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    memcpy(bounds9, got, sizeof(got));
    *nb_out = gb;
    *jmax_out = jmax;
    *balanced_walks = s->balanced_walks;
    return 0;
}

int nbmi_set_shard(nbmi_sim *s, int64_t begin, int64_t end) {
    if (int rc = check_handle(s)) return rc;
    if (begin < 0 || end < begin || end > s->n) {
        nbmi::set_error("nbmi_set_shard: bad range [%lld,%lld) for n=%lld", (long long)begin, (long long)end, (long long)s->n);
        return NBMI_ERR_ARG;
    }
    if (s->multipole == NBMI_MULTIPOLE_QUADRUPOLE && (begin != 0 || end != s->n)) {
        nbmi::set_error("nbmi_set_shard: quadrupole handles cannot be sharded (the exchange rows carry no second moments)");
        return NBMI_ERR_ARG;
    }
    if (s->integrator == NBMI_INTEGRATOR_LEAPFROG && (begin != 0 || end != s->n)) {
        nbmi::set_error("nbmi_set_shard: leapfrog handles cannot be sharded (the exchange rows carry no acceleration columns)");
        return NBMI_ERR_ARG;
    }
    if (s->tr.m && (begin != 0 || end != s->n)) {
        nbmi::set_error("nbmi_set_shard: handles with tracers cannot be sharded (nbmi_set_tracers: sharded handles are not supported)");
        return NBMI_ERR_ARG;
    }
    s->shard_begin = begin;
    s->shard_end = end;
    // the next walk's maxabs_next may cover the shard only.  Nothing moved, so a built tree stays valid, and acc_valid
    // is moot: a leapfrog handle gets here with the full range only
    s->maxabs_fused = false;
    return 0;
}

int nbmi_export_shard(nbmi_sim *s, void *dev_rows) {
    if (int rc = check_handle(s)) return rc;
    const int64_t c = s->shard_end - s->shard_begin;
    if (c <= 0) return 0;
    if (int rc = require_out(dev_rows, "null device buffer")) return rc;
    k_pack_rows<<<nblocks(c), kBlock, 0, s->stream>>>(s->buf[s->curbuf], s->shard_begin, s->shard_end, (double *)dev_rows);
    NBMI_HIP_CHECK(hipGetLastError());
    if (s->exchange_sync) NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    return 0;
}

int nbmi_import_ranks(nbmi_sim *s, const void *dev_rows, int64_t begin, int64_t end) {
    if (int rc = check_handle(s)) return rc;
    if (begin < 0 || end < begin || end > s->n) { nbmi::set_error("nbmi_import_ranks: bad range"); return NBMI_ERR_ARG; }
    const int64_t c = end - begin;
    if (c == 0) return 0;
    if (int rc = require_out(dev_rows, "null device buffer")) return rc;
    k_unpack_rows<<<nblocks(c), kBlock, 0, s->stream>>>(s->buf[s->curbuf], begin, end, (const double *)dev_rows);
    NBMI_HIP_CHECK(hipGetLastError());
    if (s->exchange_sync) NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    // rows of the state were replaced.  acc_valid is left alone: leapfrog handles are never sharded (nbmi_set_shard), and
    // the exchange is the sharded protocol
    s->maxabs_fused = false;
    s->tree_valid = false;
    return 0;
}

// =========================================================================================
// Owner mode (multi-GPU stage 2).  See include/nbmi.h for the per-step protocol.
// =========================================================================================
namespace {
int owner_check(nbmi_sim *s, const char *what) {
    if (int rc = check_handle(s)) return rc;
    if (!s->owner) {
        nbmi::set_error("%s: not an owner-mode handle (nbmi_create_owner)", what);
        return NBMI_ERR_ARG;
    }
    return 0;
}
// `batch` arrays of n (+1 output) entries, `stride` apart
int enqueue_iscan(nbmi_sim *s, const int32_t *in, int64_t n, int32_t *out, int batch = 1, int64_t stride = 0) {
    const int64_t ntiles = (n + 1 + kScanTile - 1) / kScanTile;
    const int64_t tstride = s->let_tile_stride;
    const dim3 grid((unsigned)ntiles, (unsigned)batch);
    k_iscan_reduce<<<grid, kBlock, 0, s->stream>>>(in, n, stride, s->let_tiles, tstride);
    scan::k_scan_values<<<dim3(1, (unsigned)batch), scan::kScanThreads, 0, s->stream>>>(s->let_tiles, s->let_tiles, ntiles,
                                                                                        tstride, 0, scan::Sum());
    k_iscan_apply<<<grid, kBlock, 0, s->stream>>>(in, n, stride, s->let_tiles, tstride, out);
    NBMI_HIP_CHECK(hipGetLastError());
    return 0;
}
}  // namespace

nbmi_sim *nbmi_create_owner(int64_t n, const double *pos, const double *vel, const double *mass, const int32_t *ids,
                            int64_t capacity, int64_t let_capacity, int world, int rank, double G, double softening,
                            double damping, double theta, int device) {
    nbmi::clear_error();
    if (n < 0 || capacity < n || capacity < 1 || capacity > kMaxBodies || (n > 0 && (!pos || !vel || !mass || !ids)) ||
        world < 1 || world > kMaxWorld || rank < 0 || rank >= world || let_capacity < 0 || !(softening >= 0.0) ||
        !(theta >= 0.0)) {
        nbmi::set_error("nbmi_create_owner: bad arguments (n=%lld, capacity=%lld, world=%d, rank=%d)", (long long)n,
                        (long long)capacity, world, rank);
        return nullptr;
    }
    const int count = nbmi_device_count();
    if (count <= 0 || device < 0 || device >= count) {
        nbmi::set_error("nbmi_create_owner: no HIP device %d (have %d)", device, count);
        return nullptr;
    }
    nbmi_sim *s = new nbmi_sim();
    s->n = n; s->cap = capacity; s->method = NBMI_METHOD_BARNES_HUT; s->device = device;
    s->G = G; s->softening = softening; s->damping = damping; s->theta = theta;
    s->owner = true; s->world = world; s->rank = rank;
    s->max_gm = largest_gm(G, mass, n);  // (the rank's own bodies at creation)
    s->let_capacity = let_capacity;
    // the own tree sits in the MIDDLE of the walk array: room for received pieces in front of it (lower ranks) and
    // behind it (higher ranks), a jump node at row 0
    s->node_extra = world > 1 ? 2 * let_capacity + 2 : 0;
    s->own_base = world > 1 ? let_capacity + 1 : 0;
    read_env_knobs(s);
    int rc = create_impl(s, pos, vel, mass);
    if (rc == 0) {
        const int64_t c = s->cap;
        // per-destination work arrays over the OWN tree's rows (diff / scan / keep), one row set per rank
        s->let_stride = s->own_node_rows + 8;
        s->let_tile_stride = s->let_stride / kScanTile + 4;
        const size_t all = (size_t)s->let_stride * world;
        if (dev_alloc(s, &s->let_split, kMaxWorld) || dev_alloc(s, &s->let_dest, c) ||
            dev_alloc(s, &s->let_counts, 2 * kMaxWorld) || dev_alloc(s, &s->let_dead, c) ||
            dev_alloc(s, &s->let_diff, all) || dev_alloc(s, &s->let_scan, all) || dev_alloc(s, &s->let_keep, all) ||
            dev_alloc(s, &s->let_tiles, (size_t)s->let_tile_stride * world) || dev_alloc(s, &s->let_ranges, 2 * kBoxesPerRank) ||
            dev_alloc(s, &s->let_supers, (size_t)6 * kSupersPerRank * kMaxWorld) ||
            dev_alloc(s, &s->let_megas, (size_t)6 * kMegasPerRank * kMaxWorld) || dev_alloc(s, &s->let_rankbox, 6 * kMaxWorld) ||
            dev_alloc(s, &s->chain_r, kChainLevels) || dev_alloc(s, &s->own_links, kOwnLinks))
            rc = -2;
        if (rc == 0 && (hipHostMalloc((void **)&s->h_info, sizeof(TreeInfo)) != hipSuccess || hipEventCreate(&s->ev_info) != hipSuccess ||
                        hipMemsetAsync(s->let_dead, 0, (size_t)c, s->stream) != hipSuccess)) {
            nbmi::set_error("nbmi_create_owner: host buffer / event allocation failed");
            rc = -2;
        }
    }
    if (rc == 0 && n > 0) {  // global ids instead of the row numbers k_split_state wrote
        hipError_t e = hipMemcpyAsync(s->stage, ids, (size_t)n * 4, hipMemcpyHostToDevice, s->stream);
        if (e == hipSuccess) {
            k_copy_ids<<<nblocks(n), kBlock, 0, s->stream>>>((const int32_t *)s->stage, s->buf[0].id, n);
            e = hipStreamSynchronize(s->stream);
        }
        if (e != hipSuccess) { nbmi::set_error("nbmi_create_owner: id upload failed: %s", hipGetErrorString(e)); rc = -2; }
    }
    if (rc != 0) return create_failed(s);
    return s;
}

int64_t nbmi_owner_count(nbmi_sim *s) { return s ? s->n : -1; }
int nbmi_owner_boxes_per_rank(void) { return kBoxesPerRank; }

int nbmi_owner_get_ids(nbmi_sim *s, int32_t *out) {
    if (int rc = owner_check(s, "nbmi_owner_get_ids")) return rc;
    if (s->n == 0) return 0;
    if (int rc = require_out(out)) return rc;
    NBMI_HIP_CHECK(hipMemcpyAsync(out, s->buf[s->curbuf].id, (size_t)s->n * 4, hipMemcpyDeviceToHost, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    return 0;
}

int nbmi_owner_maxabs(nbmi_sim *s, void *dev_maxabs) {
    if (int rc = owner_check(s, "nbmi_owner_maxabs")) return rc;
    if (int rc = require_out(dev_maxabs, "nbmi_owner_maxabs: null buffer")) return rc;
    if (int rc = enqueue_maxabs(s)) return rc;  // also clears the per-step tree header
    // a non-negative double and its bit pattern order the same way: the word IS the double
    NBMI_HIP_CHECK(hipMemcpyAsync(dev_maxabs, &s->info->maxabs_bits, 8, hipMemcpyDeviceToDevice, s->stream));
    if (s->exchange_sync) NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));  // (stream-ordered callers: nbmi_set_exchange_sync(0))
    return 0;
}

int nbmi_owner_sample(nbmi_sim *s, const void *dev_maxabs, void *dev_samples, int nsamples, int nvalid) {
    if (int rc = owner_check(s, "nbmi_owner_sample")) return rc;
    if (!dev_maxabs || !dev_samples || nsamples < 1 || (int64_t)nsamples * s->world > kSampleCap) {
        nbmi::set_error("nbmi_owner_sample: bad arguments (at most %d samples over all ranks)", kSampleCap);
        return NBMI_ERR_ARG;
    }
    hipStream_t st = s->stream;
    NBMI_HIP_CHECK(hipMemcpyAsync(&s->info->maxabs_bits, dev_maxabs, 8, hipMemcpyDeviceToDevice, st));
    if (s->world == 1) return 0;  // one owner: no splitters to find (nbmi_owner_adopt computes the keys it sorts by)
    Bodies cur = s->buf[s->curbuf];
    if (s->n > 0 && s->hilbert) k_keys<true><<<nblocks(s->n), kBlock, 0, st>>>(cur.x, cur.y, cur.z, s->n, s->info, s->key_hi, s->key_lo, s->idx);
    else if (s->n > 0) k_keys<false><<<nblocks(s->n), kBlock, 0, st>>>(cur.x, cur.y, cur.z, s->n, s->info, s->key_hi, s->key_lo, s->idx);
    if (nvalid < 1 || nvalid > nsamples) nvalid = nsamples;
    k_key_samples<<<(nsamples + kBlock - 1) / kBlock, kBlock, 0, st>>>(s->key_hi, s->n, nsamples, nvalid, (uint64_t *)dev_samples);
    NBMI_HIP_CHECK(hipGetLastError());
    if (s->exchange_sync) NBMI_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

int nbmi_owner_partition(nbmi_sim *s, const void *dev_all_samples, int total_samples, void *dev_send_rows,
                         int64_t *counts /* world, host */) {
    if (int rc = owner_check(s, "nbmi_owner_partition")) return rc;
    if (!dev_all_samples || !counts || total_samples < 1 || total_samples > kSampleCap || (s->n > 0 && !dev_send_rows)) {
        nbmi::set_error("nbmi_owner_partition: bad arguments");
        return NBMI_ERR_ARG;
    }
    hipStream_t st = s->stream;
    const int64_t n = s->n, stride = s->let_stride;
    const int W = s->world;
    for (int j = 0; j < W; j++) counts[j] = 0;
    if (W == 1) {  // nobody to hand bodies to (the dead flags stay clear)
        s->n_leaving = 0;
        return 0;
    }
    k_splitters<<<(total_samples + kBlock - 1) / kBlock, kBlock, 0, st>>>((const uint64_t *)dev_all_samples, total_samples, W, s->let_split);
    if (n > 0) {
        // only the bodies whose key has left this rank's range travel; everybody else stays where it is
        k_dest<<<nblocks(n), kBlock, 0, st>>>(s->key_hi, n, s->let_split, W, s->let_dest, s->idx);
        k_emigrant_flags<<<nblocks(n), kBlock, 0, st>>>(s->let_dest, n, W, s->rank, stride, s->let_keep, s->let_dead);
        if (int rc = enqueue_iscan(s, s->let_keep, n, s->let_scan, W, stride)) return rc;
        k_let_counts<<<1, 64, 0, st>>>(s->let_scan, n, stride, W, s->rank, s->let_counts);
        k_pack_emigrants<<<nblocks(n), kBlock, 0, st>>>(s->buf[s->curbuf], s->let_dest, n, s->rank, stride, s->let_scan,
                                                       s->let_counts + W, (double *)dev_send_rows);
        NBMI_HIP_CHECK(hipGetLastError());
        NBMI_HIP_CHECK(hipMemcpyAsync(counts, s->let_counts, (size_t)W * 8, hipMemcpyDeviceToHost, st));
    }
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    int64_t left = 0;
    for (int j = 0; j < W; j++) left += counts[j];
    s->n_leaving = left;
    return 0;
}

int nbmi_owner_chain_doubles(void) { return kChainDoubles; }

int nbmi_owner_adopt(nbmi_sim *s, const void *dev_recv_rows, int64_t n_recv, const void *dev_maxabs, void *dev_boxes,
                     void *dev_chain) {
    if (int rc = owner_check(s, "nbmi_owner_adopt")) return rc;
    const int64_t n_old = s->n, n_work = n_old + n_recv, n_new = n_old - s->n_leaving + n_recv;
    if (n_recv < 0 || n_work > s->cap) {
        nbmi::set_error("nbmi_owner_adopt: %lld + %lld bodies do not fit the capacity of %lld (raise the head room)",
                        (long long)n_old, (long long)n_recv, (long long)s->cap);
        return NBMI_ERR_CAPACITY;
    }
    if ((n_recv > 0 && !dev_recv_rows) || !dev_maxabs || !dev_boxes || (s->world > 1 && !dev_chain)) {
        nbmi::set_error("nbmi_owner_adopt: null buffer");
        return NBMI_ERR_ARG;
    }
    hipStream_t st = s->stream;
    Bodies cur = s->buf[s->curbuf];
    // immigrants go behind the rows already here; the emigrants' rows stay in place, flagged dead
    if (n_recv > 0) {
        k_unpack_rows<<<nblocks(n_recv), kBlock, 0, st>>>(cur, n_old, n_work, (const double *)dev_recv_rows);
        NBMI_HIP_CHECK(hipMemsetAsync(s->let_dead + n_old, 0, (size_t)n_recv, st));
    }
    s->n = n_new; s->nt = n_new; s->shard_begin = 0; s->shard_end = n_new;
    s->n_leaving = 0;
    // the tree header of this step: cleared, then the GLOBAL extent (every rank builds inside the same root cube)
    NBMI_HIP_CHECK(hipMemsetAsync(s->info, 0, offsetof(TreeInfo, wave_visits), st));
    NBMI_HIP_CHECK(hipMemcpyAsync(&s->info->maxabs_bits, dev_maxabs, 8, hipMemcpyDeviceToDevice, st));
    const DtScope dt_scope(s, s->owner_dt);
    if (n_new > 0 && s->world == 1) {
        // one owner: the plain build (no dead rows, no boxes to publish)
        if (int rc = enqueue_local_sort(s)) return rc;
        if (int rc = enqueue_global_tree(s, false)) return rc;
    } else if (n_new > 0) {
        // rank of every dead row among the dead rows (exclusive scan of the flags): their place behind the live ones
        k_dead_flags<<<nblocks(n_work), kBlock, 0, st>>>(s->let_dead, n_work, s->let_keep);
        if (int rc = enqueue_iscan(s, s->let_keep, n_work, s->let_scan)) return rc;
        SortRequest sort;
        sort.n_sort = n_work; sort.n_live = n_new; sort.dead = s->let_dead;
        if (int rc = enqueue_local_sort(s, sort)) return rc;
        if (int rc = enqueue_global_tree(s)) return rc;
        // where this rank's bodies are: boxes of the cells of its tree (see k_box_flags).  The node count lives on
        // the device: launch for the row budget, the kernels stop at num_nodes themselves.
        const int64_t rows = s->own_node_rows, ob = s->own_base;
        NBMI_HIP_CHECK(hipMemsetAsync(s->chain_r, 0xff, sizeof(int32_t) * kChainLevels, st));
        k_box_flags<<<nblocks(rows), kBlock, 0, st>>>(s->nodes + ob, s->node_level, s->node_ref, s->hi_s, s->lo_s, s->info, n_new, rows, s->let_keep,
                                                     s->chain_r, ob);
        if (int rc = enqueue_iscan(s, s->let_keep, rows, s->let_scan)) return rc;
        NBMI_HIP_CHECK(hipMemsetAsync(s->let_ranges, 0, sizeof(int32_t) * 2 * kBoxesPerRank, st));
        k_box_ranges<<<nblocks(rows), kBlock, 0, st>>>(s->nodes + ob, s->node_ref, s->let_keep, s->let_scan, s->info, rows, n_new, s->let_ranges, ob);
        // what the other ranks need to know about this rank's two ends (travels with the boxes)
        k_chain_table<<<1, 64, 0, st>>>(s->nodes + ob, s->node_ref, s->delta, s->S, s->T, s->hi_s, s->lo_s, n_new, s->info, s->chain_r, ob,
                                        (ChainTable *)dev_chain);
        k_boxes_init<<<(6 * kBoxesPerRank + kBlock - 1) / kBlock, kBlock, 0, st>>>((double *)dev_boxes);
        k_range_boxes<<<(unsigned)((n_new + (int64_t)kBoxChunk * (kBlock / 64) - 1) / ((int64_t)kBoxChunk * (kBlock / 64))), kBlock, 0, st>>>(
            s->p64_s, s->let_ranges, s->let_scan + rows, n_new, (double *)dev_boxes);
    } else {
        std::vector<double> empty(6 * kBoxesPerRank);
        for (int k = 0; k < 6 * kBoxesPerRank; k++) empty[k] = (k % 6) < 3 ? INFINITY : -INFINITY;
        NBMI_HIP_CHECK(hipMemcpyAsync(dev_boxes, empty.data(), empty.size() * 8, hipMemcpyHostToDevice, st));
        if (dev_chain) NBMI_HIP_CHECK(hipMemsetAsync(dev_chain, 0, sizeof(ChainTable), st));  // n = 0: no bodies, no part in the tree
        NBMI_HIP_CHECK(hipStreamSynchronize(st));  // `empty` dies here
    }
    NBMI_HIP_CHECK(hipGetLastError());
    // the tree header travels to the host behind the build; nbmi_owner_export_let / _step read it after their own wait
    NBMI_HIP_CHECK(hipMemcpyAsync(s->h_info, s->info, sizeof(TreeInfo), hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipEventRecord(s->ev_info, st));
    if (s->exchange_sync) NBMI_HIP_CHECK(hipStreamSynchronize(st));
    s->tree_valid = n_new > 0 && s->world > 1;
    return 0;
}

// the float64 records as the exchange sees them: present whenever the handle's trees carry them
static inline NodeD *let_nodesd(const nbmi_sim *s) { return s->force_prec != 1 ? s->nodesd : nullptr; }
int nbmi_owner_let_row_bytes(void) { return kLetRow; }

int nbmi_owner_set_dt(nbmi_sim *s, double dt) {
    if (int rc = owner_check(s, "nbmi_owner_set_dt")) return rc;
    if (!(dt >= 0.0)) { nbmi::set_error("nbmi_owner_set_dt: dt must be >= 0"); return NBMI_ERR_ARG; }
    s->owner_dt = dt;
    return 0;
}

int nbmi_owner_export_let(nbmi_sim *s, const void *dev_boxes, const void *dev_chains, void *dev_let, int64_t *counts /* world, host */) {
    if (int rc = owner_check(s, "nbmi_owner_export_let")) return rc;
    if (!dev_boxes || !dev_let || !counts || (s->world > 1 && !dev_chains)) { nbmi::set_error("nbmi_owner_export_let: null buffer"); return NBMI_ERR_ARG; }
    s->chains = (const ChainTable *)dev_chains;
    for (int j = 0; j < s->world; j++) counts[j] = 0;
    if (s->n == 0 || s->world == 1) return 0;
    hipStream_t st = s->stream;
    const int64_t stride = s->let_stride, ob = s->own_base;
    const int W = s->world;
    const ChainTable *T = s->chains;
    // the own tree becomes this rank's piece of the global pre-order array (a few nodes change; up to 43 are added)
    k_chain_fix<<<1, 64, 0, st>>>(T, W, s->rank, s->nodes + ob, s->nodes64 + ob, let_nodesd(s) ? let_nodesd(s) + ob : nullptr, s->node_level,
                                  s->node_ref, s->chain_r, s->theta > 0.0 ? 1.0 / (s->theta * s->theta) : INFINITY, s->own_node_rows,
                                  s->own_links, s->info);
    NBMI_HIP_CHECK(hipMemcpyAsync(s->h_info, s->info, sizeof(TreeInfo), hipMemcpyDeviceToHost, st));  // (read after the wait below)
    // How many nodes the own tree has is known on the device; the host needs a launch bound.  The previous step's
    // count + 2 % is one (a tree changes by a few nodes in a thousand per step): no wait for this step's header
    // before the kernels are enqueued, ONE wait at the end for the counts - and the header, which says whether the
    // bound held (if not: once more with the exact count).
    int64_t nn = -1;
    if (s->last_nodes > 0 && !s->exchange_sync) {
        nn = s->last_nodes + s->last_nodes / 50 + 4096;  // (covers the handful of cells k_chain_fix adds)
        if (nn > s->own_node_rows) nn = s->own_node_rows;
        if (getenv("NBMI_LET_UNDERESTIMATE")) nn = s->last_nodes / 2;  // test hook: forces the "bound did not hold" repeat
    }
    for (int attempt = 0; attempt < 2; attempt++) {
        if (nn < 0) {
            NBMI_HIP_CHECK(hipStreamSynchronize(st));  // this step's header, behind k_chain_fix
            if (s->h_info->error) return check_device_error(s);
            nn = s->h_info->num_nodes;
        }
        NBMI_HIP_CHECK(hipMemsetAsync(s->let_diff, 0, (size_t)stride * W * 4, st));
        k_super_boxes<<<(W * kSupersPerRank + 63) / 64, 64, 0, st>>>((const double *)dev_boxes, W * kSupersPerRank, s->let_supers);
        k_rank_boxes<<<1, kMaxWorld * kMegasPerRank, 0, st>>>(s->let_supers, W, s->let_megas, s->let_rankbox);
        k_let_mark<<<nblocks(nn), kBlock, 0, st>>>(s->nodes + ob, s->nodes64 + ob, nn, (const double *)dev_boxes, s->let_supers, s->let_megas,
                                                  s->let_rankbox, W, s->rank, s->theta, s->softening * s->softening, s->let_diff, stride,
                                                  s->info, ob);
        k_let_mark_left<<<W, 64, 0, st>>>(T, W, s->rank, (const double *)dev_boxes, s->let_supers, s->let_megas, s->let_rankbox, s->theta,
                                          s->softening * s->softening, s->let_diff, stride, s->info);
        if (int rc = enqueue_iscan(s, s->let_diff, nn, s->let_scan, W, stride)) return rc;
        k_let_keep<<<dim3((unsigned)nblocks(nn), (unsigned)W), kBlock, 0, st>>>(s->let_diff, s->let_scan, nn, stride, s->let_keep, s->info);
        if (int rc = enqueue_iscan(s, s->let_keep, nn, s->let_scan, W, stride)) return rc;
        k_let_counts<<<1, 64, 0, st>>>(s->let_scan, nn, stride, W, s->rank, s->let_counts);
        k_let_compact<<<dim3((unsigned)nblocks(nn), (unsigned)W), kBlock, 0, st>>>(s->nodes + ob, s->nodes64 + ob, let_nodesd(s) ? let_nodesd(s) + ob : nullptr,
                                                                                s->node_level, s->own_links, T, s->let_keep, s->let_scan, nn, stride,
                                                                                s->let_capacity, s->rank, s->let_counts + W, (char *)dev_let,
                                                                                s->info, ob);
        NBMI_HIP_CHECK(hipGetLastError());
        NBMI_HIP_CHECK(hipMemcpyAsync(counts, s->let_counts, (size_t)W * 8, hipMemcpyDeviceToHost, st));
        NBMI_HIP_CHECK(hipStreamSynchronize(st));  // the one wait: counts + (long since) this step's header
        if (s->h_info->error) return check_device_error(s);
        if (s->h_info->num_nodes <= nn) break;
        nn = s->h_info->num_nodes;  // the estimate was too small: the exact count now
    }
    s->last_nodes = s->h_info->num_nodes;
    int64_t total = 0;
    for (int j = 0; j < W; j++) total += counts[j];
    if (total > s->let_capacity) {
        nbmi::set_error("nbmi_owner_export_let: the trees for the other ranks have %lld nodes, more than the %lld rows reserved",
                        (long long)total, (long long)s->let_capacity);
        return NBMI_ERR_CAPACITY;
    }
    return 0;
}

int nbmi_owner_step_facts(nbmi_sim *s, int64_t *out4) {
    if (int rc = owner_check(s, "nbmi_owner_step_facts")) return rc;
    if (int rc = require_out(out4, "nbmi_owner_step_facts: null output")) return rc;
    out4[0] = out4[1] = 0;
    out4[2] = out4[3] = (int64_t)1 << 62;
    if (s->n == 0 || s->world == 1 || !s->h_info) return 0;
    NBMI_HIP_CHECK(hipEventSynchronize(s->ev_info));  // (long complete: nbmi_owner_export_let waited behind it)
    const TreeInfo &h = *s->h_info;
    if (s->force_prec == 0 && s->nodesd && s->owner_dt > 0.0) { out4[0] = h.ask_waves; out4[1] = h.n_waves; }
    out4[2] = s->own_base + h.own_skip - 1;                        // tree rows that fit in front of the own piece
    out4[3] = s->node_capacity - (s->own_base + h.num_nodes) - 1;  // ... and behind it
    return 0;
}

int nbmi_owner_set_all64(nbmi_sim *s, int verdict) {
    if (int rc = owner_check(s, "nbmi_owner_set_all64")) return rc;
    s->owner_all64 = verdict < 0 ? -1 : (verdict ? 1 : 0);
    return 0;
}

int nbmi_owner_step(nbmi_sim *s, const void *dev_recv, const int64_t *counts, double dt) {
    if (int rc = owner_check(s, "nbmi_owner_step")) return rc;
    if (!counts || (s->world > 1 && !dev_recv)) { nbmi::set_error("nbmi_owner_step: null buffer"); return NBMI_ERR_ARG; }
    if (s->n == 0) return 0;
    hipStream_t st = s->stream;
    if (s->owner_all64 >= 0) k_set_all64<<<1, 1, 0, st>>>(s->info, s->owner_all64);  // the ranks' common verdict
    if (s->world == 1) {  // nothing received: the walk array is the own tree; an overflow freezes the walk and is reported at the next sync
        k_let_finish_alone<<<1, 1, 0, st>>>(s->info);
        NBMI_HIP_CHECK(hipGetLastError());
        if (int rc = enqueue_walk(s, true, dt, nullptr)) return rc;
        s->curbuf ^= 1;
        s->tree_valid = false;
        s->maxabs_fused = s->fuse_maxabs;  // the walk left max |coordinate| of what it wrote
        return 0;
    }
    if (!s->chains) { nbmi::set_error("nbmi_owner_step: call nbmi_owner_export_let first (it cuts the own tree to its piece of the global one)"); return NBMI_ERR_ARG; }
    NBMI_HIP_CHECK(hipEventSynchronize(s->ev_info));  // (long complete: nbmi_owner_export_let waited behind it)
    const TreeInfo &h = *s->h_info;  // as nbmi_owner_export_let left it: the own piece in its global form
    if (h.error) return check_device_error(s);
    // the pieces in rank order: lower ranks packed up against the own piece, higher ranks behind it (see Pieces)
    Pieces P;
    const int W = s->world, me = s->rank;
    int64_t lower = 0, upper = 0, seen = 0;
    for (int j = 0; j < W; j++) {
        if (j == me || counts[j] <= 0) continue;
        if (j < me) lower += counts[j]; else upper += counts[j];
    }
    const int64_t own_first = s->own_base + h.own_skip, own_end = s->own_base + h.num_nodes;
    if (lower + 1 > own_first || own_end + upper + 1 > s->node_capacity) {
        nbmi::set_error("nbmi_owner_step: received trees do not fit (%lld rows in front of / %lld behind the own %lld of %lld rows)",
                        (long long)lower, (long long)upper, (long long)h.num_nodes, (long long)s->node_capacity);
        return NBMI_ERR_CAPACITY;
    }
    const int64_t walk_first = own_first - lower;
    int64_t at_lo = walk_first, at_hi = own_end;
    for (int j = 0; j < kMaxWorld; j++) { P.src[j] = nullptr; P.count[j] = 0; P.base[j] = 0; }
    for (int j = 0; j < W; j++) {
        if (j == me) { P.base[j] = own_first; continue; }
        const int64_t c = counts[j] > 0 ? counts[j] : 0;
        P.src[j] = (const char *)dev_recv + seen * kLetRow;
        P.count[j] = c;
        if (j < me) { P.base[j] = at_lo; at_lo += c; } else { P.base[j] = at_hi; at_hi += c; }
        seen += c;
    }
    P.total = at_hi;
    P.me = me;
    NodeD *nd = let_nodesd(s);
    for (int j = 0; j < W; j++) {
        if (j == me || P.count[j] == 0) continue;
        k_let_append<<<nblocks(P.count[j]), kBlock, 0, st>>>(P, j, s->nodes, s->nodes64, nd, s->info);
    }
    k_let_finish<<<1, 64, 0, st>>>(P, s->own_links, s->chains, s->own_base, walk_first, s->nodes, nd, s->info);
    NBMI_HIP_CHECK(hipGetLastError());
    if (int rc = enqueue_walk(s, true, dt, nullptr)) return rc;
    s->curbuf ^= 1;
    s->tree_valid = false;
    s->maxabs_fused = s->fuse_maxabs;  // the walk left max |coordinate| of the rows it wrote (all of this rank's live bodies)
    return 0;
}

// ---- frame codec ----------------------------------------------------------------
namespace {
int frame_current(nbmi_sim *s, float **d_pos) {  // float32 positions in the caller's order, in `stage`
    const int64_t n = s->n;
    Bodies cur = s->buf[s->curbuf];
    float *dp = (float *)s->stage;
    k_unperm3_f32<<<nblocks(n), kBlock, 0, s->stream>>>(cur.x, cur.y, cur.z, s->owner ? nullptr : cur.id, n, dp);
    NBMI_HIP_CHECK(hipGetLastError());
    *d_pos = dp;
    return 0;
}
int frame_alloc(nbmi_sim *s) {
    if (s->frame_prev) return 0;
    const int64_t c = s->cap > s->n ? s->cap : s->n;
    if (dev_alloc(s, &s->frame_prev, (size_t)6 * (c ? c : 1)) || dev_alloc(s, &s->frame_q, (size_t)6 * (c ? c : 1))) return NBMI_ERR_HIP;
    return 0;
}
}  // namespace

int nbmi_frame_keyframe(nbmi_sim *s, float *out_pos, float *out_col) {
    if (int rc = check_handle(s)) return rc;
    const int64_t n = s->n;
    if (n == 0) return 0;
    if (!out_pos || !out_col) { nbmi::set_error("nbmi_frame_keyframe: null output"); return NBMI_ERR_ARG; }
    if (int rc = frame_alloc(s)) return rc;
    float *dp = nullptr;
    if (int rc = frame_current(s, &dp)) return rc;
    hipStream_t st = s->stream;
    NBMI_HIP_CHECK(hipMemcpyAsync(s->frame_prev, dp, (size_t)n * 12, hipMemcpyDeviceToDevice, st));
    NBMI_HIP_CHECK(hipMemcpyAsync(s->frame_prev + 3 * n, s->colors, (size_t)n * 12, hipMemcpyDeviceToDevice, st));
    NBMI_HIP_CHECK(hipMemcpyAsync(out_pos, dp, (size_t)n * 12, hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipMemcpyAsync(out_col, s->colors, (size_t)n * 12, hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    s->frame_have_prev = true;
    return check_device_error(s);
}

int nbmi_frame_delta_i16(nbmi_sim *s, int16_t *out_dpos, int16_t *out_dcol) {
    if (int rc = check_handle(s)) return rc;
    const int64_t n = s->n;
    if (n == 0) return 0;
    if (!out_dpos || !out_dcol) { nbmi::set_error("nbmi_frame_delta_i16: null output"); return NBMI_ERR_ARG; }
    if (!s->frame_have_prev) {
        nbmi::set_error("nbmi_frame_delta_i16: no previous frame on the device (call nbmi_frame_keyframe or "
                        "nbmi_frame_set_previous first)");
        return NBMI_ERR_ARG;
    }
    float *dp = nullptr;
    if (int rc = frame_current(s, &dp)) return rc;
    hipStream_t st = s->stream;
    k_frame_delta<<<nblocks(3 * n), kBlock, 0, st>>>(dp, s->frame_prev, 3 * n, s->frame_q);
    k_frame_delta<<<nblocks(3 * n), kBlock, 0, st>>>(s->colors, s->frame_prev + 3 * n, 3 * n, s->frame_q + 3 * n);
    NBMI_HIP_CHECK(hipGetLastError());
    NBMI_HIP_CHECK(hipMemcpyAsync(out_dpos, s->frame_q, (size_t)n * 6, hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipMemcpyAsync(out_dcol, s->frame_q + 3 * n, (size_t)n * 6, hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    return check_device_error(s);
}

int nbmi_frame_set_previous(nbmi_sim *s, const float *pos, const float *col) {
    if (int rc = check_handle(s)) return rc;
    const int64_t n = s->n;
    if (n == 0) return 0;
    if (!pos || !col) { nbmi::set_error("nbmi_frame_set_previous: null input"); return NBMI_ERR_ARG; }
    if (int rc = frame_alloc(s)) return rc;
    NBMI_HIP_CHECK(hipMemcpyAsync(s->frame_prev, pos, (size_t)n * 12, hipMemcpyHostToDevice, s->stream));
    NBMI_HIP_CHECK(hipMemcpyAsync(s->frame_prev + 3 * n, col, (size_t)n * 12, hipMemcpyHostToDevice, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    s->frame_have_prev = true;
    return 0;
}

// ---- asynchronous frames: snapshot on the compute stream, copy on a stream of its own ------
namespace {
int frame_slots_alloc(nbmi_sim *s) {
    if (s->frame_stream) return 0;
    const size_t bytes = sizeof(FrameHeader) + (size_t)24 * (size_t)(s->n ? s->n : 1);
    for (auto &f : s->frame_slot) {
        if (!f.dev && dev_alloc(s, &f.dev, bytes)) return NBMI_ERR_HIP;
        if (!f.host) NBMI_HIP_CHECK(hipHostMalloc((void **)&f.host, bytes));
        if (!f.ev_snap) NBMI_HIP_CHECK(hipEventCreateWithFlags(&f.ev_snap, hipEventDisableTiming));
        if (!f.ev_done) NBMI_HIP_CHECK(hipEventCreateWithFlags(&f.ev_done, hipEventDisableTiming));
    }
    NBMI_HIP_CHECK(hipStreamCreateWithFlags(&s->frame_stream, hipStreamNonBlocking));
    return 0;
}
int frame_slot_check(nbmi_sim *s, int slot, const char *what) {
    if (slot < 0 || slot >= NBMI_FRAME_SLOTS || !s->frame_slot[slot].begun) {
        nbmi::set_error("%s: slot %d holds no frame (not begun, or already released)", what, slot);
        return NBMI_ERR_ARG;
    }
    return 0;
}
size_t frame_item_bytes(int kind) { return kind == NBMI_FRAME_DELTA_I16 ? 6 : 12; }  // per body and array
}  // namespace

int nbmi_frame_begin(nbmi_sim *s, int kind, double max_speed, int *slot) {
    if (int rc = check_handle(s)) return rc;
    if (int rc = require_out(slot, "nbmi_frame_begin: null output")) return rc;
    if (s->owner) { nbmi::set_error("nbmi_frame_begin: not available on an owner-mode handle"); return NBMI_ERR_ARG; }
    if (kind != NBMI_FRAME_F32 && kind != NBMI_FRAME_KEY && kind != NBMI_FRAME_DELTA_I16) {
        nbmi::set_error("nbmi_frame_begin: unknown kind %d", kind);
        return NBMI_ERR_ARG;
    }
    const int64_t n = s->n;
    if (kind == NBMI_FRAME_DELTA_I16 && !s->frame_have_prev && n != 0) {
        nbmi::set_error("nbmi_frame_begin: no previous frame on the device (call nbmi_frame_keyframe or "
                        "nbmi_frame_set_previous first)");
        return NBMI_ERR_ARG;
    }
    int k = -1;
    for (int i = 0; i < NBMI_FRAME_SLOTS && k < 0; i++)
        if (!s->frame_slot[i].begun) k = i;
    if (k < 0) { nbmi::set_error("nbmi_frame_begin: no free frame slot (release one first)"); return NBMI_ERR_ARG; }
    if (int rc = frame_slots_alloc(s)) return rc;
    if (kind != NBMI_FRAME_F32 && n != 0)
        if (int rc = frame_alloc(s)) return rc;
    nbmi_sim::FrameSlot &f = s->frame_slot[k];
    if (n != 0) {
        // (a slot released without a wait may still be in its copy: the stream waits, the host does not)
        if (f.used) NBMI_HIP_CHECK(hipStreamWaitEvent(s->stream, f.ev_done, 0));
        const size_t item = frame_item_bytes(kind) * (size_t)n;
        FrameHeader *hd = (FrameHeader *)f.dev;
        void *first = f.dev + sizeof(FrameHeader), *second = f.dev + sizeof(FrameHeader) + item;
        const Bodies cur = s->buf[s->curbuf];
        const unsigned *se = s->tmp_sort ? (const unsigned *)nbmi::radix_error_device_word(s->tmp_sort) : nullptr;
        // density colours: the query goes onto the stream in front of the snapshot (enqueued, not waited for; its
        // restored header, a capacity error of its build included, is what the snapshot copies)
        const double *dr2 = nullptr, *dmass = nullptr;
        const double dlo = s->color_lo, dhi = s->color_hi;
        if (s->color_mode == NBMI_COLOR_DENSITY) {
            if (int rc = knn_check(s, s->color_k, "nbmi_frame_begin")) return rc;
            if (int rc = knn_enqueue(s, s->color_k, false)) return rc;
            dr2 = s->q.knn.r2;
            dmass = s->q.knn.mass;
        }
        // a delta frame's positions go to the staging rows: (like frame_current) nothing later on the stream reads them
        // before writing them
        float *rows = (float *)s->stage;
        with_int<NBMI_FRAME_F32, NBMI_FRAME_KEY, NBMI_FRAME_DELTA_I16>(kind, [&](auto kv) {
            constexpr int kKind = decltype(kv)::value;
            constexpr bool kDelta = kKind == NBMI_FRAME_DELTA_I16;
            k_frame_snapshot<kKind><<<nblocks(n), kBlock, 0, s->stream>>>(
                cur, n, max_speed, s->colors, kKind == NBMI_FRAME_KEY ? s->frame_prev : nullptr, kDelta ? rows : first,
                kDelta ? nullptr : second, s->info, se, hd, dr2, dmass, dlo, dhi);
        });
        if (kind == NBMI_FRAME_DELTA_I16) {
            k_frame_delta<<<nblocks(3 * n), kBlock, 0, s->stream>>>(rows, s->frame_prev, 3 * n, (int16_t *)first);
            k_frame_delta<<<nblocks(3 * n), kBlock, 0, s->stream>>>(s->colors, s->frame_prev + 3 * n, 3 * n, (int16_t *)second);
        }
        NBMI_HIP_CHECK(hipGetLastError());
        NBMI_HIP_CHECK(hipEventRecord(f.ev_snap, s->stream));
        NBMI_HIP_CHECK(hipStreamWaitEvent(s->frame_stream, f.ev_snap, 0));
        NBMI_HIP_CHECK(hipMemcpyAsync(f.host, f.dev, sizeof(FrameHeader) + 2 * item, hipMemcpyDeviceToHost, s->frame_stream));
        NBMI_HIP_CHECK(hipEventRecord(f.ev_done, s->frame_stream));
        f.used = true;
        if (kind == NBMI_FRAME_KEY) s->frame_have_prev = true;
    }
    f.begun = true;
    f.kind = kind;
    f.steps = s->steps_taken;
    f.seq = ++s->frame_seq;
    *slot = k;
    return 0;
}

int nbmi_frame_wait(nbmi_sim *s, int slot, const void **first, const void **second, int *kind, int64_t *steps) {
    if (int rc = check_handle(s)) return rc;
    if (int rc = frame_slot_check(s, slot, "nbmi_frame_wait")) return rc;
    nbmi_sim::FrameSlot &f = s->frame_slot[slot];
    const int64_t n = s->n;
    if (n != 0) {
        NBMI_HIP_CHECK(hipEventSynchronize(f.ev_done));  // this slot's copy only: the compute stream keeps running
        // the words check_device_error reads, as they stood at the snapshot; they stay set on the device, so the next
        // nbmi_sync / getter still reports and clears them
        if (int rc = decode_device_error(s, *(const FrameHeader *)f.host)) return rc;
    }
    const char *base = f.host + sizeof(FrameHeader);
    if (first) *first = base;
    if (second) *second = base + frame_item_bytes(f.kind) * (size_t)n;
    if (kind) *kind = f.kind;
    if (steps) *steps = f.steps;
    return 0;
}

int nbmi_frame_release(nbmi_sim *s, int slot) {
    if (int rc = check_handle(s)) return rc;
    if (int rc = frame_slot_check(s, slot, "nbmi_frame_release")) return rc;
    s->frame_slot[slot].begun = false;
    return 0;
}

int nbmi_frame_pending(nbmi_sim *s, int *slots, int *kinds, int64_t *steps) {
    if (int rc = check_handle(s)) return rc;
    int order[NBMI_FRAME_SLOTS], count = 0;
    for (int i = 0; i < NBMI_FRAME_SLOTS; i++) {
        if (!s->frame_slot[i].begun) continue;
        int j = count++;
        for (; j > 0 && s->frame_slot[order[j - 1]].seq > s->frame_slot[i].seq; j--) order[j] = order[j - 1];
        order[j] = i;
    }
    for (int j = 0; j < count; j++) {
        if (slots) slots[j] = order[j];
        if (kinds) kinds[j] = s->frame_slot[order[j]].kind;
        if (steps) steps[j] = s->frame_slot[order[j]].steps;
    }
    return count;
}

namespace {
struct EmitPoints {
    const double *x, *y, *z;
    const float *colors;  // (N,3), original order
    float *out_pos, *out_col;
    __device__ void operator()(int64_t k, int64_t i, uint32_t slot) const {
        out_pos[3 * k] = (float)x[slot];
        out_pos[3 * k + 1] = (float)y[slot];
        out_pos[3 * k + 2] = (float)z[slot];
        out_col[3 * k] = colors[3 * i];
        out_col[3 * k + 1] = colors[3 * i + 1];
        out_col[3 * k + 2] = colors[3 * i + 2];
    }
};
}  // namespace

int nbmi_visible_points(nbmi_sim *s, const double *cam12, double tan_h, double tan_v, double far_dist, float *out_pos,
                        float *out_col, int64_t capacity, int64_t *count) {
    if (int rc = check_handle(s)) return rc;
    if (s->owner) { nbmi::set_error("nbmi_visible_points: not available on an owner-mode handle"); return NBMI_ERR_ARG; }
    if (!cam12 || !count || capacity < 0 || (capacity > 0 && (!out_pos || !out_col))) {
        nbmi::set_error("nbmi_visible_points: null argument");
        return NBMI_ERR_ARG;
    }
    const int64_t n = s->n;
    *count = 0;
    if (n == 0) return 0;
    const int64_t ntiles = scan::tiles_for(n);
    if (!s->vis_flag) {
        if (dev_alloc(s, &s->vis_flag, vis::flag_bytes(n)) || dev_alloc(s, &s->vis_slot, (size_t)ntiles * scan::kTile) ||
            dev_alloc(s, &s->vis_tiles, ntiles + 1))
            return NBMI_ERR_HIP;
        NBMI_HIP_CHECK(hipMemsetAsync(s->vis_flag, 0, vis::flag_bytes(n), s->stream));
    }
    vis::Camera c;
    for (int k = 0; k < 3; k++) { c.p[k] = cam12[k]; c.f[k] = cam12[3 + k]; c.r[k] = cam12[6 + k]; c.u[k] = cam12[9 + k]; }
    c.tan_h = tan_h; c.tan_v = tan_v; c.z_near = 0.1; c.z_far = far_dist; c.margin = 1.2;
    Bodies cur = s->buf[s->curbuf];
    hipStream_t st = s->stream;
    float *d_pos = (float *)s->stage, *d_col = d_pos + 3 * n;  // stage holds 7 N doubles
    vis::k_mark<<<nblocks(n), kBlock, 0, st>>>(cur.x, cur.y, cur.z, cur.id, n, c, s->vis_flag, s->vis_slot);
    vis::enqueue_visible(s->vis_flag, s->vis_slot, n, s->vis_tiles,
                         EmitPoints{cur.x, cur.y, cur.z, s->colors, d_pos, d_col}, st);
    NBMI_HIP_CHECK(hipGetLastError());
    uint32_t total = 0;
    NBMI_HIP_CHECK(hipMemcpyAsync(&total, s->vis_tiles + ntiles, 4, hipMemcpyDeviceToHost, st));
    NBMI_HIP_CHECK(hipStreamSynchronize(st));
    *count = total;
    const int64_t rows = (int64_t)total < capacity ? (int64_t)total : capacity;
    if (rows > 0) {
        NBMI_HIP_CHECK(hipMemcpyAsync(out_pos, d_pos, (size_t)rows * 12, hipMemcpyDeviceToHost, st));
        NBMI_HIP_CHECK(hipMemcpyAsync(out_col, d_col, (size_t)rows * 12, hipMemcpyDeviceToHost, st));
        NBMI_HIP_CHECK(hipStreamSynchronize(st));
    }
    return 0;
}

int nbmi_set_force_precision(nbmi_sim *s, int mode, double tau) {
    if (int rc = check_handle(s)) return rc;
    if (mode < 0 || mode > 2 || (mode == 0 && !(tau >= 0.0))) {
        nbmi::set_error("nbmi_set_force_precision: mode must be 0 (auto), 1 (fp32) or 2 (float64), tau >= 0");
        return NBMI_ERR_ARG;
    }
    if (s->method != NBMI_METHOD_BARNES_HUT) { nbmi::set_error("not a Barnes-Hut handle"); return NBMI_ERR_ARG; }
    if (mode != 1 && !s->nodesd) {
        if (s->node_capacity + 2 > kMaxNodeDRows) {
            nbmi::set_error("nbmi_set_force_precision: float64 forces need at most %lld node rows",
                            (long long)kMaxNodeDRows);
            return NBMI_ERR_ARG;
        }
        if (dev_alloc(s, &s->nodesd, s->node_capacity + 2)) return NBMI_ERR_HIP;
        if (int rc = upload_walk_table(s)) return rc;
        s->tree_valid = false;  // the tree lacks the new records; positions and forces as computed stand (the other two survive)
    }
    s->force_prec = mode;
    if (mode == 0 && tau > 0.0) s->prec_tau = tau;
    return 0;
}

int nbmi_force_precision_share(nbmi_sim *s, double *share, int *all64) {
    if (int rc = check_handle(s)) return rc;
    if (!share || !all64) { nbmi::set_error("nbmi_force_precision_share: null output"); return NBMI_ERR_ARG; }
    *share = 0.0;
    *all64 = 0;
    if (s->method != NBMI_METHOD_BARNES_HUT || !s->nodesd || s->n == 0) return 0;
    if (s->force_prec == 2) { *share = 1.0; *all64 = 1; return 0; }
    if (s->force_prec == 1) return 0;
    const int64_t nw = (s->n + 63) / 64;
    std::vector<unsigned char> h((size_t)nw);
    TreeInfo ti;
    NBMI_HIP_CHECK(hipMemcpyAsync(h.data(), s->wave_flag, (size_t)nw, hipMemcpyDeviceToHost, s->stream));
    NBMI_HIP_CHECK(hipMemcpyAsync(&ti, s->info, sizeof(ti), hipMemcpyDeviceToHost, s->stream));
    NBMI_HIP_CHECK(hipStreamSynchronize(s->stream));
    int64_t c = 0;
    for (int64_t i = 0; i < nw; i++) c += h[i] ? 1 : 0;
    *share = (double)c / (double)nw;
    *all64 = ti.force_all64;
    return 0;
}

int nbmi_set_exchange_sync(nbmi_sim *s, int sync) {
    if (int rc = check_handle(s)) return rc;
    s->exchange_sync = sync != 0;
    return 0;
}

void *nbmi_stream(nbmi_sim *s) { return s ? (void *)s->stream : nullptr; }

}  // extern "C"

// ---- point renderer source (render.hip) ----------------------------------------------------------
namespace nbmi {
// Body count and device of a handle the renderer may draw (not an owner-mode handle).
int render_source(nbmi_sim *s, int64_t *n, int *device) {
    if (int rc = check_handle(s)) return rc;
    if (s->owner) { nbmi::set_error("nbmi_render_sim: not available on an owner-mode handle"); return NBMI_ERR_ARG; }
    *n = s->n;
    *device = s->device;
    return 0;
}
// The handle's current float32 positions (as nbmi_get_positions_f32) and the colours of its last
// nbmi_compute_colors, copied in the caller's row order into the device buffers d_pos / d_col (N x 3 each) on the
// handle's own stream; `done` is recorded behind the copies for the renderer's stream to wait on.
int render_fetch(nbmi_sim *s, float *d_pos, float *d_col, hipEvent_t done) {
    if (int rc = check_handle(s)) return rc;
    const int64_t n = s->n;
    if (n > 0) {
        Bodies cur = s->buf[s->curbuf];
        k_unperm3_f32<<<nblocks(n), kBlock, 0, s->stream>>>(cur.x, cur.y, cur.z, cur.id, n, d_pos);
        NBMI_HIP_CHECK(hipGetLastError());
        NBMI_HIP_CHECK(hipMemcpyAsync(d_col, s->colors, (size_t)n * 12, hipMemcpyDeviceToDevice, s->stream));
    }
    NBMI_HIP_CHECK(hipEventRecord(done, s->stream));
    if (s->method == NBMI_METHOD_BARNES_HUT) {
        NBMI_HIP_CHECK(hipEventSynchronize(done));
        return check_device_error(s);
    }
    return 0;
}
}  // namespace nbmi
