// Hand-written device radix sort for gfx950, in two forms: (key, 32-bit value) pairs - the boids' 24-bit cell indices,
// the octree build's 63-bit key word + body index where the packed form does not fit - and bare keys sorted on a bit
// field [begin_bit, end_bit), the bits outside it travelling along: the octree build's packed word (sorted key prefix
// << 24 | body index), which moves 8 bytes per body and pass in each direction instead of 12 and reorders the tile in
// LDS once instead of twice.
//
// Least-significant-digit first, ONE kernel per pass ("onesweep"): a workgroup owns a tile of 4 096 pairs, ranks them
// by digit with wave-level match operations (ballots), learns how many pairs of each digit the tiles before it hold
// through a decoupled look-back over per-tile status words, reorders the tile in LDS so that every digit's pairs leave
// as one contiguous run, and writes them to their final place of this pass.  Stable.  Per pass every pair is read once
// and written once (24 B of traffic for a u64 key + u32 value, 16 B for a bare u64 key).
//
// Digit width (8 or 10 bits) and threads per tile (256, 512 or 1 024) are template parameters of the pass
// (k_radix_pass; LDS and workgroups per CU of every combination are listed there); RadixConfig asks for a combination,
// and resolve_shape() holds the size rule for what is not asked for: pairs and sorts of up to 524 288 keys run 8 bits
// on 256 threads (tiles of 1 024 / 2 048 / 4 096 by size), keys-only sorts above that 10 bits on 1 024 threads up to
// 2 097 152 keys - four passes over the octree's 40-bit field instead of five - and 8 bits on 512 threads beyond
// (profiles/sort_wide_ab.txt: the sweep, losers included).  More waves on the same tile shorten a wave's serial
// ranking without adding a tile to the look-back chain.
//
// The digit counts of ALL passes are taken before the first: by k_radix_hist in one extra read of the keys, or - the
// octree build's packed sort - by the kernel that writes the keys (radix_hist.h; radix_keys_prepare_u64 clears the
// temp buffer in front of that kernel and hands out the histogram).  The counts stay raw: every workgroup of a pass
// scans the pass's counts itself, in the same block scan as its tile's digit totals, so there is no offsets kernel.
// One fill per sort clears the tickets, the histogram and the status rows this sort's tile size and pass count use.
//
// Look-back notes (gfx950: eight XCDs, L2s not coherent with each other): a status word carries flag and
// count in ONE 32-bit granule and is written / polled with agent-scope relaxed atomics (sc1), so no
// payload has to be ordered behind a flag (a thread that owns several digits moves its words 8 bytes at a time: two
// self-contained granules).  Tile numbers come from an atomic ticket, so a tile only ever
// waits for tiles whose workgroups are already running.  A tile inspects kLookBatch = 8 predecessors per round trip
// (their loads are issued together): with a whole grid starting at once the serial form would walk up to
// `tiles` predecessors one memory round trip at a time.  Batches of 16 and 32 were measured and lose at 1 M keys
// (profiles/build_lean_ab.txt).  Every spin is bounded; a timeout sets an error
// word instead of hanging the GPU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "common.h"
#include "radix_hist.h"
#include "scan.h"
#include <stddef.h>

namespace nbmi {
namespace {

constexpr int kItems = 16, kItemsMin = 4;   // keys per thread of the 8-bit, 256-thread pass: its tile is 4 096, 2 048 or 1 024
                                            // keys by size; every other configuration runs 4 096-key tiles
constexpr int kWideTile = 4096;
constexpr unsigned kFlagAgg = 1u << 30, kFlagIncl = 2u << 30, kValueMask = (1u << 30) - 1;
// predecessors a tile inspects per look-back round trip (their loads are issued together and consumed in order);
// a compile-time constant of the pass
#ifndef NBMI_LOOK_BATCH
#define NBMI_LOOK_BATCH 8
#endif
constexpr int kLookBatch = NBMI_LOOK_BATCH;
constexpr int kMaxPasses = kRadixMaxPasses;
// What the size rule gives keys-only sorts of more than kLargeMinKeys keys (profiles/sort_wide_ab.txt has the sweep);
// pairs and small sorts keep 8 bits and 256 threads.
//   up to kWideMaxKeys: 10-bit digits on 1 024 threads where the field is a whole number of them or they save a pass -
//     at 1 M keys four such passes beat five 8-bit ones on 512 threads by 0.006 ms (0.101 against 0.107);
//   above: 8-bit digits on 512 threads - at 10 M the 10-bit passes lose 0.06 ms (a 4 096-key tile leaves a 10-bit digit
//     runs of four keys to write, and four times the status words to publish and look back over).
// Measured at 1 M and 10 M only: the boundary between them - 512 tiles, two workgroups of 1 024 threads on every CU,
// the most that run at once - is an estimate.
constexpr size_t kLargeMinKeys = 524288, kWideMaxKeys = 2097152;
constexpr int kLargeThreads = 512, kWideThreads = 1024;

struct Control {                 // lives at the start of the temp buffer
    unsigned error;              // 1: a look-back spin timed out.  STICKY: cleared by radix_init_temp() only, not by the
    unsigned pad0[15];           // per-sort clear (which starts at tile_ticket), so that the owner of the buffer still
                                 // finds it at its next synchronisation however many sorts have run since
    unsigned tile_ticket[kMaxPasses];
    unsigned pad[8];
    unsigned hist[kMaxPasses * kRadixMaxBins];  // global digit counts, pass p at [p << digit bits]; every pass scans its own
};

// dmask: all ones, or fewer in the last pass of a field that is no whole number of digits wide (radix_digit_mask)
template <typename K>
__device__ __forceinline__ unsigned digit_of(K k, int shift, unsigned dmask) {
    return (unsigned)(k >> shift) & dmask;
}

// ---- digit histograms of all passes: one read of the keys ------------------------------------
// (sorts whose keys no earlier kernel has counted: pairs, and keys-only sorts without a prepared histogram)
constexpr int kHistThreads = 256;
template <typename K>
__global__ __launch_bounds__(kHistThreads) void k_radix_hist(const K *__restrict__ keys, int64_t n, int bits, int first_bit,
                                                            int digit_bits, Control *ctl) {
    const int passes = radix_passes(bits, digit_bits);
    extern __shared__ unsigned h[];  // [passes][1 << digit_bits]
    for (int i = threadIdx.x; i < (passes << digit_bits); i += kHistThreads) h[i] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kHistThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kHistThreads)
        radix_hist_count(h, (uint64_t)(keys[i] >> first_bit), bits, digit_bits, passes);
    __syncthreads();
    radix_hist_flush(h, ctl->hist, digit_bits, passes, kHistThreads);
}

// the OWN consecutive status words of a thread, agent-scope relaxed like the single word: 8 bytes at a time where a
// thread owns more than one (every word is a self-contained 32-bit granule, so a wider access tears nothing)
template <int OWN>
__device__ __forceinline__ void status_load(const unsigned *p, unsigned (&w)[OWN]) {
    if constexpr (OWN == 1) {
        w[0] = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
#pragma unroll
        for (int o = 0; o < OWN; o += 2) {
            const unsigned long long v = __hip_atomic_load(reinterpret_cast<const unsigned long long *>(p + o), __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT);
            w[o] = (unsigned)v;
            w[o + 1] = (unsigned)(v >> 32);
        }
    }
}
template <int OWN>
__device__ __forceinline__ void status_store(unsigned *p, unsigned flag, const unsigned (&v)[OWN]) {
    if constexpr (OWN == 1) {
        __hip_atomic_store(p, flag | v[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
#pragma unroll
        for (int o = 0; o < OWN; o += 2)
            __hip_atomic_store(reinterpret_cast<unsigned long long *>(p + o),
                               (unsigned long long)(flag | v[o]) | ((unsigned long long)(flag | v[o + 1]) << 32), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- one pass --------------------------------------------------------------------------------
// BITS: the digit (8 or 10); THREADS x ITEMS: the tile.  kPairs = false: the keys-only form (no vin / vout, no second
// trip through the reorder buffer, no slot registers) - for keys that carry their value in the bits below the sorted
// field, like the octree build's packed word.
// More threads on the same tile shorten a wave's serial ranking (ITEMS rounds of BITS ballots) without adding a tile
// to the look-back chain.  With more digits than threads a thread owns OWN consecutive digits in the totals, the scan
// and the look-back; with more threads than digits only the first BINS threads take part in them.
// LDS per workgroup for 8-byte keys (cnt_w + tile_off + glob_off + the reorder buffer; 160 KiB per CU):
//    8 bits x  256 x 16:   4 +  2 + 32 =  38 KiB, 4 workgroups (16 waves) per CU        (x 8: 22 KiB, x 4: 14 KiB)
//    8 bits x  512 x  8:   8 +  2 + 32 =  42 KiB, 3 workgroups (24 waves)
//    8 bits x 1024 x  4:  16 +  2 + 32 =  50 KiB, 2 workgroups (32 waves: the CU's wave limit)
//   10 bits x  256 x 16:   8 +  8 + 32 =  48 KiB, 3 workgroups by LDS, 2 (8 waves) by its 177 VGPRs
//   10 bits x  512 x  8:  16 +  8 + 32 =  56 KiB, 2 workgroups (16 waves)
//   10 bits x 1024 x  4:  32 +  8 + 32 =  72 KiB, 2 workgroups (32 waves)
// (10 bits: 16-bit per-wave counters - a count never exceeds the tile, 4 096; with 32-bit ones the last line would
// be 104 KiB and one workgroup per CU.)
template <typename K, int BITS, int THREADS, int ITEMS, bool kPairs, int LOOK = kLookBatch>
__global__ __launch_bounds__(THREADS) void k_radix_pass(const K *__restrict__ kin, K *__restrict__ kout,
                                                       const uint32_t *__restrict__ vin, uint32_t *__restrict__ vout,
                                                       int64_t n, int shift, unsigned dmask, int pass, Control *ctl,
                                                       unsigned *__restrict__ status /* [tiles][BINS] of this pass */) {
    constexpr int BINS = 1 << BITS, WAVES = THREADS / 64, TILE = THREADS * ITEMS;
    constexpr int OWN = BINS > THREADS ? BINS / THREADS : 1;  // digits a thread owns: OWN * t .. OWN * t + OWN - 1
    static_assert(TILE <= 65536 && (OWN == 1 || OWN % 2 == 0), "16-bit slots; owned status words go in 8-byte accesses");
    using cnt_t = typename std::conditional<(BITS > 8), uint16_t, unsigned>::type;
    __shared__ unsigned s_tile;
    __shared__ cnt_t cnt_w[WAVES][BINS];        // per-wave digit counts, then the wave's base inside the digit
    __shared__ unsigned tile_off[BINS];         // first slot of the digit inside the reordered tile
    __shared__ unsigned glob_off[BINS];         // global slot of reordered slot q of digit d = glob_off[d] + q
    // the reorder buffer is used twice, for the keys and then for the values
    __shared__ K lds_k[TILE];

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const bool owner = BINS >= THREADS || t < BINS;
    const int d0 = t * OWN;
    if (t == 0) s_tile = atomicAdd(&ctl->tile_ticket[pass], 1u);
    for (int i = t; i < (int)(sizeof(cnt_w) / sizeof(unsigned)); i += THREADS) reinterpret_cast<unsigned *>(&cnt_w[0][0])[i] = 0u;
    // the pass's raw global counts of the owned digits (scanned below, with the tile's totals)
    unsigned graw[OWN];
#pragma unroll
    for (int o = 0; o < OWN; o++) graw[o] = owner ? ctl->hist[(pass << BITS) + d0 + o] : 0u;
    __syncthreads();
    const unsigned tile = s_tile;
    const int64_t tile_base = (int64_t)tile * TILE;
    const int valid_in_tile = (int)((n - tile_base) < TILE ? (n - tile_base) : TILE);

    // a wave owns (64 * ITEMS) consecutive pairs and loads them 64 at a time (coalesced); the order inside
    // the tile is wave-major, then round, then lane
    K key[ITEMS];
    uint32_t val[kPairs ? ITEMS : 1];
    unsigned rank[ITEMS];
    const int64_t wave_base = tile_base + (int64_t)w * (64 * ITEMS);
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const int64_t idx = wave_base + i * 64 + lane;
        const bool ok = idx < n;
        key[i] = ok ? kin[idx] : (K)~(K)0;
        if (kPairs) val[i] = ok ? vin[idx] : 0u;
    }
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const int64_t idx = wave_base + i * 64 + lane;
        const bool ok = idx < n;
        const unsigned d = digit_of(key[i], shift, dmask);
        // lanes of this round with the same digit
        unsigned long long peers = __builtin_amdgcn_ballot_w64(ok);
#pragma unroll
        for (int b = 0; b < BITS; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __builtin_amdgcn_ballot_w64(bit);
            peers &= bit ? m : ~m;
        }
        const unsigned before = (unsigned)__popcll(peers & lt_mask);
        const unsigned pre = ok ? (unsigned)cnt_w[w][d] : 0u;  // pairs of this digit in the wave's earlier rounds
        rank[i] = pre + before;
        // the wave's LDS operations execute in order: every peer has read `pre` before the leader's update
        if (ok && before == 0u) cnt_w[w][d] = (cnt_t)(pre + (unsigned)__popcll(peers));
    }
    __syncthreads();

    // thread t = digits d0 .. d0 + OWN - 1: totals, wave bases, tile offsets, look-back
    unsigned total[OWN];
    unsigned tsum = 0, gsum = 0;
#pragma unroll
    for (int o = 0; o < OWN; o++) {
        unsigned run = 0;
        if (owner) {
            unsigned c[WAVES];
#pragma unroll
            for (int k = 0; k < WAVES; k++) { c[k] = cnt_w[k][d0 + o]; }
#pragma unroll
            for (int k = 0; k < WAVES; k++) { cnt_w[k][d0 + o] = (cnt_t)run; run += c[k]; }
        }
        total[o] = run;
        tsum += run;
        gsum += graw[o];
    }
    // ONE exclusive scan across the workgroup for both: the tile's totals in the upper word, the pass's global counts
    // (at most n < 2^30 in all, so no carry leaves the lower word) below; a short serial prefix over the owned digits
    const unsigned long long ex =
        scan::block_scan<THREADS>(((unsigned long long)tsum << 32) | gsum, 0ull, scan::Sum()).excl;
    unsigned my_tile_off[OWN], my_glob[OWN];
    {
        unsigned rt = (unsigned)(ex >> 32), rg = (unsigned)ex;
#pragma unroll
        for (int o = 0; o < OWN; o++) {
            my_tile_off[o] = rt;
            my_glob[o] = rg;
            rt += total[o];
            rg += graw[o];
            if (owner) tile_off[d0 + o] = my_tile_off[o];
        }
    }

    // decoupled look-back: pairs of the owned digits in the tiles before this one.  Every owned digit keeps its own
    // prefix and its own `done` bit; a predecessor is consumed for all digits still looked for at once, so it has to
    // have published all of them.
    unsigned prefix[OWN];
#pragma unroll
    for (int o = 0; o < OWN; o++) prefix[o] = 0u;
    if (owner) {
        unsigned *mine = status + (size_t)tile * BINS + d0;
        if (tile == 0) {
            status_store<OWN>(mine, kFlagIncl, total);
        } else {
            status_store<OWN>(mine, kFlagAgg, total);
            constexpr unsigned kAll = (1u << OWN) - 1u;
            int p = (int)tile - 1;
            unsigned spins = 0;
            unsigned done = 0;  // bit o: digit d0 + o has met an inclusive word
            while (done != kAll) {
                unsigned sw[LOOK][OWN];
#pragma unroll
                for (int j = 0; j < LOOK; j++) {
                    const int q = p - j;
                    if (q >= 0) {
                        status_load<OWN>(status + (size_t)q * BINS + d0, sw[j]);
                    } else {  // before tile 0: nothing
#pragma unroll
                        for (int o = 0; o < OWN; o++) sw[j][o] = kFlagIncl;
                    }
                }
#pragma unroll
                for (int j = 0; j < LOOK; j++) {
                    if (done == kAll) break;
                    bool ready = true;
#pragma unroll
                    for (int o = 0; o < OWN; o++)
                        if (!((done >> o) & 1u) && (sw[j][o] & ~kValueMask) == 0u) ready = false;
                    if (!ready) {  // not published yet: poll again from this tile
                        if (++spins > (1u << 22)) { ctl->error = 1u; done = kAll; }
                        __builtin_amdgcn_s_sleep(2);
                        break;
                    }
#pragma unroll
                    for (int o = 0; o < OWN; o++) {
                        if ((done >> o) & 1u) continue;
                        prefix[o] += sw[j][o] & kValueMask;
                        if ((sw[j][o] & ~kValueMask) == kFlagIncl) done |= 1u << o;
                    }
                    p--;
                }
            }
            unsigned incl[OWN];
#pragma unroll
            for (int o = 0; o < OWN; o++) incl[o] = prefix[o] + total[o];
            status_store<OWN>(mine, kFlagIncl, incl);
        }
#pragma unroll
        for (int o = 0; o < OWN; o++) glob_off[d0 + o] = my_glob[o] + prefix[o] - my_tile_off[o];
    }
    __syncthreads();

    // reorder inside the tile: digit runs, each in input order
    unsigned slot[kPairs ? (ITEMS + 1) / 2 : 1];  // two 16-bit slots per register
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const int64_t idx = wave_base + i * 64 + lane;
        unsigned q = 0;
        if (idx < n) {
            const unsigned d = digit_of(key[i], shift, dmask);
            q = tile_off[d] + (unsigned)cnt_w[w][d] + rank[i];
            lds_k[q] = key[i];
        }
        if (kPairs) {
            if (i & 1) slot[i >> 1] |= q << 16; else slot[i >> 1] = q;
        }
    }
    __syncthreads();
    unsigned dst[kPairs ? ITEMS : 1];
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const int q = i * THREADS + t;
        if (q < valid_in_tile) {
            const K k = lds_k[q];
            const unsigned g = glob_off[digit_of(k, shift, dmask)] + (unsigned)q;
            kout[g] = k;
            if (kPairs) dst[i] = g;
        }
    }
    if (!kPairs) return;
    __syncthreads();
    uint32_t *lds_v = reinterpret_cast<uint32_t *>(lds_k);
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const int64_t idx = wave_base + i * 64 + lane;
        if (idx < n) lds_v[(slot[i >> 1] >> ((i & 1) * 16)) & 0xffffu] = val[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const int q = i * THREADS + t;
        if (q < valid_in_tile) vout[dst[i]] = lds_v[q];
    }
}

inline size_t tiles_for(size_t n, size_t tile) { return (n + tile - 1) / tile; }
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// The status rows of the largest configuration a sort of n keys on `bits` bits can run: the smallest 8-bit tile, or
// (a few keys) one row of 10-bit digits per pass.  The layout of the temp buffer does not depend on the configuration.
inline size_t status_bytes_max(size_t n, int bits) {
    const size_t narrow = (size_t)radix_passes(bits, 8) * tiles_for(n, 256 * kItemsMin) * 256;
    const size_t wide = (size_t)radix_passes(bits, kRadixMaxBits) * tiles_for(n, kWideTile) * kRadixMaxBins;
    return align256((narrow > wide ? narrow : wide) * sizeof(unsigned));
}

// kPairs = false: the keys-only sort needs no value buffer
template <typename K, bool kPairs = true>
size_t temp_bytes(size_t n, int bits) {
    return align256(sizeof(Control)) + status_bytes_max(n, bits) + align256(n * sizeof(K)) +
           (kPairs ? align256(n * sizeof(uint32_t)) : 0);
}

// digit bits, threads and keys per thread of a sort: the caller's wish (RadixConfig; 0 = by the size rule) resolved
struct Shape {
    int bits = 0, threads = 0, items = 0;
    size_t tile() const { return (size_t)threads * items; }
};
// false: a value the sort has no kernel for
inline bool resolve_shape(RadixConfig want, size_t n, int field_bits, bool pairs, Shape *out) {
    if ((want.digit_bits != 0 && want.digit_bits != 8 && want.digit_bits != 10) ||
        (want.threads != 0 && want.threads != 256 && want.threads != 512 && want.threads != 1024))
        return false;
    Shape s;
    const bool large = !pairs && n > kLargeMinKeys;
    const bool wide = large && n <= kWideMaxKeys && !want.digit_bits && !want.threads &&
                      (field_bits % 10 == 0 || radix_passes(field_bits, 10) < radix_passes(field_bits, 8));
    s.bits = want.digit_bits ? want.digit_bits : (wide ? 10 : 8);
    s.threads = want.threads ? want.threads : (wide ? kWideThreads : (large ? kLargeThreads : 256));
    // [r4] keys per thread of the 256-thread pass by size (profiles/r04_small_systems.txt): a pass over few pairs is a
    // chain of latencies, and more, smaller workgroups shorten it - sort phase at 10 k bodies 0.067 / 0.054 / 0.050 ms
    // with 16 / 8 / 4, at 262 k 0.126 / 0.120 / 0.125; from 1 M on the large tile wins (0.151 against 0.169 ms with 8,
    // 10 M: 0.70 against 0.82)
    if (s.bits == 8 && s.threads == 256) s.items = n <= 65536 ? kItemsMin : (n <= 524288 ? 8 : kItems);
    else s.items = kWideTile / s.threads;
    *out = s;
    return true;
}

template <typename K, bool kPairs>
hipError_t check_sort(size_t temp_size, size_t n, int bits, RadixConfig want, Shape *shape) {
    if (n > (size_t)kValueMask) return hipErrorInvalidValue;  // counts travel in 30 bits
    if (bits < 1 || !resolve_shape(want, n, bits, kPairs, shape)) return hipErrorInvalidValue;
    const int passes = radix_passes(bits, shape->bits);
    if (passes < 1 || passes > kMaxPasses || temp_size < temp_bytes<K, kPairs>(n, bits)) return hipErrorInvalidValue;
    return hipSuccess;
}

// Clears what one sort of this shape uses - tickets, histogram, the status rows of its tile size and pass count - in
// one fill; everything but the sticky error word at the head of the control block.
inline hipError_t clear_sort(char *base, size_t n, int bits, const Shape &shape, hipStream_t st) {
    const size_t rows = (size_t)radix_passes(bits, shape.bits) * tiles_for(n, shape.tile());
    return hipMemsetAsync(base + offsetof(Control, tile_ticket), 0,
                          align256(sizeof(Control)) - offsetof(Control, tile_ticket) + rows * ((size_t)sizeof(unsigned) << shape.bits), st);
}

template <typename K, int BITS, int THREADS, int ITEMS, bool kPairs>
void launch_pass(size_t tiles, hipStream_t st, const K *ksrc, K *kdst, const uint32_t *vsrc, uint32_t *vdst, int64_t n, int shift,
                 unsigned dmask, int p, Control *ctl, unsigned *status) {
    k_radix_pass<K, BITS, THREADS, ITEMS, kPairs><<<(int)tiles, THREADS, 0, st>>>(ksrc, kdst, vsrc, vdst, n, shift, dmask, p, ctl, status);
}

// Sorts on the bits [begin_bit, end_bit) of the keys.  kPairs = false (sort_keys): vin / vout are not touched; the
// bits outside the sorted field travel with their key, and keys equal in the field keep their input order.
// have_hist: radix_keys_prepare has cleared the temp buffer for this very sort and an earlier kernel has counted the
// digits into the histogram it handed out.
template <typename K, bool kPairs>
hipError_t sort_impl(void *temp, size_t temp_size, const K *kin, K *kout, const uint32_t *vin, uint32_t *vout,
                     size_t n, int begin_bit, int end_bit, RadixConfig want, bool have_hist, hipStream_t st) {
    const int bits = end_bit - begin_bit;
    if (n == 0) return hipSuccess;
    Shape shape;
    if (hipError_t e = check_sort<K, kPairs>(temp_size, n, bits, want, &shape)) return e;
    const int passes = radix_passes(bits, shape.bits);
    char *base = (char *)temp;
    Control *ctl = (Control *)base;
    const size_t tiles = tiles_for(n, shape.tile());
    unsigned *status = (unsigned *)(base + align256(sizeof(Control)));
    K *ktmp = (K *)((char *)status + status_bytes_max(n, bits));
    uint32_t *vtmp = kPairs ? (uint32_t *)((char *)ktmp + align256(n * sizeof(K))) : nullptr;
    if (!have_hist) {
        if (hipError_t e = clear_sort(base, n, bits, shape, st)) return e;
        int hb = (int)((n + kHistThreads * 8 - 1) / (kHistThreads * 8));
        if (hb > 1024) hb = 1024;
        k_radix_hist<K><<<hb, kHistThreads, ((size_t)passes << shape.bits) * sizeof(unsigned), st>>>(kin, (int64_t)n, bits, begin_bit,
                                                                                                    shape.bits, ctl);
    }
    // ping-pong so that the last pass writes the caller's output: ... -> tmp -> out
    const K *ksrc = kin;
    const uint32_t *vsrc = vin;
    for (int p = 0; p < passes; p++) {
        const bool to_out = ((passes - 1 - p) % 2) == 0;
        K *kdst = to_out ? kout : ktmp;
        uint32_t *vdst = to_out ? vout : vtmp;
        const int shift = begin_bit + p * shape.bits;
        const unsigned dmask = radix_digit_mask(bits, shape.bits, p);
        unsigned *srow = status + ((size_t)p * tiles << shape.bits);
#define NBMI_PASS(B, T, I)                                                                                                 \
    if (shape.bits == B && shape.threads == T && shape.items == I)                                                        \
        launch_pass<K, B, T, I, kPairs>(tiles, st, ksrc, kdst, vsrc, vdst, (int64_t)n, shift, dmask, p, ctl, srow)
        NBMI_PASS(8, 256, 4);
        NBMI_PASS(8, 256, 8);
        NBMI_PASS(8, 256, 16);
        NBMI_PASS(8, 512, 8);
        NBMI_PASS(8, 1024, 4);
        NBMI_PASS(10, 256, 16);
        NBMI_PASS(10, 512, 8);
        NBMI_PASS(10, 1024, 4);
#undef NBMI_PASS
        ksrc = kdst;
        vsrc = vdst;
    }
    return hipGetLastError();
}

template <typename K>
hipError_t sort_keys(void *temp, size_t temp_size, const K *kin, K *kout, size_t n, int begin_bit, int end_bit,
                     RadixConfig want, bool have_hist, hipStream_t st) {
    if (begin_bit < 0 || end_bit > (int)(8 * sizeof(K)) || begin_bit >= end_bit) return hipErrorInvalidValue;
    return sort_impl<K, false>(temp, temp_size, kin, kout, nullptr, nullptr, n, begin_bit, end_bit, want, have_hist, st);
}

}  // namespace

// ---- entry points used by nbmi.hip / bdmi.hip ---------------------------------------------------
size_t radix_temp_bytes_u64(size_t n, int bits) { return temp_bytes<uint64_t>(n, bits); }
size_t radix_temp_bytes_u32(size_t n, int bits) { return temp_bytes<uint32_t>(n, bits); }
hipError_t radix_sort_pairs_u64(void *temp, size_t temp_size, const uint64_t *kin, uint64_t *kout, const uint32_t *vin,
                                uint32_t *vout, size_t n, int begin_bit, int end_bit, hipStream_t s, RadixConfig cfg) {
    return sort_impl<uint64_t, true>(temp, temp_size, kin, kout, vin, vout, n, begin_bit, end_bit, cfg, false, s);
}
hipError_t radix_sort_pairs_u32(void *temp, size_t temp_size, const uint32_t *kin, uint32_t *kout, const uint32_t *vin,
                                uint32_t *vout, size_t n, int begin_bit, int end_bit, hipStream_t s, RadixConfig cfg) {
    return sort_impl<uint32_t, true>(temp, temp_size, kin, kout, vin, vout, n, begin_bit, end_bit, cfg, false, s);
}
size_t radix_keys_temp_bytes_u64(size_t n, int bits) { return temp_bytes<uint64_t, false>(n, bits); }
size_t radix_keys_temp_bytes_u32(size_t n, int bits) { return temp_bytes<uint32_t, false>(n, bits); }
hipError_t radix_sort_keys_u64(void *temp, size_t temp_size, const uint64_t *kin, uint64_t *kout, size_t n, int begin_bit,
                               int end_bit, hipStream_t s, RadixConfig cfg, bool have_hist) {
    return sort_keys<uint64_t>(temp, temp_size, kin, kout, n, begin_bit, end_bit, cfg, have_hist, s);
}
hipError_t radix_sort_keys_u32(void *temp, size_t temp_size, const uint32_t *kin, uint32_t *kout, size_t n, int begin_bit,
                               int end_bit, hipStream_t s, RadixConfig cfg) {
    return sort_keys<uint32_t>(temp, temp_size, kin, kout, n, begin_bit, end_bit, cfg, false, s);
}
bool radix_config_ok(RadixConfig cfg) {
    Shape s;
    return resolve_shape(cfg, 1, 8, false, &s);
}
// First half of a keys-only u64 sort whose digits an earlier kernel of the caller counts: clears the control block and
// the status rows of this sort (n keys, this field, this configuration) and hands out the device histogram.  Enqueue
// it before the counting kernel; then radix_sort_keys_u64(..., have_hist = true) with the same n, field and cfg.
hipError_t radix_keys_prepare_u64(void *temp, size_t temp_size, size_t n, int begin_bit, int end_bit, RadixConfig cfg,
                                  hipStream_t s, RadixHist *out) {
    const int bits = end_bit - begin_bit;
    if (n == 0 || begin_bit < 0 || end_bit > 64 || bits < 1 || !out) return hipErrorInvalidValue;
    Shape shape;
    if (hipError_t e = check_sort<uint64_t, false>(temp_size, n, bits, cfg, &shape)) return e;
    out->counts = ((Control *)temp)->hist;
    out->bits = bits;
    out->digit_bits = shape.bits;
    out->passes = radix_passes(bits, shape.bits);
    return clear_sort((char *)temp, n, bits, shape, s);
}
// A freshly allocated temp buffer: clears the sticky error word (once, by whoever allocated the buffer).
hipError_t radix_init_temp(void *temp, hipStream_t s) { return hipMemsetAsync(temp, 0, offsetof(Control, tile_ticket), s); }
// 1 if a look-back of ANY sort on this temp buffer since radix_init_temp() timed out (never observed; the spin is
// bounded so that a lost status word cannot hang the GPU).  Such a pass scattered to wrong offsets: the product
// paths read this word wherever they synchronise anyway and report NBMI_ERR_HIP.
hipError_t radix_error_word(const void *temp, unsigned *out, hipStream_t s) {
    return hipMemcpyAsync(out, &((const Control *)temp)->error, sizeof(unsigned), hipMemcpyDeviceToHost, s);
}
const void *radix_error_device_word(const void *temp) { return &((const Control *)temp)->error; }

}  // namespace nbmi
