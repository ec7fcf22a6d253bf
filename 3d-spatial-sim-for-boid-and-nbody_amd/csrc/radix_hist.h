// Digit counting for the radix sort's histograms (radix.hip), shared with the kernels that already hold the sorted field
// in registers and count on the sort's behalf (nbmi.hip: k_keys, whose packed words k_radix_hist would otherwise read
// back one kernel later).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nbmi {

constexpr int kRadixMaxPasses = 8;
constexpr int kRadixMaxBits = 10;                  // widest digit of a pass
constexpr int kRadixMaxBins = 1 << kRadixMaxBits;

// digit mask of pass `pass` of a field `bits` wide cut into `digit_bits`-bit digits: all ones, or fewer in the last
// pass of a field that is no whole number of digits wide
inline __host__ __device__ unsigned radix_digit_mask(int bits, int digit_bits, int pass) {
    const int left = bits - pass * digit_bits;
    return left >= digit_bits ? (1u << digit_bits) - 1u : (1u << left) - 1u;
}
inline __host__ __device__ int radix_passes(int bits, int digit_bits) { return (bits + digit_bits - 1) / digit_bits; }

// Where a sort's device histogram lives and how its field is cut (radix_keys_prepare_u64 hands it out).
struct RadixHist {
    unsigned *counts = nullptr;  // [passes][1 << digit_bits], cleared by the prepare call
    int bits = 0, digit_bits = 0, passes = 0;
};

// Counts the digits of `field` (the sorted field, shifted down to bit 0) in the LDS histogram h[passes][1 << digit_bits].
// Called by the lanes that hold a key, in wave-uniform control flow up to lanes that have run out of keys.
// The octree keys arrive nearly sorted (the state is kept in last step's key order), so the 64 keys of a wave share
// their upper digits: 64 LDS atomics on ONE counter, serialised.  A digit the whole wave agrees on is counted by one
// lane.
__device__ __forceinline__ void radix_hist_count(unsigned *h, uint64_t field, int bits, int digit_bits, int passes) {
    const unsigned long long act = __builtin_amdgcn_ballot_w64(true);
    const unsigned live = (unsigned)__builtin_popcountll(act);
    const bool first = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == (unsigned)__builtin_ctzll(act);
    for (int p = 0; p < passes; p++) {
        const unsigned d = (unsigned)(field >> (p * digit_bits)) & radix_digit_mask(bits, digit_bits, p);
        const unsigned d0 = __builtin_amdgcn_readfirstlane(d);
        unsigned *hp = h + ((size_t)p << digit_bits);
        if (__builtin_amdgcn_ballot_w64(d != d0) == 0ull) {
            if (first) atomicAdd(&hp[d0], live);
        } else {
            atomicAdd(&hp[d], 1u);
        }
    }
}

// the workgroup's non-zero counts to the device histogram, one atomic each (after a barrier behind the last count)
__device__ __forceinline__ void radix_hist_flush(const unsigned *h, unsigned *__restrict__ counts, int digit_bits, int passes,
                                                 int threads) {
    for (int i = threadIdx.x; i < (passes << digit_bits); i += threads) {
        const unsigned v = h[i];
        if (v) atomicAdd(&counts[i], v);
    }
}

}  // namespace nbmi
