// Internal helpers shared by the translation units of libnbmi.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

namespace nbmi {

void set_error(const char *fmt, ...);
const char *get_error();
void clear_error();

#define NBMI_HIP_CHECK(expr)                                                                \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            (void)hipGetLastError(); /* clear the sticky error so later calls start clean */ \
            nbmi::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                            __LINE__);                                                      \
            return -2;                                                                      \
        }                                                                                   \
    } while (0)

// The sum of a counter over the wave, added to *dst by one agent-scope relaxed integer atomic (what atomicAdd is) unless
// it is 0: integers, so the result does not depend on any order.  Every lane of the wave calls it, with its lane number.
__device__ __forceinline__ void wave_add(unsigned long long *dst, long long v, int lane) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0 && v != 0ll) (void)__hip_atomic_fetch_add(dst, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// {m, m*x, m*y, m*z} prefix-sum element, each a double-double (high word, low word).
struct Moment {
    double m, ml, x, xl, y, yl, z, zl;
};

// ---- device sort (radix.hip) ------------------------------------------------------------
// by key bits [begin_bit, end_bit), stable, ping-pong inside `temp`
// Digit width (8 or 10 bits) and threads per tile (256, 512 or 1024) of the passes; 0 = chosen by size and form.
struct RadixConfig {
    int digit_bits = 0, threads = 0;
};
struct RadixHist;  // radix_hist.h
bool radix_config_ok(RadixConfig cfg);
size_t radix_temp_bytes_u64(size_t n, int bits);
size_t radix_temp_bytes_u32(size_t n, int bits);
hipError_t radix_sort_pairs_u64(void *temp, size_t temp_bytes, const uint64_t *kin, uint64_t *kout, const uint32_t *vin,
                                uint32_t *vout, size_t n, int begin_bit, int end_bit, hipStream_t s, RadixConfig cfg = {});
hipError_t radix_sort_pairs_u32(void *temp, size_t temp_bytes, const uint32_t *kin, uint32_t *kout, const uint32_t *vin,
                                uint32_t *vout, size_t n, int begin_bit, int end_bit, hipStream_t s, RadixConfig cfg = {});
// keys-only: sorts on the bits [begin_bit, end_bit) of the keys, the other bits travel along (stable); the pair
// form's temp buffer is the larger and serves both
size_t radix_keys_temp_bytes_u64(size_t n, int bits);
size_t radix_keys_temp_bytes_u32(size_t n, int bits);
// have_hist: radix_keys_prepare_u64 ran for this sort and the caller's own kernel has counted the digits since
hipError_t radix_sort_keys_u64(void *temp, size_t temp_bytes, const uint64_t *kin, uint64_t *kout, size_t n, int begin_bit,
                               int end_bit, hipStream_t s, RadixConfig cfg = {}, bool have_hist = false);
hipError_t radix_sort_keys_u32(void *temp, size_t temp_bytes, const uint32_t *kin, uint32_t *kout, size_t n, int begin_bit,
                               int end_bit, hipStream_t s, RadixConfig cfg = {});
// clears the temp buffer for one keys-only sort and hands out its device histogram (to be enqueued BEFORE the kernel
// that counts into it)
hipError_t radix_keys_prepare_u64(void *temp, size_t temp_bytes, size_t n, int begin_bit, int end_bit, RadixConfig cfg,
                                  hipStream_t s, RadixHist *out);
hipError_t radix_init_temp(void *temp, hipStream_t s);                          // once per freshly allocated temp buffer
hipError_t radix_error_word(const void *temp, unsigned *out, hipStream_t s);  // sticky: 1 = some sort since then went wrong
const void *radix_error_device_word(const void *temp);  // where that word lives on the device (kernels that copy it along)

// ---- point renderer (render.hip) reads a simulation handle through these (nbmi.hip) ---------------
}  // namespace nbmi
struct nbmi_sim;
namespace nbmi {
int render_source(::nbmi_sim *s, int64_t *n, int *device);
int render_fetch(::nbmi_sim *s, float *d_pos, float *d_col, hipEvent_t done);
}  // namespace nbmi
struct bdmi_flock;
namespace nbmi {
// ---- triangle rasteriser (raster.hip) reads a flock handle through these (bdmi.hip) ----------------
int flock_source(::bdmi_flock *f, int64_t *n, int *device, int *slab);
// Frustum test + cone building of bdmi_visible_vertices, left on the device: (6 count, 3) float32 vertices and
// colours in the handle's scratch, valid until the handle's next call.  Returns with the flock's stream idle.
int flock_visible_device(::bdmi_flock *f, const double *cam12, double tan_h, double tan_v, double fog_end,
                         double cone_length, double cone_radius, const float **d_verts, const float **d_cols,
                         int64_t *count, hipEvent_t done);

// One body of a key-sorted run as it travels between GPUs (multi-GPU run exchange): the two
// octant-path key words and the fp32 {x, y, z, G*m} the octree is built from.  32 bytes.
struct RunRec {
    uint64_t hi, lo;
    float x, y, z, gm;
};

// ---- device-side initial conditions (icgen.hip) ---------------------------------------------
#define NBMI_IC_GALAXY 0
#define NBMI_IC_COLLISION 1
#define NBMI_IC_CLUSTER 2
#define NBMI_IC_SPIRAL 3
#define NBMI_IC_FILAMENT 4
struct IcArrays {
    double *x, *y, *z, *vx, *vy, *vz, *m;
    int32_t *id;
};
int ic_generate(int distribution, int64_t n, double R, double G, uint64_t seed, IcArrays out, hipStream_t s);

// Philox4x32-10 (Salmon et al., SC'11): counter-based generator, 4 x 32 bits per call.
__host__ __device__ inline void philox4x32_10(const uint32_t ctr_in[4], const uint32_t key_in[2], uint32_t out[4]) {
    uint32_t c0 = ctr_in[0], c1 = ctr_in[1], c2 = ctr_in[2], c3 = ctr_in[3];
    uint32_t k0 = key_in[0], k1 = key_in[1];
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
}  // namespace nbmi
