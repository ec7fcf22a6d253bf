// Test / measurement hooks of the device sort (radix.hip): nbmi_debug_sort_pairs / nbmi_debug_sort_keys run the product's
// sorts on caller-supplied host arrays.  rocPRIM is not compiled into the product: its cross-check lives in
// tests/native/rocprim_check.hip (a test-only library that tests/test_gpu_sort.py compares this sort with, bit for bit).
#include <cstdlib>
#include <cstring>

#include "../../include/nbmi.h"
#include "common.h"

// The hooks' temp buffer: ONE per process, kept from call to call and only ever grown, so that successive sorts of
// different sizes, fields and configurations run on the same buffer as a handle's do - what a sort leaves behind in it
// is the next one's to clear.  Used on the default device, one call at a time.
static void *g_tmp = nullptr;
static size_t g_tmp_bytes = 0;
static hipError_t debug_temp(size_t need, hipStream_t st, void **out) {
    if (need > g_tmp_bytes) {
        if (g_tmp) (void)hipFree(g_tmp);
        g_tmp = nullptr;
        g_tmp_bytes = 0;
        if (hipError_t e = hipMalloc(&g_tmp, need)) return e;
        g_tmp_bytes = need;
        if (hipError_t e = nbmi::radix_init_temp(g_tmp, st)) return e;
    }
    *out = g_tmp;
    return hipSuccess;
}

// values == null: the keys-only form on the bits [begin_bit, end_bit); otherwise pairs.
static int debug_sort(const char *who, int key_bytes, int64_t n, const void *keys, const uint32_t *values, void *keys_out,
                      uint32_t *values_out, int begin_bit, int end_bit, int repeats, double *ms_per_sort,
                      nbmi::RadixConfig cfg = {}) {
    if (n == 0) return 0;
    const bool pairs = values != nullptr;
    const int bits = end_bit - begin_bit;
    const size_t kb = (size_t)n * key_bytes, vb = (size_t)n * 4;
    const size_t own = pairs ? (key_bytes == 8 ? nbmi::radix_temp_bytes_u64(n, bits) : nbmi::radix_temp_bytes_u32(n, bits))
                             : (key_bytes == 8 ? nbmi::radix_keys_temp_bytes_u64(n, bits) : nbmi::radix_keys_temp_bytes_u32(n, bits));
    size_t tb = own + 256;
    void *dk = nullptr, *dko = nullptr, *dv = nullptr, *dvo = nullptr, *tmp = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = 0;
    auto fail = [&](const char *what, hipError_t e) {
        nbmi::set_error("%s: %s: %s", who, what, hipGetErrorString(e));
        rc = NBMI_ERR_HIP;
    };
    hipError_t e;
    if ((e = hipMalloc(&dk, kb)) || (e = hipMalloc(&dko, kb)) || (pairs && ((e = hipMalloc(&dv, vb)) || (e = hipMalloc(&dvo, vb)))) ||
        (e = hipStreamCreate(&st)) || (e = debug_temp(tb, st, &tmp)) || (e = hipEventCreate(&e0)) || (e = hipEventCreate(&e1)) ||
        (e = hipMemcpyAsync(dk, keys, kb, hipMemcpyHostToDevice, st)) ||
        (pairs && (e = hipMemcpyAsync(dv, values, vb, hipMemcpyHostToDevice, st))))
        fail("setup", e);
    for (int r = 0; rc == 0 && r < (repeats < 1 ? 1 : repeats) + 1; r++) {  // first run untimed
        if (r == 1) (void)hipEventRecord(e0, st);
        if (!pairs && key_bytes == 8) {
            e = nbmi::radix_sort_keys_u64(tmp, tb, (const uint64_t *)dk, (uint64_t *)dko, (size_t)n, begin_bit, end_bit, st, cfg);
        } else if (!pairs) {
            e = nbmi::radix_sort_keys_u32(tmp, tb, (const uint32_t *)dk, (uint32_t *)dko, (size_t)n, begin_bit, end_bit, st, cfg);
        } else if (key_bytes == 8) {
            e = nbmi::radix_sort_pairs_u64(tmp, tb, (const uint64_t *)dk, (uint64_t *)dko, (const uint32_t *)dv,
                                           (uint32_t *)dvo, (size_t)n, begin_bit, end_bit, st, cfg);
        } else {
            e = nbmi::radix_sort_pairs_u32(tmp, tb, (const uint32_t *)dk, (uint32_t *)dko, (const uint32_t *)dv,
                                           (uint32_t *)dvo, (size_t)n, begin_bit, end_bit, st, cfg);
        }
        if (e != hipSuccess) fail("sort", e);
    }
    if (rc == 0) {
        (void)hipEventRecord(e1, st);
        unsigned err = 0;
        (void)nbmi::radix_error_word(tmp, &err, st);
        if ((e = hipMemcpyAsync(keys_out, dko, kb, hipMemcpyDeviceToHost, st)) ||
            (pairs && (e = hipMemcpyAsync(values_out, dvo, vb, hipMemcpyDeviceToHost, st))) || (e = hipStreamSynchronize(st)))
            fail("copy back", e);
        float ms = 0.f;
        if (rc == 0 && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms_per_sort)
            *ms_per_sort = ms / (repeats < 1 ? 1 : repeats);
        if (rc == 0 && err) {
            nbmi::set_error("%s: a look-back spin timed out", who);
            rc = NBMI_ERR_HIP;
            (void)nbmi::radix_init_temp(tmp, st);  // the sticky word has been reported
            (void)hipStreamSynchronize(st);
        }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (st) (void)hipStreamDestroy(st);
    for (void *q : {dk, dko, dv, dvo})
        if (q) (void)hipFree(q);
    return rc;
}

// impl must be 0
extern "C" int nbmi_debug_sort_pairs(int key_bytes, int64_t n, const void *keys, const uint32_t *values, void *keys_out,
                                     uint32_t *values_out, int bits, int impl, int repeats, double *ms_per_sort) {
    if ((key_bytes != 4 && key_bytes != 8) || n < 0 || bits < 1 || bits > 8 * key_bytes || (n && (!keys || !values)) || impl != 0) {
        nbmi::set_error("nbmi_debug_sort_pairs: bad arguments");
        return NBMI_ERR_ARG;
    }
    return debug_sort("nbmi_debug_sort_pairs", key_bytes, n, keys, values, keys_out, values_out, 0, bits, repeats, ms_per_sort);
}

extern "C" int nbmi_debug_sort_keys(int key_bytes, int64_t n, const void *keys, void *keys_out, int begin_bit, int end_bit,
                                    int repeats, double *ms_per_sort) {
    if ((key_bytes != 4 && key_bytes != 8) || n < 0 || begin_bit < 0 || end_bit <= begin_bit || end_bit > 8 * key_bytes ||
        end_bit - begin_bit > 64 || (n && (!keys || !keys_out))) {
        nbmi::set_error("nbmi_debug_sort_keys: bad arguments");
        return NBMI_ERR_ARG;
    }
    return debug_sort("nbmi_debug_sort_keys", key_bytes, n, keys, nullptr, keys_out, nullptr, begin_bit, end_bit, repeats, ms_per_sort);
}

// Either form (values == null: keys only) with the passes' digit width (8 or 10) and threads per tile (256, 512 or
// 1024) given, so that small inputs reach the configurations the size rule keeps for large ones; 0 = by the size rule.
extern "C" int nbmi_debug_sort_config(int key_bytes, int64_t n, const void *keys, const uint32_t *values, void *keys_out,
                                      uint32_t *values_out, int begin_bit, int end_bit, int digit_bits, int threads, int repeats,
                                      double *ms_per_sort) {
    const nbmi::RadixConfig cfg{digit_bits, threads};
    if ((key_bytes != 4 && key_bytes != 8) || n < 0 || begin_bit < 0 || end_bit <= begin_bit || end_bit > 8 * key_bytes ||
        (n && (!keys || !keys_out)) || (n && values && !values_out) || !nbmi::radix_config_ok(cfg)) {
        nbmi::set_error("nbmi_debug_sort_config: bad arguments");
        return NBMI_ERR_ARG;
    }
    return debug_sort("nbmi_debug_sort_config", key_bytes, n, keys, values, keys_out, values_out, begin_bit, end_bit, repeats, ms_per_sort,
                      cfg);
}
