// The renderer handle shared by the point renderer (render.hip) and the triangle rasteriser (raster.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct nbmi_render {
    int W = 0, H = 0, device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[7] = {};
    hipEvent_t ev_src = nullptr;
    bool timed = false;
    // inputs
    float *d_pos = nullptr, *d_col = nullptr;  // N x 3 each
    float *h_stage = nullptr;                  // pinned upload staging, 6 N floats
    int64_t cap_pts = 0;
    // per point / per tile
    uint64_t *rec = nullptr;
    uint32_t *tile_cnt = nullptr;
    uint64_t *tile_off = nullptr;
    // fragments
    uint32_t *keys = nullptr, *vals = nullptr, *keys2 = nullptr, *vals2 = nullptr;
    uint64_t *tile_min = nullptr, *tile_pre = nullptr;
    void *sort_tmp = nullptr;
    size_t sort_bytes = 0;
    int64_t cap_frags = 0;
    // image
    unsigned long long *acc = nullptr, *stats = nullptr;
    uint8_t *d_img = nullptr, *h_img = nullptr;
    uint64_t *h_small = nullptr;  // pinned: [0] fragment total, [1..4] stats, [5] sort error word
    int64_t last_stats[4] = {0, 0, 0, 0};
    // triangle frames (raster.hip), allocated at the first one
    bool tri_frame = false;                    // the last frame was one: ev[0..3] = start, rasterised, resolved, copied
    unsigned long long *zbuf = nullptr;        // W H words (depth << 32 | triangle)
    unsigned long long *tri_ctl = nullptr;     // stats[4], large-list counter, error word
    void *tri_large = nullptr;                 // large-triangle list
    int64_t cap_large = 0;
    float *d_tri = nullptr, *h_tri = nullptr;  // uploaded vertices then colours, 9 floats per triangle each; pinned staging
    int64_t cap_tri = 0;
};

namespace nbmi {
void raster_free(::nbmi_render *r);  // raster.hip: the triangle path's buffers
}
