// The flow warp shared by ssim_warp.hip and summaries.hip: F.interpolate(mode="bilinear") of a low-resolution flow, the
// reference's `warp` (utils_training/utils.py:642-671) and grid_sample's tap selection, each in the fp32 expression sequence
// of the stock ops.  Units that include this are compiled with -ffp-contract=off (csrc/build.py).
#pragma once
#include "common.h"

struct WarpTaps {
    int x0, y0, x1, y1;             // clamped tap indices (valid only where the flag is set)
    bool vx0, vx1, vy0, vy1;
    float wx0, wx1, wy0, wy1;       // ATen's (ix_se - ix), (ix - ix_nw), (iy_se - iy), (iy - iy_nw)
};

// ATen area_pixel_compute_source_index(align_corners=False): rs = in / out in fp32 (1 / s for an integer scale s)
__device__ __forceinline__ void up_index(int dst, float rs, int in, int& i0, int& i1, float& l0, float& l1) {
    float src = rs * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    i0 = i0 > in - 1 ? in - 1 : i0;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.0f - l1;
}

// s * bilinear(flow) at pixel (gx, gy) of the (H, W) grid: both components of fl (2, h, w)
__device__ __forceinline__ void up_flow(const float* __restrict__ fl, int h, int w, float s, float rs, int gx, int gy, float& ux,
                                        float& uy) {
    int xa, xb, ya, yb;
    float lx0, lx1, ly0, ly1;
    up_index(gx, rs, w, xa, xb, lx0, lx1);
    up_index(gy, rs, h, ya, yb, ly0, ly1);
    const float* const fx = fl;
    const float* const fy = fl + (size_t)h * w;
    ux = (ly0 * (lx0 * fx[ya * w + xa] + lx1 * fx[ya * w + xb]) + ly1 * (lx0 * fx[yb * w + xa] + lx1 * fx[yb * w + xb])) * s;
    uy = (ly0 * (lx0 * fy[ya * w + xa] + lx1 * fy[ya * w + xb]) + ly1 * (lx0 * fy[yb * w + xa] + lx1 * fy[yb * w + xb])) * s;
}

// utils.warp's normalisation of pixel (gx, gy) + flow (ux, uy), then grid_sample's unnormalisation, in their order
__device__ __forceinline__ void warp_coord(int H, int W, int gx, int gy, float ux, float uy, float& ix, float& iy) {
    const float vx = (float)gx + ux, vy = (float)gy + uy;
    const float nx = 2.0f * vx / (float)(W - 1 > 1 ? W - 1 : 1) - 1.0f;
    const float ny = 2.0f * vy / (float)(H - 1 > 1 ? H - 1 : 1) - 1.0f;
    ix = ((nx + 1.0f) * (float)W - 1.0f) / 2.0f;
    iy = ((ny + 1.0f) * (float)H - 1.0f) / 2.0f;
}

__device__ __forceinline__ void sample_coord(const float* __restrict__ fl, int h, int w, int H, int W, float s, float rs, int gx,
                                             int gy, float& ix, float& iy) {
    float ux, uy;
    up_flow(fl, h, w, s, rs, gx, gy, ux, uy);
    warp_coord(H, W, gx, gy, ux, uy, ix, iy);
}

// tap indices are formed only from floats known to lie inside the image: a coordinate of 1e9, inf or NaN selects no tap
__device__ __forceinline__ WarpTaps warp_taps(float ix, float iy, int H, int W) {
    WarpTaps t;
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const float fx1 = fx0 + 1.0f, fy1 = fy0 + 1.0f;
    t.vx0 = fx0 >= 0.f && fx0 <= (float)(W - 1);
    t.vx1 = fx1 >= 0.f && fx1 <= (float)(W - 1);
    t.vy0 = fy0 >= 0.f && fy0 <= (float)(H - 1);
    t.vy1 = fy1 >= 0.f && fy1 <= (float)(H - 1);
    t.x0 = t.vx0 ? (int)fx0 : 0;
    t.x1 = t.vx1 ? (int)fx1 : 0;
    t.y0 = t.vy0 ? (int)fy0 : 0;
    t.y1 = t.vy1 ? (int)fy1 : 0;
    t.wx0 = fx1 - ix;
    t.wx1 = ix - fx0;
    t.wy0 = fy1 - iy;
    t.wy1 = iy - fy0;
    return t;
}
