// The 11-tap sigma-1.5 SSIM window over a 16 x 32 tile with a 5-pixel halo, once: the tile geometry, the constants and the two
// separable passes that image_metrics.hip and ssim_warp.hip share.
//
// LDS of a forward tile: x and y, three channels each, as RH x RW planes (6 x 26 x 42 floats) and the five moments of ONE
// channel after the rows pass as RH x TW planes (5 x 26 x 32 floats) = 42.9 KB -> 3 workgroups per CU.  The rows of a wave are
// 42 or 32 floats apart, so the 32 lanes of one LDS pass read 32 consecutive banks.  ssim_warp.hip's backward keeps three
// planes of either size (23.1 KB).
//
// The window arrives as `const float*` because the two units hold DIFFERENT numbers on purpose and keep them where they
// are: the loss's window is normalised in fp32 as the reference's torch code does it (the caller's device tensor, copied to
// LDS), the metrics' in float64 as scipy does it (a by-value kernel argument).  Do not merge them.
//
// Every product-sum is an FMA asked for by name: image_metrics.hip is compiled with contraction on and ssim_warp.hip with
// -ffp-contract=off, and these bodies mean the same in both.  The SSIM quotients stay in their units (one is centred, the
// other is not, and an expression shared across two contraction settings would not keep both units' bits).
#pragma once
#include "common.h"

namespace {

constexpr int TW = 32, TH = 16, RAD = 5, WIN = 2 * RAD + 1;
constexpr int RW = TW + 2 * RAD, RH = TH + 2 * RAD;
constexpr int NT = 256;
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;       // (K1 L)^2, (K2 L)^2 at data_range L = 1

// Rows pass of one channel: x, y (RH x RW) -> sum_k g_k of x, y, x^2, y^2, x y at columns col .. col + 10, for every row of the
// halo, into sh[0 .. 4] (RH x TW).  k ascending from 0.0f.  All NT threads; the caller's barrier follows.
__device__ __forceinline__ void moment_rows(const float* win, const float* sx, const float* sy, float (*sh)[RH * TW]) {
    for (int idx = threadIdx.x; idx < RH * TW; idx += NT) {
        const int r = idx / TW, col = idx - r * TW;
        const float* const qx = &sx[r * RW + col];
        const float* const qy = &sy[r * RW + col];
        float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float g = win[k], x = qx[k], y = qy[k];
            m1 = __builtin_fmaf(g, x, m1);
            m2 = __builtin_fmaf(g, y, m2);
            e11 = __builtin_fmaf(g, x * x, e11);
            e22 = __builtin_fmaf(g, y * y, e22);
            e12 = __builtin_fmaf(g, x * y, e12);
        }
        sh[0][idx] = m1;
        sh[1][idx] = m2;
        sh[2][idx] = e11;
        sh[3][idx] = e22;
        sh[4][idx] = e12;
    }
}

// Columns pass at tile pixel (py, px): out[n] = sum_k g_k sh[n][(py + k) TW + px], k ascending from 0.0f, for N planes
template <int N>
__device__ __forceinline__ void window_cols(const float* win, const float (*sh)[RH * TW], int py, int px, float (&out)[N]) {
#pragma unroll
    for (int n = 0; n < N; ++n) out[n] = 0.f;
#pragma unroll
    for (int k = 0; k < WIN; ++k) {
        const float g = win[k];
        const int o = (py + k) * TW + px;
#pragma unroll
        for (int n = 0; n < N; ++n) out[n] = __builtin_fmaf(g, sh[n][o], out[n]);
    }
}

}  // namespace
