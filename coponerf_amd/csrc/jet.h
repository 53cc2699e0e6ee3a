// matplotlib's index rule for `jet` over depth / 10 on a float32 array, once (summaries.hip's depth_jet_kernel, novel_views.hip's
// pack_frames_kernel): the value times the table size, truncated, clamped to the table; a NaN takes the map's `bad` entry.
#pragma once
#include "common.h"

constexpr int JET_N = 256;

// row of the JET_N x 3 table for a depth, or -1 for a NaN (`bad`: black).  Each operation rounded on its own.
__device__ __forceinline__ int jet_index(float depth) {
    const float x = (depth / 10.0f) * (float)JET_N;
    if (!(x == x)) return -1;
    return x < 0.f ? 0 : (x >= (float)JET_N ? JET_N - 1 : (int)x);
}
