// The z-buffer of splat.hip (points) and raster.hip (faces), once: (K, B, H, W) 64-bit keys (bits of the fp32 depth) << 32 | row,
// all ones where nothing fell.  The minimum of a set of integers does not depend on the order in which they arrive, so two
// runs give the same bytes (include/coponerf_hip.h).
#pragma once
#include "common.h"

namespace {

constexpr unsigned long long ZBUF_EMPTY = ~0ULL;

// z32 >= 0: the bit patterns of such floats are ordered as their values; equal depths fall to the lower row
__device__ __forceinline__ unsigned long long zbuf_key(float z32, unsigned row) {
    return ((unsigned long long)__float_as_uint(z32) << 32) | row;
}
// keys only decrease: a stored key that is already smaller when it is read stays smaller, and needs no atomic
__device__ __forceinline__ void zbuf_min(unsigned long long* p, unsigned long long key) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(p, key);
}
__device__ __forceinline__ unsigned zbuf_row(unsigned long long key) { return (unsigned)key; }
// a row beyond the `cap` rows its writer could name reads nothing
__device__ __forceinline__ bool zbuf_hit(unsigned long long key, int cap) { return key != ZBUF_EMPTY && zbuf_row(key) < (unsigned)cap; }

// background = r | g << 8 | b << 16: the bytes of a pixel nothing fell on
__device__ __forceinline__ void zbuf_background(int background, uint8_t (&out)[3]) {
    for (int ch = 0; ch < 3; ++ch) out[ch] = (uint8_t)((background >> (8 * ch)) & 255);
}
// what a resolved pixel stores: its bytes, on request the depth (NaN where empty) and the row (-1 where empty)
__device__ __forceinline__ void zbuf_store(int i, bool hit, unsigned long long key, const uint8_t (&out)[3],
                                           uint8_t* __restrict__ frames, float* __restrict__ depth, int* __restrict__ index) {
    for (int ch = 0; ch < 3; ++ch) frames[(size_t)i * 3 + ch] = out[ch];
    if (depth) depth[i] = hit ? __uint_as_float((unsigned)(key >> 32)) : __builtin_nanf("");
    if (index) index[i] = hit ? (int)zbuf_row(key) : -1;
}

bool image_ok(int K, int B, int H, int W) {
    return K >= 1 && K <= 255 && B >= 1 && H >= 1 && W >= 1 && (long long)K * B * H * W < (1LL << 31);
}

// max_side > 0: the longest side the caller's pixel arithmetic allows
int check_image(const char* who, int K, int B, int H, int W, int max_side = 0) {
    CPN_REQUIRE(image_ok(K, B, H, W), CPN_E_SHAPE,
                "%s: need 1 <= K <= 255 cameras, B, H, W >= 1 and K B H W < 2^31 (got K %d, B %d, H %d, W %d)", who, K, B, H, W);
    CPN_REQUIRE(max_side <= 0 || (H <= max_side && W <= max_side), CPN_E_SHAPE, "%s: need H, W <= %d", who, max_side);
    return 0;
}

// every key all ones, in stream order before the kernel that takes the minima
int zbuf_clear(unsigned long long* zbuf, int K, int B, int H, int W, hipStream_t stream, const char* who) {
    const hipError_t e = hipMemsetAsync(zbuf, 0xFF, (size_t)K * B * H * W * sizeof(unsigned long long), stream);
    CPN_REQUIRE(e == hipSuccess, (int)e, "%s: clearing the z-buffer failed: %s", who, hipGetErrorString(e));
    return 0;
}

}  // namespace
