// Shared helpers for the gfx950 kernels of libcoponerf_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/coponerf_hip.h"

void cpn_set_error(const char* fmt, ...);
// CUs a launch on `stream` may occupy: the device's count, or the share of a CU-masked stream (streams.cpp)
int cpn_stream_cus(void* stream);

#define CPN_REQUIRE(cond, code, ...)                 \
    do {                                             \
        if (!(cond)) {                               \
            cpn_set_error(__VA_ARGS__);              \
            return (code);                           \
        }                                            \
    } while (0)

#define CPN_LAUNCH_CHECK(name)                                                   \
    do {                                                                         \
        hipError_t e_ = hipGetLastError();                                       \
        if (e_ != hipSuccess) {                                                  \
            cpn_set_error("%s: launch failed: %s", name, hipGetErrorString(e_)); \
            return (int)e_;                                                      \
        }                                                                        \
    } while (0)

static inline unsigned cpn_cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// Index of sample s of ray r as view v of batch element b sees it, in the (B V, R, S) arrays that travel per sample: at_wt,
// dw_ext, the parked w1 / w2, and - times 2 or 6 at the call site - pixel_val, sec_grid and the point encodings.
// (Here rather than in encode_geometry.h: rayout.hip, gemm_f16.hip and attend.hip have no use for the node tables.)
__host__ __device__ __forceinline__ size_t sample_index(int b, int V, int v, int R, int r, int S, int s) {
    return (((size_t)(b * V + v)) * R + r) * S + s;
}

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// sum / maximum of a value over the 64 lanes of a wave, returned in every lane (xor butterfly, 32 .. 1); float or double
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the same over each aligned group of 16 lanes (xor butterfly, 8 .. 1), returned in every lane of the group
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

namespace {          // internal linkage: the LDS scratch below belongs to the kernel of the unit that uses it

// N values that each of the four waves of a 256-thread workgroup holds (the same in all lanes of a wave), summed over the
// waves behind ONE barrier: wave w parks its values in LDS, every thread then reads (w0 + w1) + (w2 + w3).  Must be called
// by all 256 threads, once per kernel and value type (a second use would need a barrier before it parks again).
template <class T, int N>
__device__ __forceinline__ void waves4_sum(T (&v)[N]) {
    __shared__ T red[N][4];
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int n = 0; n < N; ++n) red[n][threadIdx.x >> 6] = v[n];
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = (red[n][0] + red[n][1]) + (red[n][2] + red[n][3]);
}
// N per-thread values summed over a 256-thread workgroup: wave_sum's butterfly in each wave, then waves4_sum
template <class T, int N>
__device__ __forceinline__ void block256_sum(T (&v)[N]) {
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = wave_sum(v[n]);
    waves4_sum(v);
}

}  // namespace
