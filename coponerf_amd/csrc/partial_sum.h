// The fixed-order sums of partial results, once each.  Two keep the training gradients bit-reproducible: the reducers of
// ufc_wgrad.hip and ufc_strided_bwd.hip (sum_partials_16x64), of wgrad_f32.hip and wgrad_tall.hip (sum_slabs_f32x4).  The third
// is the float64 finish of the image-side units (sum_partials_f64: image_metrics.hip, ssim_warp.hip, lpips.hip, summaries.hip).
// The fourth adds the block counts of the stream compaction (sum_counts_256: compact.h) in the same thread order.
#pragma once
#include "common.h"

namespace {

// Body of a 1 024-thread workgroup that finishes the outputs blockIdx.x * 64 + lane < n_out from n_part partials each:
//   wave p (0 .. 15) adds the partials p, p + 16, p + 32, ... in ascending order, starting from 0.0f;
//   wave 0 then adds the 16 wave sums in the order 0 .. 15, starting from 0.0f, and stores.
// load(part, out) returns a partial, store(out, value) writes the result.  Eight loads are in flight per thread (issued
// together, added in ascending order), the rest is walked with stride 16: the same sequence of additions either way.
// Why 16 x 64: few outputs, hundreds of partials; one thread per output waits for one load at a time on a handful of
// workgroups.  Measured per call: 4 waves walking 64 partials each took 17 us (conv_wgrad_planes); one thread per output
// 70 us on 40 workgroups, 2.4 x the kernel that produces the partials (dwconv3x3_tokens_wgrad), and 21 us on five (strided
// Conv4d).  Must be called by all threads of the workgroup (contains a barrier).
template <class Load, class Store>
__device__ __forceinline__ void sum_partials_16x64(int n_out, long long n_part, Load load, Store store) {
    __shared__ float sh[16][64];
    const int j = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + j;
    float sacc = 0.0f;
    if (i < n_out) {
        long long b = wave;
        for (; b + 16 * 7 < n_part; b += 16 * 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = load(b + 16 * u, i);
#pragma unroll
            for (int u = 0; u < 8; ++u) sacc += v[u];
        }
        for (; b < n_part; b += 16) sacc += load(b, i);
    }
    sh[wave][j] = sacc;
    __syncthreads();
    if (wave != 0 || i >= n_out) return;
    float v = 0.0f;
#pragma unroll
    for (int q = 0; q < 16; ++q) v += sh[q][j];
    store(i, v);
}

// The float64 finish of n float partials of N values each, partial i holding its values at p[N i .. N i + N - 1] (image
// metrics, SSIM-warp, LPIPS, attention entropy).  Called by a workgroup of NT threads, for value k:
//   thread t adds p[N i + k] for i = t, t + NT, t + 2 NT, ... in ascending order, each widened to double, starting from 0.0;
//   wave_sum's butterfly (xor 32, 16, .. 1) then adds the 64 lanes of each wave.
// s[k] is returned in every lane of a wave.  NT = 64: the sum itself; NT = 256: four wave sums that block256_sum's second
// half (waves4_sum) finishes as (0 + 1) + (2 + 3).
template <int NT, int N>
__device__ __forceinline__ void sum_partials_f64(const float* __restrict__ p, int n, double (&s)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = 0.0;
    for (int i = threadIdx.x; i < n; i += NT) {
#pragma unroll
        for (int k = 0; k < N; ++k) s[k] += (double)p[N * i + k];          // N n < 2^31: the entry points check it
    }
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = wave_sum(s[k]);
}

// The sum of n integer block counts by a workgroup of 256 threads, sum_partials_f64's walk on integers: thread t adds
// p[t], p[t + 256], p[t + 512], ... in ascending order, block256_sum adds the threads.  One pass of the walk covers 256 counts.
// Returned in every thread; must be called by all 256 threads, once per kernel (waves4_sum's LDS).
__device__ __forceinline__ int sum_counts_256(const int* __restrict__ p, int n) {
    int s[1] = {0};
    for (int i = threadIdx.x; i < n; i += 256) s[0] += p[i];
    block256_sum(s);
    return s[0];
}

// Element i of the sum of nslab slabs of n4 16-byte vectors each, in slab order: part[i] + part[n4 + i] + part[2 n4 + i] ...
__device__ __forceinline__ f32x4 sum_slabs_f32x4(const float* __restrict__ part, long long n4, int nslab, long long i) {
    f32x4 s = reinterpret_cast<const f32x4*>(part)[i];
#pragma unroll 8
    for (int q = 1; q < nslab; ++q) s += reinterpret_cast<const f32x4*>(part)[q * n4 + i];
    return s;
}

}  // namespace
