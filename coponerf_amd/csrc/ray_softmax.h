// The joint softmax over the T = V*S samples of one ray by one 256-thread workgroup - the one form of it behind
// cpn_attend_hidden, cpn_attend_hidden_f32 (attend.hip) and cpn_logit_guard (guard.hip), whose weights must be the same bits.
// The logits, already divided by 11.31f, sit in wts[0 .. T) of LDS; red is 8 floats of LDS.  Order of operations:
//   1. per-thread maximum over the rows the thread has seen (rows tid, tid + 256, ... when the logits are given; the rows of its
//      lane group when the caller formed them from qa . qb) - the caller's loop, handed in as lmax;
//   2. wave_max, then max(max(m0, m1), max(m2, m3)) over the four waves                                         -> gmax;
//   3. e = __expf(wts[row] - gmax), per-thread sums over rows tid, tid + 256, ... in that order;
//   4. wave_sum, then (s0 + s1) + (s2 + s3), and inv = 1.0f / that sum;
//   5. w = e * inv.
// ray_softmax_stats runs 2 - 4 and leaves either the logits (KEEP_LOGITS, the guard: it needs l next to w and forms e again,
// the same __expf of the same difference) or the exponentials in wts; ray_softmax_normalise runs 5 over stored exponentials.
// (cpn_attend_units forms its softmax per wave, in another order: attend_units.hip.)
#pragma once
#include "common.h"

struct RaySoftmax { float gmax, inv; };

// logits[0 .. T) / 11.31f -> wts, rows tid, tid + 256, ...; returns the thread's maximum (step 1 of the `logits` modes)
__device__ __forceinline__ float ray_logits_to_lds(const float* __restrict__ logits, float* __restrict__ wts, const int T) {
    float lmax = -INFINITY;
    for (int row = threadIdx.x; row < T; row += 256) {
        const float logit = logits[row] / 11.31f;
        wts[row] = logit;
        lmax = fmaxf(lmax, logit);
    }
    return lmax;
}

template <bool KEEP_LOGITS>
__device__ __forceinline__ RaySoftmax ray_softmax_stats(float lmax, float* __restrict__ wts, float* __restrict__ red, const int T) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    lmax = wave_max(lmax);
    if (lane == 0) red[wave] = lmax;
    __syncthreads();
    const float gmax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float lsum = 0.f;
    for (int row = tid; row < T; row += 256) {
        const float e = __expf(wts[row] - gmax);
        if constexpr (!KEEP_LOGITS) wts[row] = e;
        lsum += e;
    }
    lsum = wave_sum(lsum);
    if (lane == 0) red[4 + wave] = lsum;
    __syncthreads();
    return RaySoftmax{gmax, 1.0f / ((red[4] + red[5]) + (red[6] + red[7]))};
}

// wts[row] = e[row] * inv for the thread's rows; each weight is also handed to store(row, w).  No barrier behind it.
template <class Store>
__device__ __forceinline__ void ray_softmax_normalise(float* __restrict__ wts, const int T, const float inv, Store store) {
    for (int row = threadIdx.x; row < T; row += 256) {
        const float w = wts[row] * inv;
        wts[row] = w;
        store(row, w);
    }
}
