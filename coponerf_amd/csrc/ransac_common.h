// What ransac.hip and ransac5.hip share beside their arithmetic (epipolar_system.h, sampson.h): the sampler - the counter hash of
// include/coponerf_hip.h, round 20 -, the count clamp (matches.hip's refinement takes it too), the fp32 finite test, and the
// chunk and shape rule of the entry points.
#pragma once
#include "common.h"

namespace {

constexpr int CH = CPN_RANSAC_CHUNK;

__device__ __forceinline__ int clamp_count(int c, int N) { return c < 0 ? 0 : (c > N ? N : c); }
__device__ __forceinline__ bool finite32(float v) { return fabsf(v) <= 3.402823466e38f; }               // false for NaN

// B pairs of N rows and `slots` hypothesis slots (the 5-point solver's are 10 per sample): what the grids and the partial counts hold
inline bool shape_ok(int B, int N, long long slots) {
    return B >= 1 && B <= 32767 && N >= 1 && N <= (1 << 24) && slots >= 0 && slots <= (1 << 20) &&
           (long long)B * cpn_cdiv(N, CH) * (slots + 1) < (1LL << 31);
}
inline bool px_ok(double px) { return px >= 0.0 && px <= 1.79769313486231570815e308; }

}  // namespace

// For equal (seed, h, n) the K rows are the first K of any longer draw: the loop stops at K distinct rows, nothing else.
namespace ransac_draw {

constexpr int DRAWS = 64;
constexpr unsigned long long GOLDEN = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {      // splitmix64's finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// K distinct rows below n for hypothesis h in the order drawn, -1 where none was -> the number drawn
template <int K>
__device__ __forceinline__ int draw_rows(unsigned long long seed, int h, int n, int (&s)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) s[j] = -1;
    int got = 0;
    const unsigned long long key = mix64(seed + GOLDEN * (unsigned long long)(h + 1));
    for (int d = 0; d < DRAWS && got < K; ++d) {
        const unsigned long long u = mix64(key + GOLDEN * (unsigned long long)(d + 1));
        const int idx = (int)(((u >> 32) * (unsigned long long)n) >> 32);
        bool dup = false;
#pragma unroll
        for (int j = 0; j < K; ++j) dup = dup || s[j] == idx;
        if (!dup && n > 0) {
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (j == got) s[j] = idx;
            ++got;
        }
    }
    return got;
}

}  // namespace ransac_draw
