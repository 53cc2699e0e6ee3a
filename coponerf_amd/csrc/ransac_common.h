// What ransac.hip, ransac5.hip and ransac_h.hip share beside their arithmetic (epipolar_system.h, sampson.h): the sampler - the
// counter hash of include/coponerf_hip.h, round 20 -, the count clamp (matches.hip's refinement takes it too), the fp32 finite
// test, the chunk and shape rule of the entry points, and the finish kernels' block reduction, usable count and winner.
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

// ---- what the finish kernels of ransac.hip and ransac_h.hip share: one workgroup of 256 per pair
// a value of every thread of the 256 combined by op, returned in every thread; red: 4 values in LDS
template <class Op>
__device__ __forceinline__ long long block_all(long long v, Op op, long long* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    __syncthreads();                                       // red is free of its last use
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return op(op(red[0], red[1]), op(red[2], red[3]));
}
__device__ __forceinline__ long long add_ll(long long x, long long y) { return x + y; }
__device__ __forceinline__ long long larger_ll(long long x, long long y) { return x > y ? x : y; }

// the rows below n with four finite values, in every thread
__device__ __forceinline__ long long usable_rows(const float* __restrict__ rows, int n, long long* red) {
    long long mine = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float* const m = rows + (size_t)i * 4;
        mine += (finite32(m[0]) && finite32(m[1]) && finite32(m[2]) && finite32(m[3])) ? 1 : 0;
    }
    return block_all(mine, add_ll, red);
}
// the winner among the pair's Hn hypotheses: most inliers - the sum of `used` partial counts, `width` apart -, the lower index on
// ties: the largest of count << 32 | ~index over the valid ones, -1 where there is none or `score` is false; n_valid: the valid ones
__device__ __forceinline__ long long best_hypothesis(const uint8_t* __restrict__ valid, const int* __restrict__ part, int Hn, int width,
                                                     int used, bool score, long long* red, long long& n_valid) {
    long long best = -1;
    n_valid = 0;
    for (int h = threadIdx.x; h < Hn; h += 256) {
        if (!valid[h]) continue;
        ++n_valid;
        if (!score) continue;
        long long sum = 0;
        for (int c = 0; c < used; ++c) sum += part[(size_t)c * width + h];
        best = larger_ll(best, (sum << 32) | (long long)(0x7FFFFFFF - h));
    }
    best = block_all(best, larger_ll, red);
    n_valid = block_all(n_valid, add_ll, red);
    return best;
}
__device__ __forceinline__ long long smaller_ll(long long x, long long y) { return x < y ? x : y; }

// best_hypothesis for scores that need all 64 bits (round 24: a graded sum reaches 2^44) and for the ranks beyond the first: the
// order is (score descending, slot ascending) as a PAIR; slot -1 stands for "none" and ranks behind every slot.
struct Ranked {
    long long score;
    int slot;
};
__device__ __forceinline__ bool ranks_before(long long sa, int ha, long long sb, int hb) {
    return ha >= 0 && (hb < 0 || sa > sb || (sa == sb && ha < hb));
}
// the first in that order of one candidate per thread, in every thread: the largest score, then its lowest slot
__device__ __forceinline__ Ranked first_ranked(long long score, int slot, long long* red) {
    const long long best = block_all(slot >= 0 ? score : -1, larger_ll, red);
    const long long at = block_all((slot >= 0 && score == best) ? slot : 0x7FFFFFFF, smaller_ll, red);
    Ranked r;
    r.score = best < 0 ? 0 : best;
    r.slot = best < 0 ? -1 : (int)at;
    return r;
}

// The first `want` + 1 <= DEPTH of the `slots` slots h with ok(h) in that order - their score the int64 sum of `used`
// partials, `width` apart - in ONE sweep: thread t keeps the DEPTH best of its slots t, t + 256, .. in registers (a chain
// of compare-and-swaps at fixed indices: no private array under a runtime index), sorted; then want + 1 times the workgroup
// takes the first of the threads' heads and the thread that held it moves its chain up -> the one taken last (rank `want`),
// slot -1 where there are no more than `want` such slots; in every thread.  (k + 1 sweeps of a winner search give the same
// slot; on 10 240 slots and 24 chunks they took 1.69 ms of the polish kernel's 1.93.)  The finish asks for the winner alone:
// DEPTH 1.
template <int DEPTH, class Ok>
__device__ __forceinline__ Ranked ranked_slot(Ok ok, const int* __restrict__ part, int slots, int width, int used, int want,
                                              long long* red) {
    long long top_score[DEPTH];
    int top_slot[DEPTH];
#pragma unroll
    for (int j = 0; j < DEPTH; ++j) {
        top_score[j] = 0;
        top_slot[j] = -1;
    }
    for (int h = threadIdx.x; h < slots; h += 256) {
        if (!ok(h)) continue;
        long long s = 0;
        for (int c = 0; c < used; ++c) s += part[(size_t)c * width + h];
        int at = h;
#pragma unroll
        for (int j = 0; j < DEPTH; ++j)
            if (ranks_before(s, at, top_score[j], top_slot[j])) {        // the better one stays, the other moves down the chain
                const long long ts = top_score[j];
                const int th = top_slot[j];
                top_score[j] = s;
                top_slot[j] = at;
                s = ts;
                at = th;
            }
    }
    Ranked r = {0, -1};
    for (int k = 0; k <= want; ++k) {
        r = first_ranked(top_score[0], top_slot[0], red);
        if (r.slot < 0) break;
        if (top_slot[0] == r.slot) {
#pragma unroll
            for (int j = 0; j + 1 < DEPTH; ++j) {
                top_score[j] = top_score[j + 1];
                top_slot[j] = top_slot[j + 1];
            }
            top_slot[DEPTH - 1] = -1;
        }
    }
    return r;
}

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
