// The deterministic two-launch stream compaction, once: point_cloud.hip (cpn_compact_points) and matches.hip
// (cpn_compact_matches) both select elements of a pair's (view, row, column) sequence by a byte mask and differ only in what a
// selected element writes.  A workgroup of 256 threads owns CPN_COMPACT_TILE consecutive elements of the sequence.  The first
// launch stores compact_tile_count per workgroup; the second (compact_tile_rows) adds the counts of the workgroups before its
// own (sum_counts_256), ranks its own elements by wave ballots and hands every selected element its output row.  No atomics:
// an element's row depends on the mask alone.
#pragma once
#include "common.h"
#include "partial_sum.h"

namespace {

constexpr int COMPACT_NT = 256;
constexpr int COMPACT_SUB = CPN_COMPACT_TILE / COMPACT_NT;     // elements per thread of a compaction workgroup
static_assert(CPN_COMPACT_FINISH == COMPACT_NT && CPN_COMPACT_TILE % COMPACT_NT == 0, "the compaction kernels run 256 threads");

// Element j of pair b's sequence (cap = K hw of them) is pixel j % hw of view j / hw: its index in the (K, B, hw) arrays
__device__ __forceinline__ int seq_source(int j, int b, int B, int hw) {
    const int k = j / hw;
    return (k * B + b) * hw + (j - k * hw);                    // < K B hw < 2^31
}

// The number of selected elements of tile blockIdx.x, in every thread.  sel(j) is asked for j < cap only.  Must be called by
// all 256 threads, once per kernel (waves4_sum's LDS).
template <class Sel>
__device__ __forceinline__ int compact_tile_count(int cap, Sel sel) {
    int n[1] = {0};
    for (int s = 0; s < COMPACT_SUB; ++s) {
        const int j = blockIdx.x * CPN_COMPACT_TILE + s * COMPACT_NT + threadIdx.x;
        n[0] += (j < cap && sel(j)) ? 1 : 0;
    }
    block256_sum(n);
    return n[0];
}

// put(j, row) for every selected element j of tile blockIdx.x, row counting the selected elements of the pair before j;
// counts: the pair's tile counts of the first launch.  Returns, in every thread, the number of selected elements up to the
// end of this tile (the pair's count in the last tile).  Must be called by all 256 threads, once per kernel.
template <class Sel, class Put>
__device__ __forceinline__ int compact_tile_rows(const int* __restrict__ counts, int cap, Sel sel, Put put) {
    __shared__ int wc[COMPACT_SUB][4];                         // selected elements of wave wv in sub-tile s
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int before = sum_counts_256(counts, (int)blockIdx.x);
    int below[COMPACT_SUB];
    bool on[COMPACT_SUB];
    for (int s = 0; s < COMPACT_SUB; ++s) {
        const int j = blockIdx.x * CPN_COMPACT_TILE + s * COMPACT_NT + threadIdx.x;
        on[s] = j < cap && sel(j);
        const unsigned long long m = __ballot(on[s]);
        below[s] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wc[s][wave] = __popcll(m);
    }
    __syncthreads();
    int at = before;                                           // output row of the first element of (sub-tile, wave), in order
    for (int s = 0; s < COMPACT_SUB; ++s) {
        for (int wv = 0; wv < 4; ++wv) {
            if (wv == wave && on[s]) put(blockIdx.x * CPN_COMPACT_TILE + s * COMPACT_NT + (int)threadIdx.x, at + below[s]);
            at += wc[s][wv];
        }
    }
    return at;
}

}  // namespace
