// Exact order statistics of non-negative doubles by a radix descent, for ONE workgroup of NT threads: what cpn_residual_stats
// (pose_eval.hip, round 25 of include/coponerf_hip.h) and cpn_depth_scale (triangulate.hip, round 26) rank with, once.
//
// Non-negative doubles order as their 64-bit patterns.  The descent takes the pattern 8 bits a pass from the top: every pass
// counts, per wanted rank ("slot"), the digits of the rows that carry the prefix found so far, and takes the first digit whose
// rows reach beyond the rank.  The value being ranked is a template parameter: `value(i, v)` says whether row i takes part and
// writes its value, and is called again in every pass - it must return the same bits every time, so nothing is kept in global
// memory.  The counts are integer LDS adds, which do not depend on the order of arrival: the result is the same every run.
// Eight passes over the rows, no sort.  tests/pose_eval_ref.py's radix_select restates the descent.
#pragma once
#include "common.h"

namespace {
namespace radix {

constexpr int DIGITS = 8, BINS = 256;                      // 8 passes of 8 bits

template <int SLOTS>
struct Select {
    int hist[SLOTS][BINS];
    unsigned long long prefix[SLOTS];                      // the digits found so far, in place
    long long rank[SLOTS];                                 // the wanted rank among the rows that carry the prefix
};

__device__ __forceinline__ unsigned long long key_of(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ double value_of(unsigned long long key) { return __longlong_as_double((long long)key); }

// the digit that holds rank k of a histogram - the first whose rows reach beyond k -; k becomes the rank among that digit's rows
__device__ __forceinline__ int descend(const int* hist, long long& k) {
    long long below = 0;
    int d = 0;
    for (; d < BINS - 1; ++d) {                            // the last digit takes what is left
        const int c = hist[d];
        if (k < below + c) break;
        below += c;
    }
    k -= below;
    return d;
}

// Pass 0: the top digit of every row below n that takes part, into hist[0] -> their number, in every thread.  each(v) is
// called once per such row (cpn_residual_stats counts the rows within its thresholds there).  Ends behind a barrier.
template <int NT, int SLOTS, class Value, class Each>
__device__ __forceinline__ int top_digits(Select<SLOTS>& sh, int n, Value value, Each each) {
    const int tid = threadIdx.x;
    for (int i = tid; i < BINS; i += NT) sh.hist[0][i] = 0;
    __syncthreads();
    int last = -1, run = 0;                                // equal digits in a row - the rule, at the top - make one add
    for (int i = tid; i < n; i += NT) {
        double v;
        if (!value(i, v)) continue;
        const int d = (int)(key_of(v) >> 56);
        if (d != last) {
            if (run) atomicAdd(&sh.hist[0][last], run);
            last = d;
            run = 0;
        }
        ++run;
        each(v);
    }
    if (run) atomicAdd(&sh.hist[0][last], run);
    __syncthreads();
    int total = 0;
    for (int d = 0; d < BINS; ++d) total += sh.hist[0][d]; // every thread, the same integers
    return total;
}

// Passes 1 .. 7 for `slots` <= SLOTS ranks: rank_of(j) is the wanted rank of slot j among the rows top_digits counted (it is
// asked by thread j alone).  Afterwards prefix[j] is the pattern of the element of that rank; ends behind a barrier.
template <int NT, int SLOTS, class Value, class Rank>
__device__ __forceinline__ void select(Select<SLOTS>& sh, int slots, int n, Value value, Rank rank_of) {
    const int tid = threadIdx.x;
    if (tid < slots) {
        long long k = rank_of(tid);
        sh.prefix[tid] = (unsigned long long)descend(sh.hist[0], k) << 56;
        sh.rank[tid] = k;
    }
    __syncthreads();
    for (int pass = 1; pass < DIGITS; ++pass) {
        const int shift = 56 - 8 * pass;
        for (int i = tid; i < slots * BINS; i += NT) (&sh.hist[0][0])[i] = 0;
        unsigned long long want[SLOTS];
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) want[j] = j < slots ? sh.prefix[j] >> (shift + 8) : ~0ull;      // no key has all 56 bits set
        __syncthreads();
        for (int i = tid; i < n; i += NT) {
            double v;
            if (!value(i, v)) continue;
            const unsigned long long key = key_of(v);
            const unsigned long long head = key >> (shift + 8);
            const int d = (int)(key >> shift) & (BINS - 1);
#pragma unroll
            for (int j = 0; j < SLOTS; ++j)
                if (head == want[j]) atomicAdd(&sh.hist[j][d], 1);
        }
        __syncthreads();
        if (tid < slots) {
            long long k = sh.rank[tid];
            sh.prefix[tid] |= (unsigned long long)descend(sh.hist[tid], k) << shift;
            sh.rank[tid] = k;
        }
        __syncthreads();
    }
}

}  // namespace radix
}  // namespace
