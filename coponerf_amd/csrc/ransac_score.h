// The scoring of hypotheses against matches, once: cpn_ransac_score (ransac.hip: essential matrices under the Sampson rule) and
// cpn_ransac_score_h (ransac_h.hip: homographies under the transfer rule) are this kernel with two rules.
//
// Grid (tiles of 256 slots, chunks of CPN_RANSAC_CHUNK matches, pairs).  The workgroup normalises its chunk into LDS once and
// packs the tile's slots that have something to count to its first lanes (a ballot and four counts: invalid slots, most of the
// 5-point solver's, write their 0 and cost no wave); each lane then holds one model in registers and walks the chunk - every lane
// reads the same LDS address, a broadcast - and counts in a register.  Integers only, no atomics.
//
// The launch scores the Hn models of M into the columns first .. first + Hn - 1 of partial's rows of `width` columns; the launch
// whose models end the row (first + Hn + EXTRA == width) also scores the extra slot into the last column.  The round-20 entry
// points pass first = 0 and width = Hn + EXTRA; cpn_ransac_score_slots (round 24) scores the polished slots beside the others.
// GRADED: the sum of Rule::weight - the fixed-point MSAC of round 24, at most 2^20 a match and 2^28 a chunk - instead of the count.
//
// A Rule holds one model in registers:
//   Rule::EXTRA                      1: slot Hn is rel_pose's own model where rel_pose is given; 0: Hn slots, rel_pose is not read
//   void from_matrix(const double*)  the 9 doubles of a hypothesis
//   void from_pose(const float*)     rel_pose's 16 floats (EXTRA == 1 only)
//   bool inlier(k0, k1, a0, a1, b0, b1, px)
//   int weight(k0, k1, a0, a1, b0, b1, px)   0 where inlier() is false, otherwise 0 .. 2^20 (GRADED launches only)
#pragma once
#include "pinhole.h"
#include "ransac_common.h"

namespace {

constexpr int SCORE_NT = 256;

template <class Rule, bool GRADED = false>
__global__ __launch_bounds__(SCORE_NT) void ransac_score_kernel(const double* __restrict__ M, const uint8_t* __restrict__ valid,
                                                                const float* __restrict__ xy, const int* __restrict__ count,
                                                                const float* __restrict__ intrinsics,
                                                                const float* __restrict__ rel_pose, int N, int Hn, int first, int width,
                                                                double inlier_px, int* __restrict__ partial) {
    constexpr int NT = SCORE_NT;
    __shared__ double pts[CH][4];
    __shared__ int packed[NT], packed_n[NT / 64];
    const int tid = threadIdx.x, chunk = blockIdx.y, b = blockIdx.z;
    const int n = clamp_count(count[b], N), start = chunk * CH;
    const int m = n - start < CH ? n - start : CH;         // the rows of this chunk below the count (<= 0: none)
    const int slot = blockIdx.x * NT + tid;
    const int mine_n = Hn + ((Rule::EXTRA && first + Hn + 1 == width) ? 1 : 0);       // the slots of this launch
    int* const out = partial + ((size_t)b * gridDim.y + chunk) * width + first;
    if (m <= 0) {                                          // the whole workgroup: its zeros, and nothing else
        if (slot < mine_n) out[slot] = 0;
        return;
    }
    const Cam k0 = load_cam(intrinsics + ((size_t)b * 2 + 0) * 16), k1 = load_cam(intrinsics + ((size_t)b * 2 + 1) * 16);
    for (int i = tid; i < m; i += NT) {
        const float* const row = xy + ((size_t)b * N + start + i) * 4;
        pts[i][0] = ((double)row[0] - k0.cx) / k0.fx;
        pts[i][1] = ((double)row[1] - k0.cy) / k0.fy;
        pts[i][2] = ((double)row[2] - k1.cx) / k1.fx;
        pts[i][3] = ((double)row[3] - k1.cy) / k1.fy;
    }
    // the slots of this tile that have something to count, packed in slot order: the 5-point solver leaves more than half of
    // its 10 slots per sample invalid, scattered among the valid ones, and a wave is busy while one of its lanes is
    bool on = slot < mine_n;
    if (slot < Hn) on = on && valid[(size_t)b * Hn + slot] != 0;
    if (Rule::EXTRA && slot == Hn) on = on && rel_pose != nullptr;        // the extra slot: rel_pose's own model, where there is one
    if (slot < mine_n && !on) out[slot] = 0;
    const unsigned long long wave_on = __ballot(on);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) packed_n[wave] = __popcll(wave_on);
    __syncthreads();                                       // pts and packed_n are written
    int before = 0;
    for (int w = 0; w < wave; ++w) before += packed_n[w];
    if (on) packed[before + __popcll(wave_on & ((1ull << lane) - 1ull))] = slot;
    __syncthreads();
    if (tid >= (packed_n[0] + packed_n[1]) + (packed_n[2] + packed_n[3])) return;
    const int mine = packed[tid];
    Rule rule;
    if (!Rule::EXTRA || mine < Hn)
        rule.from_matrix(M + ((size_t)b * Hn + mine) * 9);
    else
        rule.from_pose(rel_pose + (size_t)b * 16);
    int cnt = 0;
    for (int i = 0; i < m; ++i) {
        if constexpr (GRADED)
            cnt += rule.weight(k0, k1, pts[i][0], pts[i][1], pts[i][2], pts[i][3], inlier_px);
        else if (rule.inlier(k0, k1, pts[i][0], pts[i][1], pts[i][2], pts[i][3], inlier_px))
            ++cnt;
    }
    out[mine] = cnt;
}

}  // namespace
