// The relative pose of two photos from their matches alone (coponerf_amd/matches.py: ransac_pose): 8-point RANSAC.
//
//   ransac_hypotheses_kernel  cpn_ransac_hypotheses: one thread per hypothesis index h (workgroups of 64), every pair in the
//                             launch.  The thread draws 8 distinct rows by a counter hash of (seed, h, draw) (ransac_common.h),
//                             forms the 8 x 9 system of a^T E b = 0, eliminates it with complete pivoting and takes its null
//                             vector (epipolar_system.h, which ransac5.hip shares).  The 72 doubles, the solution and the column
//                             permutation live in LDS, one column per lane ([entry][lane]: a lane's accesses never meet another
//                             lane's bank), so that the pivot's runtime indices never touch a private array.
//   ransac_score_kernel       cpn_ransac_score: ransac_score.h's kernel (tiles of 256 slots, chunks of CPN_RANSAC_CHUNK matches,
//                             pairs; ransac_h.hip shares it) with SampsonRule: each lane holds one E in registers.
//   ransac_finish_kernel      cpn_ransac_finish: one workgroup per pair sums the partial counts, picks the winner
//                             (ransac_common.h), thread 0 splits its E by a one-sided Jacobi SVD (essential_split.h), all
//                             threads mark the inliers and vote on the four poses.
//
// LO-MSAC (round 24), opt-in beside the three above:
//   ransac_score_kernel       cpn_ransac_score_slots: the same kernel on a range of a wider partial row, counting or - GRADED -
//                             summing sampson.h's fixed-point MSAC weight, an integer as well.
//   ransac_polish_kernel      cpn_ransac_polish: grid (K, pairs).  Workgroup (k, b) finds the slot of rank k - the one k + 1
//                             winner searches would end at, in one sweep (ransac_common.h: ranked_slot) -, splits its E and lets
//                             its inliers vote exactly as the finish does (essential_split.h), runs cpn_refine_pose's passes from
//                             that pose (pose_gauss_newton.h, which matches.hip shares) and writes E = [t]x R with round 20's
//                             norm and sign.
//                             float64, fixed-order sums through block_all and wave_sum, no atomics, no private array under a
//                             runtime index, no private segment.
//   ransac_finish_kernel      cpn_ransac_finish_lo: the finish over the hypotheses and the K polished slots behind them, the
//                             scores summed in int64 and compared as (score, slot) pairs.
//
// Every decision is an integer or a comparison of values that tests/ransac_ref.py forms in the same float64 sequence
// (-ffp-contract=off): no atomics, integer sums only, the same bytes every run.  The residual and the inlier rule are
// sampson.h's; the use of rel_pose, the pose's 16 floats and its angles are pose_out.h's, which matches.hip's refinement shares.
#include "common.h"
#include "epipolar_system.h"
#include "essential_split.h"
#include "jacobi_svd.h"
#include "pinhole.h"
#include "pose_gauss_newton.h"
#include "pose_out.h"
#include "ransac_common.h"
#include "ransac_score.h"
#include "sampson.h"

#include "../../include/coponerf_hip.h"

#include <math.h>

namespace {

namespace es = epipolar_system;
constexpr int NT = 256;
constexpr int HT = 64;                                     // hypotheses: threads per workgroup

__global__ __launch_bounds__(HT) void ransac_hypotheses_kernel(const float* __restrict__ xy, const int* __restrict__ count,
                                                               const float* __restrict__ intrinsics, int N, int Hn,
                                                               unsigned long long seed, double* __restrict__ E,
                                                               int* __restrict__ sample, uint8_t* __restrict__ valid) {
    __shared__ double A[72][HT];                           // the system, row-major entry 9 r + c of lane l at A[9 r + c][l]
    __shared__ double X[9][HT];                            // the solution in the permuted column order
    __shared__ int perm[9][HT];                            // the column of E at each permuted position
    const int l = threadIdx.x, h = blockIdx.x * HT + l, b = blockIdx.y;
    if (h >= Hn) return;                                   // no barrier below: a lane touches its own LDS column only
    const int n = clamp_count(count[b], N);
    const size_t at = (size_t)b * Hn + h;

    // ---- the draw
    int s[8];
    const int got = ransac_draw::draw_rows<8>(seed, h, n, s);
#pragma unroll
    for (int j = 0; j < 8; ++j) sample[at * 8 + j] = s[j];

    // ---- the system, its elimination and the null vector: back substitution with the free (last) unknown 1
    bool ok = got == 8;
    if (ok) {
        const Cam k0 = load_cam(intrinsics + ((size_t)b * 2 + 0) * 16), k1 = load_cam(intrinsics + ((size_t)b * 2 + 1) * 16);
        ok = es::fill_rows<8>(A, l, xy + (size_t)b * N * 4, s, k0, k1);
    }
    if (ok) ok = es::eliminate<8>(A, perm, l, es::RANK_TOL);
    double e[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) e[c] = 0.0;
    if (ok) {
        es::null_vector<8>(A, X, perm, l, 0, A);            // the system is spent: entries 0 .. 8 take E
#pragma unroll
        for (int c = 0; c < 9; ++c) e[c] = A[c][l];
        ok = es::unit_essential(e);
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) E[at * 9 + c] = ok ? e[c] : 0.0;
    valid[at] = ok ? 1 : 0;
}

// the rule of cpn_ransac_score for ransac_score.h's kernel: one E in registers, sampson.h's residual and inlier rule
struct SampsonRule {
    static constexpr int EXTRA = 1;                        // slot Hn: rel_pose's own E
    double e[9];
    __device__ __forceinline__ void from_matrix(const double* __restrict__ E) {
#pragma unroll
        for (int c = 0; c < 9; ++c) e[c] = E[c];
    }
    __device__ __forceinline__ void from_pose(const float* __restrict__ P) {
        const Pose rel = load_pose(P);
        essential(&rel.R[0][0], rel.t, e);
    }
    __device__ __forceinline__ bool inlier(const Cam& k0, const Cam& k1, double a0, double a1, double b0, double b1, double px) const {
        return within(sampson_normalised(e, k0, k1, a0, a1, b0, b1), px);
    }
    __device__ __forceinline__ int weight(const Cam& k0, const Cam& k1, double a0, double a1, double b0, double b1, double px) const {
        return msac_weight(sampson_normalised(e, k0, k1, a0, a1, b0, b1), px);
    }
};

struct FinishState {
    double E[9];
    EssentialSplit sp;
    long long red[4];
    int ok;
};

// slot h of a pair's Hn hypotheses and K polished ones: the two buffers side by side
struct Slots {
    const double* E;
    const uint8_t* valid;
    const double* E_lo;
    const uint8_t* valid_lo;
    int Hn;
    __device__ __forceinline__ bool ok(int h) const { return (h < Hn ? valid[h] : valid_lo[h - Hn]) != 0; }
    __device__ __forceinline__ const double* matrix(int h) const { return h < Hn ? E + (size_t)h * 9 : E_lo + (size_t)(h - Hn) * 9; }
};

// cpn_ransac_finish (K = 0, graded = 0, no score, no lo) and cpn_ransac_finish_lo
__global__ __launch_bounds__(NT) void ransac_finish_kernel(const double* __restrict__ E, const uint8_t* __restrict__ valid,
                                                           const double* __restrict__ E_lo, const uint8_t* __restrict__ valid_lo,
                                                           const double* __restrict__ lo_info, const int* __restrict__ partial,
                                                           const float* __restrict__ xy, const int* __restrict__ count,
                                                           const float* __restrict__ intrinsics, const float* __restrict__ rel_pose,
                                                           int N, int Hn, int K, int chunks, int graded, double inlier_px,
                                                           float* __restrict__ pose, uint8_t* __restrict__ inlier,
                                                           double* __restrict__ stats, long long* __restrict__ score,
                                                           double* __restrict__ lo) {
    __shared__ FinishState st;
    const int b = blockIdx.x, tid = threadIdx.x, T = Hn + K;
    const int n = clamp_count(count[b], N);
    const float* const rows = xy + (size_t)b * N * 4;
    const float* const P = rel_pose ? rel_pose + (size_t)b * 16 : nullptr;
    uint8_t* const mask = inlier + (size_t)b * N;
    float* const o = pose + (size_t)b * 16;
    double* const so = stats + (size_t)b * 8;
    const long long usable = usable_rows(rows, n, st.red);
    const Slots slots = {E + (size_t)b * Hn * 9, valid + (size_t)b * Hn, E_lo + (size_t)b * K * 9, valid_lo + (size_t)b * K, Hn};

    // the winner: the largest score, the lower index on ties
    const int used = (n + CH - 1) / CH;                    // the chunks beyond hold zeros
    const int* const part = partial + (size_t)b * chunks * (T + 1);
    long long n_valid = 0, rel_count = 0;
    for (int h = tid; h < T; h += NT) n_valid += slots.ok(h) ? 1 : 0;
    n_valid = block_all(n_valid, add_ll, st.red);
    Ranked win = {0, -1};
    if (usable >= 8) win = ranked_slot<1>([&](int h) { return slots.ok(h); }, part, T, T + 1, used, 0, st.red);
    if (P && !graded)
        for (int c = tid; c < used; c += NT) rel_count += part[(size_t)c * (T + 1) + T];
    const int winner = win.slot < 0 ? 0 : win.slot;

    if (tid == 0) {
        st.ok = 0;
        if (win.slot >= 0) {
            const double* const Ew = slots.matrix(winner);
            for (int c = 0; c < 9; ++c) st.E[c] = Ew[c];
            st.ok = split_essential(st.E, st.sp) ? 1 : 0;
        }
    }
    __syncthreads();
    const bool solved = st.ok != 0;

    // the inliers of the winner and their votes; under the graded score the counts of the winner and of rel_pose are taken here
    long long votes[4] = {0, 0, 0, 0}, counted = 0;
    const Cam k0 = load_cam(intrinsics + ((size_t)b * 2 + 0) * 16), k1 = load_cam(intrinsics + ((size_t)b * 2 + 1) * 16);
    double e_rel[9];
    const bool count_rel = P && graded;
    if (count_rel) {
        const Pose rel = load_pose(P);
        essential(&rel.R[0][0], rel.t, e_rel);
    }
    for (int i = tid; i < N; i += NT) {
        bool in = false;
        if (i < n) {
            const float* const m = rows + (size_t)i * 4;
            if (solved) {
                const Sampson s = sampson(st.E, k0, k1, (double)m[0], (double)m[1], (double)m[2], (double)m[3]);
                in = within(s, inlier_px);
                if (in) {
                    ++counted;
                    depth_votes(st.sp, s, votes);
                }
            }
            if (count_rel && within(sampson(e_rel, k0, k1, (double)m[0], (double)m[1], (double)m[2], (double)m[3]), inlier_px))
                ++rel_count;
        }
        mask[i] = in ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) votes[k] = block_all(votes[k], add_ll, st.red);
    rel_count = block_all(rel_count, add_ll, st.red);
    if (graded) counted = block_all(counted, add_ll, st.red);
    if (tid != 0) return;

    const bool nothing = usable < 8 || T == 0;
    if (lo)
        for (int k = 0; k < 4; ++k) lo[(size_t)b * 4 + k] = (k == 0 || k == 3) ? 0.0 : -1.0;
    if (nothing || !solved) {                              // status 2, or 1: no valid hypothesis
        for (int k = 0; k < 16; ++k) o[k] = P ? P[k] : ((k % 5 == 0) ? 1.0f : 0.0f);
        for (int k = 0; k < 8; ++k) so[k] = 0.0;
        so[1] = nothing ? 0.0 : (double)usable;
        so[4] = (P && !nothing) ? (double)rel_count : -1.0;
        so[7] = nothing ? 2.0 : 1.0;
        if (score) score[b] = 0;
        return;
    }
    const int pick = pick_candidate(votes);
    const double* const R = st.sp.R[pick >> 1];
    const double sign = (pick & 1) ? -1.0 : 1.0;
    const double t[3] = {sign * st.sp.t[0], sign * st.sp.t[1], sign * st.sp.t[2]};
    // rel_pose, where it is finite and not zero: its length scales t, and the angles are measured from it (0 where it is not)
    const RelStart start = rel_start(P);
    store_pose(o, R, t, start.ok ? start.len0 : 1.0);
    double deg_R = 0.0, deg_t = 0.0;
    if (start.ok) pose_angles(R, t, start.rel, start.len0, deg_R, deg_t);
    so[0] = (double)(graded ? counted : win.score);
    so[1] = (double)usable;
    so[2] = (double)winner;
    so[3] = (double)n_valid;
    so[4] = P ? (double)rel_count : -1.0;
    so[5] = deg_R;
    so[6] = deg_t;
    so[7] = 0.0;
    if (score) score[b] = win.score;
    if (lo && winner >= Hn) {
        const double* const info = lo_info + ((size_t)b * K + (winner - Hn)) * 8;
        double* const l = lo + (size_t)b * 4;
        l[0] = 1.0;
        l[1] = info[0];
        l[2] = info[1];
        l[3] = info[2];
    }
}

// cpn_ransac_polish: workgroup (k, b) polishes the slot of rank k of pair b into slot k of the polished buffers
struct PolishState {
    RefineState gn;
    EssentialSplit sp;
    double E[9];
    long long red[4];
    int ok;
};

__global__ __launch_bounds__(NT) void ransac_polish_kernel(const double* __restrict__ E, const uint8_t* __restrict__ valid,
                                                           const int* __restrict__ partial, const float* __restrict__ xy,
                                                           const int* __restrict__ count, const float* __restrict__ intrinsics,
                                                           int N, int Hn, int K, int chunks, int iters, double inlier_px,
                                                           double scale_px, double* __restrict__ E_lo,
                                                           uint8_t* __restrict__ valid_lo, double* __restrict__ info) {
    __shared__ PolishState st;
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int n = clamp_count(count[b], N);
    const float* const rows = xy + (size_t)b * N * 4;
    const size_t at = (size_t)b * K + k;
    const long long usable = usable_rows(rows, n, st.red);

    // the rank: the slot that k + 1 winner searches, each without the slots found before it, end at - found in one sweep
    const int used = (n + CH - 1) / CH;
    const int* const part = partial + (size_t)b * chunks * (Hn + K + 1);
    const uint8_t* const vb = valid + (size_t)b * Hn;
    Ranked src = {0, -1};
    if (usable >= 8) src = ranked_slot<CPN_RANSAC_LO_MAX>([&](int h) { return vb[h] != 0; }, part, Hn, Hn + K + 1, used, k, st.red);
    if (tid == 0) {
        st.ok = 0;
        if (src.slot >= 0) {
            for (int c = 0; c < 9; ++c) st.E[c] = E[((size_t)b * Hn + src.slot) * 9 + c];
            st.ok = split_essential(st.E, st.sp) ? 1 : 0;
        }
    }
    __syncthreads();
    if (!st.ok) {                                          // no slot of this rank (status 2), or a split that is not finite (3)
        if (tid < 9) E_lo[at * 9 + tid] = 0.0;
        if (tid < 8) info[at * 8 + tid] = tid == 7 ? (src.slot < 0 ? 2.0 : 3.0) : (tid < 2 ? -1.0 : 0.0);
        if (tid == 0) valid_lo[at] = 0;
        return;
    }

    // the slot's inliers vote on the four poses, as in the finish
    long long votes[4] = {0, 0, 0, 0};
    const Cam k0 = load_cam(intrinsics + ((size_t)b * 2 + 0) * 16), k1 = load_cam(intrinsics + ((size_t)b * 2 + 1) * 16);
    for (int i = tid; i < n; i += NT) {
        const float* const m = rows + (size_t)i * 4;
        const Sampson s = sampson(st.E, k0, k1, (double)m[0], (double)m[1], (double)m[2], (double)m[3]);
        if (within(s, inlier_px)) depth_votes(st.sp, s, votes);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) votes[j] = block_all(votes[j], add_ll, st.red);
    if (tid == 0) {
        const int pick = pick_candidate(votes);
        const double sign = (pick & 1) ? -1.0 : 1.0;
        for (int c = 0; c < 9; ++c) st.gn.R[c] = st.sp.R[pick >> 1][c];
        for (int c = 0; c < 3; ++c) st.gn.t[c] = sign * st.sp.t[c];
        set_matrices(st.gn);
        st.gn.go = 1;
    }
    __syncthreads();

    // the passes on every usable match of the pair, then E = [t]x R with round 20's norm and sign
    const int slot = src.slot;
    pose_passes(st.gn, rows, n, k0, k1, iters, scale_px, [&](double, const double (&)[POSE_NSUM], int done, int status) {
        double e[9];
        for (int c = 0; c < 9; ++c) e[c] = st.gn.E[c];
        const bool fin = es::unit_essential(e);
        for (int c = 0; c < 9; ++c) E_lo[at * 9 + c] = fin ? e[c] : 0.0;
        valid_lo[at] = fin ? 1 : 0;
        double* const io = info + at * 8;
        io[0] = (double)slot;
        io[1] = (double)k;
        io[2] = (double)done;
        for (int j = 0; j < 4; ++j) io[3 + j] = (double)votes[j];
        io[7] = fin ? (double)status : 3.0;
    });
}

bool lo_ok(int K) { return K >= 0 && K <= CPN_RANSAC_LO_MAX; }

}  // namespace

extern "C" int cpn_ransac_hypotheses(const float* xy, const int* count, const float* intrinsics, int B, int N, int Hn, long long seed,
                                     double* E, int* sample, uint8_t* valid, void* stream) {
    CPN_REQUIRE(xy && count && intrinsics && E && sample && valid, CPN_E_ARG, "cpn_ransac_hypotheses: null pointer");
    CPN_REQUIRE(shape_ok(B, N, Hn) && Hn >= 1, CPN_E_SHAPE,
                "cpn_ransac_hypotheses: need 1 <= B <= 32767, 1 <= N <= 2^24, 1 <= Hn <= 2^20 and B chunks (Hn + 1) < 2^31 (got B %d, "
                "N %d, Hn %d)", B, N, Hn);
    hipLaunchKernelGGL(ransac_hypotheses_kernel, dim3(cpn_cdiv(Hn, HT), B), dim3(HT), 0, (hipStream_t)stream, xy, count, intrinsics, N,
                       Hn, (unsigned long long)seed, E, sample, valid);
    CPN_LAUNCH_CHECK("cpn_ransac_hypotheses");
    return 0;
}

extern "C" int cpn_ransac_score(const double* E, const uint8_t* valid, const float* xy, const int* count, const float* intrinsics,
                                const float* rel_pose, int B, int N, int Hn, double inlier_px, int* partial, void* stream) {
    CPN_REQUIRE(xy && count && intrinsics && partial && (Hn == 0 || (E && valid)), CPN_E_ARG, "cpn_ransac_score: null pointer");
    CPN_REQUIRE(shape_ok(B, N, Hn), CPN_E_SHAPE,
                "cpn_ransac_score: need 1 <= B <= 32767, 1 <= N <= 2^24, 0 <= Hn <= 2^20 and B chunks (Hn + 1) < 2^31 (got B %d, N %d, "
                "Hn %d)", B, N, Hn);
    CPN_REQUIRE(px_ok(inlier_px), CPN_E_ARG, "cpn_ransac_score: need a finite inlier_px >= 0 (got %g)", inlier_px);
    const dim3 grid(cpn_cdiv(Hn + 1, NT), cpn_cdiv(N, CH), B);
    hipLaunchKernelGGL(ransac_score_kernel<SampsonRule>, grid, dim3(SCORE_NT), 0, (hipStream_t)stream, E, valid, xy, count, intrinsics,
                       rel_pose, N, Hn, 0, Hn + 1, inlier_px, partial);
    CPN_LAUNCH_CHECK("cpn_ransac_score");
    return 0;
}

extern "C" int cpn_ransac_finish(const double* E, const uint8_t* valid, const int* partial, const float* xy, const int* count,
                                 const float* intrinsics, const float* rel_pose, int B, int N, int Hn, double inlier_px, float* pose,
                                 uint8_t* inlier, double* stats, void* stream) {
    CPN_REQUIRE(partial && xy && count && intrinsics && pose && inlier && stats && (Hn == 0 || (E && valid)), CPN_E_ARG,
                "cpn_ransac_finish: null pointer");
    CPN_REQUIRE(shape_ok(B, N, Hn), CPN_E_SHAPE,
                "cpn_ransac_finish: need 1 <= B <= 32767, 1 <= N <= 2^24, 0 <= Hn <= 2^20 and B chunks (Hn + 1) < 2^31 (got B %d, N %d, "
                "Hn %d)", B, N, Hn);
    CPN_REQUIRE(px_ok(inlier_px), CPN_E_ARG, "cpn_ransac_finish: need a finite inlier_px >= 0 (got %g)", inlier_px);
    hipLaunchKernelGGL(ransac_finish_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, E, valid, (const double*)nullptr,
                       (const uint8_t*)nullptr, (const double*)nullptr, partial, xy, count, intrinsics, rel_pose, N, Hn, 0,
                       (int)cpn_cdiv(N, CH), 0, inlier_px, pose, inlier, stats, (long long*)nullptr, (double*)nullptr);
    CPN_LAUNCH_CHECK("cpn_ransac_finish");
    return 0;
}

extern "C" int cpn_ransac_score_slots(const double* E, const uint8_t* valid, const float* xy, const int* count, const float* intrinsics,
                                      const float* rel_pose, int B, int N, int Hn, int first, int total, int graded, double inlier_px,
                                      int* partial, void* stream) {
    CPN_REQUIRE(xy && count && intrinsics && partial && (Hn == 0 || (E && valid)), CPN_E_ARG, "cpn_ransac_score_slots: null pointer");
    CPN_REQUIRE(Hn >= 0 && first >= 0 && total >= 0 && (long long)first + Hn <= total && shape_ok(B, N, total), CPN_E_SHAPE,
                "cpn_ransac_score_slots: need 1 <= B <= 32767, 1 <= N <= 2^24, 0 <= first, 0 <= Hn, first + Hn <= total <= 2^20 and "
                "B chunks (total + 1) < 2^31 (got B %d, N %d, Hn %d, first %d, total %d)", B, N, Hn, first, total);
    CPN_REQUIRE(px_ok(inlier_px) && (graded == 0 || graded == 1), CPN_E_ARG,
                "cpn_ransac_score_slots: need a finite inlier_px >= 0 and graded 0 or 1 (got %g, %d)", inlier_px, graded);
    const int mine = Hn + (first + Hn == total ? 1 : 0);   // the launch that ends the row scores rel_pose's slot too
    if (mine == 0) return 0;
    const dim3 grid(cpn_cdiv(mine, NT), cpn_cdiv(N, CH), B);
    if (graded)
        hipLaunchKernelGGL((ransac_score_kernel<SampsonRule, true>), grid, dim3(SCORE_NT), 0, (hipStream_t)stream, E, valid, xy, count,
                           intrinsics, rel_pose, N, Hn, first, total + 1, inlier_px, partial);
    else
        hipLaunchKernelGGL((ransac_score_kernel<SampsonRule, false>), grid, dim3(SCORE_NT), 0, (hipStream_t)stream, E, valid, xy, count,
                           intrinsics, rel_pose, N, Hn, first, total + 1, inlier_px, partial);
    CPN_LAUNCH_CHECK("cpn_ransac_score_slots");
    return 0;
}

extern "C" int cpn_ransac_polish(const double* E, const uint8_t* valid, const int* partial, const float* xy, const int* count,
                                 const float* intrinsics, int B, int N, int Hn, int K, int iters, double inlier_px, double scale_px,
                                 double* E_lo, uint8_t* valid_lo, double* info, void* stream) {
    CPN_REQUIRE(partial && xy && count && intrinsics && E_lo && valid_lo && info && (Hn == 0 || (E && valid)), CPN_E_ARG,
                "cpn_ransac_polish: null pointer");
    CPN_REQUIRE(Hn >= 0 && lo_ok(K) && K >= 1 && shape_ok(B, N, (long long)Hn + K), CPN_E_SHAPE,
                "cpn_ransac_polish: need 1 <= B <= 32767, 1 <= N <= 2^24, 0 <= Hn, 1 <= K <= 16, Hn + K <= 2^20 and "
                "B chunks (Hn + K + 1) < 2^31 (got B %d, N %d, Hn %d, K %d)", B, N, Hn, K);
    CPN_REQUIRE(px_ok(inlier_px) && iters >= 0 && scale_px > 0.0 && scale_px <= 1.79769313486231570815e308, CPN_E_ARG,
                "cpn_ransac_polish: need a finite inlier_px >= 0, iters >= 0 and a finite scale_px > 0 (got %g, %d, %g)", inlier_px,
                iters, scale_px);
    hipLaunchKernelGGL(ransac_polish_kernel, dim3(K, B), dim3(NT), 0, (hipStream_t)stream, E, valid, partial, xy, count, intrinsics, N,
                       Hn, K, (int)cpn_cdiv(N, CH), iters, inlier_px, scale_px, E_lo, valid_lo, info);
    CPN_LAUNCH_CHECK("cpn_ransac_polish");
    return 0;
}

extern "C" int cpn_ransac_finish_lo(const double* E, const uint8_t* valid, const double* E_lo, const uint8_t* valid_lo,
                                    const double* info, const int* partial, const float* xy, const int* count,
                                    const float* intrinsics, const float* rel_pose, int B, int N, int Hn, int K, int graded,
                                    double inlier_px, float* pose, uint8_t* inlier, double* stats, long long* score, double* lo,
                                    void* stream) {
    CPN_REQUIRE(partial && xy && count && intrinsics && pose && inlier && stats && score && lo && (Hn == 0 || (E && valid)) &&
                    (K == 0 || (E_lo && valid_lo && info)), CPN_E_ARG, "cpn_ransac_finish_lo: null pointer");
    CPN_REQUIRE(Hn >= 0 && lo_ok(K) && shape_ok(B, N, (long long)Hn + K), CPN_E_SHAPE,
                "cpn_ransac_finish_lo: need 1 <= B <= 32767, 1 <= N <= 2^24, 0 <= Hn, 0 <= K <= 16, Hn + K <= 2^20 and "
                "B chunks (Hn + K + 1) < 2^31 (got B %d, N %d, Hn %d, K %d)", B, N, Hn, K);
    CPN_REQUIRE(px_ok(inlier_px) && (graded == 0 || graded == 1), CPN_E_ARG,
                "cpn_ransac_finish_lo: need a finite inlier_px >= 0 and graded 0 or 1 (got %g, %d)", inlier_px, graded);
    hipLaunchKernelGGL(ransac_finish_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, E, valid, E_lo, valid_lo, info, partial, xy,
                       count, intrinsics, rel_pose, N, Hn, K, (int)cpn_cdiv(N, CH), graded, inlier_px, pose, inlier, stats, score, lo);
    CPN_LAUNCH_CHECK("cpn_ransac_finish_lo");
    return 0;
}
