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
//                             (ransac_common.h), thread 0 splits its E by a one-sided Jacobi SVD (jacobi_svd.h), all threads
//                             mark the inliers and vote on the four poses.
//
// Every decision is an integer or a comparison of values that tests/ransac_ref.py forms in the same float64 sequence
// (-ffp-contract=off): no atomics, integer sums only, the same bytes every run.  The residual and the inlier rule are
// sampson.h's; the use of rel_pose, the pose's 16 floats and its angles are pose_out.h's, which matches.hip's refinement shares.
#include "common.h"
#include "epipolar_system.h"
#include "jacobi_svd.h"
#include "pinhole.h"
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
};

struct FinishState {
    double E[9], R[2][9], t[3];
    long long red[4];
    int ok;
};

__global__ __launch_bounds__(NT) void ransac_finish_kernel(const double* __restrict__ E, const uint8_t* __restrict__ valid,
                                                           const int* __restrict__ partial, const float* __restrict__ xy,
                                                           const int* __restrict__ count, const float* __restrict__ intrinsics,
                                                           const float* __restrict__ rel_pose, int N, int Hn, int chunks,
                                                           double inlier_px, float* __restrict__ pose,
                                                           uint8_t* __restrict__ inlier, double* __restrict__ stats) {
    __shared__ FinishState st;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = clamp_count(count[b], N);
    const float* const rows = xy + (size_t)b * N * 4;
    const float* const P = rel_pose ? rel_pose + (size_t)b * 16 : nullptr;
    uint8_t* const mask = inlier + (size_t)b * N;
    float* const o = pose + (size_t)b * 16;
    double* const so = stats + (size_t)b * 8;
    const long long usable = usable_rows(rows, n, st.red);

    // the winner: most inliers, the lower index on ties
    const int used = (n + CH - 1) / CH;                    // the chunks beyond hold zeros
    const int* const part = partial + (size_t)b * chunks * (Hn + 1);
    long long n_valid = 0, rel_count = 0;
    const long long best = best_hypothesis(valid + (size_t)b * Hn, part, Hn, Hn + 1, used, usable >= 8, st.red, n_valid);
    if (P)
        for (int c = tid; c < used; c += NT) rel_count += part[(size_t)c * (Hn + 1) + Hn];
    rel_count = block_all(rel_count, add_ll, st.red);
    const int winner = best < 0 ? 0 : 0x7FFFFFFF - (int)(best & 0x7FFFFFFF);
    const long long winner_count = best < 0 ? 0 : best >> 32;

    if (tid == 0) {
        st.ok = 0;
        if (best >= 0) {
            double G[9], V[9], sg[3];
            for (int c = 0; c < 9; ++c) G[c] = st.E[c] = E[((size_t)b * Hn + winner) * 9 + c];
            jacobi_svd(G, V, sg);
            double U[3][3], W[3][3];                       // the frames' vectors by rows: U[k] = u_k, W[k] = v_k
            frame(G, 0, 1, U);
            frame(V, 0, 1, W);
            bool fin = true;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    const double r1 = (U[1][i] * W[0][j] - U[0][i] * W[1][j]) + U[2][i] * W[2][j];
                    const double r2 = (U[0][i] * W[1][j] - U[1][i] * W[0][j]) + U[2][i] * W[2][j];
                    st.R[0][3 * i + j] = r1;
                    st.R[1][3 * i + j] = r2;
                    fin = fin && finite64(r1) && finite64(r2);
                }
            for (int i = 0; i < 3; ++i) st.t[i] = U[2][i];
            st.ok = fin ? 1 : 0;
        }
    }
    __syncthreads();
    const bool solved = st.ok != 0;

    // the inliers of the winner and their votes: candidate (R, +t) holds where both depths are positive, (R, -t) where both
    // are negative
    long long votes[4] = {0, 0, 0, 0};
    const Cam k0 = load_cam(intrinsics + ((size_t)b * 2 + 0) * 16), k1 = load_cam(intrinsics + ((size_t)b * 2 + 1) * 16);
    for (int i = tid; i < N; i += NT) {
        bool in = false;
        if (solved && i < n) {
            const float* const m = rows + (size_t)i * 4;
            const Sampson s = sampson(st.E, k0, k1, (double)m[0], (double)m[1], (double)m[2], (double)m[3]);
            in = within(s, inlier_px);
            if (in) {
                const double a[3] = {s.a0, s.a1, 1.0};
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const double* const R = st.R[k];
                    double c[3], ac[3], tc[3], ta[3];
                    for (int j = 0; j < 3; ++j) c[j] = (R[3 * j] * s.b0 + R[3 * j + 1] * s.b1) + R[3 * j + 2];
                    cross3(a, c, ac);
                    cross3(st.t, c, tc);
                    cross3(st.t, a, ta);
                    const double z0 = (tc[0] * ac[0] + tc[1] * ac[1]) + tc[2] * ac[2];
                    const double z1 = (ta[0] * ac[0] + ta[1] * ac[1]) + ta[2] * ac[2];
                    votes[2 * k + 0] += (z0 > 0.0 && z1 > 0.0) ? 1 : 0;
                    votes[2 * k + 1] += (z0 < 0.0 && z1 < 0.0) ? 1 : 0;
                }
            }
        }
        mask[i] = in ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) votes[k] = block_all(votes[k], add_ll, st.red);
    if (tid != 0) return;

    const bool nothing = usable < 8 || Hn == 0;
    if (nothing || !solved) {                              // status 2, or 1: no valid hypothesis
        for (int k = 0; k < 16; ++k) o[k] = P ? P[k] : ((k % 5 == 0) ? 1.0f : 0.0f);
        for (int k = 0; k < 8; ++k) so[k] = 0.0;
        so[1] = nothing ? 0.0 : (double)usable;
        so[4] = (P && !nothing) ? (double)rel_count : -1.0;
        so[7] = nothing ? 2.0 : 1.0;
        return;
    }
    int pick = 0;
    for (int k = 1; k < 4; ++k)
        if (votes[k] > votes[pick]) pick = k;              // most votes, the lowest candidate on ties
    const double* const R = st.R[pick >> 1];
    const double sign = (pick & 1) ? -1.0 : 1.0;
    const double t[3] = {sign * st.t[0], sign * st.t[1], sign * st.t[2]};
    // rel_pose, where it is finite and not zero: its length scales t, and the angles are measured from it (0 where it is not)
    const RelStart start = rel_start(P);
    store_pose(o, R, t, start.ok ? start.len0 : 1.0);
    double deg_R = 0.0, deg_t = 0.0;
    if (start.ok) pose_angles(R, t, start.rel, start.len0, deg_R, deg_t);
    so[0] = (double)winner_count;
    so[1] = (double)usable;
    so[2] = (double)winner;
    so[3] = (double)n_valid;
    so[4] = P ? (double)rel_count : -1.0;
    so[5] = deg_R;
    so[6] = deg_t;
    so[7] = 0.0;
}

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
                       rel_pose, N, Hn, inlier_px, partial);
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
    hipLaunchKernelGGL(ransac_finish_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, E, valid, partial, xy, count, intrinsics,
                       rel_pose, N, Hn, (int)cpn_cdiv(N, CH), inlier_px, pose, inlier, stats);
    CPN_LAUNCH_CHECK("cpn_ransac_finish");
    return 0;
}
