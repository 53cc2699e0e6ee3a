// The homography model of coponerf_amd/matches.py: homography_pose - RANSAC for the pairs whose matches one plane or a pure
// rotation explains, where the essential matrix of ransac.hip and ransac5.hip is under-determined.
//
//   ransac_homographies_kernel  cpn_ransac_homographies: one thread per hypothesis index h (workgroups of 64), every pair in the
//                               launch.  The thread draws 4 distinct rows (ransac_common.h: the first 4 of round 20's 8), forms
//                               the 8 x 9 system of a ~ H b (epipolar_system.h: fill_rows_h), eliminates it with complete
//                               pivoting and takes its null vector - the 8-point solver's code and LDS layout, one column per
//                               lane -, normalises H to det > 0 and drops it where it maps one of its own four points behind a
//                               camera.
//   ransac_score_kernel         cpn_ransac_score_h: ransac_score.h's kernel, which ransac.hip shares, with TransferRule: each
//                               lane holds one H and its adjugate in registers, 18 doubles.
//   ransac_finish_h_kernel      cpn_ransac_finish_h: one workgroup per pair sums the partial counts and picks the winner
//                               (ransac_common.h); thread 0 takes its singular values by the one-sided Jacobi method
//                               (jacobi_svd.h) and forms the four (R, T, N) of H = R + T N^T; all threads mark the inliers, let
//                               them vote on the side of the plane and count the Sampson inliers of the two essential matrices.
//
// Every decision is an integer or a comparison of values that tests/homography_ref.py forms in the same float64 sequence
// (-ffp-contract=off): no atomics, integer sums only, the same bytes every run.  The transfer rule is homography.h's, the Sampson
// rule sampson.h's, the use of rel_pose and the pose's 16 floats pose_out.h's.
#include "common.h"
#include "epipolar_system.h"
#include "homography.h"
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

__global__ __launch_bounds__(HT) void ransac_homographies_kernel(const float* __restrict__ xy, const int* __restrict__ count,
                                                                 const float* __restrict__ intrinsics, int N, int Hn,
                                                                 unsigned long long seed, double* __restrict__ H,
                                                                 int* __restrict__ sample, uint8_t* __restrict__ valid) {
    __shared__ double A[72][HT];                           // the system, row-major entry 9 r + c of lane l at A[9 r + c][l]
    __shared__ double X[9][HT];                            // the solution in the permuted column order
    __shared__ int perm[9][HT];                            // the column of H at each permuted position
    const int l = threadIdx.x, h = blockIdx.x * HT + l, b = blockIdx.y;
    if (h >= Hn) return;                                   // no barrier below: a lane touches its own LDS column only
    const int n = clamp_count(count[b], N);
    const size_t at = (size_t)b * Hn + h;

    // ---- the draw
    int s[4];
    const int got = ransac_draw::draw_rows<4>(seed, h, n, s);
#pragma unroll
    for (int j = 0; j < 4; ++j) sample[at * 4 + j] = s[j];

    // ---- the system, its elimination and the null vector: back substitution with the free (last) unknown 1
    bool ok = got == 4;
    double p[4][4];                                        // the sample's (a0, a1, b0, b1)
    if (ok) {
        const Cam k0 = load_cam(intrinsics + ((size_t)b * 2 + 0) * 16), k1 = load_cam(intrinsics + ((size_t)b * 2 + 1) * 16);
        ok = es::fill_rows_h<8>(A, l, xy + (size_t)b * N * 4, s, k0, k1, p);
    }
    if (ok) ok = es::eliminate<8>(A, perm, l, es::RANK_TOL);
    double m[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) m[c] = 0.0;
    if (ok) {
        es::null_vector<8>(A, X, perm, l, 0, A);            // the system is spent: entries 0 .. 8 take H
#pragma unroll
        for (int c = 0; c < 9; ++c) m[c] = A[c][l];
        // ---- unit Frobenius norm, det > 0, and its own four points in front of both cameras
        double ss = m[0] * m[0];
#pragma unroll
        for (int c = 1; c < 9; ++c) ss = ss + m[c] * m[c];
        const double nrm = sqrt(ss);
#pragma unroll
        for (int c = 0; c < 9; ++c) m[c] = m[c] / nrm;
        double g[9];
        adjugate(m, g);
        if (determinant(m, g) < 0.0) {
#pragma unroll
            for (int c = 0; c < 9; ++c) m[c] = -m[c];
            adjugate(m, g);
        }
        const double det = determinant(m, g);
        ok = det > 0.0 && finite64(det);
#pragma unroll
        for (int c = 0; c < 9; ++c) ok = ok && finite64(m[c]);
#pragma unroll
        for (int j = 0; j < 4; ++j) ok = ok && third(m, p[j][2], p[j][3]) > 0.0 && third(g, p[j][0], p[j][1]) > 0.0;
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) H[at * 9 + c] = ok ? m[c] : 0.0;
    valid[at] = ok ? 1 : 0;
}

// the rule of cpn_ransac_score_h for ransac_score.h's kernel: one H and its adjugate in registers, homography.h's inlier rule
struct TransferRule {
    static constexpr int EXTRA = 0;                        // a pose has no homography without a plane: no slot for rel_pose
    double h[9], g[9];
    __device__ __forceinline__ void from_matrix(const double* __restrict__ H) {
#pragma unroll
        for (int c = 0; c < 9; ++c) h[c] = H[c];
        adjugate(h, g);
    }
    __device__ __forceinline__ void from_pose(const float* __restrict__) {}
    __device__ __forceinline__ bool inlier(const Cam& k0, const Cam& k1, double a0, double a1, double b0, double b1, double px) const {
        return transfer_inlier(h, g, k0, k1, a0, a1, b0, b1, px);
    }
};

struct FinishStateH {
    double H[9], G[9];                                     // the winner as it was scored, and its adjugate
    double Hs[9];                                          // the winner over sigma_2
    double R[2][9], T[2][3], t[2][3], Nv[2][3], E[2][9];   // of u_1 and u_2: H = R + T N^T, t = T / |T|, E = [T]x R
    double Rn[9];                                          // the rotation nearest to H
    double s1, s3;
    long long red[4];
    int mode;                                              // 0 nothing solved, 1 the four candidates, 2 rotation only
};

__global__ __launch_bounds__(NT) void ransac_finish_h_kernel(const double* __restrict__ H, const uint8_t* __restrict__ valid,
                                                             const int* __restrict__ partial, const float* __restrict__ xy,
                                                             const int* __restrict__ count, const float* __restrict__ intrinsics,
                                                             const float* __restrict__ rel_pose, int N, int Hn, int chunks,
                                                             double inlier_px, double min_baseline, float* __restrict__ pose,
                                                             float* __restrict__ twin, double* __restrict__ Hout,
                                                             uint8_t* __restrict__ inlier, double* __restrict__ stats) {
    __shared__ FinishStateH st;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = clamp_count(count[b], N);
    const float* const rows = xy + (size_t)b * N * 4;
    const float* const P = rel_pose ? rel_pose + (size_t)b * 16 : nullptr;
    uint8_t* const mask = inlier + (size_t)b * N;
    float* const o = pose + (size_t)b * 16;
    float* const ot = twin + (size_t)b * 16;
    double* const ho = Hout + (size_t)b * 9;
    double* const so = stats + (size_t)b * 12;

    const long long usable = usable_rows(rows, n, st.red);
    const int used = (n + CH - 1) / CH;                    // the chunks beyond hold zeros
    long long n_valid = 0;
    const long long best = best_hypothesis(valid + (size_t)b * Hn, partial + (size_t)b * chunks * Hn, Hn, Hn, used, usable >= 4,
                                           st.red, n_valid);
    const int winner = best < 0 ? 0 : 0x7FFFFFFF - (int)(best & 0x7FFFFFFF);
    const long long winner_count = best < 0 ? 0 : best >> 32;

    if (tid == 0) {
        st.mode = 0;
        if (best >= 0) {
            double G[9], V[9], sg[3];
            for (int c = 0; c < 9; ++c) G[c] = st.H[c] = H[((size_t)b * Hn + winner) * 9 + c];
            adjugate(st.H, st.G);
            jacobi_svd(G, V, sg);
            double U[3][3], W[3][3];                       // the frames' vectors by rows: U[k] = u_k, W[k] = v_k
            frame(G, 0, 1, U);
            frame(V, 0, 1, W);
            const double s1 = sg[0] / sg[1], s3 = sg[2] / sg[1];
            st.s1 = s1;
            st.s3 = s3;
            bool fin = finite64(s1) && finite64(s3);
            for (int c = 0; c < 9; ++c) {
                st.Hs[c] = st.H[c] / sg[1];
                fin = fin && finite64(st.Hs[c]);
            }
            const double gap = s1 * s1 - s3 * s3;
            if (!(gap > 0.0) || s1 - s3 <= min_baseline) {     // ROTATION ONLY: R_n = (u_1 v_1^T + u_2 v_2^T) + u_3 v_3^T
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) {
                        const double r = (U[0][i] * W[0][j] + U[1][i] * W[1][j]) + U[2][i] * W[2][j];
                        st.Rn[3 * i + j] = r;
                        fin = fin && finite64(r);
                    }
                st.mode = fin ? 2 : 0;
            } else {
                const double c1 = 1.0 - s3 * s3, c3 = s1 * s1 - 1.0;
                const double x1 = sqrt(c1 > 0.0 ? c1 : 0.0), x3 = sqrt(c3 > 0.0 ? c3 : 0.0), den = sqrt(gap);
                const double* const v2 = W[1];
                for (int k = 0; k < 2; ++k) {
                    double u[3], hv[3], hu[3], hn[3];
                    for (int i = 0; i < 3; ++i) {
                        const double pa = x1 * W[0][i], pb = x3 * W[2][i];
                        u[i] = (k == 0 ? pa + pb : pa - pb) / den;
                    }
                    cross3(v2, u, st.Nv[k]);
                    for (int i = 0; i < 3; ++i) {
                        hv[i] = (st.Hs[3 * i] * v2[0] + st.Hs[3 * i + 1] * v2[1]) + st.Hs[3 * i + 2] * v2[2];
                        hu[i] = (st.Hs[3 * i] * u[0] + st.Hs[3 * i + 1] * u[1]) + st.Hs[3 * i + 2] * u[2];
                    }
                    cross3(hv, hu, hn);
                    for (int i = 0; i < 3; ++i)
                        for (int j = 0; j < 3; ++j) {
                            st.R[k][3 * i + j] = (hv[i] * v2[j] + hu[i] * u[j]) + hn[i] * st.Nv[k][j];
                            fin = fin && finite64(st.R[k][3 * i + j]);
                        }
                    for (int i = 0; i < 3; ++i)
                        st.T[k][i] = ((st.Hs[3 * i] - st.R[k][3 * i]) * st.Nv[k][0] + (st.Hs[3 * i + 1] - st.R[k][3 * i + 1]) * st.Nv[k][1]) +
                                     (st.Hs[3 * i + 2] - st.R[k][3 * i + 2]) * st.Nv[k][2];
                    const double len = norm3(st.T[k]);
                    for (int i = 0; i < 3; ++i) {
                        st.t[k][i] = st.T[k][i] / len;
                        fin = fin && finite64(st.t[k][i]) && finite64(st.Nv[k][i]);
                    }
                    essential(st.R[k], st.T[k], st.E[k]);
                }
                st.mode = fin ? 1 : 0;
            }
        }
    }
    __syncthreads();
    const int mode = st.mode;

    // the inliers of the winner; with candidates, their votes - candidate (R, T, N) where N . b > 0, (R, -T, -N) where
    // N . b < 0 - and the Sampson inliers of E = [T]x R of u_1 and of u_2 among all rows below n
    long long pos[2] = {0, 0}, neg[2] = {0, 0}, samp[2] = {0, 0};
    const Cam k0 = load_cam(intrinsics + ((size_t)b * 2 + 0) * 16), k1 = load_cam(intrinsics + ((size_t)b * 2 + 1) * 16);
    for (int i = tid; i < N; i += NT) {
        bool in = false;
        if (mode != 0 && i < n) {
            const float* const m = rows + (size_t)i * 4;
            const double a0 = ((double)m[0] - k0.cx) / k0.fx, a1 = ((double)m[1] - k0.cy) / k0.fy;
            const double b0 = ((double)m[2] - k1.cx) / k1.fx, b1 = ((double)m[3] - k1.cy) / k1.fy;
            in = transfer_inlier(st.H, st.G, k0, k1, a0, a1, b0, b1, inlier_px);
            if (mode == 1) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    if (in) {
                        const double nb = (st.Nv[k][0] * b0 + st.Nv[k][1] * b1) + st.Nv[k][2];
                        pos[k] += nb > 0.0 ? 1 : 0;
                        neg[k] += nb < 0.0 ? 1 : 0;
                    }
                    samp[k] += within(sampson_normalised(st.E[k], k0, k1, a0, a1, b0, b1), inlier_px) ? 1 : 0;
                }
            }
        }
        mask[i] = in ? 1 : 0;
    }
    long long votes[4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        votes[2 * k] = block_all(pos[k], add_ll, st.red);
        votes[2 * k + 1] = block_all(neg[k], add_ll, st.red);
        samp[k] = block_all(samp[k], add_ll, st.red);
    }
    if (tid != 0) return;

    const bool nothing = usable < 4 || Hn == 0;
    for (int k = 0; k < 12; ++k) so[k] = 0.0;
    if (nothing || mode == 0) {                            // status 2, or 1: no valid hypothesis
        for (int k = 0; k < 16; ++k) o[k] = ot[k] = P ? P[k] : ((k % 5 == 0) ? 1.0f : 0.0f);
        for (int c = 0; c < 9; ++c) ho[c] = 0.0;
        so[1] = nothing ? 0.0 : (double)usable;
        so[11] = nothing ? 2.0 : 1.0;
        return;
    }
    for (int c = 0; c < 9; ++c) ho[c] = st.Hs[c];
    so[0] = (double)winner_count;
    so[1] = (double)usable;
    so[2] = (double)winner;
    so[3] = (double)n_valid;
    so[8] = st.s1;
    so[9] = st.s3;
    so[10] = st.s1 - st.s3;
    if (mode == 2) {                                       // status 3: [R_n | 0], the twin is the pose
        const double zero[3] = {0.0, 0.0, 0.0};
        store_pose(o, st.Rn, zero, 1.0);
        store_pose(ot, st.Rn, zero, 1.0);
        so[11] = 3.0;
        return;
    }
    // most votes; on a tie the candidate whose E has more Sampson inliers; on a tie the lower index
    int pick = 0;
    for (int c = 1; c < 4; ++c)
        if (votes[c] > votes[pick] || (votes[c] == votes[pick] && samp[c >> 1] > samp[pick >> 1])) pick = c;
    const int other = 1 - (pick >> 1);
    const int tw = votes[2 * other + 1] > votes[2 * other] ? 2 * other + 1 : 2 * other;
    const RelStart start = rel_start(P);
    const double scale = start.ok ? start.len0 : 1.0;
    const int both[2] = {pick, tw};
    for (int w = 0; w < 2; ++w) {
        const int c = both[w], k = c >> 1;
        const double sign = (c & 1) ? -1.0 : 1.0;
        const double t[3] = {sign * st.t[k][0], sign * st.t[k][1], sign * st.t[k][2]};
        store_pose(w == 0 ? o : ot, st.R[k], t, scale);
    }
    so[4] = (double)votes[pick];
    so[5] = (double)votes[tw];
    so[6] = (double)samp[pick >> 1];
    so[7] = (double)samp[other];
}

}  // namespace

extern "C" int cpn_ransac_homographies(const float* xy, const int* count, const float* intrinsics, int B, int N, int Hn, long long seed,
                                       double* H, int* sample, uint8_t* valid, void* stream) {
    CPN_REQUIRE(xy && count && intrinsics && H && sample && valid, CPN_E_ARG, "cpn_ransac_homographies: null pointer");
    CPN_REQUIRE(shape_ok(B, N, Hn) && Hn >= 1, CPN_E_SHAPE,
                "cpn_ransac_homographies: need 1 <= B <= 32767, 1 <= N <= 2^24, 1 <= Hn <= 2^20 and B chunks (Hn + 1) < 2^31 (got B %d, "
                "N %d, Hn %d)", B, N, Hn);
    hipLaunchKernelGGL(ransac_homographies_kernel, dim3(cpn_cdiv(Hn, HT), B), dim3(HT), 0, (hipStream_t)stream, xy, count, intrinsics,
                       N, Hn, (unsigned long long)seed, H, sample, valid);
    CPN_LAUNCH_CHECK("cpn_ransac_homographies");
    return 0;
}

extern "C" int cpn_ransac_score_h(const double* H, const uint8_t* valid, const float* xy, const int* count, const float* intrinsics,
                                  int B, int N, int Hn, double inlier_px, int* partial, void* stream) {
    CPN_REQUIRE(xy && count && intrinsics && (Hn == 0 || (H && valid && partial)), CPN_E_ARG, "cpn_ransac_score_h: null pointer");
    CPN_REQUIRE(shape_ok(B, N, Hn), CPN_E_SHAPE,
                "cpn_ransac_score_h: need 1 <= B <= 32767, 1 <= N <= 2^24, 0 <= Hn <= 2^20 and B chunks (Hn + 1) < 2^31 (got B %d, N %d, "
                "Hn %d)", B, N, Hn);
    CPN_REQUIRE(px_ok(inlier_px), CPN_E_ARG, "cpn_ransac_score_h: need a finite inlier_px >= 0 (got %g)", inlier_px);
    if (Hn == 0) return 0;                                 // no slot: partial holds nothing
    const dim3 grid(cpn_cdiv(Hn, SCORE_NT), cpn_cdiv(N, CH), B);
    hipLaunchKernelGGL(ransac_score_kernel<TransferRule>, grid, dim3(SCORE_NT), 0, (hipStream_t)stream, H, valid, xy, count, intrinsics,
                       (const float*)nullptr, N, Hn, 0, Hn, inlier_px, partial);
    CPN_LAUNCH_CHECK("cpn_ransac_score_h");
    return 0;
}

extern "C" int cpn_ransac_finish_h(const double* H, const uint8_t* valid, const int* partial, const float* xy, const int* count,
                                   const float* intrinsics, const float* rel_pose, int B, int N, int Hn, double inlier_px,
                                   double min_baseline, float* pose, float* twin, double* Hout, uint8_t* inlier, double* stats,
                                   void* stream) {
    CPN_REQUIRE(xy && count && intrinsics && pose && twin && Hout && inlier && stats && (Hn == 0 || (H && valid && partial)), CPN_E_ARG,
                "cpn_ransac_finish_h: null pointer");
    CPN_REQUIRE(shape_ok(B, N, Hn), CPN_E_SHAPE,
                "cpn_ransac_finish_h: need 1 <= B <= 32767, 1 <= N <= 2^24, 0 <= Hn <= 2^20 and B chunks (Hn + 1) < 2^31 (got B %d, N %d, "
                "Hn %d)", B, N, Hn);
    CPN_REQUIRE(px_ok(inlier_px), CPN_E_ARG, "cpn_ransac_finish_h: need a finite inlier_px >= 0 (got %g)", inlier_px);
    CPN_REQUIRE(px_ok(min_baseline), CPN_E_ARG, "cpn_ransac_finish_h: need a finite min_baseline >= 0 (got %g)", min_baseline);
    hipLaunchKernelGGL(ransac_finish_h_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, H, valid, partial, xy, count, intrinsics,
                       rel_pose, N, Hn, (int)cpn_cdiv(N, CH), inlier_px, min_baseline, pose, twin, Hout, inlier, stats);
    CPN_LAUNCH_CHECK("cpn_ransac_finish_h");
    return 0;
}
