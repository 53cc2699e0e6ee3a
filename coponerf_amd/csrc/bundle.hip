// Two-view bundle adjustment over the pose and the points, with covariances (coponerf_amd/triangulate.py: bundle_adjust): round 27
// of include/coponerf_hip.h, which states the operation order.
//
//   bundle_kernel   cpn_bundle_adjust: ONE workgroup of 256 threads per pair, every sweep inside the one launch.  Levenberg-Marquardt
//                   on the reprojection error of both views over R, t (|t| = 1) and one point per used row; the points are
//                   eliminated row by row (a 3 x 3 Cholesky), which leaves the 6 x 6 system and the 30 sums of pose_gauss_newton.h,
//                   reduced by its park_wave_sums / four_waves and solved by cholesky_solve.h in thread 0.  Sweep A sums the
//                   reduced system at the kept state, sweep B back-substitutes, writes the tentative points and sums their cost
//                   under the tentative pose; nothing per row is kept between the sweeps but the points themselves, float64 in
//                   the caller's workspace (HBM / L2, not LDS: a pair of 131 072 rows works).  After the last state one sweep A at
//                   lambda = 0, the pose's covariance in thread 0 and one sweep for the points' covariances and the outputs.
//
// float64 from the fp32 inputs, one rounding per operation (-ffp-contract=off), sums left to right: tests/bundle_ref.py restates it.
// Cam, project and cam_finite are pinhole.h's; rel_start, store_pose and pose_angles pose_out.h's; RefineState (R, t and the parked
// wave sums), apply_step and the reduction pose_gauss_newton.h's; finite64 sampson.h's; the count clamp and finite32
// ransac_common.h's.  No array below is indexed by a value the compiler does not know: every loop over one is unrolled.
#include "cholesky_solve.h"
#include "common.h"
#include "pinhole.h"
#include "pose_gauss_newton.h"
#include "pose_out.h"
#include "ransac_common.h"

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr double DEG = 57.29577951308232;

__device__ __forceinline__ float nan32() { return __builtin_nanf(""); }
__device__ __forceinline__ double nan64() { return __builtin_nan(""); }

// what a row sees of the pair: a state (R row-major, the unit t) and the two cameras
struct View {
    double R[9], t[3];
};
__device__ __forceinline__ View load_view(const RefineState& st) {
    View v;
#pragma unroll
    for (int i = 0; i < 9; ++i) v.R[i] = st.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) v.t[i] = st.t[i];
    return v;
}

// the residual of a row at (R, t, X): d, Y, r, e2, and round 16's cost and weight
struct Resid {
    double d[3], Y[3], r[4], e2, cost, w;
};
__device__ __forceinline__ Resid residual(const View& v, const Cam& k0, const Cam& k1, const double (&X)[3], const float* __restrict__ m,
                                          double s2) {
    Resid q;
#pragma unroll
    for (int j = 0; j < 3; ++j) q.d[j] = X[j] - v.t[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) q.Y[j] = (v.R[j] * q.d[0] + v.R[3 + j] * q.d[1]) + v.R[6 + j] * q.d[2];
    double p0, p1, p2, p3;
    project(k0, X, p0, p1);
    project(k1, q.Y, p2, p3);
    q.r[0] = p0 - (double)m[0];
    q.r[1] = p1 - (double)m[1];
    q.r[2] = p2 - (double)m[2];
    q.r[3] = p3 - (double)m[3];
    q.e2 = ((q.r[0] * q.r[0] + q.r[1] * q.r[1]) + q.r[2] * q.r[2]) + q.r[3] * q.r[3];
    const double u = 1.0 + q.e2 / s2;
    q.cost = (q.e2 / 2.0) / u;
    q.w = 1.0 / (u * u);
    return q;
}

// the blocks of a row: V (damped), W, gx always; U and gp where FULL
struct Blocks {
    double V[3][3], W[6][3], gx[3], U[21], gp[6];
};
template <bool FULL>
__device__ __forceinline__ void blocks(const View& v, const Cam& k0, const Cam& k1, const double (&X)[3], const Resid& q, double lambda,
                                       Blocks& o) {
    double Jx[4][3], Jp[2][6];
    Jx[0][0] = k0.fx / X[2];
    Jx[0][1] = 0.0;
    Jx[0][2] = -(((k0.fx * X[0]) / X[2]) / X[2]);
    Jx[1][0] = 0.0;
    Jx[1][1] = k0.fy / X[2];
    Jx[1][2] = -(((k0.fy * X[1]) / X[2]) / X[2]);
    double P[2][3];
    P[0][0] = k1.fx / q.Y[2];
    P[0][1] = 0.0;
    P[0][2] = -(((k1.fx * q.Y[0]) / q.Y[2]) / q.Y[2]);
    P[1][0] = 0.0;
    P[1][1] = k1.fy / q.Y[2];
    P[1][2] = -(((k1.fy * q.Y[1]) / q.Y[2]) / q.Y[2]);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Jx[2 + a][c] = (P[a][0] * v.R[3 * c] + P[a][1] * v.R[3 * c + 1]) + P[a][2] * v.R[3 * c + 2];
        const double* const M = Jx[2 + a];
        Jp[a][0] = M[1] * q.d[2] - M[2] * q.d[1];
        Jp[a][1] = M[2] * q.d[0] - M[0] * q.d[2];
        Jp[a][2] = M[0] * q.d[1] - M[1] * q.d[0];
        Jp[a][3] = -M[0];
        Jp[a][4] = -M[1];
        Jp[a][5] = -M[2];
    }
    double wJx[4][3], wJp[2][6];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) wJx[a][c] = q.w * Jx[a][c];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int j = 0; j < 6; ++j) wJp[a][j] = q.w * Jp[a][j];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int k = c; k < 3; ++k)
            o.V[c][k] = o.V[k][c] = ((wJx[0][c] * Jx[0][k] + wJx[1][c] * Jx[1][k]) + wJx[2][c] * Jx[2][k]) + wJx[3][c] * Jx[3][k];
        o.gx[c] = ((wJx[0][c] * q.r[0] + wJx[1][c] * q.r[1]) + wJx[2][c] * q.r[2]) + wJx[3][c] * q.r[3];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o.V[c][c] = o.V[c][c] + lambda * o.V[c][c];
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) o.W[j][c] = wJp[0][j] * Jx[2][c] + wJp[1][j] * Jx[3][c];
    if (FULL) {
        int at = 0;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
#pragma unroll
            for (int k = j; k < 6; ++k) o.U[at++] = wJp[0][j] * Jp[0][k] + wJp[1][j] * Jp[1][k];
            o.gp[j] = wJp[0][j] * q.r[2] + wJp[1][j] * q.r[3];
        }
    }
}

// Vi = V^-1, column k by cholesky_solve on a fresh copy of V with the right side -e_k; false where a solve fails
__device__ __forceinline__ bool inverse3(const double (&V)[3][3], double (&Vi)[3][3]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double A[3][3], g[3], y[3], x[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) A[i][j] = V[i][j];
            g[i] = i == k ? -1.0 : 0.0;
            y[i] = x[i] = 0.0;
        }
        ok = cholesky_solve<3>(A, g, y, x) && ok;
#pragma unroll
        for (int i = 0; i < 3; ++i) Vi[i][k] = x[i];
    }
    return ok;
}

// T = W Vi
__device__ __forceinline__ void times_inverse(const double (&W)[6][3], const double (&Vi)[3][3], double (&T)[6][3]) {
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) T[j][c] = (W[j][0] * Vi[0][c] + W[j][1] * Vi[1][c]) + W[j][2] * Vi[2][c];
}

struct BundleShared {
    RefineState st, trial;          // the kept and the tentative R and t; st.red parks the wave sums of every sweep
    double A[6][6], g[6], y[6], x[6];        // thread 0's 6 x 6 solves
    double C[6][6], S0[6][6];       // the pose's covariance and the matrix it inverts
    double len, lambda, len0;
    int go, cur, final, cov_ok;
};

__global__ __launch_bounds__(NT) void bundle_kernel(const float* __restrict__ xy, const int* __restrict__ count,
                                                    const float* __restrict__ intrinsics, const float* __restrict__ pose,
                                                    const float* __restrict__ xyz_in, const uint8_t* __restrict__ flag,
                                                    const uint8_t* __restrict__ inlier, int N, int iters, double scale_px, double ftol,
                                                    int min_rows, double* __restrict__ work, float* __restrict__ pose_out,
                                                    float* __restrict__ xyz, float* __restrict__ geom, float* __restrict__ cov_x,
                                                    double* __restrict__ cov, double* __restrict__ stats) {
    __shared__ BundleShared sh;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = clamp_count(count[b], N);
    const float* const P = pose + (size_t)b * 16;
    const float* const rows = xy + (size_t)b * N * 4;
    const Cam k0 = load_cam(intrinsics + ((size_t)b * 2 + 0) * 16), k1 = load_cam(intrinsics + ((size_t)b * 2 + 1) * 16);
    double* const half0 = work + (size_t)b * 2 * N * 3;
    double* const half1 = half0 + (size_t)N * 3;
    float* const xo = xyz + (size_t)b * N * 3;
    float* const go = geom + (size_t)b * N * 4;
    float* const co = cov_x + (size_t)b * N * 6;
    double* const so = stats + (size_t)b * CPN_BUNDLE_STATS;
    const double s2 = scale_px * scale_px;

    if (tid == 0) {
        const RelStart start = rel_start(P);
        sh.go = (start.ok && cam_finite(k0) && cam_finite(k1)) ? 1 : 0;
        sh.len0 = start.len0;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) sh.st.R[3 * r + c] = start.rel.R[r][c];
            sh.st.t[r] = start.rel.t[r] / start.len0;
        }
        sh.cur = 0;
        sh.final = iters == 0 ? 1 : 0;
        sh.lambda = 1e-3;
        sh.cov_ok = 0;
    }
    __syncthreads();
    const bool pose_ok = sh.go != 0;
    const double len0 = sh.len0;

    // ---- the start points and the used rows: a row that is not used holds NaN in both halves of the workspace
    double used[1] = {0.0};
    if (pose_ok) {
        const View v = load_view(sh.st);
        const float* const xin = xyz_in + (size_t)b * N * 3;
        const uint8_t* const f = flag + (size_t)b * N;
        for (int i = tid; i < n; i += NT) {
            const float* const m = rows + (size_t)i * 4;
            double X[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) X[c] = (double)xin[(size_t)i * 3 + c] / len0;
            bool ok = finite32(m[0]) && finite32(m[1]) && finite32(m[2]) && finite32(m[3]) && f[i] == 0;
            ok = ok && finite64(X[0]) && finite64(X[1]) && finite64(X[2]);
            if (inlier) ok = ok && inlier[(size_t)b * N + i] != 0;
            if (ok) {
                const Resid q = residual(v, k0, k1, X, m, s2);
                ok = X[2] > 0.0 && q.Y[2] > 0.0;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) half0[(size_t)i * 3 + c] = half1[(size_t)i * 3 + c] = ok ? X[c] : nan64();
            used[0] += ok ? 1.0 : 0.0;
        }
    }
    park_wave_sums(used, sh.st.red);
    __syncthreads();
    const int n_used = (int)four_waves(sh.st.red[0]);
    __syncthreads();
    if (!pose_ok || n_used < min_rows) {                   // not usable: the pose as it came, status 2
        for (int i = tid; i < N; i += NT) {
            for (int c = 0; c < 3; ++c) xo[(size_t)i * 3 + c] = nan32();
            for (int c = 0; c < 4; ++c) go[(size_t)i * 4 + c] = nan32();
            for (int c = 0; c < 6; ++c) co[(size_t)i * 6 + c] = nan32();
        }
        if (tid < 16) pose_out[(size_t)b * 16 + tid] = P[tid];
        if (tid < 36) cov[(size_t)b * 36 + tid] = nan64();
        if (tid < CPN_BUNDLE_STATS) so[tid] = tid == 3 ? (double)n_used : (tid == 4 || tid == 5) ? 0.0 : tid == 11 ? 2.0 : nan64();
        return;
    }

    // ---- the iteration
    double cost0 = 0.0, kept = 0.0;                        // thread 0's
    int accepted = 0, rejected = 0, solves = 0, status = 0;
    bool first = true;
    for (;;) {
        // sweep A at the kept state
        {
            const double lambda = sh.final ? 0.0 : sh.lambda;
            const double* const Xk = sh.cur ? half1 : half0;
            const View v = load_view(sh.st);
            double acc[POSE_NSUM];
#pragma unroll
            for (int k = 0; k < POSE_NSUM; ++k) acc[k] = 0.0;
            for (int i = tid; i < n; i += NT) {
                const double X[3] = {Xk[(size_t)i * 3], Xk[(size_t)i * 3 + 1], Xk[(size_t)i * 3 + 2]};
                if (!finite64(X[0])) continue;
                const Resid q = residual(v, k0, k1, X, rows + (size_t)i * 4, s2);
                Blocks bl;
                blocks<true>(v, k0, k1, X, q, lambda, bl);
                double Vi[3][3], T[6][3];
                if (inverse3(bl.V, Vi)) {
                    times_inverse(bl.W, Vi, T);
                    int at = 0;
#pragma unroll
                    for (int j = 0; j < 6; ++j) {
#pragma unroll
                        for (int k = j; k < 6; ++k) {
                            acc[at] += bl.U[at] - ((T[j][0] * bl.W[k][0] + T[j][1] * bl.W[k][1]) + T[j][2] * bl.W[k][2]);
                            ++at;
                        }
                        acc[21 + j] += bl.gp[j] - ((T[j][0] * bl.gx[0] + T[j][1] * bl.gx[1]) + T[j][2] * bl.gx[2]);
                    }
                }
                acc[27] += q.cost;
                acc[28] += q.w;
                acc[29] += 1.0;
            }
            park_wave_sums(acc, sh.st.red);
        }
        __syncthreads();
        if (tid == 0) {
            double sum[POSE_NSUM];
            for (int k = 0; k < POSE_NSUM; ++k) sum[k] = four_waves(sh.st.red[k]);
            kept = sum[27];
            if (first) cost0 = kept;
            int at = 0;
            for (int j = 0; j < 6; ++j) {
                for (int k = j; k < 6; ++k) sh.A[j][k] = sh.A[k][j] = sum[at++];
                sh.g[j] = sum[21 + j];
            }
            double trace = 0.0;
            for (int j = 0; j < 6; ++j) trace += sh.A[j][j];
            const double pin = trace / 6.0;                // the gauge: the residual cannot see the length of t
            if (!sh.final) {
                for (int j = 0; j < 6; ++j) sh.A[j][j] = sh.A[j][j] + sh.lambda * sh.A[j][j];
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) sh.A[3 + i][3 + j] = sh.A[3 + i][3 + j] + pin * (sh.st.t[i] * sh.st.t[j]);
                bool ok = cholesky_solve<6>(sh.A, sh.g, sh.y, sh.x);
                if (ok) {
                    double tn[3];
                    for (int i = 0; i < 9; ++i) sh.trial.R[i] = sh.st.R[i];
                    for (int i = 0; i < 3; ++i) {
                        sh.trial.t[i] = sh.st.t[i];
                        tn[i] = sh.st.t[i] + sh.x[3 + i];
                    }
                    sh.len = sqrt((tn[0] * tn[0] + tn[1] * tn[1]) + tn[2] * tn[2]);
                    ok = apply_step(sh.trial, sh.x);
                }
                if (ok) {
                    ++solves;
                    sh.go = 1;                             // sweep B follows
                } else {
                    status = 1;                            // the pair keeps its state; the covariance follows
                    sh.final = 1;
                    sh.go = 2;
                }
            } else {
                // the pose's covariance in the gauge |t| = 1 and the pair's outputs
                double (&S0)[6][6] = sh.S0;
                for (int j = 0; j < 6; ++j)
                    for (int k = 0; k < 6; ++k) S0[j][k] = sh.A[j][k];
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) S0[3 + i][3 + j] = S0[3 + i][3 + j] + pin * (sh.st.t[i] * sh.st.t[j]);
                bool ok = true;
                for (int k = 0; k < 6 && ok; ++k) {
                    for (int i = 0; i < 6; ++i) {
                        for (int j = 0; j < 6; ++j) sh.A[i][j] = S0[i][j];
                        sh.g[i] = i == k ? -1.0 : 0.0;
                    }
                    ok = cholesky_solve<6>(sh.A, sh.g, sh.y, sh.x);
                    for (int i = 0; i < 6; ++i) sh.C[i][k] = sh.x[i];
                }
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) sh.C[3 + i][3 + j] = sh.C[3 + i][3 + j] - (sh.st.t[i] * sh.st.t[j]) / pin;
                if (!ok) {
                    status = 1;
                    for (int i = 0; i < 6; ++i)
                        for (int j = 0; j < 6; ++j) sh.C[i][j] = nan64();
                }
                sh.cov_ok = ok ? 1 : 0;
                const double sigma = sum[29] > 5.0 ? sqrt((2.0 * kept) / (sum[29] - 5.0)) : nan64();
                double deg_R, deg_t;
                pose_angles(sh.st.R, sh.st.t, load_pose(P), len0, deg_R, deg_t);
                store_pose(pose_out + (size_t)b * 16, sh.st.R, sh.st.t, len0);
                for (int i = 0; i < 6; ++i)
                    for (int j = 0; j < 6; ++j) cov[(size_t)b * 36 + 6 * i + j] = sh.C[i][j];
                so[0] = cost0;
                so[1] = kept;
                so[2] = sum[28];
                so[3] = sum[29];
                so[4] = (double)accepted;
                so[5] = (double)rejected;
                so[6] = sh.lambda;
                so[7] = sigma;
                so[8] = (sigma * sqrt((sh.C[0][0] + sh.C[1][1]) + sh.C[2][2])) * DEG;
                so[9] = (sigma * sqrt((sh.C[3][3] + sh.C[4][4]) + sh.C[5][5])) * DEG;
                so[10] = deg_R;
                so[11] = (double)status;
                sh.go = 0;
            }
            first = false;
        }
        __syncthreads();
        const int next = sh.go;
        if (next == 0) break;
        if (next == 2) continue;

        // sweep B: the tentative points and their cost under the tentative pose
        {
            const double lambda = sh.lambda, len = sh.len;
            const double* const Xk = sh.cur ? half1 : half0;
            double* const Xt = sh.cur ? half0 : half1;
            const View v = load_view(sh.st), vn = load_view(sh.trial);
            double delta[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) delta[j] = sh.x[j];
            double acc[2] = {0.0, 0.0};                    // the cost, the rows that left the front of a camera
            for (int i = tid; i < n; i += NT) {
                const double X[3] = {Xk[(size_t)i * 3], Xk[(size_t)i * 3 + 1], Xk[(size_t)i * 3 + 2]};
                if (!finite64(X[0])) continue;
                const float* const m = rows + (size_t)i * 4;
                const Resid q = residual(v, k0, k1, X, m, s2);
                Blocks bl;
                blocks<false>(v, k0, k1, X, q, lambda, bl);
                double Vi[3][3], dX[3] = {0.0, 0.0, 0.0};
                if (inverse3(bl.V, Vi)) {
                    double vv[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        vv[c] = bl.gx[c] + (((((bl.W[0][c] * delta[0] + bl.W[1][c] * delta[1]) + bl.W[2][c] * delta[2]) + bl.W[3][c] * delta[3]) +
                                             bl.W[4][c] * delta[4]) + bl.W[5][c] * delta[5]);
#pragma unroll
                    for (int a = 0; a < 3; ++a) dX[a] = -((Vi[a][0] * vv[0] + Vi[a][1] * vv[1]) + Vi[a][2] * vv[2]);
                }
                double Xn[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    Xn[c] = (X[c] + dX[c]) / len;
                    Xt[(size_t)i * 3 + c] = Xn[c];
                }
                const Resid qn = residual(vn, k0, k1, Xn, m, s2);
                const bool ok = finite64(Xn[0]) && finite64(Xn[1]) && finite64(Xn[2]) && Xn[2] > 0.0 && qn.Y[2] > 0.0;
                if (ok)
                    acc[0] += qn.cost;
                else
                    acc[1] += 1.0;
            }
            park_wave_sums(acc, sh.st.red);
        }
        __syncthreads();
        if (tid == 0) {
            const double cost = four_waves(sh.st.red[0]), bad = four_waves(sh.st.red[1]);
            const double trial = bad > 0.0 ? (double)INFINITY : cost;
            if (trial < kept) {
                ++accepted;
                sh.cur ^= 1;
                for (int i = 0; i < 9; ++i) sh.st.R[i] = sh.trial.R[i];
                for (int i = 0; i < 3; ++i) sh.st.t[i] = sh.trial.t[i];
                sh.lambda = fmax(sh.lambda / 3.0, 1e-12);
                if (kept - trial <= ftol * kept) sh.final = 1;
            } else {
                ++rejected;
                sh.lambda = 4.0 * sh.lambda;
                if (sh.lambda > 1e8) sh.final = 1;
            }
            if (solves >= iters) sh.final = 1;
        }
        __syncthreads();
    }

    // ---- the points, their covariances and the rows' figures at the last state (lambda = 0)
    {
        const double* const Xk = sh.cur ? half1 : half0;
        const View v = load_view(sh.st);
        const bool cov_ok = sh.cov_ok != 0;
        const double l2 = len0 * len0;
        for (int i = tid; i < N; i += NT) {
            bool on = false;
            double X[3] = {0.0, 0.0, 0.0};
            if (i < n) {
#pragma unroll
                for (int c = 0; c < 3; ++c) X[c] = Xk[(size_t)i * 3 + c];
                on = finite64(X[0]);
            }
            if (!on) {
                for (int c = 0; c < 3; ++c) xo[(size_t)i * 3 + c] = nan32();
                for (int c = 0; c < 4; ++c) go[(size_t)i * 4 + c] = nan32();
                for (int c = 0; c < 6; ++c) co[(size_t)i * 6 + c] = nan32();
                continue;
            }
            const Resid q = residual(v, k0, k1, X, rows + (size_t)i * 4, s2);
            Blocks bl;
            blocks<false>(v, k0, k1, X, q, 0.0, bl);
            double Vi[3][3], T[6][3], Cov[6];
            if (cov_ok && inverse3(bl.V, Vi)) {
                times_inverse(bl.W, Vi, T);
                double CT[6][3];
#pragma unroll
                for (int j = 0; j < 6; ++j)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        CT[j][c] = ((((sh.C[j][0] * T[0][c] + sh.C[j][1] * T[1][c]) + sh.C[j][2] * T[2][c]) + sh.C[j][3] * T[3][c]) +
                                    sh.C[j][4] * T[4][c]) + sh.C[j][5] * T[5][c];
                int at = 0;
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int c = a; c < 3; ++c)
                        Cov[at++] = Vi[a][c] + (((((T[0][a] * CT[0][c] + T[1][a] * CT[1][c]) + T[2][a] * CT[2][c]) + T[3][a] * CT[3][c]) +
                                                 T[4][a] * CT[4][c]) + T[5][a] * CT[5][c]);
            } else {
#pragma unroll
                for (int c = 0; c < 6; ++c) Cov[c] = nan64();
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) xo[(size_t)i * 3 + c] = (float)(len0 * X[c]);
            go[(size_t)i * 4 + 0] = (float)(len0 * X[2]);
            go[(size_t)i * 4 + 1] = (float)(len0 * q.Y[2]);
            go[(size_t)i * 4 + 2] = (float)sqrt(q.e2);
            go[(size_t)i * 4 + 3] = (float)q.w;
#pragma unroll
            for (int c = 0; c < 6; ++c) co[(size_t)i * 6 + c] = (float)(l2 * Cov[c]);
        }
    }
}

}  // namespace

extern "C" int cpn_bundle_adjust(const float* xy, const int* count, const float* intrinsics, const float* pose, const float* xyz_in,
                                 const uint8_t* flag, const uint8_t* inlier, int B, int N, int iters, double scale_px, double ftol,
                                 int min_rows, double* work, float* pose_out, float* xyz, float* geom, float* cov_x, double* cov,
                                 double* stats, void* stream) {
    CPN_REQUIRE(xy && count && intrinsics && pose && xyz_in && flag && work && pose_out && xyz && geom && cov_x && cov && stats, CPN_E_ARG,
                "cpn_bundle_adjust: null pointer");
    CPN_REQUIRE(B >= 1 && B <= 32767 && N >= 1 && N <= (1 << 24), CPN_E_SHAPE,
                "cpn_bundle_adjust: need 1 <= B <= 32767 and 1 <= N <= 2^24 (got B %d, N %d)", B, N);
    CPN_REQUIRE(iters >= 0 && scale_px > 0.0 && px_ok(scale_px) && px_ok(ftol) && min_rows >= 1, CPN_E_ARG,
                "cpn_bundle_adjust: need iters >= 0, a finite scale_px > 0, a finite ftol >= 0 and min_rows >= 1 (got %d, %g, %g, %d)", iters,
                scale_px, ftol, min_rows);
    hipLaunchKernelGGL(bundle_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, xy, count, intrinsics, pose, xyz_in, flag, inlier, N, iters,
                       scale_px, ftol, min_rows, work, pose_out, xyz, geom, cov_x, cov, stats);
    CPN_LAUNCH_CHECK("cpn_bundle_adjust");
    return 0;
}
