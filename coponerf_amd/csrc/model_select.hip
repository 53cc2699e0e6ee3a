// Which of the three models of coponerf_amd/matches.py explains a pair - E, one plane, a rotation alone - and the refinement of the
// homography that the verdict needs (select_pose): include/coponerf_hip.h, round 23.
//
//   refine_homography_kernel<NP>  cpn_refine_homography: cpn_refine_pose's shape with sampson_h.h's residual.  ONE workgroup of 256
//                                 threads per pair, all Gauss-Newton passes inside it.  NP = 9, the plane: the state is the unit h,
//                                 the directions are the nine entries; NP = 3, the rotation alone: the state is R, the directions
//                                 are [e_k]x R.  Per pass thread t walks the matches t, t + 256, .. in ascending order and keeps
//                                 NP (NP + 1) / 2 + NP + 3 float64 sums in registers (57 for the plane: every loop over them is
//                                 unrolled, none is indexed at run time); wave_sum's butterfly, then LDS and (w0 + w1) + (w2 + w3)
//                                 in thread 0, which solves the damped system by Cholesky IN LDS - a 9 x 9 matrix indexed at run
//                                 time would otherwise live in scratch memory -, updates the state and leaves H and the directions
//                                 in LDS for the next pass.  Two barriers a pass.  Pass `iters` only measures.
//   model_gric_kernel             cpn_model_gric: ONE workgroup per pair walks the rows in the same order, forms the three
//                                 residuals of a row, its label byte and seven sums (block256_sum), and thread 0 scores and picks.
//
// float64 from the fp32 inputs, one rounding per operation (-ffp-contract=off), sums in a fixed order, no atomics:
// tests/model_select_ref.py restates both in numpy.  The residual under H is sampson_h.h's, under E sampson.h's; the nearest
// rotation is formed as ransac_h.hip forms it (jacobi_svd.h), the rotation step is rotation_step.h's, the Cholesky solve
// cholesky_solve.h's (matches.hip shares both), the pose pose_out.h's.
#include "cholesky_solve.h"
#include "common.h"
#include "homography.h"
#include "jacobi_svd.h"
#include "pinhole.h"
#include "pose_out.h"
#include "ransac_common.h"
#include "rotation_step.h"
#include "sampson.h"
#include "sampson_h.h"

#include "../../include/coponerf_hip.h"

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr double INF = __builtin_inf();

constexpr int n_sums(int NP) { return NP * (NP + 1) / 2 + NP + 3; }     // the normal matrix, the gradient, cost, weights, rows

template <int NP>
struct RefineStateH {
    double H[9];                    // what the residual is taken under: the unit h (NP = 9), R (NP = 3)
    double H0[9];                   // the state the passes began at
    double dH[NP][9];               // the directions: the nine unit matrices, or [e_k]x R
    double red[n_sums(NP)][4];      // the four wave sums of a pass
    double sum[n_sums(NP)];
    double A[NP][NP], g[NP], y[NP], x[NP];
    int go;                         // another pass follows
};

__device__ __forceinline__ double sum_squares9(const double* h) {
    double ss = h[0] * h[0];
    for (int c = 1; c < 9; ++c) ss = ss + h[c] * h[c];
    return ss;
}

// the state at the start from the pair's H0 -> whether there is one
template <int NP>
__device__ bool start_state(RefineStateH<NP>& st, const double* __restrict__ H0) {
    double h[9];
    bool fin = true;
    for (int c = 0; c < 9; ++c) {
        h[c] = H0[c];
        fin = fin && finite64(h[c]);
    }
    if constexpr (NP == 9) {                                // H0 over its Frobenius norm, negated where det < 0
        const double nrm = sqrt(sum_squares9(h));
        if (!fin || !(nrm > 0.0) || !finite64(nrm)) return false;
        double u[9], g[9];
        for (int c = 0; c < 9; ++c) u[c] = h[c] / nrm;
        adjugate(u, g);
        const bool flip = determinant(u, g) < 0.0;
        for (int c = 0; c < 9; ++c) {
            st.H[c] = flip ? -u[c] : u[c];
            fin = fin && finite64(u[c]);
        }
        for (int k = 0; k < NP; ++k)
            for (int c = 0; c < 9; ++c) st.dH[k][c] = k == c ? 1.0 : 0.0;
        return fin;
    }
    // the rotation nearest to H0: R_n = (u_1 v_1^T + u_2 v_2^T) + u_3 v_3^T, as cpn_ransac_finish_h forms it
    if (!fin) return false;
    double G[9], V[9], sg[3], U[3][3], W[3][3];
    for (int c = 0; c < 9; ++c) G[c] = h[c];
    jacobi_svd(G, V, sg);
    frame(G, 0, 1, U);
    frame(V, 0, 1, W);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double r = (U[0][i] * W[0][j] + U[1][i] * W[1][j]) + U[2][i] * W[2][j];
            st.H[3 * i + j] = r;
            fin = fin && finite64(r);
        }
    return fin;
}

// the directions of the next pass (the plane's never change)
template <int NP>
__device__ void set_directions(RefineStateH<NP>& st) {
    if constexpr (NP == 3)
        for (int k = 0; k < 3; ++k) cross_rows(st.H, k, st.dH[k]);
}

// h <- (h + delta) / |h + delta|, or R <- exp([delta]x) R; false (state untouched) where not finite
template <int NP>
__device__ bool apply_step_h(RefineStateH<NP>& st) {
    double n[9];
    if constexpr (NP == 9) {
        for (int c = 0; c < 9; ++c) n[c] = st.H[c] + st.x[c];
        const double len = sqrt(sum_squares9(n));
        if (!(len > 0.0) || !finite64(len)) return false;
        for (int c = 0; c < 9; ++c) n[c] = n[c] / len;
    } else {
        const double w[3] = {st.x[0], st.x[1], st.x[2]};
        rotate_left(w, st.H, n);
    }
    for (int c = 0; c < 9; ++c)
        if (!finite64(n[c])) return false;
    for (int c = 0; c < 9; ++c) st.H[c] = n[c];
    return true;
}

template <int NP>
__global__ __launch_bounds__(NT) void refine_homography_kernel(const float* __restrict__ xy, const int* __restrict__ count,
                                                               const float* __restrict__ intrinsics, const double* __restrict__ H0,
                                                               int N, int iters, double scale_px, double* __restrict__ Hout,
                                                               float* __restrict__ pose, double* __restrict__ stats) {
    constexpr int NA = NP * (NP + 1) / 2, NS = n_sums(NP);
    __shared__ RefineStateH<NP> st;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* const Hb = H0 + (size_t)b * 9;
    const int n = clamp_count(count[b], N);
    if (tid == 0) {
        const bool ok = n > 0 && iters > 0 && start_state(st, Hb);
        st.go = ok ? 1 : 0;
        if (ok) {
            for (int c = 0; c < 9; ++c) st.H0[c] = st.H[c];
            set_directions(st);
        }
    }
    __syncthreads();
    if (!st.go) {                                          // nothing to do: H0 as it came, the identity, status 2
        if (tid < 9) Hout[(size_t)b * 9 + tid] = Hb[tid];
        if (tid < 16) pose[(size_t)b * 16 + tid] = (tid % 5 == 0) ? 1.0f : 0.0f;
        if (tid < 8) stats[(size_t)b * 8 + tid] = tid == 7 ? 2.0 : 0.0;
        return;
    }
    const Cam k0 = load_cam(intrinsics + ((size_t)b * 2 + 0) * 16), k1 = load_cam(intrinsics + ((size_t)b * 2 + 1) * 16);
    const float* const rows = xy + (size_t)b * N * 4;
    const double s2 = scale_px * scale_px;
    int done = 0, status = 0;
    double cost0 = 0.0;

    for (int pass = 0;; ++pass) {
        double acc[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) acc[k] = 0.0;
        for (int i = tid; i < n; i += NT) {
            const float* const m = rows + (size_t)i * 4;
            const SampsonH s = sampson_h_px(st.H, k0, k1, (double)m[0], (double)m[1], (double)m[2], (double)m[3]);
            if (!s.ok) continue;                            // weight 0, not counted
            double J0[NP], J1[NP];
#pragma unroll
            for (int k = 0; k < NP; ++k) sampson_h_along(s, st.dH[k], k0, k1, J0[k], J1[k]);
            const double u = 1.0 + s.e2 / s2, w = 1.0 / (u * u);
            int at = 0;
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const double w0 = w * J0[j], w1 = w * J1[j];
#pragma unroll
                for (int k = j; k < NP; ++k) acc[at++] += w0 * J0[k] + w1 * J1[k];
                acc[NA + j] += w0 * s.y0 + w1 * s.y1;
            }
            acc[NA + NP] += (s.e2 / 2.0) / u;
            acc[NA + NP + 1] += w;
            acc[NA + NP + 2] += 1.0;
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) acc[k] = wave_sum(acc[k]);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < NS; ++k) st.red[k][wave] = acc[k];
        }
        __syncthreads();
        if (tid == 0) {
            for (int k = 0; k < NS; ++k) st.sum[k] = (st.red[k][0] + st.red[k][1]) + (st.red[k][2] + st.red[k][3]);
            if (pass == 0) cost0 = st.sum[NA + NP];
            bool more = pass < iters;
            if (more) {
                int at = 0;
                for (int j = 0; j < NP; ++j) {
                    for (int k = j; k < NP; ++k) st.A[j][k] = st.A[k][j] = st.sum[at++];
                    st.g[j] = st.sum[NA + j];
                }
                double trace = 0.0;
                for (int j = 0; j < NP; ++j) trace += st.A[j][j];
                for (int j = 0; j < NP; ++j) st.A[j][j] = st.A[j][j] + 1e-3 * st.A[j][j];
                if constexpr (NP == 9) {                   // the gauge: the residual cannot see the length of h
                    const double pin = trace / 9.0;
                    for (int i = 0; i < NP; ++i)
                        for (int j = 0; j < NP; ++j) st.A[i][j] = st.A[i][j] + pin * (st.H[i] * st.H[j]);
                }
                more = cholesky_solve<NP>(st.A, st.g, st.y, st.x) && apply_step_h(st);
                if (more) {
                    set_directions(st);
                    ++done;
                } else {
                    status = 1;                            // the pair keeps its state and stops
                }
            }
            st.go = more ? 1 : 0;
            if (!more) {
                double moved = 0.0, spread = 0.0;
                for (int c = 0; c < 9; ++c) {
                    const double e = st.H[c] - st.H0[c];
                    moved += e * e;
                }
                float* const po = pose + (size_t)b * 16;
                if constexpr (NP == 9) {
                    moved = sqrt(moved);
                    double G[9], V[9], sg[3];
                    for (int c = 0; c < 9; ++c) G[c] = st.H[c];
                    jacobi_svd(G, V, sg);
                    spread = sg[0] / sg[1] - sg[2] / sg[1];
                    for (int k = 0; k < 16; ++k) po[k] = (k % 5 == 0) ? 1.0f : 0.0f;
                } else {
                    moved = 2.0 * asin(fmin(sqrt(moved) / 2.8284271247461903, 1.0)) * 57.29577951308232;
                    const double zero[3] = {0.0, 0.0, 0.0};
                    store_pose(po, st.H, zero, 1.0);
                }
                for (int c = 0; c < 9; ++c) Hout[(size_t)b * 9 + c] = st.H[c];
                double* const so = stats + (size_t)b * 8;
                so[0] = cost0;
                so[1] = st.sum[NA + NP];
                so[2] = st.sum[NA + NP + 1];
                so[3] = st.sum[NA + NP + 2];
                so[4] = moved;
                so[5] = spread;
                so[6] = (double)done;
                so[7] = (double)status;
            }
        }
        __syncthreads();
        if (!st.go) return;
    }
}

// ---- the choice
constexpr double LN4 = 1.3862943611198906;                 // ln 4 rounded to float64
struct GricState {
    double M[3][9];                                        // E = [t]x R of pose_e, H_plane, H_rot
    int in[3];
};

__global__ __launch_bounds__(NT) void model_gric_kernel(const float* __restrict__ xy, const int* __restrict__ count,
                                                        const float* __restrict__ intrinsics, const float* __restrict__ pose_e,
                                                        const double* __restrict__ H_plane, const double* __restrict__ H_rot,
                                                        const uint8_t* __restrict__ avail, const double* __restrict__ ln4n, int N,
                                                        double sigma_px, double* __restrict__ gric, uint8_t* __restrict__ label,
                                                        double* __restrict__ stats) {
    __shared__ GricState st;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = clamp_count(count[b], N);
    if (tid == 0) {
        const Pose P = load_pose(pose_e + (size_t)b * 16);
        essential(&P.R[0][0], P.t, st.M[0]);
        for (int c = 0; c < 9; ++c) {
            st.M[1][c] = H_plane[(size_t)b * 9 + c];
            st.M[2][c] = H_rot[(size_t)b * 9 + c];
        }
        for (int m = 0; m < 3; ++m) {
            bool fin = avail[(size_t)b * 3 + m] != 0;
            for (int c = 0; c < 9; ++c) fin = fin && finite64(st.M[m][c]);
            st.in[m] = fin ? 1 : 0;
        }
    }
    __syncthreads();
    const Cam k0 = load_cam(intrinsics + ((size_t)b * 2 + 0) * 16), k1 = load_cam(intrinsics + ((size_t)b * 2 + 1) * 16);
    const float* const rows = xy + (size_t)b * N * 4;
    const double s2 = sigma_px * sigma_px;
    const double cap[3] = {2.0, 4.0, 4.0};                 // 2 (4 - d): d = 3 for E, 2 for the plane and the rotation
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // rho per model, the rows below the cap per model, the usable rows
    for (int i = tid; i < N; i += NT) {
        uint8_t bits = 0;
        if (i < n) {
            const float* const m = rows + (size_t)i * 4;
            if (finite32(m[0]) && finite32(m[1]) && finite32(m[2]) && finite32(m[3])) {
                const double a0 = ((double)m[0] - k0.cx) / k0.fx, a1 = ((double)m[1] - k0.cy) / k0.fy;
                const double b0 = ((double)m[2] - k1.cx) / k1.fx, b1 = ((double)m[3] - k1.cy) / k1.fy;
                const Sampson se = sampson_normalised(st.M[0], k0, k1, a0, a1, b0, b1);
                const double r = se.n / sqrt(se.D);
                const SampsonH sp = sampson_h(st.M[1], k0, k1, a0, a1, b0, b1), sr = sampson_h(st.M[2], k0, k1, a0, a1, b0, b1);
                const double e2[3] = {r * r, sp.e2, sr.e2};
                const bool counts[3] = {residual_ok(se, r), sp.ok, sr.ok};
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double x = e2[k] / s2;
                    const bool below = st.in[k] && counts[k] && x < cap[k];
                    acc[k] += below ? x : cap[k];
                    acc[3 + k] += below ? 1.0 : 0.0;
                    bits |= below ? (uint8_t)(1 << k) : (uint8_t)0;
                }
                acc[6] += 1.0;
            }
        }
        label[(size_t)b * N + i] = bits;
    }
    block256_sum(acc);
    if (tid != 0) return;

    double* const go = gric + (size_t)b * 3;
    double* const so = stats + (size_t)b * 7;
    const double nu = acc[6];
    const double dim[3] = {3.0, 2.0, 2.0}, par[3] = {5.0, 8.0, 3.0};
    bool any = false;
    double val[3];
    for (int m = 0; m < 3; ++m) {
        const bool in = st.in[m] && nu > 0.0;
        val[m] = in ? (acc[m] + (LN4 * dim[m]) * nu) + ln4n[(int)nu] * par[m] : INF;
        go[m] = val[m];
        any = any || in;
    }
    // the smallest; a tie goes to the model with fewer parameters: the rotation, then the plane, then E
    const int order[3] = {2, 1, 0};
    int best = -1, second = -1;
    for (int k = 0; k < 3; ++k) {
        const int m = order[k];
        if (val[m] < INF && (best < 0 || val[m] < val[best])) best = m;
    }
    for (int k = 0; k < 3; ++k) {
        const int m = order[k];
        if (m != best && val[m] < INF && (second < 0 || val[m] < val[second])) second = m;
    }
    so[0] = (double)best;
    so[1] = nu;
    for (int m = 0; m < 3; ++m) so[2 + m] = (nu > 0.0 && st.in[m]) ? acc[3 + m] : 0.0;
    so[5] = (best >= 0 && second >= 0) ? val[second] - val[best] : INF;
    so[6] = nu > 0.0 ? (any ? 0.0 : 1.0) : 2.0;
}

bool pairs_ok(int B, int N) { return B >= 1 && B <= 32767 && N >= 1 && N <= (1 << 24); }
bool positive_finite(double v) { return v > 0.0 && v <= 1.79769313486231570815e308; }

}  // namespace

extern "C" int cpn_refine_homography(const float* xy, const int* count, const float* intrinsics, const double* H0, int B, int N,
                                     int mode, int iters, double scale_px, double* H, float* pose, double* stats, void* stream) {
    CPN_REQUIRE(xy && count && intrinsics && H0 && H && pose && stats, CPN_E_ARG, "cpn_refine_homography: null pointer");
    CPN_REQUIRE(pairs_ok(B, N), CPN_E_SHAPE, "cpn_refine_homography: need 1 <= B <= 32767 pairs of 1 <= N <= 2^24 rows (got B %d, N %d)", B,
                N);
    CPN_REQUIRE((mode == 0 || mode == 1) && iters >= 0 && positive_finite(scale_px), CPN_E_ARG,
                "cpn_refine_homography: need mode 0 or 1, iters >= 0 and a finite scale_px > 0 (got %d, %d, %g)", mode, iters, scale_px);
    if (mode == 0)
        hipLaunchKernelGGL(refine_homography_kernel<9>, dim3(B), dim3(NT), 0, (hipStream_t)stream, xy, count, intrinsics, H0, N, iters,
                           scale_px, H, pose, stats);
    else
        hipLaunchKernelGGL(refine_homography_kernel<3>, dim3(B), dim3(NT), 0, (hipStream_t)stream, xy, count, intrinsics, H0, N, iters,
                           scale_px, H, pose, stats);
    CPN_LAUNCH_CHECK("cpn_refine_homography");
    return 0;
}

extern "C" int cpn_model_gric(const float* xy, const int* count, const float* intrinsics, const float* pose_e, const double* H_plane,
                              const double* H_rot, const uint8_t* avail, const double* ln4n, int B, int N, double sigma_px,
                              double* gric, uint8_t* label, double* stats, void* stream) {
    CPN_REQUIRE(xy && count && intrinsics && pose_e && H_plane && H_rot && avail && ln4n && gric && label && stats, CPN_E_ARG,
                "cpn_model_gric: null pointer");
    CPN_REQUIRE(pairs_ok(B, N), CPN_E_SHAPE, "cpn_model_gric: need 1 <= B <= 32767 pairs of 1 <= N <= 2^24 rows (got B %d, N %d)", B, N);
    CPN_REQUIRE(positive_finite(sigma_px), CPN_E_ARG, "cpn_model_gric: need a finite sigma_px > 0 (got %g)", sigma_px);
    hipLaunchKernelGGL(model_gric_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, xy, count, intrinsics, pose_e, H_plane, H_rot, avail,
                       ln4n, N, sigma_px, gric, label, stats);
    CPN_LAUNCH_CHECK("cpn_model_gric");
    return 0;
}
