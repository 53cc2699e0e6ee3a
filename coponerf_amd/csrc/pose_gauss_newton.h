// The robust Gauss-Newton passes of the relative pose on the Sampson residuals of a pair's matches, once: refine_pose_kernel
// (matches.hip) runs them from rel_pose, ransac_polish_kernel (ransac.hip, round 24) from the pose an essential matrix splits into.
// ONE workgroup of 256 threads per state.  Per pass thread t walks the matches t, t + 256, .. in ascending order and keeps 30
// float64 sums (21 of H, 6 of g, the cost, the weights, the finite matches) in registers; the butterfly of wave_sum, then LDS and
// (w0 + w1) + (w2 + w3) in thread 0, which solves the damped 6 x 6 system by Cholesky, updates R and t and leaves E and the six
// dE_k in LDS for the next pass.  Two barriers a pass, no partials in HBM.  Pass `iters` only measures.
// float64, one rounding per operation (-ffp-contract=off), sums left to right: tests/matches_ref.py restates it (pass_sums, damped,
// solve6, apply_step).
#pragma once
#include "cholesky_solve.h"
#include "common.h"
#include "pinhole.h"
#include "rotation_step.h"
#include "sampson.h"

#include <math.h>

namespace {

constexpr int POSE_NSUM = 30;                              // H (21), g (6), cost, sum of weights, finite matches

// what thread 0 keeps for the pair between the passes, and what every thread reads in a pass
struct RefineState {
    double R[9], t[3];
    double E[9], dE[6][9];          // E = [t]x R; dE_k = [t]x [e_k]x R (k < 3), [e_(k-3)]x R (k >= 3)
    double red[POSE_NSUM][4];       // the four wave sums of a pass
    int go;                         // another pass follows
};

__device__ void set_matrices(RefineState& st) {
    essential(st.R, st.t, st.E);
    for (int k = 0; k < 3; ++k) {
        cross_rows(st.R, k, st.dE[3 + k]);
        essential(st.dE[3 + k], st.t, st.dE[k]);
    }
}

// The sums of a pass, 256 threads: the butterfly of wave_sum on each of the first V values of acc, lane 0 of wave w parks them in
// red[.][w]; behind the caller's barrier four_waves(red[k]) is sum k.  bundle.hip (round 27) reduces its sweeps with the same two.
template <int V, int NV>
__device__ __forceinline__ void park_wave_sums(double (&acc)[NV], double (*red)[4]) {
    static_assert(V <= NV, "more sums than values");
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < V; ++k) red[k][threadIdx.x >> 6] = acc[k];
    }
}
template <int NV>
__device__ __forceinline__ void park_wave_sums(double (&acc)[NV], double (*red)[4]) { park_wave_sums<NV, NV>(acc, red); }
__device__ __forceinline__ double four_waves(const double (&r)[4]) { return (r[0] + r[1]) + (r[2] + r[3]); }

// R <- exp([w]x) R (Rodrigues; the identity below 1e-12), t <- (t + dt) / |t + dt|; false (state untouched) where not finite
__device__ bool apply_step(RefineState& st, const double (&x)[6]) {
    double Rn[9], tn[3];
    rotate_left(x, st.R, Rn);
    for (int i = 0; i < 3; ++i) tn[i] = st.t[i] + x[3 + i];
    const double len = sqrt((tn[0] * tn[0] + tn[1] * tn[1]) + tn[2] * tn[2]);
    if (!(len > 0.0) || !finite64(len)) return false;
    for (int i = 0; i < 9; ++i)
        if (!finite64(Rn[i])) return false;
    for (int i = 0; i < 9; ++i) st.R[i] = Rn[i];
    for (int i = 0; i < 3; ++i) st.t[i] = tn[i] / len;
    return true;
}

// The passes from the state st - R, t and set_matrices' E and dE, written by thread 0 and behind a barrier - over the n rows of
// `rows`, every thread of the workgroup.  When they end - after pass `iters`, or at a failed solve, which keeps the state before
// it - thread 0 calls done(cost at the start, the last pass's 30 sums, updates made, status 0 / 1) and every thread returns.
template <class Done>
__device__ __forceinline__ void pose_passes(RefineState& st, const float* __restrict__ rows, int n, const Cam& k0, const Cam& k1,
                                            int iters, double scale_px, Done done_fn) {
    constexpr int NT = 256, NSUM = POSE_NSUM;
    const int tid = threadIdx.x;
    double cost0 = 0.0;
    int done = 0, status = 0;

    for (int pass = 0;; ++pass) {
        double acc[NSUM];
#pragma unroll
        for (int k = 0; k < NSUM; ++k) acc[k] = 0.0;
        for (int i = tid; i < n; i += NT) {
            const float* const m = rows + (size_t)i * 4;
            const Sampson s = sampson(st.E, k0, k1, (double)m[0], (double)m[1], (double)m[2], (double)m[3]);
            const double sd = sqrt(s.D), r = s.n / sd;
            if (!residual_ok(s, r)) continue;               // weight 0, not counted
            double J[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const double* const dE = st.dE[k];
                const double db0 = (dE[0] * s.b0 + dE[1] * s.b1) + dE[2];
                const double db1 = (dE[3] * s.b0 + dE[4] * s.b1) + dE[5];
                const double db2 = (dE[6] * s.b0 + dE[7] * s.b1) + dE[8];
                const double da0 = (dE[0] * s.a0 + dE[3] * s.a1) + dE[6];
                const double da1 = (dE[1] * s.a0 + dE[4] * s.a1) + dE[7];
                const double dn = (s.a0 * db0 + s.a1 * db1) + db2;
                const double dD = 2.0 * (((s.g[0] * (db0 / k0.fx) + s.g[1] * (db1 / k0.fy)) + s.g[2] * (da0 / k1.fx)) +
                                         s.g[3] * (da1 / k1.fy));
                J[k] = dn / sd - (s.n * dD) / ((2.0 * s.D) * sd);
            }
            const double z = r / scale_px, u = 1.0 + z * z, w = 1.0 / (u * u);
            int at = 0;
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const double wj = w * J[j];
#pragma unroll
                for (int k = j; k < 6; ++k) acc[at++] += wj * J[k];
                acc[21 + j] += wj * r;
            }
            acc[27] += ((r * r) / 2.0) / u;
            acc[28] += w;
            acc[29] += 1.0;
        }
        park_wave_sums(acc, st.red);
        __syncthreads();
        if (tid == 0) {
            double sum[NSUM];
            for (int k = 0; k < NSUM; ++k) sum[k] = four_waves(st.red[k]);
            if (pass == 0) cost0 = sum[27];
            bool more = pass < iters;
            if (more) {
                double A[6][6], g[6], y[6], x[6];
                int at = 0;
                for (int j = 0; j < 6; ++j) {
                    for (int k = j; k < 6; ++k) A[j][k] = A[k][j] = sum[at++];
                    g[j] = sum[21 + j];
                }
                double trace = 0.0;
                for (int j = 0; j < 6; ++j) trace += A[j][j];
                for (int j = 0; j < 6; ++j) A[j][j] = A[j][j] + 1e-3 * A[j][j];
                const double pin = trace / 6.0;            // the gauge: the residual cannot see the length of t
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) A[3 + i][3 + j] = A[3 + i][3 + j] + pin * (st.t[i] * st.t[j]);
                more = cholesky_solve<6>(A, g, y, x) && apply_step(st, x);
                if (more) {
                    set_matrices(st);
                    ++done;
                } else {
                    status = 1;                            // the pair keeps its state and stops
                }
            }
            st.go = more ? 1 : 0;
            if (!more) done_fn(cost0, sum, done, status);
        }
        __syncthreads();
        if (!st.go) return;
    }
}

}  // namespace
