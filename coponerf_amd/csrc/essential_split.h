// What ransac_finish_kernel does with the winner's E and ransac_polish_kernel with the E it polishes, once (ransac.hip, round 24):
// the split of an essential matrix into two rotations and +- t by the one-sided Jacobi method (jacobi_svd.h), the vote of one
// inlier on the four candidate poses, and the pick.  include/coponerf_hip.h (round 20) states the sequence, tests/ransac_ref.py
// restates it (split, depths, votes); float64, one rounding per operation, sums left to right as the parentheses say.
#pragma once
#include "jacobi_svd.h"
#include "sampson.h"

namespace {

struct EssentialSplit {
    double R[2][9], t[3];
};

// one thread: R1 = (u_2 v_1^T - u_1 v_2^T) + u_3 v_3^T, R2 = (u_1 v_2^T - u_2 v_1^T) + u_3 v_3^T, t = u_3 -> all of them finite
__device__ __forceinline__ bool split_essential(const double* E, EssentialSplit& sp) {
    double G[9], V[9], sg[3];
    for (int c = 0; c < 9; ++c) G[c] = E[c];
    jacobi_svd(G, V, sg);
    double U[3][3], W[3][3];                               // the frames' vectors by rows: U[k] = u_k, W[k] = v_k
    frame(G, 0, 1, U);
    frame(V, 0, 1, W);
    bool fin = true;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double r1 = (U[1][i] * W[0][j] - U[0][i] * W[1][j]) + U[2][i] * W[2][j];
            const double r2 = (U[0][i] * W[1][j] - U[1][i] * W[0][j]) + U[2][i] * W[2][j];
            sp.R[0][3 * i + j] = r1;
            sp.R[1][3 * i + j] = r2;
            fin = fin && finite64(r1) && finite64(r2);
        }
    for (int i = 0; i < 3; ++i) sp.t[i] = U[2][i];
    return fin;
}

// the votes of one inlier: candidate (R, +t) holds where both depths are positive, (R, -t) where both are negative
__device__ __forceinline__ void depth_votes(const EssentialSplit& sp, const Sampson& s, long long (&votes)[4]) {
    const double a[3] = {s.a0, s.a1, 1.0};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double* const R = sp.R[k];
        double c[3], ac[3], tc[3], ta[3];
        for (int j = 0; j < 3; ++j) c[j] = (R[3 * j] * s.b0 + R[3 * j + 1] * s.b1) + R[3 * j + 2];
        cross3(a, c, ac);
        cross3(sp.t, c, tc);
        cross3(sp.t, a, ta);
        const double z0 = (tc[0] * ac[0] + tc[1] * ac[1]) + tc[2] * ac[2];
        const double z1 = (ta[0] * ac[0] + ta[1] * ac[1]) + ta[2] * ac[2];
        votes[2 * k + 0] += (z0 > 0.0 && z1 > 0.0) ? 1 : 0;
        votes[2 * k + 1] += (z0 < 0.0 && z1 < 0.0) ? 1 : 0;
    }
}

// most votes, the lowest candidate of (R1, +t), (R1, -t), (R2, +t), (R2, -t) on ties
__device__ __forceinline__ int pick_candidate(const long long (&votes)[4]) {
    int pick = 0;
    for (int k = 1; k < 4; ++k)
        if (votes[k] > votes[pick]) pick = k;
    return pick;
}

}  // namespace
