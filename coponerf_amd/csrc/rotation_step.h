// The rotation update of the Gauss-Newton kernels, once: refine_pose_kernel (matches.hip) and refine_homography_kernel
// (model_select.hip) take the generators [e_k]x R and the step R <- exp([w]x) R from here.  float64, sums left to right as the
// parentheses say; tests/matches_ref.py restates both (cross_rows, apply_step).  Matrices are row-major 9 doubles.
#pragma once

#include <math.h>

namespace {

// rows of [e_k]x R
__device__ __forceinline__ void cross_rows(const double* R, int k, double* M) {
    const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
    for (int j = 0; j < 3; ++j) {
        M[3 * k + j] = 0.0;
        M[3 * k1 + j] = -R[3 * k2 + j];
        M[3 * k2 + j] = R[3 * k1 + j];
    }
}

// Rn = exp([w]x) R by Rodrigues' formula (the identity below |w| = 1e-12)
__device__ __forceinline__ void rotate_left(const double* w, const double* R, double* Rn) {
    const double th = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    double Q[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (th >= 1e-12) {
        const double k0 = w[0] / th, k1 = w[1] / th, k2 = w[2] / th, s = sin(th), c = 1.0 - cos(th);
        const double K[9] = {0.0, -k2, k1, k2, 0.0, -k0, -k1, k0, 0.0};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double kk = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
                Q[3 * i + j] = (Q[3 * i + j] + s * K[3 * i + j]) + c * kk;
            }
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (Q[3 * i] * R[j] + Q[3 * i + 1] * R[3 + j]) + Q[3 * i + 2] * R[6 + j];
}

}  // namespace
