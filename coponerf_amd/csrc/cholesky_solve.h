// The damped normal equations of the Gauss-Newton kernels, solved once: refine_pose_kernel (matches.hip) at 6 parameters out of
// registers, refine_homography_kernel (model_select.hip) at 9 and 3 out of LDS.  float64, one rounding per operation, every
// subtraction in the order written; tests/matches_ref.py (solve6) and tests/model_select_ref.py (solve) restate it.
#pragma once
#include "sampson.h"

#include <math.h>

namespace {

// x = -A^-1 g by Cholesky (A = L L^T, lower, L left in A; y the intermediate L y = -g); false where a pivot is not positive or a
// value not finite.  Mat is double[NP][NP], Vec double[NP], in whatever memory the caller keeps them.
template <int NP, class Mat, class Vec>
__device__ bool cholesky_solve(Mat& A, const Vec& g, Vec& y, Vec& x) {
    for (int j = 0; j < NP; ++j) {
        double s = A[j][j];
        for (int k = 0; k < j; ++k) s -= A[j][k] * A[j][k];
        if (!(s > 0.0) || !finite64(s)) return false;
        const double l = sqrt(s);
        A[j][j] = l;
        for (int i = j + 1; i < NP; ++i) {
            double v = A[i][j];
            for (int k = 0; k < j; ++k) v -= A[i][k] * A[j][k];
            A[i][j] = v / l;
        }
    }
    for (int i = 0; i < NP; ++i) {
        double v = -g[i];
        for (int k = 0; k < i; ++k) v -= A[i][k] * y[k];
        y[i] = v / A[i][i];
    }
    for (int i = NP - 1; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < NP; ++k) v -= A[k][i] * x[k];
        x[i] = v / A[i][i];
    }
    for (int i = 0; i < NP; ++i)
        if (!finite64(x[i])) return false;
    return true;
}

}  // namespace
