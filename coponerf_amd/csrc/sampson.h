// The essential matrix, the Sampson residual and the inlier rule of matches.hip, ransac.hip, ransac5.hip and ransac_h.hip, once:
// include/coponerf_hip.h (round 16) states the sequence, tests/matches_ref.py restates it.  float64 from the fp32 inputs, one
// rounding per operation, sums left to right as the parentheses say; the units that include this are built with
// -ffp-contract=off.  Cam is pinhole.h's.
#pragma once
#include "common.h"
#include "pinhole.h"

#include <math.h>

namespace {

// E = [t]x R, row-major (a Pose's R[3][3] is such a matrix)
__device__ __forceinline__ void essential(const double* R, const double* t, double* E) {
    for (int j = 0; j < 3; ++j) {
        E[0 + j] = t[1] * R[6 + j] - t[2] * R[3 + j];
        E[3 + j] = t[2] * R[0 + j] - t[0] * R[6 + j];
        E[6 + j] = t[0] * R[3 + j] - t[1] * R[0 + j];
    }
}

// The pieces of the Sampson residual of the pixel pair (x0, y0) of view 0 and (x1, y1) of view 1
struct Sampson {
    double a0, a1, b0, b1;          // the normalised points (third component 1)
    double g[4];                    // (E b)_0 / fx0, (E b)_1 / fy0, (E^T a)_0 / fx1, (E^T a)_1 / fy1
    double n, D;
};
// .. from the normalised points (ransac.hip's tiles hold them)
template <class Mat>
__device__ __forceinline__ Sampson sampson_normalised(const Mat& E, const Cam& k0, const Cam& k1, double a0, double a1, double b0,
                                                      double b1) {
    Sampson s;
    s.a0 = a0;
    s.a1 = a1;
    s.b0 = b0;
    s.b1 = b1;
    const double eb0 = (E[0] * s.b0 + E[1] * s.b1) + E[2];
    const double eb1 = (E[3] * s.b0 + E[4] * s.b1) + E[5];
    const double eb2 = (E[6] * s.b0 + E[7] * s.b1) + E[8];
    const double ea0 = (E[0] * s.a0 + E[3] * s.a1) + E[6];
    const double ea1 = (E[1] * s.a0 + E[4] * s.a1) + E[7];
    s.n = (s.a0 * eb0 + s.a1 * eb1) + eb2;
    s.g[0] = eb0 / k0.fx;
    s.g[1] = eb1 / k0.fy;
    s.g[2] = ea0 / k1.fx;
    s.g[3] = ea1 / k1.fy;
    s.D = ((s.g[0] * s.g[0] + s.g[1] * s.g[1]) + s.g[2] * s.g[2]) + s.g[3] * s.g[3];
    return s;
}
template <class Mat>
__device__ __forceinline__ Sampson sampson(const Mat& E, const Cam& k0, const Cam& k1, double x0, double y0, double x1, double y1) {
    return sampson_normalised(E, k0, k1, (x0 - k0.cx) / k0.fx, (y0 - k0.cy) / k0.fy, (x1 - k1.cx) / k1.fx, (y1 - k1.cy) / k1.fy);
}
__device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.79769313486231570815e308; }      // false for NaN
// the residual n / sqrt(D) counts iff D > 0 and n, D and the quotient are finite
__device__ __forceinline__ bool residual_ok(const Sampson& s, double r) {
    return s.D > 0.0 && finite64(s.D) && finite64(s.n) && finite64(r);
}
// .. and the match is an inlier iff it counts and lies within px pixels
__device__ __forceinline__ bool within(const Sampson& s, double px) {
    const double r = s.n / sqrt(s.D);
    return residual_ok(s, r) && fabs(r) <= px;
}
// .. and weighs, in round 24's fixed-point MSAC, 0 where it is no inlier and otherwise floor(2^20 (1 - r^2 / px^2)) held to
// [0, 2^20] (2^20 for px == 0; 0 where the quotient is not a number)
__device__ __forceinline__ int msac_weight(const Sampson& s, double px) {
    const double r = s.n / sqrt(s.D);
    if (!(residual_ok(s, r) && fabs(r) <= px)) return 0;
    if (!(px > 0.0)) return CPN_MSAC_ONE;
    const double v = floor((double)CPN_MSAC_ONE * (1.0 - (r * r) / (px * px)));
    return v >= (double)CPN_MSAC_ONE ? CPN_MSAC_ONE : (v > 0.0 ? (int)v : 0);
}

}  // namespace
