// The homography a ~ H b of ransac_h.hip, its adjugate and the transfer-error inlier rule, once: include/coponerf_hip.h (round 22)
// states the sequence, tests/homography_ref.py restates it.  float64, one rounding per operation, sums left to right as the
// parentheses say; the unit that includes this is built with -ffp-contract=off.  H is row-major 9 doubles; Cam is pinhole.h's.
#pragma once
#include "pinhole.h"
#include "sampson.h"

#include <math.h>

namespace {

// g = adj(H) = det(H) H^-1: it maps a back to b up to scale
__device__ __forceinline__ void adjugate(const double (&h)[9], double (&g)[9]) {
    g[0] = h[4] * h[8] - h[5] * h[7];
    g[1] = h[2] * h[7] - h[1] * h[8];
    g[2] = h[1] * h[5] - h[2] * h[4];
    g[3] = h[5] * h[6] - h[3] * h[8];
    g[4] = h[0] * h[8] - h[2] * h[6];
    g[5] = h[2] * h[3] - h[0] * h[5];
    g[6] = h[3] * h[7] - h[4] * h[6];
    g[7] = h[1] * h[6] - h[0] * h[7];
    g[8] = h[0] * h[4] - h[1] * h[3];
}
// det H by its first row and the adjugate's first column
__device__ __forceinline__ double determinant(const double (&h)[9], const double (&g)[9]) {
    return (h[0] * g[0] + h[1] * g[3]) + h[2] * g[6];
}
// the third component of M (p0, p1, 1): the depth, up to a positive scale, at which M puts the point
__device__ __forceinline__ double third(const double (&M)[9], double p0, double p1) { return (M[6] * p0 + M[7] * p1) + M[8]; }

// is the point (p0, p1, 1) mapped by M in front of the camera and within px pixels of (q0, q1, 1) in the pixels of the camera
// (fx, fy)?  m = M p; m_2 > 0 and finite; d = sqrt((fx (m_0 / m_2 - q0))^2 + (fy (m_1 / m_2 - q1))^2) finite and <= px
__device__ __forceinline__ bool transfers(const double (&M)[9], double fx, double fy, double p0, double p1, double q0, double q1,
                                          double px) {
    const double m0 = (M[0] * p0 + M[1] * p1) + M[2];
    const double m1 = (M[3] * p0 + M[4] * p1) + M[5];
    const double m2 = (M[6] * p0 + M[7] * p1) + M[8];
    const double dx = fx * (m0 / m2 - q0), dy = fy * (m1 / m2 - q1);
    const double d = sqrt(dx * dx + dy * dy);
    return m2 > 0.0 && finite64(m2) && finite64(d) && d <= px;
}
// THE INLIER RULE: the match (a, b) transfers both ways, b to a by H in view 0's pixels and a to b by adj(H) in view 1's
__device__ __forceinline__ bool transfer_inlier(const double (&h)[9], const double (&g)[9], const Cam& k0, const Cam& k1, double a0,
                                                double a1, double b0, double b1, double px) {
    return transfers(h, k0.fx, k0.fy, b0, b1, a0, a1, px) && transfers(g, k1.fx, k1.fy, a0, a1, b0, b1, px);
}

}  // namespace
