// The Sampson residual of a match under a homography a ~ H b and its derivative along a direction dH, once: both kernels of
// model_select.hip take it.  include/coponerf_hip.h (round 23) states the sequence, tests/model_select_ref.py restates it.
// float64 from the fp32 inputs, one rounding per operation, sums left to right as the parentheses say; the unit that includes
// this is built with -ffp-contract=off.  H is row-major 9 doubles; Cam is pinhole.h's, finite64 sampson.h's.
//
// The constraint C = (m0 - a0 m2, m1 - a1 m2) with m = H b has the 2 x 4 Jacobian J in the PIXELS (x0, y0, x1, y1); J01 = J10 = 0.
// S = J J^T = [[A, Bq], [Bq, Cq]] in the order
//   A = (J00 J00 + J02 J02) + J03 J03,  Bq = J02 J12 + J03 J13,  Cq = (J11 J11 + J12 J12) + J13 J13
// (the products with J01 and J10 are not formed).  S = L L^T, y = L^-1 C, e^2 = y0 y0 + y1 y1: to first order the squared distance
// in pixels from the match to the matches that satisfy H, the same kind of quantity as sampson.h's r^2 under E.
#pragma once
#include "pinhole.h"
#include "sampson.h"

#include <math.h>

namespace {

struct SampsonH {
    double a0, a1, b0, b1;          // the normalised points (third component 1)
    double C0, C1;
    double J00, J02, J03, J11, J12, J13;
    double l00, l10, l11;
    double y0, y1, e2;
    bool ok;                        // the residual counts
};

template <class Mat>
__device__ __forceinline__ SampsonH sampson_h(const Mat& H, const Cam& k0, const Cam& k1, double a0, double a1, double b0, double b1) {
    SampsonH s;
    s.a0 = a0;
    s.a1 = a1;
    s.b0 = b0;
    s.b1 = b1;
    const double m0 = (H[0] * b0 + H[1] * b1) + H[2];
    const double m1 = (H[3] * b0 + H[4] * b1) + H[5];
    const double m2 = (H[6] * b0 + H[7] * b1) + H[8];
    s.C0 = m0 - a0 * m2;
    s.C1 = m1 - a1 * m2;
    s.J00 = -m2 / k0.fx;
    s.J02 = (H[0] - a0 * H[6]) / k1.fx;
    s.J03 = (H[1] - a0 * H[7]) / k1.fy;
    s.J11 = -m2 / k0.fy;
    s.J12 = (H[3] - a1 * H[6]) / k1.fx;
    s.J13 = (H[4] - a1 * H[7]) / k1.fy;
    const double A = (s.J00 * s.J00 + s.J02 * s.J02) + s.J03 * s.J03;
    const double Bq = s.J02 * s.J12 + s.J03 * s.J13;
    const double Cq = (s.J11 * s.J11 + s.J12 * s.J12) + s.J13 * s.J13;
    s.l00 = sqrt(A);
    s.l10 = Bq / s.l00;
    const double d = Cq - s.l10 * s.l10;
    s.l11 = sqrt(d);
    s.y0 = s.C0 / s.l00;
    s.y1 = (s.C1 - s.l10 * s.y0) / s.l11;
    s.e2 = s.y0 * s.y0 + s.y1 * s.y1;
    // it counts iff A > 0, Cq - l10 l10 > 0 and every value above is finite (the six J are where A and Cq are)
    s.ok = A > 0.0 && d > 0.0 && finite64(m0) && finite64(m1) && finite64(m2) && finite64(s.C0) && finite64(s.C1) && finite64(A) &&
           finite64(Bq) && finite64(Cq) && finite64(s.l00) && finite64(s.l10) && finite64(s.l11) && finite64(s.y0) && finite64(s.y1) &&
           finite64(s.e2);
    return s;
}
// the match in pixels
template <class Mat>
__device__ __forceinline__ SampsonH sampson_h_px(const Mat& H, const Cam& k0, const Cam& k1, double x0, double y0, double x1, double y1) {
    return sampson_h(H, k0, k1, (x0 - k0.cx) / k0.fx, (y0 - k0.cy) / k0.fy, (x1 - k1.cx) / k1.fx, (y1 - k1.cy) / k1.fy);
}

// (dy0, dy1): the FULL derivative of y along dH (9 doubles, the change of H), the whitening L differentiated with it - the product
// rule through S = L L^T, as cpn_refine_pose differentiates n / sqrt(D).  Every J entry is linear in H, so dJ is J's expression on dH.
template <class Mat>
__device__ __forceinline__ void sampson_h_along(const SampsonH& s, const Mat& dH, const Cam& k0, const Cam& k1, double& dy0, double& dy1) {
    const double dm0 = (dH[0] * s.b0 + dH[1] * s.b1) + dH[2];
    const double dm1 = (dH[3] * s.b0 + dH[4] * s.b1) + dH[5];
    const double dm2 = (dH[6] * s.b0 + dH[7] * s.b1) + dH[8];
    const double dC0 = dm0 - s.a0 * dm2;
    const double dC1 = dm1 - s.a1 * dm2;
    const double dJ00 = -dm2 / k0.fx;
    const double dJ02 = (dH[0] - s.a0 * dH[6]) / k1.fx;
    const double dJ03 = (dH[1] - s.a0 * dH[7]) / k1.fy;
    const double dJ11 = -dm2 / k0.fy;
    const double dJ12 = (dH[3] - s.a1 * dH[6]) / k1.fx;
    const double dJ13 = (dH[4] - s.a1 * dH[7]) / k1.fy;
    const double dA = 2.0 * ((s.J00 * dJ00 + s.J02 * dJ02) + s.J03 * dJ03);
    const double dBq = ((dJ02 * s.J12 + s.J02 * dJ12) + dJ03 * s.J13) + s.J03 * dJ13;
    const double dCq = 2.0 * ((s.J11 * dJ11 + s.J12 * dJ12) + s.J13 * dJ13);
    const double dl00 = dA / (2.0 * s.l00);
    const double dl10 = (dBq - s.l10 * dl00) / s.l00;
    const double dl11 = (dCq - (2.0 * s.l10) * dl10) / (2.0 * s.l11);
    dy0 = (dC0 - s.y0 * dl00) / s.l00;
    dy1 = (((dC1 - dl10 * s.y0) - s.l10 * dy0) - s.y1 * dl11) / s.l11;
}

}  // namespace
