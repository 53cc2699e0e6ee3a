// What refine_pose_kernel (matches.hip) and the finish kernels of ransac.hip and ransac_h.hip do with rel_pose and with the pose they found, once:
// is rel_pose usable, the pose as 16 floats, and its two angles to rel_pose.  float64, sums left to right as the parentheses say;
// tests/matches_ref.py and tests/ransac_ref.py restate it.
#pragma once
#include "pinhole.h"
#include "sampson.h"

#include <math.h>

namespace {

// rel_pose as a start and a yardstick: usable iff every entry is finite and the translation's length len0 is finite and not 0
struct RelStart {
    Pose rel;
    double len0;
    bool ok;
};
__device__ __forceinline__ RelStart rel_start(const float* P) {                 // P: the pair's 16 floats, or null: not usable
    RelStart s;
    s.len0 = 0.0;
    s.ok = false;
    if (P) {
        s.rel = load_pose(P);
        s.len0 = sqrt((s.rel.t[0] * s.rel.t[0] + s.rel.t[1] * s.rel.t[1]) + s.rel.t[2] * s.rel.t[2]);
        s.ok = pose_finite(s.rel) && s.len0 > 0.0 && finite64(s.len0);
    }
    return s;
}

// o = [R | scale t] in fp32 above the row 0 0 0 1; R row-major
__device__ __forceinline__ void store_pose(float* __restrict__ o, const double* R, const double* t, double scale) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o[4 * r + c] = (float)R[3 * r + c];
        o[4 * r + 3] = (float)(scale * t[r]);
        o[12 + r] = 0.0f;
    }
    o[15] = 1.0f;
}

// the angles in degrees from rel's rotation to R and from rel's direction rel.t / len0 to the unit t:
// |R - R0|_F = 2 sqrt(2) sin(angle / 2), |t - t0| = 2 sin(angle / 2): exact down to the smallest angles
__device__ __forceinline__ void pose_angles(const double* R, const double* t, const Pose& rel, double len0, double& deg_R,
                                            double& deg_t) {
    double dR = 0.0, dt = 0.0;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            const double e = R[3 * r + c] - rel.R[r][c];
            dR += e * e;
        }
        const double e = t[r] - rel.t[r] / len0;
        dt += e * e;
    }
    const double deg = 57.29577951308232;
    deg_R = 2.0 * asin(fmin(sqrt(dR) / 2.8284271247461903, 1.0)) * deg;
    deg_t = 2.0 * asin(fmin(sqrt(dt) / 2.0, 1.0)) * deg;
}

}  // namespace
