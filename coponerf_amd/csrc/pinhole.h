// The pinhole camera of point_cloud.hip, matches.hip, splat.hip, mesh.hip and raster.hip (and novel_views.hip's pose load), once.
// float64 from the fp32 inputs, one rounding per operation, sums left to right as the parentheses say: the numpy restatements
// (tests/*_ref.py) spell out the same order and the GPU tests compare bits.  Every body switches contraction off by pragma, so
// a unit built without -ffp-contract=off cannot fuse a product into a sum here.
#pragma once
#include "common.h"

#include <math.h>

namespace {

struct Cam {
    double fx, fy, cx, cy;
};
struct Pose {                                              // camera to reference: X = R p + t
    double R[3][3], t[3];
};

__device__ __forceinline__ Cam load_cam(const float* __restrict__ Kb) {        // a row-major 4 x 4 intrinsics matrix
    return Cam{(double)Kb[0], (double)Kb[5], (double)Kb[2], (double)Kb[6]};
}
__device__ __forceinline__ Pose load_pose(const float* __restrict__ P) {       // a row-major 4 x 4 rigid pose
    Pose o;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o.R[r][c] = (double)P[4 * r + c];
        o.t[r] = (double)P[4 * r + 3];
    }
    return o;
}
// splat and raster drop what a non-finite camera would draw; point_cloud and mesh let the NaN run into their own tests
__device__ __forceinline__ bool finite3(double a, double b, double c) { return isfinite(a) && isfinite(b) && isfinite(c); }
__device__ __forceinline__ bool cam_finite(const Cam& k) { return finite3(k.fx, k.fy, k.cx) && isfinite(k.cy); }
__device__ __forceinline__ bool pose_finite(const Pose& P) {
    bool ok = true;
    for (int r = 0; r < 3; ++r) ok = ok && finite3(P.R[r][0], P.R[r][1], P.R[r][2]) && isfinite(P.t[r]);
    return ok;
}
// a depth counts iff it is finite and strictly inside the clamp range of depth_ray: both clamp ends are saturated values
__device__ __forceinline__ bool depth_valid(float d) { return d > 0.0f && d < 10.0f; }

// the point of depth d on the ray of pixel (u, v), in the camera's frame
__device__ __forceinline__ void on_ray(const Cam& k, double u, double v, double d, double (&p)[3]) {
#pragma clang fp contract(off)
    p[0] = d * ((u - k.cx) / k.fx);
    p[1] = d * ((v - k.cy) / k.fy);
    p[2] = d;
}
__device__ __forceinline__ void to_reference(const Pose& P, const double (&p)[3], double (&X)[3]) {
#pragma clang fp contract(off)
    for (int r = 0; r < 3; ++r) X[r] = ((P.R[r][0] * p[0] + P.R[r][1] * p[1]) + P.R[r][2] * p[2]) + P.t[r];
}
// The inverse of a rigid pose, [R^T | -R^T t], in TWO forms that round differently and must not be exchanged: each is pinned
// bit for bit by its callers' restatements.  to_camera, R^T X + (-(R^T t)), is point_cloud.hip's; to_camera_centred,
// R^T (X - t), is splat.hip's, mesh.hip's and raster.hip's.  (One form for all would change results: a possible later issue.)
__device__ __forceinline__ void to_camera(const Pose& P, const double (&X)[3], double (&Y)[3]) {
#pragma clang fp contract(off)
    for (int r = 0; r < 3; ++r) {
        const double ti = -((P.R[0][r] * P.t[0] + P.R[1][r] * P.t[1]) + P.R[2][r] * P.t[2]);
        Y[r] = ((P.R[0][r] * X[0] + P.R[1][r] * X[1]) + P.R[2][r] * X[2]) + ti;
    }
}
__device__ __forceinline__ void to_camera_centred(const Pose& P, const double (&X)[3], double (&Y)[3]) {
#pragma clang fp contract(off)
    const double d[3] = {X[0] - P.t[0], X[1] - P.t[1], X[2] - P.t[2]};
    for (int j = 0; j < 3; ++j) Y[j] = (P.R[0][j] * d[0] + P.R[1][j] * d[1]) + P.R[2][j] * d[2];
}
__device__ __forceinline__ void project(const Cam& k, const double (&Y)[3], double& x, double& y) {
#pragma clang fp contract(off)
    x = (k.fx * Y[0]) / Y[2] + k.cx;
    y = (k.fy * Y[1]) / Y[2] + k.cy;
}

}  // namespace
