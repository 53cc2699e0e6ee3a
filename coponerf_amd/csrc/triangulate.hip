// The matches as geometry (coponerf_amd/triangulate.py): round 26 of include/coponerf_hip.h, which states the operation order.
//
//   triangulate_kernel   cpn_triangulate_matches: one thread per (pair, row).  Lindstrom's optimal correction of the match in
//                        pixels, CPN_TRIANGULATE_PASSES passes of the iterated form that ends every pass exactly on the epipolar
//                        constraint (+ - x / sqrt only), then the one point of the two corrected, coplanar rays: the two cheirality
//                        numerators of essential_split.h over |a x R b|^2, with t as given.  The point, both depths, the
//                        reprojection error, the parallax, a flag byte and - with the photos - a colour.  No loop over rows, no
//                        runtime-indexed private array, nothing shared.
//   depth_scale_kernel   cpn_depth_scale: ONE workgroup of 256 threads per pair.  q = depth of view 0 at the nearest pixel over the
//                        triangulated z0 of the rows the keep rule takes; the exact lower median of q and of |q / median - 1| by
//                        radix_select.h's descent, the value recomputed in every pass: sixteen passes over the rows, no sort, no
//                        global atomics, nothing in HBM but the outputs.
//
// float64 from the fp32 inputs, one rounding per operation (-ffp-contract=off), sums left to right: tests/triangulate_ref.py
// restates both kernels in numpy.  Cam, Pose and depth_valid are pinhole.h's; essential, sampson and finite64 sampson.h's; the count
// clamp and finite32 ransac_common.h's.
#include "common.h"
#include "pinhole.h"
#include "radix_select.h"
#include "ransac_common.h"
#include "sampson.h"

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr double DEG = 57.29577951308232;

__device__ __forceinline__ float nan32() { return __builtin_nanf(""); }
__device__ __forceinline__ double nan64() { return __builtin_nan(""); }
__device__ __forceinline__ double dot3(const double (&u)[3], const double (&v)[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }
__device__ __forceinline__ void cross(const double (&u)[3], const double (&v)[3], double (&o)[3]) {
    o[0] = u[1] * v[2] - u[2] * v[1];
    o[1] = u[2] * v[0] - u[0] * v[2];
    o[2] = u[0] * v[1] - u[1] * v[0];
}

// the bilinear sample of channel ch of one S x S x 3 image at (x, y), the coordinate and the taps held to the image
__device__ __forceinline__ double bilinear(const float* __restrict__ img, int S, double x, double y, int ch) {
    const double top = (double)(S - 1);
    const double u = fmin(fmax(x, 0.0), top), v = fmin(fmax(y, 0.0), top);
    int ix = (int)floor(u), iy = (int)floor(v);
    ix = ix > S - 2 ? (S > 1 ? S - 2 : 0) : ix;
    iy = iy > S - 2 ? (S > 1 ? S - 2 : 0) : iy;
    const int jx = ix + 1 < S ? ix + 1 : S - 1, jy = iy + 1 < S ? iy + 1 : S - 1;
    const double lx = u - (double)ix, ly = v - (double)iy;
    const double p00 = (double)img[((size_t)iy * S + ix) * 3 + ch], p01 = (double)img[((size_t)iy * S + jx) * 3 + ch];
    const double p10 = (double)img[((size_t)jy * S + ix) * 3 + ch], p11 = (double)img[((size_t)jy * S + jx) * 3 + ch];
    return (1.0 - ly) * ((1.0 - lx) * p00 + lx * p01) + ly * ((1.0 - lx) * p10 + lx * p11);
}

__global__ __launch_bounds__(NT) void triangulate_kernel(const float* __restrict__ xy, const int* __restrict__ count,
                                                         const float* __restrict__ intrinsics, const float* __restrict__ poses,
                                                         const float* __restrict__ images, int N, int S, float* __restrict__ xyz,
                                                         float* __restrict__ geom, uint8_t* __restrict__ flag, float* __restrict__ rgb) {
    const int i = blockIdx.x * NT + threadIdx.x, b = blockIdx.y;
    if (i >= N) return;
    const size_t row = (size_t)b * N + i;
    const int n = clamp_count(count[b], N);
    const float* const m = xy + row * 4;
    const Pose pose = load_pose(poses + (size_t)b * 16);
    const Cam k0 = load_cam(intrinsics + ((size_t)b * 2 + 0) * 16), k1 = load_cam(intrinsics + ((size_t)b * 2 + 1) * 16);
    const bool pair_ok = pose_finite(pose) && !(pose.t[0] == 0.0 && pose.t[1] == 0.0 && pose.t[2] == 0.0) && cam_finite(k0) && cam_finite(k1);
    const bool inside = i < n;
    if (!inside || !pair_ok || !(finite32(m[0]) && finite32(m[1]) && finite32(m[2]) && finite32(m[3]))) {
        for (int c = 0; c < 3; ++c) xyz[row * 3 + c] = nan32();
        for (int c = 0; c < 4; ++c) geom[row * 4 + c] = nan32();
        if (rgb)
            for (int c = 0; c < 3; ++c) rgb[row * 3 + c] = nan32();
        flag[row] = inside ? (uint8_t)CPN_TRI_INPUT : (uint8_t)255;
        return;
    }
    const double x0 = (double)m[0], y0 = (double)m[1], x1 = (double)m[2], y1 = (double)m[3];

    // ---- the correction
    const double tl = sqrt((pose.t[0] * pose.t[0] + pose.t[1] * pose.t[1]) + pose.t[2] * pose.t[2]);
    const double th[3] = {pose.t[0] / tl, pose.t[1] / tl, pose.t[2] / tl};
    double E[9];
    essential(&pose.R[0][0], th, E);
    const Sampson s = sampson(E, k0, k1, x0, y0, x1, y1);
    const double c = s.n;
    const double F00 = (E[0] / k0.fx) / k1.fx, F01 = (E[1] / k0.fx) / k1.fy;
    const double F10 = (E[3] / k0.fy) / k1.fx, F11 = (E[4] / k0.fy) / k1.fy;
    const double p0 = s.g[0], p1 = s.g[1], q0 = s.g[2], q1 = s.g[3];       // n0 and n0'
    double n_0 = p0, n_1 = p1, m_0 = q0, m_1 = q1;                         // n and n'
    double D0 = 0.0, D1 = 0.0, G0 = 0.0, G1 = 0.0;                         // D and D'
    bool failed = false;
#pragma unroll
    for (int pass = 0; pass < CPN_TRIANGULATE_PASSES; ++pass) {
        const double A = n_0 * (F00 * m_0 + F01 * m_1) + n_1 * (F10 * m_0 + F11 * m_1);
        const double Bq = 0.5 * ((n_0 * p0 + n_1 * p1) + (m_0 * q0 + m_1 * q1));
        const double disc = Bq * Bq - A * c;
        const double d = sqrt(disc);
        const double den = Bq + d;
        const double lambda = c / den;
        failed = failed || !(disc >= 0.0) || !(den != 0.0);
        D0 = lambda * n_0;
        D1 = lambda * n_1;
        G0 = lambda * m_0;
        G1 = lambda * m_1;
        n_0 = p0 - (F00 * G0 + F01 * G1);
        n_1 = p1 - (F10 * G0 + F11 * G1);
        m_0 = q0 - (F00 * D0 + F10 * D1);
        m_1 = q1 - (F01 * D0 + F11 * D1);
    }
    const double xh0 = x0 - D0, yh0 = y0 - D1, xh1 = x1 - G0, yh1 = y1 - G1;

    // ---- the point
    const double ah[3] = {(xh0 - k0.cx) / k0.fx, (yh0 - k0.cy) / k0.fy, 1.0};
    const double bh0 = (xh1 - k1.cx) / k1.fx, bh1 = (yh1 - k1.cy) / k1.fy;
    double cr[3], w[3], tc[3], ta[3];
    for (int j = 0; j < 3; ++j) cr[j] = (pose.R[j][0] * bh0 + pose.R[j][1] * bh1) + pose.R[j][2];
    cross(ah, cr, w);
    cross(pose.t, cr, tc);
    cross(pose.t, ah, ta);
    const double ww = dot3(w, w);
    const double z0 = dot3(tc, w) / ww, z1 = dot3(ta, w) / ww;
    const double err = sqrt(((D0 * D0 + D1 * D1) + G0 * G0) + G1 * G1);
    const double par = atan2(sqrt(ww), dot3(ah, cr)) * DEG;
    xyz[row * 3 + 0] = (float)(z0 * ah[0]);
    xyz[row * 3 + 1] = (float)(z0 * ah[1]);
    xyz[row * 3 + 2] = (float)z0;
    geom[row * 4 + 0] = (float)z0;
    geom[row * 4 + 1] = (float)z1;
    geom[row * 4 + 2] = (float)err;
    geom[row * 4 + 3] = (float)par;
    flag[row] = (uint8_t)((failed ? CPN_TRI_CORRECTION : 0) | (!(ww > 0.0) ? CPN_TRI_PARALLAX : 0) | (!(z0 > 0.0) ? CPN_TRI_BEHIND0 : 0) |
                          (!(z1 > 0.0) ? CPN_TRI_BEHIND1 : 0));
    if (rgb) {
        const float* const im0 = images + ((size_t)b * 2 + 0) * S * S * 3;
        const float* const im1 = images + ((size_t)b * 2 + 1) * S * S * 3;
        for (int ch = 0; ch < 3; ++ch) rgb[row * 3 + ch] = (float)(0.5 * (bilinear(im0, S, x0, y0, ch) + bilinear(im1, S, x1, y1, ch)));
    }
}

struct ScaleShared {
    radix::Select<1> sel;
};

__global__ __launch_bounds__(NT) void depth_scale_kernel(const float* __restrict__ geom, const uint8_t* __restrict__ flag,
                                                         const float* __restrict__ xy, const int* __restrict__ count,
                                                         const float* __restrict__ depth, const float* __restrict__ rel_pose, int N, int S,
                                                         double max_reproj_px, double min_parallax_deg, int min_rows,
                                                         double* __restrict__ scale, double* __restrict__ stats) {
    __shared__ ScaleShared sh;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = clamp_count(count[b], N);
    const float* const g = geom + (size_t)b * N * 4;
    const uint8_t* const f = flag + (size_t)b * N;
    const float* const rows = xy + (size_t)b * N * 4;
    const float* const map = depth + (size_t)b * S * S;
    // q of row i, and whether the row is used
    const auto ratio = [&](int i, double& q) {
        if (f[i] != 0) return false;
        if (!((double)g[(size_t)i * 4 + 2] <= max_reproj_px && (double)g[(size_t)i * 4 + 3] >= min_parallax_deg)) return false;
        const double u = floor((double)rows[(size_t)i * 4 + 0] + 0.5), v = floor((double)rows[(size_t)i * 4 + 1] + 0.5);
        if (!(u >= 0.0 && u <= (double)(S - 1) && v >= 0.0 && v <= (double)(S - 1))) return false;
        const float d = map[(size_t)(int)v * S + (int)u];
        if (!depth_valid(d)) return false;
        q = (double)d / (double)g[(size_t)i * 4 + 0];
        return finite64(q) && q > 0.0;
    };
    const int n_u = radix::top_digits<NT>(sh.sel, n, ratio, [](double) {});
    if (n_u < min_rows) {                                  // every thread, the same integer
        if (tid == 0) {
            scale[b] = nan64();
            stats[b * 4 + 0] = (double)n_u;
            stats[b * 4 + 1] = stats[b * 4 + 2] = nan64();
            stats[b * 4 + 3] = 1.0;
        }
        return;
    }
    const long long middle = (long long)((n_u - 1) >> 1);
    radix::select<NT>(sh.sel, 1, n, ratio, [&](int) { return middle; });
    const double sc = radix::value_of(sh.sel.prefix[0]);

    // |q / scale - 1| of the same rows
    const auto spread = [&](int i, double& e) {
        double q;
        if (!ratio(i, q)) return false;
        e = fabs(q / sc - 1.0);
        return true;
    };
    radix::top_digits<NT>(sh.sel, n, spread, [](double) {});
    radix::select<NT>(sh.sel, 1, n, spread, [&](int) { return middle; });
    if (tid == 0) {
        double len = nan64();
        if (rel_pose) {
            const float* const P = rel_pose + (size_t)b * 16;
            const double t0 = (double)P[3], t1 = (double)P[7], t2 = (double)P[11];
            len = sqrt((t0 * t0 + t1 * t1) + t2 * t2);
        }
        scale[b] = sc;
        stats[b * 4 + 0] = (double)n_u;
        stats[b * 4 + 1] = radix::value_of(sh.sel.prefix[0]);
        stats[b * 4 + 2] = len / sc;
        stats[b * 4 + 3] = 0.0;
    }
}

}  // namespace

extern "C" int cpn_triangulate_matches(const float* xy, const int* count, const float* intrinsics, const float* pose, const float* images,
                                       int B, int N, int S, float* xyz, float* geom, uint8_t* flag, float* rgb, void* stream) {
    CPN_REQUIRE(xy && count && intrinsics && pose && xyz && geom && flag, CPN_E_ARG, "cpn_triangulate_matches: null pointer");
    CPN_REQUIRE((images != nullptr) == (rgb != nullptr), CPN_E_ARG, "cpn_triangulate_matches: images and rgb go together");
    CPN_REQUIRE(B >= 1 && B <= 32767 && N >= 1 && N <= (1 << 24) && (!images || (S >= 1 && S <= 16384)), CPN_E_SHAPE,
                "cpn_triangulate_matches: need 1 <= B <= 32767, 1 <= N <= 2^24 and, with images, 1 <= S <= 16384 (got B %d, N %d, S %d)",
                B, N, S);
    hipLaunchKernelGGL(triangulate_kernel, dim3(cpn_cdiv(N, NT), B), dim3(NT), 0, (hipStream_t)stream, xy, count, intrinsics, pose, images,
                       N, S, xyz, geom, flag, rgb);
    CPN_LAUNCH_CHECK("cpn_triangulate_matches");
    return 0;
}

extern "C" int cpn_depth_scale(const float* geom, const uint8_t* flag, const float* xy, const int* count, const float* depth,
                               const float* rel_pose, int B, int N, int S, double max_reproj_px, double min_parallax_deg, int min_rows,
                               double* scale, double* stats, void* stream) {
    CPN_REQUIRE(geom && flag && xy && count && depth && scale && stats, CPN_E_ARG, "cpn_depth_scale: null pointer");
    CPN_REQUIRE(B >= 1 && B <= 32767 && N >= 1 && N <= (1 << 24) && S >= 1 && S <= 16384, CPN_E_SHAPE,
                "cpn_depth_scale: need 1 <= B <= 32767, 1 <= N <= 2^24 and 1 <= S <= 16384 (got B %d, N %d, S %d)", B, N, S);
    CPN_REQUIRE(px_ok(max_reproj_px) && px_ok(min_parallax_deg) && min_rows >= 1, CPN_E_ARG,
                "cpn_depth_scale: need finite max_reproj_px and min_parallax_deg >= 0 and min_rows >= 1 (got %g, %g, %d)", max_reproj_px,
                min_parallax_deg, min_rows);
    hipLaunchKernelGGL(depth_scale_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, geom, flag, xy, count, depth, rel_pose, N, S,
                       max_reproj_px, min_parallax_deg, min_rows, scale, stats);
    CPN_LAUNCH_CHECK("cpn_depth_scale");
    return 0;
}
