// The two OpenCV pieces of the reference's validation log (summary/summaries.py:img_summaries), drawn on the device: the
// epipolar panels of summary/inspect_epipolar_geometry.py (tags epipolar_GT / epipolar_pred) and the 1-pixel contour that
// overlay_semantic_mask puts around the masked region (summaries.py:65-71).  The reference draws them on the host with a
// .cpu().numpy() per image; here no render waits for a host read:
//
//   epipolar_lines_kernel    one thread per (kind, pair, point): two_view_geometry in float64 from the fp32 inputs as numpy forms
//                            it (F = inv(K0)^T [t]x R inv(K1), each inverse rounded to fp32 as np.linalg.inv returns it for an
//                            fp32 matrix; every thread of a pair forms the same F, point 0 stores it), the
//                            epiline F (x, y, 1), the end points of drawpointslines truncated toward zero, and a validity byte.
//   epipolar_panels_kernel   one thread per pixel of the (S, 2 S) panel of one kind and pair (32 x 8 tiles): the view scaled to
//                            [0, 255], the P integer disc tests on the left half, the P capsule tests on the right half - exact
//                            in int64 while the end points stay within 2^15, the same expressions in float64 beyond - and the
//                            0.4 / 0.6 blend on a line pixel.  The last point or line that covers a pixel gives its colour.
//   mask_contour_kernel      one thread per pixel: an invalid pixel with a valid or outside 4-neighbour takes the colour.
// Coverage is this library's definition (include/coponerf_hip.h); agreement with OpenCV's rasteriser on edge pixels has not
// been checked.  Compiled with -ffp-contract=off: every float64 operation of the line geometry is rounded once, in the order
// written.  No atomics: every result is bit-reproducible, and an image's panels do not depend on the batch around it.
#include "common.h"

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int PTW = 32, PTH = NT / PTW;                   // panels and contour: the tile of one workgroup
constexpr int EXACT_Y = 1 << 15, EXACT_S = 4096;          // within these every product of the capsule test fits an int64


// np.linalg.inv of a row-major 3 x 3 fp32 matrix: worked out in float64 (by cofactors: for a pinhole matrix, upper triangular,
// every cofactor is a single product) and returned ROUNDED TO fp32, as numpy returns the inverse of an fp32 array
__device__ __forceinline__ void inv3(const double m[9], double out[9]) {
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double det = (m[0] * c00 + m[1] * c01) + m[2] * c02;
    out[0] = c00 / det;
    out[1] = (m[2] * m[7] - m[1] * m[8]) / det;
    out[2] = (m[1] * m[5] - m[2] * m[4]) / det;
    out[3] = c01 / det;
    out[4] = (m[0] * m[8] - m[2] * m[6]) / det;
    out[5] = (m[2] * m[3] - m[0] * m[5]) / det;
    out[6] = c02 / det;
    out[7] = (m[1] * m[6] - m[0] * m[7]) / det;
    out[8] = (m[0] * m[4] - m[1] * m[3]) / det;
#pragma unroll
    for (int j = 0; j < 9; ++j) out[j] = (double)(float)out[j];
}

__device__ __forceinline__ void load3(const float* __restrict__ m44, double out[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) out[3 * i + j] = (double)m44[4 * i + j];
}

__device__ __forceinline__ bool fits_i32(double v) { return v > -2147483649.0 && v < 2147483648.0; }   // false for a NaN


__global__ __launch_bounds__(NT) void epipolar_lines_kernel(const float* __restrict__ intrinsics, const float* __restrict__ rel,
                                                            const float* __restrict__ gt_rel, const int* __restrict__ points, int B,
                                                            int P, int W, double* __restrict__ Fout, double* __restrict__ lines,
                                                            int* __restrict__ ends, uint8_t* __restrict__ valid) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= 2LL * B * P) return;
    const int p = (int)(i % P), kb = (int)(i / P), k = kb / B, b = kb - k * B;
    const float* const pose = (k ? gt_rel : rel) + (size_t)b * 16;

    double K0[9], K1[9], R[9], A[9], Bi[9];
    load3(intrinsics + ((size_t)b * 2 + 0) * 16, K0);
    load3(intrinsics + ((size_t)b * 2 + 1) * 16, K1);
    load3(pose, R);
    inv3(K0, A);
    inv3(K1, Bi);
    const double t0 = (double)pose[3], t1 = (double)pose[7], t2 = (double)pose[11];
    const double tx[9] = {0.0, -t2, t1, t2, 0.0, -t0, -t1, t0, 0.0};
    double E[9], M[9], F[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) E[3 * r + c] = (tx[3 * r] * R[c] + tx[3 * r + 1] * R[3 + c]) + tx[3 * r + 2] * R[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r)                            // inv(K0).T . E
#pragma unroll
        for (int c = 0; c < 3; ++c) M[3 * r + c] = (A[r] * E[c] + A[3 + r] * E[3 + c]) + A[6 + r] * E[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r)                            // . inv(K1)
#pragma unroll
        for (int c = 0; c < 3; ++c) F[3 * r + c] = (M[3 * r] * Bi[c] + M[3 * r + 1] * Bi[3 + c]) + M[3 * r + 2] * Bi[6 + c];
    if (p == 0) {
#pragma unroll
        for (int j = 0; j < 9; ++j) Fout[(size_t)kb * 9 + j] = F[j];
    }

    const double x = (double)points[2 * p], y = (double)points[2 * p + 1];
    const double la = (F[0] * x + F[1] * y) + F[2], lb = (F[3] * x + F[4] * y) + F[5], lc = (F[6] * x + F[7] * y) + F[8];
    lines[(size_t)i * 3 + 0] = la;
    lines[(size_t)i * 3 + 1] = lb;
    lines[(size_t)i * 3 + 2] = lc;
    const double y0 = -lc / lb, y1 = -(lc + la * (double)W) / lb;
    const bool ok = lb != 0.0 && isfinite(la) && isfinite(lb) && isfinite(lc) && isfinite(y0) && isfinite(y1) && fits_i32(y0) &&
                    fits_i32(y1);
    valid[i] = ok ? 1 : 0;
    ends[(size_t)i * 4 + 0] = 0;
    ends[(size_t)i * 4 + 1] = ok ? (int)y0 : 0;            // int(): truncation toward zero
    ends[(size_t)i * 4 + 2] = ok ? W : 0;
    ends[(size_t)i * 4 + 3] = ok ? (int)y1 : 0;
}


// the capsule of half-width T / 2 around the segment p0 p1, at pixel (x, y): the three tests of include/coponerf_hip.h
template <typename T>
__device__ __forceinline__ bool on_line(T x, T y, T x0, T y0, T x1, T y1, T TT) {
    const T dx = x1 - x0, dy = y1 - y0, wx = x - x0, wy = y - y0;
    const T LL = dx * dx + dy * dy, s = wx * dx + wy * dy;
    if (s <= 0) return 4 * (wx * wx + wy * wy) <= TT;
    if (s >= LL) {
        const T ex = x - x1, ey = y - y1;
        return 4 * (ex * ex + ey * ey) <= TT;
    }
    const T cr = wx * dy - wy * dx;
    return 4 * (cr * cr) <= TT * LL;
}


__global__ __launch_bounds__(NT) void epipolar_panels_kernel(const float* __restrict__ rgb, const int* __restrict__ points,
                                                             const float* __restrict__ colors, const int* __restrict__ ends,
                                                             const uint8_t* __restrict__ valid, int B, int S, int P, int rr, int TT,
                                                             float* __restrict__ out) {
    const int tid = threadIdx.x;
    const int gx = blockIdx.x * PTW + (tid & (PTW - 1)), gy = blockIdx.y * PTH + tid / PTW;
    if (gx >= 2 * S || gy >= S) return;
    const int item = blockIdx.z, k = item / B, b = item - k * B;
    const bool left = gx < S;
    const int x = left ? gx : gx - S;
    const float* const src = rgb + (((size_t)b * 2 + (left ? 1 : 0)) * S * S + (size_t)gy * S + x) * 3;

    int hit = -1;
    if (left) {
        for (int p = 0; p < P; ++p) {
            const long long ex = (long long)x - points[2 * p], ey = (long long)gy - points[2 * p + 1];
            if (ex * ex + ey * ey <= (long long)rr) hit = p;
        }
    } else {
        const int* const e = ends + (size_t)item * P * 4;
        const uint8_t* const ok = valid + (size_t)item * P;
        for (int p = 0; p < P; ++p) {
            if (!ok[p]) continue;
            const int x0 = e[4 * p], y0 = e[4 * p + 1], x1 = e[4 * p + 2], y1 = e[4 * p + 3];
            const bool exact = S <= EXACT_S && y0 >= -EXACT_Y && y0 <= EXACT_Y && y1 >= -EXACT_Y && y1 <= EXACT_Y;
            const bool on = exact ? on_line<long long>(x, gy, x0, y0, x1, y1, TT)
                                  : on_line<double>((double)x, (double)gy, (double)x0, (double)y0, (double)x1, (double)y1, (double)TT);
            if (on) hit = p;
        }
    }
    float* const dst = out + (((size_t)item * S + gy) * 2 * S + gx) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = (src[c] + 1.0f) * 127.5f;
        float o = v;
        if (hit >= 0) o = left ? colors[3 * hit + c] : 0.4f * colors[3 * hit + c] + 0.6f * v;
        dst[c] = o;
    }
}


__global__ __launch_bounds__(NT) void mask_contour_kernel(const uint8_t* __restrict__ overlay, const uint8_t* __restrict__ mask, int S,
                                                          uint8_t* __restrict__ out) {
    const int tid = threadIdx.x;
    const int gx = blockIdx.x * PTW + (tid & (PTW - 1)), gy = blockIdx.y * PTH + tid / PTW;
    if (gx >= S || gy >= S) return;
    const uint8_t* const m = mask + (size_t)blockIdx.z * S * S;
    const size_t px = (size_t)gy * S + gx;
    bool edge = false;
    if (m[px] == 0)
        edge = gx == 0 || gy == 0 || gx == S - 1 || gy == S - 1 || m[px - 1] != 0 || m[px + 1] != 0 || m[px - S] != 0 || m[px + S] != 0;
    const size_t at = ((size_t)blockIdx.z * S * S + px) * 3;
    const uint8_t colour[3] = {255, 102, 51};
#pragma unroll
    for (int c = 0; c < 3; ++c) out[at + c] = edge ? colour[c] : overlay[at + c];
}

}  // namespace

extern "C" int cpn_epipolar_lines(const float* intrinsics, const float* rel_pose, const float* gt_rel_pose, const int* points, int B,
                                  int P, int W, double* F, double* lines, int* ends, uint8_t* valid, void* stream) {
    CPN_REQUIRE(intrinsics && rel_pose && gt_rel_pose && points && F && lines && ends && valid, CPN_E_ARG,
                "cpn_epipolar_lines: null pointer");
    CPN_REQUIRE(B > 0 && P > 0 && W > 0 && 2LL * B * P <= (1LL << 30), CPN_E_SHAPE,
                "cpn_epipolar_lines: need B > 0, P > 0, W > 0 and 2 B P <= 2^30 (got B %d, P %d, W %d)", B, P, W);
    hipLaunchKernelGGL(epipolar_lines_kernel, dim3(cpn_cdiv(2LL * B * P, NT)), dim3(NT), 0, (hipStream_t)stream, intrinsics, rel_pose,
                       gt_rel_pose, points, B, P, W, F, lines, ends, valid);
    CPN_LAUNCH_CHECK("cpn_epipolar_lines");
    return 0;
}

extern "C" int cpn_epipolar_panels(const float* rgb, const int* points, const float* colors, const int* ends, const uint8_t* valid,
                                   int B, int S, int P, int radius, int thickness, float* out, void* stream) {
    CPN_REQUIRE(rgb && points && colors && ends && valid && out, CPN_E_ARG, "cpn_epipolar_panels: null pointer");
    CPN_REQUIRE(B > 0 && S > 0 && P > 0, CPN_E_SHAPE, "cpn_epipolar_panels: need B > 0, S > 0 and P > 0 (got B %d, S %d, P %d)", B, S,
                P);
    CPN_REQUIRE(2 * (long long)B <= 65535 && S <= 16384, CPN_E_SHAPE, "cpn_epipolar_panels: %d pairs of side %d are too many for one launch",
                B, S);
    CPN_REQUIRE(radius >= 0 && radius <= 255 && thickness >= 1 && thickness <= 255, CPN_E_ARG,
                "cpn_epipolar_panels: need 0 <= radius <= 255 and 1 <= thickness <= 255 (got %d, %d)", radius, thickness);
    const dim3 grid(cpn_cdiv(2 * S, PTW), cpn_cdiv(S, PTH), 2 * B);
    hipLaunchKernelGGL(epipolar_panels_kernel, grid, dim3(NT), 0, (hipStream_t)stream, rgb, points, colors, ends, valid, B, S, P,
                       radius * radius, thickness * thickness, out);
    CPN_LAUNCH_CHECK("cpn_epipolar_panels");
    return 0;
}

extern "C" int cpn_mask_contour(const uint8_t* overlay, const uint8_t* mask, int N, int S, uint8_t* out, void* stream) {
    CPN_REQUIRE(overlay && mask && out, CPN_E_ARG, "cpn_mask_contour: null pointer");
    CPN_REQUIRE(N > 0 && S > 0, CPN_E_SHAPE, "cpn_mask_contour: need N > 0 and S > 0 (got N %d, S %d)", N, S);
    CPN_REQUIRE(N <= 65535 && S <= 16384, CPN_E_SHAPE, "cpn_mask_contour: %d images of side %d are too many for one launch", N, S);
    CPN_REQUIRE(overlay != out, CPN_E_ARG, "cpn_mask_contour: out must not be the overlay");
    hipLaunchKernelGGL(mask_contour_kernel, dim3(cpn_cdiv(S, PTW), cpn_cdiv(S, PTH), N), dim3(NT), 0, (hipStream_t)stream, overlay, mask,
                       S, out);
    CPN_LAUNCH_CHECK("cpn_mask_contour");
    return 0;
}
