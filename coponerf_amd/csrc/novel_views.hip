// Two photos in, views in between out (coponerf_amd/novel_views.py): the three device pieces around the render path.
//
//   fit_rows_kernel / fit_cols_kernel   cpn_fit_images_u8: the loader's centre square crop (utils_training/data_util.py:116-121) of
//                             uint8 photos of ANY size, the resample to size x size the loader leaves to cv2.resize, and
//                             `v / 127.5 - 1` (realestate10k_dataio.py:353) on the fp32 resampled value.  Separable, the vertical
//                             pass first: a workgroup owns one output row and 256 consecutive BYTES of the cropped input row, so
//                             every tap is one coalesced line of the uint8 image; the row's weights are formed once per
//                             workgroup in LDS.  The horizontal pass reads the fp32 intermediate (size x side x 3 per image) and
//                             forms its weights per thread.  Tap geometry and weights in float64, rounded to fp32 once; products
//                             and sums in fp32, one rounding each (-ffp-contract=off), in tap order.
//   camera_path_kernel        cpn_camera_path: one thread per (pose, pair).  exp(t log R_rel) and t t_rel in float64 from the
//                             estimated rel_pose where it lies - on the device -, fp32 stores.
//   pack_frames_kernel        cpn_pack_frames: one thread per output byte of a frame: the render's fp32 rgb to uint8 and, beside
//                             it, the `jet` panel of depth_ray / 10 (jet.h's lookup rule), written into the output tensor.
#include "common.h"
#include "byte_pack.h"
#include "jet.h"
#include "pinhole.h"

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int MAX_TAPS = 1024;                             // per axis: inputs up to 500 x the output side

// The resample rule of one axis (ATen's antialiased bilinear kernel, upsample_bilinear2d_aa): output i of n_out reads the taps
// j in [lo, hi) of n_in with weights max(0, 1 - |j + 0.5 - c| / sup) over their sum, c = (i + 0.5) n_in / n_out and
// sup = max(n_in / n_out, 1).  antialias off: sup = 1, which is the half-pixel two-tap bilinear rule with clamped ends.
struct Taps {
    double c, sup;
    int lo, hi;
};

__device__ __forceinline__ Taps taps_of(int i, int n_in, int n_out, int antialias) {
    Taps t;
    const double scale = (double)n_in / (double)n_out;
    t.sup = (antialias && scale > 1.0) ? scale : 1.0;
    t.c = ((double)i + 0.5) * scale;
    const int lo = (int)(t.c - t.sup + 0.5), hi = (int)(t.c + t.sup + 0.5);       // truncation, as ATen's
    t.lo = lo > 0 ? lo : 0;
    t.hi = hi < n_in ? hi : n_in;
    return t;
}

__device__ __forceinline__ float tap_weight(const Taps& t, int j) {
    const double w = 1.0 - fabs((double)j + 0.5 - t.c) / t.sup;
    return (float)(w > 0.0 ? w : 0.0);
}

// vertical pass: tmp (N, size, side * 3) fp32 = the weighted mean over the rows of the crop
__global__ __launch_bounds__(NT) void fit_rows_kernel(const uint8_t* __restrict__ img, int Hi, int Wi, int y0, int x0, int side,
                                                      int size, int antialias, float* __restrict__ tmp) {
    __shared__ float w[MAX_TAPS];
    const int oy = blockIdx.y, n = blockIdx.z;
    const Taps t = taps_of(oy, side, size, antialias);
    const int nt = t.hi - t.lo;                            // <= MAX_TAPS: checked by the entry point
    for (int k = threadIdx.x; k < nt; k += NT) w[k] = tap_weight(t, t.lo + k);
    __syncthreads();
    const int xb = blockIdx.x * NT + threadIdx.x;          // byte of the cropped row
    if (xb >= side * 3) return;
    const size_t pitch = (size_t)Wi * 3;
    const uint8_t* p = img + ((size_t)n * Hi + (size_t)(y0 + t.lo)) * pitch + (size_t)x0 * 3 + xb;
    float acc = 0.f, ws = 0.f;
    for (int k = 0; k < nt; ++k, p += pitch) {
        acc += w[k] * (float)*p;
        ws += w[k];
    }
    tmp[((size_t)n * size + oy) * ((size_t)side * 3) + xb] = acc / ws;
}

// horizontal pass and the normalisation: out image n at out + (n % B) * batch_stride + (n / B) * view_stride, (size, size, 3)
__global__ __launch_bounds__(NT) void fit_cols_kernel(const float* __restrict__ tmp, int B, int side, int size, int antialias,
                                                      float* __restrict__ out, long long batch_stride, long long view_stride) {
    const int e = blockIdx.x * NT + threadIdx.x;           // element of the output row: ox * 3 + channel
    if (e >= size * 3) return;
    const int oy = blockIdx.y, n = blockIdx.z, ox = e / 3, ch = e - ox * 3;
    const Taps t = taps_of(ox, side, size, antialias);
    const float* const row = tmp + ((size_t)n * size + oy) * ((size_t)side * 3) + ch;
    float acc = 0.f, ws = 0.f;
    for (int j = t.lo; j < t.hi; ++j) {
        const float wj = tap_weight(t, j);
        acc += wj * row[(size_t)j * 3];
        ws += wj;
    }
    const float v = acc / ws;
    float* const o = out + (long long)(n % B) * batch_stride + (long long)(n / B) * view_stride;
    o[(size_t)oy * size * 3 + e] = v / 127.5f - 1.0f;
}


// pose k of pair b: the camera t_k of the way from view 0 (the identity) to view 1 (rel_pose), in view 0's frame
__global__ __launch_bounds__(NT) void camera_path_kernel(const float* __restrict__ rel_pose, const double* __restrict__ ts, int B,
                                                         int K, double sway, double turns, float* __restrict__ out) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= K * B) return;
    const int k = i / B, b = i - k * B;
    const Pose rel = load_pose(rel_pose + (size_t)b * 16);
    const double(&R)[3][3] = rel.R, (&tr)[3] = rel.t;
    const double t = ts[k];
    double Q[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    if (t == 1.0) {                                        // the end of the path is view 1's camera itself, not its projection
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Q[r][c] = R[r][c];
    } else if (t != 0.0) {
        const double a[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};      // 2 sin(theta) axis
        const double s = 0.5 * sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        const double cs = fmin(fmax(0.5 * (R[0][0] + R[1][1] + R[2][2] - 1.0), -1.0), 1.0);
        const double theta = atan2(s, cs);
        if (theta >= 1e-12) {
            double n[3];
            if (cs >= 0.0) {
                for (int r = 0; r < 3; ++r) n[r] = a[r] / (2.0 * s);
            } else {
                // beyond a quarter turn the antisymmetric part fades (it is 0 at pi): the axis comes from the symmetric part
                // (R + R^T) / 2 = cos I + (1 - cos) n n^T, its sign from what is left of the antisymmetric one
                double M[3][3];
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) M[r][c] = (0.5 * (R[r][c] + R[c][r]) - (r == c ? cs : 0.0)) / (1.0 - cs);
                const int m = (M[0][0] >= M[1][1] && M[0][0] >= M[2][2]) ? 0 : (M[1][1] >= M[2][2] ? 1 : 2);
                const double d = sqrt(M[m][m]);
                for (int r = 0; r < 3; ++r) n[r] = M[r][m] / d;
                const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
                const double sgn = (n[0] * a[0] + n[1] * a[1] + n[2] * a[2]) < 0.0 ? -1.0 : 1.0;
                for (int r = 0; r < 3; ++r) n[r] *= sgn / len;
            }
            const double ang = t * theta, sn = sin(ang), vc = 1.0 - cos(ang);
            const double N[3][3] = {{0.0, -n[2], n[1]}, {n[2], 0.0, -n[0]}, {-n[1], n[0], 0.0}};
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) {
                    double nn = 0.0;                       // (N N)[r][c] = n_r n_c - delta_rc
                    for (int q = 0; q < 3; ++q) nn += N[r][q] * N[q][c];
                    Q[r][c] += sn * N[r][c] + vc * nn;
                }
        }
    }
    double p[3] = {t * tr[0], t * tr[1], t * tr[2]};
    if (sway > 0.0) {                                      // test.py's make_circle, in the camera's own frame
        const double ph = 2.0 * M_PI * turns * t, ox = sway * cos(ph), oy = sway * sin(ph);
        for (int r = 0; r < 3; ++r) p[r] += Q[r][0] * ox + Q[r][1] * oy;
    }
    float* const o = out + (size_t)i * 16;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o[4 * r + c] = (float)Q[r][c];
        o[4 * r + 3] = (float)p[r];
    }
    o[12] = 0.f;
    o[13] = 0.f;
    o[14] = 0.f;
    o[15] = 1.f;
}


// out (B, h, wo, 3) bytes, wo = w or 2 w: [rgb | jet(depth / 10)]
__global__ __launch_bounds__(NT) void pack_frames_kernel(const float* __restrict__ rgb, const float* __restrict__ depth,
                                                         const float* __restrict__ table, long long total, int w, int wo,
                                                         uint8_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const long long px = i / 3, row = px / wo;             // row = b * h + y
    const int ch = (int)(i - px * 3), x = (int)(px - row * wo);
    if (x < w) {
        out[i] = to_byte((rgb[(row * w + x) * 3 + ch] + 1.0f) * 127.5f);
        return;
    }
    const int idx = jet_index(depth[row * w + (x - w)]);
    out[i] = to_byte(idx >= 0 ? table[3 * idx + ch] * 255.0f : 0.f);      // NaN: the colour map's `bad` entry
}

}  // namespace

extern "C" int cpn_fit_images_u8(const uint8_t* img, int N, int B, int Hi, int Wi, int size, int antialias, float* tmp, float* out,
                                 long long batch_stride, long long view_stride, void* stream) {
    CPN_REQUIRE(img && tmp && out, CPN_E_ARG, "cpn_fit_images_u8: null pointer");
    CPN_REQUIRE(N > 0 && B > 0 && N % B == 0 && N <= 65535, CPN_E_SHAPE,
                "cpn_fit_images_u8: need 0 < N <= 65535 images, a multiple of B > 0 (got N %d, B %d)", N, B);
    const int m = Hi < Wi ? Hi : Wi, side = (m / 2) * 2;
    CPN_REQUIRE(side >= 2 && size >= 1 && size <= 16384 && Hi <= (1 << 24) && Wi <= (1 << 24), CPN_E_SHAPE,
                "cpn_fit_images_u8: need images of at least 2 x 2 and 1 <= size <= 16384 (got %d x %d -> %d)", Hi, Wi, size);
    const double scale = (double)side / (double)size;
    CPN_REQUIRE(!antialias || 2.0 * scale + 2.0 <= (double)MAX_TAPS, CPN_E_SHAPE,
                "cpn_fit_images_u8: %d -> %d needs more than %d taps per axis", side, size, MAX_TAPS);
    CPN_REQUIRE(batch_stride >= 0 && view_stride >= 0, CPN_E_ARG, "cpn_fit_images_u8: negative output stride");
    const int y0 = Hi / 2 - m / 2, x0 = Wi / 2 - m / 2;    // utils_training/data_util.py:116-121
    hipLaunchKernelGGL(fit_rows_kernel, dim3(cpn_cdiv((long long)side * 3, NT), size, N), dim3(NT), 0, (hipStream_t)stream, img, Hi,
                       Wi, y0, x0, side, size, antialias ? 1 : 0, tmp);
    CPN_LAUNCH_CHECK("cpn_fit_images_u8 (rows)");
    hipLaunchKernelGGL(fit_cols_kernel, dim3(cpn_cdiv((long long)size * 3, NT), size, N), dim3(NT), 0, (hipStream_t)stream,
                       (const float*)tmp, B, side, size, antialias ? 1 : 0, out, batch_stride, view_stride);
    CPN_LAUNCH_CHECK("cpn_fit_images_u8 (columns)");
    return 0;
}

extern "C" int cpn_camera_path(const float* rel_pose, const double* t, int B, int K, double sway, double turns, float* out,
                               void* stream) {
    CPN_REQUIRE(rel_pose && t && out, CPN_E_ARG, "cpn_camera_path: null pointer");
    CPN_REQUIRE(B > 0 && K > 0 && (long long)B * K <= (1LL << 24), CPN_E_SHAPE,
                "cpn_camera_path: need B > 0, K > 0 and at most 2^24 poses (got B %d, K %d)", B, K);
    CPN_REQUIRE(sway >= 0.0, CPN_E_ARG, "cpn_camera_path: sway must be >= 0 (got %g)", sway);
    hipLaunchKernelGGL(camera_path_kernel, dim3(cpn_cdiv((long long)B * K, NT)), dim3(NT), 0, (hipStream_t)stream, rel_pose, t, B, K,
                       sway, turns, out);
    CPN_LAUNCH_CHECK("cpn_camera_path");
    return 0;
}

extern "C" int cpn_pack_frames(const float* rgb, const float* depth, const float* table, int B, int h, int w, uint8_t* out,
                               void* stream) {
    CPN_REQUIRE(rgb && out && ((depth != nullptr) == (table != nullptr)), CPN_E_ARG,
                "cpn_pack_frames: null pointer (depth and table are given together or not at all)");
    CPN_REQUIRE(B > 0 && h > 0 && w > 0 && w <= (1 << 20), CPN_E_SHAPE, "cpn_pack_frames: need B, h, w > 0 (got %d, %d, %d)", B, h, w);
    const int wo = depth ? 2 * w : w;
    const long long total = (long long)B * h * wo * 3;
    CPN_REQUIRE(total <= (1LL << 31) * NT - NT, CPN_E_SHAPE, "cpn_pack_frames: %lld bytes are too many for one launch", total);
    hipLaunchKernelGGL(pack_frames_kernel, dim3(cpn_cdiv(total, NT)), dim3(NT), 0, (hipStream_t)stream, rgb, depth, table, total, w, wo,
                       out);
    CPN_LAUNCH_CHECK("cpn_pack_frames");
    return 0;
}
