// The image metrics of the reference's evaluation script (test.py:227-229, 246-253, 267): per image MSE, PSNR and the SSIM of
// skimage.metrics.structural_similarity(win_size=11, gaussian_weights=True, channel_axis=-1, data_range=1) - an 11-tap
// sigma-1.5 separable gaussian with scipy's `reflect` boundary, no sample-covariance factor, the map cropped by 5 pixels on
// every side, the mean over the three channels.  The reference copies both images to the host and filters them on the CPU;
// as stock device ops the same arithmetic is a reflect pad, five depthwise convolutions and a dozen elementwise kernels per
// call.  Here it is 2 launches for any number of images, and nothing is read back.
//
//   image_metrics_kernel         one workgroup per 16 x 32 tile of one image.  The tile + a 5-pixel halo of both images -> LDS
//                                (all three channels), the prediction clamped to [-1, 1] with NaNs kept.  Both are stored
//                                CENTRED: x = p - 1/2 = clamp(pred) / 2, y = t - 1/2 = target / 2.  Variances do not move
//                                under a shift, the means shift back, and the squares that `E[x^2] - E[x]^2` subtracts are up
//                                to 4 x smaller - measured on the flat case in DESIGN.md 4.8.  Per channel: rows through the
//                                window (five moments -> LDS), then columns, then the quotient S of every pixel inside the
//                                crop.  The tile's squared error and its sum of S leave as one pair of floats.
//   image_metrics_finish_kernel  one wave per image: its tiles' pairs in a fixed order, in float64 -> mse, psnr, ssim.
// No atomics: two runs give the same bits, and an image's values do not depend on which other images share the launch.
//
// The tile geometry, the LDS layout (42.9 KB -> 3 workgroups per CU) and the two window passes are ssim_window.h's, the
// workgroup reduction common.h's, the float64 finish partial_sum.h's.  Register and scratch use are printed by
// -Rpass-analysis=kernel-resource-usage.
#include "partial_sum.h"
#include "ssim_window.h"

#include <math.h>

namespace {

// scipy's window: float64 weights, normalised in float64, rounded once (ssim_window.h: not the loss's fp32 window)
struct Window {
    float g[WIN];
};

// scipy.ndimage's `reflect` (d c b a | a b c d | d c b a).  One fold is enough for a 5-pixel halo of an image of 11 or more;
// positions further out belong to the unused part of a ragged tile and are only kept inside the image.  What it does for the
// RESULT is keep every load inside the image: skimage's crop drops all outputs within 5 pixels of a border, and an output
// inside the crop reads rows and columns g - 5 .. g + 5, none of them reflected.  The reflected halo of a border tile feeds
// only moments that the crop discards, so no test of the outputs can tell a wrong fold from a right one (the float64
// yardstick's own reflection is pinned against scipy's filter on the CPU instead).
__device__ __forceinline__ int reflect(int i, int n) {
    i = i < 0 ? -i - 1 : i;
    i = i >= n ? 2 * n - 1 - i : i;
    return i < 0 ? 0 : i;
}

// torch.clamp: a NaN stays a NaN (both comparisons are false)
__device__ __forceinline__ float clamp_unit(float v) { return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v); }


__global__ __launch_bounds__(NT) void image_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                           int H, int W, Window win, float* __restrict__ partial) {
    __shared__ float sx[3][RH * RW];
    __shared__ float sy[3][RH * RW];
    __shared__ float sh[5][RH * TW];
    const int tid = threadIdx.x;
    const int n = blockIdx.z;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const size_t img = (size_t)n * H * W * 3;
    const float* const pp = pred + img;
    const float* const tp = target + img;

    float se = 0.f;
    for (int idx = tid; idx < RH * RW; idx += NT) {
        const int ry = idx / RW, rx = idx - ry * RW;
        const int py = ty0 + ry - RAD, px = tx0 + rx - RAD;
        const size_t o = ((size_t)reflect(py, H) * W + reflect(px, W)) * 3;
        const bool own = ry >= RAD && ry < RAD + TH && rx >= RAD && rx < RAD + TW && py < H && px < W;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x = 0.5f * clamp_unit(pp[o + c]);
            const float y = 0.5f * tp[o + c];
            sx[c][idx] = x;
            sy[c][idx] = y;
            if (own) {
                const float d = x - y;                                     // = p - t
                se = __builtin_fmaf(d, d, se);
            }
        }
    }
    __syncthreads();

    float ss = 0.f;
    for (int c = 0; c < 3; ++c) {
        moment_rows(win.g, sx[c], sy[c], sh);
        __syncthreads();
        for (int p = tid; p < TH * TW; p += NT) {
            const int py = p / TW, px = p - py * TW;
            const int gy = ty0 + py, gx = tx0 + px;
            if (gy >= RAD && gy < H - RAD && gx >= RAD && gx < W - RAD) {          // skimage's crop
                float m[5];
                window_cols(win.g, sh, py, px, m);
                const float m1 = m[0], m2 = m[1], e11 = m[2], e22 = m[3], e12 = m[4];
                const float vx = e11 - m1 * m1, vy = e22 - m2 * m2, vxy = e12 - m1 * m2;
                const float ux = m1 + 0.5f, uy = m2 + 0.5f;                         // the means of p and t themselves
                const float a1 = 2.0f * ux * uy + SSIM_C1, a2 = 2.0f * vxy + SSIM_C2;
                const float b1 = ux * ux + uy * uy + SSIM_C1, b2 = vx + vy + SSIM_C2;
                ss += (a1 * a2) / (b1 * b2);
            }
        }
        __syncthreads();
    }
    float v[2] = {se, ss};
    block256_sum(v);
    if (tid == 0) {
        const size_t blk = ((size_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[2 * blk + 0] = v[0];
        partial[2 * blk + 1] = v[1];
    }
}

// one workgroup of 64 lanes per image: sum_partials_f64 over its tiles' pairs
__global__ __launch_bounds__(64) void image_metrics_finish_kernel(const float* __restrict__ partial, int nblk, int H, int W,
                                                                  float* __restrict__ out) {
    const int n = blockIdx.x, lane = threadIdx.x;
    double s[2];                                                          // squared error, sum of S
    sum_partials_f64<64>(partial + (size_t)n * nblk * 2, nblk, s);
    if (lane == 0) {
        const double mse = s[0] / (3.0 * (double)H * (double)W);
        out[3 * n + 0] = (float)mse;
        out[3 * n + 1] = (float)(-10.0 * log(mse) / log(10.0));           // mse = 0: +inf, as the reference's mse2psnr
        out[3 * n + 2] = (float)(s[1] / (3.0 * (double)(H - 2 * RAD) * (double)(W - 2 * RAD)));
    }
}

Window make_window() {
    Window w;
    double g[WIN], sum = 0.0;
    for (int k = 0; k < WIN; ++k) {
        const double x = (double)(k - RAD);
        g[k] = exp(-x * x / (2.0 * 1.5 * 1.5));
        sum += g[k];
    }
    for (int k = 0; k < WIN; ++k) w.g[k] = (float)(g[k] / sum);
    return w;
}

bool shape_ok(int N, int H, int W) {
    return N > 0 && N <= 65535 && H >= WIN && W >= WIN && H <= 32768 && W <= 32768 &&
           (long long)N * cpn_cdiv(H, TH) * cpn_cdiv(W, TW) * 2 < (1LL << 31);
}

}  // namespace

extern "C" int cpn_image_metrics_scratch(int N, int H, int W) {
    if (!shape_ok(N, H, W)) return 0;
    return (int)((long long)N * cpn_cdiv(H, TH) * cpn_cdiv(W, TW) * 2);
}

extern "C" int cpn_image_metrics(const float* pred, const float* target, int N, int H, int W, float* partial, float* out,
                                 void* stream) {
    CPN_REQUIRE(pred && target && partial && out, CPN_E_ARG, "cpn_image_metrics: null pointer");
    CPN_REQUIRE(N > 0 && H > 0 && W > 0, CPN_E_SHAPE, "cpn_image_metrics: need positive sizes");
    CPN_REQUIRE(H >= WIN && W >= WIN, CPN_E_SHAPE, "cpn_image_metrics: the %d-tap window needs H, W >= %d (got %d x %d)", WIN, WIN,
                H, W);
    CPN_REQUIRE(shape_ok(N, H, W), CPN_E_SHAPE, "cpn_image_metrics: %d images of %d x %d are too many for one launch", N, H, W);
    static const Window win = make_window();
    const dim3 grid(cpn_cdiv(W, TW), cpn_cdiv(H, TH), N);
    hipLaunchKernelGGL(image_metrics_kernel, grid, dim3(NT), 0, (hipStream_t)stream, pred, target, H, W, win, partial);
    CPN_LAUNCH_CHECK("cpn_image_metrics");
    hipLaunchKernelGGL(image_metrics_finish_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, partial, (int)(grid.x * grid.y), H,
                       W, out);
    CPN_LAUNCH_CHECK("cpn_image_metrics (finish)");
    return 0;
}
