// The flow-warp SSIM term of the training loss (the reference's models/loss_function.py:19-60, 109-120 with
// utils_training/utils.py:642-671 `warp`): per direction of a stereo pair, the other view warped by the upsampled flow,
// compared with this view by a masked 11 x 11 sigma-1.5 SSIM.  As stock ops that is ~170 launches per step for both
// directions, backward included; here it is 2 + 2.
//
// An ITEM is one direction of one pair: item k = 2 b + d reads source view 1 - d and target view d of rgb (B, 2, H, W, 3) as it
// is stored (channels last), flow_d[b] (2, h, w) and mask[k] (H, W).  The loss of direction d is normalised over the whole
// batch as upstream does it: sum_b num / sum_b den / 3.
//
//   ssim_warp_fwd_kernel   one workgroup per 16 x 32 tile of an item.  Over the tile + a 5-pixel halo: upsampled flow (ATen's
//                          align_corners=False rule), sampling coordinate (the fp32 expression sequence of `warp` followed by
//                          ATen's unnormalisation - the unit is compiled with -ffp-contract=off; the window sums ask for their
//                          FMAs by name), four zero-padded bilinear taps -> LDS.  A halo position outside the image holds 0 for
//                          every moment, as conv2d(padding=5) pads the WARPED image.  Per channel the five moments go through the
//                          window separably (rows, then columns, both in LDS), then the SSIM quotient, the three mask-weighted
//                          derivative maps (d(1 - ssim)/d mu1, /d E[x^2], /d E[xy]) and the block's partial (num, den).
//   ssim_warp_finish_kernel  per direction: the partials of its items in a fixed order (float64) -> loss, 1 / (3 den).
//   ssim_warp_bwd_kernel   the same tiles: the window (its own adjoint) over the three maps, dL/dwarped = G*A + 2 x G*B + y G*C,
//                          the bilinear spatial gradient at the stored coordinates, the factors W/(W-1), H/(H-1), s, the upstream
//                          gradient and 1 / (3 den) (device scalars) -> per-pixel gradient of the upsampled flow.
//   ssim_upsample_adjoint_kernel  one thread per low-resolution cell: gathers its footprint (border clamping included).
// No atomics anywhere: loss and dflow are bit-reproducible.
//
// The tile geometry, the forward's LDS layout and the window passes (the forward's rows, both column passes) are
// ssim_window.h's, the workgroup reduction common.h's, the float64 finish partial_sum.h's.  The forward runs 3 waves per SIMD
// without scratch (-Rpass-analysis=kernel-resource-usage); the 42 x 42 x 15 form of all channels at once (106 KB) would
// hold one workgroup.  The backward: 23.1 KB, 4 waves per SIMD.  At 4 pairs of 256 x 256 the four launches take
// 53 + 5 + 24 + 10 us of a 89 ms step: what they replace cost 3 ms as ~180 launches, mostly on the host.
#include "flow_warp.h"
#include "partial_sum.h"
#include "ssim_window.h"

namespace {

__global__ __launch_bounds__(NT) void ssim_warp_fwd_kernel(const float* __restrict__ rgb, const float* __restrict__ flow0,
                                                           const float* __restrict__ flow1, const uint8_t* __restrict__ mask,
                                                           const float* __restrict__ window, int H, int W, int h, int w, int s,
                                                           float* __restrict__ coords, float* __restrict__ maps,
                                                           float* __restrict__ partial) {
    __shared__ float sx[3][RH * RW];
    __shared__ float sy[3][RH * RW];
    __shared__ float sh[5][RH * TW];
    __shared__ float swin[WIN];
    const int tid = threadIdx.x;
    const int item = blockIdx.z, b = item >> 1, d = item & 1;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const size_t HW = (size_t)H * W;
    const float* const src = rgb + ((size_t)b * 2 + (1 - d)) * HW * 3;
    const float* const tgt = rgb + ((size_t)b * 2 + d) * HW * 3;
    const float* const fl = (d ? flow1 : flow0) + (size_t)b * 2 * h * w;
    const float fs = (float)s, rs = 1.0f / (float)s;
    if (tid < WIN) swin[tid] = window[tid];

    for (int idx = tid; idx < RH * RW; idx += NT) {
        const int ry = idx / RW, rx = idx - ry * RW;
        const int gy = ty0 + ry - RAD, gx = tx0 + rx - RAD;
        float xv[3] = {0.f, 0.f, 0.f}, yv[3] = {0.f, 0.f, 0.f};
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            float ix, iy;
            sample_coord(fl, h, w, H, W, fs, rs, gx, gy, ix, iy);
            const WarpTaps t = warp_taps(ix, iy, H, W);
            const float w00 = t.wx0 * t.wy0, w01 = t.wx1 * t.wy0, w10 = t.wx0 * t.wy1, w11 = t.wx1 * t.wy1;
            const float* const p00 = src + ((size_t)t.y0 * W + t.x0) * 3;
            const float* const p01 = src + ((size_t)t.y0 * W + t.x1) * 3;
            const float* const p10 = src + ((size_t)t.y1 * W + t.x0) * 3;
            const float* const p11 = src + ((size_t)t.y1 * W + t.x1) * 3;
            const float* const pt = tgt + ((size_t)gy * W + gx) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v = 0.f;
                if (t.vy0 && t.vx0) v += p00[c] * w00;
                if (t.vy0 && t.vx1) v += p01[c] * w01;
                if (t.vy1 && t.vx0) v += p10[c] * w10;
                if (t.vy1 && t.vx1) v += p11[c] * w11;
                xv[c] = v;
                yv[c] = pt[c];
            }
            if (ry >= RAD && ry < RAD + TH && rx >= RAD && rx < RAD + TW) {
                coords[((size_t)item * 2 + 0) * HW + (size_t)gy * W + gx] = ix;
                coords[((size_t)item * 2 + 1) * HW + (size_t)gy * W + gx] = iy;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            sx[c][idx] = xv[c];
            sy[c][idx] = yv[c];
        }
    }
    __syncthreads();

    float num = 0.f, den = 0.f;
    for (int c = 0; c < 3; ++c) {
        moment_rows(swin, sx[c], sy[c], sh);
        __syncthreads();
        for (int p = tid; p < TH * TW; p += NT) {
            const int py = p / TW, px = p - py * TW;
            const int gy = ty0 + py, gx = tx0 + px;
            if (gy < H && gx < W) {
                float m[5];
                window_cols(swin, sh, py, px, m);
                const float mu1 = m[0], mu2 = m[1], e11 = m[2], e22 = m[3], e12 = m[4];
                const float mu1mu2 = mu1 * mu2, mu1sq = mu1 * mu1, mu2sq = mu2 * mu2;
                const float s1 = e11 - mu1sq, s2 = e22 - mu2sq, s12 = e12 - mu1mu2;
                const float a1 = 2.0f * mu1mu2 + SSIM_C1, a2 = 2.0f * s12 + SSIM_C2;
                const float b1 = mu1sq + mu2sq + SSIM_C1, b2 = s1 + s2 + SSIM_C2;
                const float rb = 1.0f / (b1 * b2);
                const float ssim = (a1 * a2) / (b1 * b2);
                const float mk = mask[(size_t)item * HW + (size_t)gy * W + gx] ? 1.0f : 0.0f;
                // d ssim / d mu1 (E[x^2], E[xy] held), / d E[x^2], / d E[xy]
                const float dmu = 2.0f * mu2 * (a2 - a1) * rb - 2.0f * mu1 * ssim * (1.0f / b1 - 1.0f / b2);
                const float de11 = -ssim / b2;
                const float de12 = 2.0f * a1 * rb;
                float* const mp = maps + ((size_t)item * 9 + c * 3) * HW + (size_t)gy * W + gx;
                mp[0] = -mk * dmu;
                mp[HW] = -mk * de11;
                mp[2 * HW] = -mk * de12;
                num += (1.0f - ssim) * mk;
                if (c == 0) den += mk;
            }
        }
        __syncthreads();
    }
    float v[2] = {num, den};
    block256_sum(v);
    if (tid == 0) {
        const size_t blk = ((size_t)item * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[2 * blk + 0] = v[0];
        partial[2 * blk + 1] = v[1];
    }
}

// one workgroup of 64 lanes per direction: sum_partials_f64 over the blocks of each pair's item, the pairs added in order
__global__ __launch_bounds__(64) void ssim_warp_finish_kernel(const float* __restrict__ partial, int B, int nblk,
                                                              float* __restrict__ sums, float* __restrict__ loss,
                                                              float* __restrict__ inv3den) {
    const int d = blockIdx.x, lane = threadIdx.x;
    double tn = 0.0, td = 0.0;
    for (int b = 0; b < B; ++b) {
        double s[2];                                                      // num, den of item 2 b + d
        sum_partials_f64<64>(partial + (size_t)(2 * b + d) * nblk * 2, nblk, s);
        if (lane == 0) {
            sums[(2 * b + d) * 2 + 0] = (float)s[0];
            sums[(2 * b + d) * 2 + 1] = (float)s[1];
        }
        tn += s[0];
        td += s[1];
    }
    if (lane == 0) {
        const float fn = (float)tn, fd = (float)td;
        loss[d] = fn / fd / 3.0f;                 // 0 / 0 = NaN on an empty mask, as upstream
        inv3den[d] = 1.0f / (3.0f * fd);
    }
}

__global__ __launch_bounds__(NT) void ssim_warp_bwd_kernel(const float* __restrict__ rgb, const float* __restrict__ coords,
                                                           const float* __restrict__ maps, const float* __restrict__ window,
                                                           const float* __restrict__ gout, const float* __restrict__ inv3den,
                                                           int H, int W, int s, float* __restrict__ gup) {
    __shared__ float sm[3][RH * RW];
    __shared__ float sh[3][RH * TW];
    __shared__ float swin[WIN];
    const int tid = threadIdx.x;
    const int item = blockIdx.z, b = item >> 1, d = item & 1;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const size_t HW = (size_t)H * W;
    const float* const src = rgb + ((size_t)b * 2 + (1 - d)) * HW * 3;
    const float* const tgt = rgb + ((size_t)b * 2 + d) * HW * 3;
    if (tid < WIN) swin[tid] = window[tid];
    constexpr int PER = TH * TW / NT;
    float gix[PER], giy[PER];
    WarpTaps tp[PER];
    bool in[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int p = tid + j * NT, py = p / TW, px = p - py * TW;
        const int gy = ty0 + py, gx = tx0 + px;
        in[j] = gy < H && gx < W;
        gix[j] = giy[j] = 0.f;
        float ix = 0.f, iy = 0.f;
        if (in[j]) {
            ix = coords[((size_t)item * 2 + 0) * HW + (size_t)gy * W + gx];
            iy = coords[((size_t)item * 2 + 1) * HW + (size_t)gy * W + gx];
        }
        tp[j] = warp_taps(ix, iy, H, W);
    }
    for (int c = 0; c < 3; ++c) {
        for (int idx = tid; idx < RH * RW; idx += NT) {
            const int ry = idx / RW, rx = idx - ry * RW;
            const int gy = ty0 + ry - RAD, gx = tx0 + rx - RAD;
            const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
            const float* const mp = maps + ((size_t)item * 9 + c * 3) * HW + (size_t)(ok ? gy : 0) * W + (ok ? gx : 0);
            sm[0][idx] = ok ? mp[0] : 0.f;
            sm[1][idx] = ok ? mp[HW] : 0.f;
            sm[2][idx] = ok ? mp[2 * HW] : 0.f;
        }
        __syncthreads();
        for (int idx = tid; idx < RH * TW; idx += NT) {
            const int r = idx / TW, col = idx - r * TW;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const float g = swin[k];
                a0 = __builtin_fmaf(g, sm[0][r * RW + col + k], a0);
                a1 = __builtin_fmaf(g, sm[1][r * RW + col + k], a1);
                a2 = __builtin_fmaf(g, sm[2][r * RW + col + k], a2);
            }
            sh[0][idx] = a0;
            sh[1][idx] = a1;
            sh[2][idx] = a2;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (!in[j]) continue;
            const int p = tid + j * NT, py = p / TW, px = p - py * TW;
            const int gy = ty0 + py, gx = tx0 + px;
            float gm[3];                                                   // G * A, G * B, G * C
            window_cols(swin, sh, py, px, gm);
            const float ga = gm[0], gb = gm[1], gc = gm[2];
            const WarpTaps& t = tp[j];
            const float v00 = (t.vy0 && t.vx0) ? src[((size_t)t.y0 * W + t.x0) * 3 + c] : 0.f;
            const float v01 = (t.vy0 && t.vx1) ? src[((size_t)t.y0 * W + t.x1) * 3 + c] : 0.f;
            const float v10 = (t.vy1 && t.vx0) ? src[((size_t)t.y1 * W + t.x0) * 3 + c] : 0.f;
            const float v11 = (t.vy1 && t.vx1) ? src[((size_t)t.y1 * W + t.x1) * 3 + c] : 0.f;
            float x = 0.f;
            x += v00 * (t.wx0 * t.wy0);
            x += v01 * (t.wx1 * t.wy0);
            x += v10 * (t.wx0 * t.wy1);
            x += v11 * (t.wx1 * t.wy1);
            const float y = tgt[((size_t)gy * W + gx) * 3 + c];
            const float gw = ga + 2.0f * x * gb + y * gc;                  // dL / d warped[c]
            // grid_sample's backward: an out-of-range tap has no value, the in-range ones keep their weight derivative
            gix[j] += gw * ((v01 - v00) * t.wy0 + (v11 - v10) * t.wy1);
            giy[j] += gw * ((v10 - v00) * t.wx0 + (v11 - v01) * t.wx1);
        }
        __syncthreads();
    }
    // d ix / d up_x = (W / 2) (2 / max(W - 1, 1)), up = s * bilinear(flow): s joins here, the interpolation weights in the gather
    const float scale = gout[d] * inv3den[d] * (float)s;
    const float kx = (float)W / (float)(W - 1 > 1 ? W - 1 : 1), ky = (float)H / (float)(H - 1 > 1 ? H - 1 : 1);
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        if (!in[j]) continue;
        const int p = tid + j * NT, py = p / TW, px = p - py * TW;
        const size_t o = (size_t)(ty0 + py) * W + (tx0 + px);
        gup[((size_t)item * 2 + 0) * HW + o] = gix[j] * kx * scale;
        gup[((size_t)item * 2 + 1) * HW + o] = giy[j] * ky * scale;
    }
}

// out (planes, h, w) from g (planes, H, W): cell (j, i) gathers every pixel whose lower or upper tap it is
__global__ __launch_bounds__(NT) void ssim_upsample_adjoint_kernel(const float* __restrict__ g, int planes, int h, int w, int H,
                                                                   int W, int s, float* __restrict__ out) {
    const long long n = (long long)planes * h * w;
    const long long t = (long long)blockIdx.x * NT + threadIdx.x;
    if (t >= n) return;
    const int i = (int)(t % w), j = (int)((t / w) % h);
    const long long pl = t / ((long long)w * h);
    const float rs = 1.0f / (float)s;
    const int half = s / 2;
    int y_lo = s * (j - 1) + half, y_hi = s * (j + 1) + half;            // [lo, hi)
    int x_lo = s * (i - 1) + half, x_hi = s * (i + 1) + half;
    if (j == 0) y_lo = 0;
    if (i == 0) x_lo = 0;
    if (j == h - 1) y_hi = H;
    if (i == w - 1) x_hi = W;
    y_lo = y_lo < 0 ? 0 : y_lo;
    x_lo = x_lo < 0 ? 0 : x_lo;
    y_hi = y_hi > H ? H : y_hi;
    x_hi = x_hi > W ? W : x_hi;
    const float* const gp = g + (size_t)pl * H * W;
    float acc = 0.f;
    for (int y = y_lo; y < y_hi; ++y) {
        int ya, yb;
        float ly0, ly1;
        up_index(y, rs, h, ya, yb, ly0, ly1);
        const float wy = (ya == j ? ly0 : 0.f) + (yb == j ? ly1 : 0.f);
        float row = 0.f;
        for (int x = x_lo; x < x_hi; ++x) {
            int xa, xb;
            float lx0, lx1;
            up_index(x, rs, w, xa, xb, lx0, lx1);
            const float wx = (xa == i ? lx0 : 0.f) + (xb == i ? lx1 : 0.f);
            row = __builtin_fmaf(wx, gp[(size_t)y * W + x], row);
        }
        acc = __builtin_fmaf(wy, row, acc);
    }
    out[t] = acc;
}

int check_shape(const char* who, int B, int H, int W, int h, int w, int* s) {
    CPN_REQUIRE(B > 0 && H > 0 && W > 0 && h > 0 && w > 0, CPN_E_SHAPE, "%s: need positive sizes", who);
    CPN_REQUIRE(H % h == 0 && W % w == 0 && H / h == W / w, CPN_E_SHAPE, "%s: H/h and W/w must be one integer scale (got %dx%d from %dx%d)",
                who, H, W, h, w);
    *s = H / h;
    CPN_REQUIRE(*s == 1 || *s == 2 || *s == 4 || *s == 8, CPN_E_SHAPE, "%s: scale %d not in {1, 2, 4, 8}", who, *s);
    CPN_REQUIRE((long long)2 * B * 9 * H * W < (1LL << 31) && 2LL * B <= 65535, CPN_E_SHAPE, "%s: batch too large for one launch", who);
    return 0;
}

}  // namespace

extern "C" int cpn_ssim_warp_blocks(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return (int)(cpn_cdiv(H, TH) * cpn_cdiv(W, TW));
}

extern "C" int cpn_ssim_warp(const float* rgb, const float* flow0, const float* flow1, const uint8_t* mask, const float* window,
                             int B, int H, int W, int h, int w, float* coords, float* maps, float* partial, float* sums,
                             float* loss, float* inv3den, void* stream) {
    CPN_REQUIRE(rgb && flow0 && flow1 && mask && window && coords && maps && partial && sums && loss && inv3den, CPN_E_ARG,
                "cpn_ssim_warp: null pointer");
    int s = 0;
    if (int e = check_shape("cpn_ssim_warp", B, H, W, h, w, &s)) return e;
    const dim3 grid(cpn_cdiv(W, TW), cpn_cdiv(H, TH), 2 * B);
    hipLaunchKernelGGL(ssim_warp_fwd_kernel, grid, dim3(NT), 0, (hipStream_t)stream, rgb, flow0, flow1, mask, window, H, W, h, w, s,
                       coords, maps, partial);
    CPN_LAUNCH_CHECK("cpn_ssim_warp");
    hipLaunchKernelGGL(ssim_warp_finish_kernel, dim3(2), dim3(64), 0, (hipStream_t)stream, partial, B, (int)(grid.x * grid.y), sums,
                       loss, inv3den);
    CPN_LAUNCH_CHECK("cpn_ssim_warp (finish)");
    return 0;
}

extern "C" int cpn_ssim_warp_bwd(const float* rgb, const float* coords, const float* maps, const float* window, const float* gout,
                                 const float* inv3den, int B, int H, int W, int h, int w, float* gup, float* dflow, void* stream) {
    CPN_REQUIRE(rgb && coords && maps && window && gout && inv3den && gup && dflow, CPN_E_ARG, "cpn_ssim_warp_bwd: null pointer");
    int s = 0;
    if (int e = check_shape("cpn_ssim_warp_bwd", B, H, W, h, w, &s)) return e;
    const dim3 grid(cpn_cdiv(W, TW), cpn_cdiv(H, TH), 2 * B);
    hipLaunchKernelGGL(ssim_warp_bwd_kernel, grid, dim3(NT), 0, (hipStream_t)stream, rgb, coords, maps, window, gout, inv3den, H, W,
                       s, gup);
    CPN_LAUNCH_CHECK("cpn_ssim_warp_bwd");
    const int planes = 2 * B * 2;
    hipLaunchKernelGGL(ssim_upsample_adjoint_kernel, dim3(cpn_cdiv((long long)planes * h * w, NT)), dim3(NT), 0, (hipStream_t)stream,
                       gup, planes, h, w, H, W, s, dflow);
    CPN_LAUNCH_CHECK("cpn_ssim_warp_bwd (adjoint)");
    return 0;
}
