// The device side of the reference's training / validation log (summary/summaries.py:img_summaries, wrapper.py:126-130).
// As the reference writes it, one validation batch costs two F.interpolate and four grid_sample calls with norms and masks as
// stock ops, a Python loop with a .cpu().numpy() per image and direction for the mask overlay, the whole depth map copied to
// the host for a matplotlib colour map, and five reductions over at_wt.  Here:
//
//   flow_panels_kernel        one thread per output pixel of one direction of one pair (32 x 8 tiles; item = d B + b).  Its own
//                             upsampled flow (ATen's align_corners=False rule), the sampling coordinate (the fp32 expression
//                             sequence of `warp` followed by ATen's unnormalisation: flow_warp.h, -ffp-contract=off), the four
//                             zero-padded taps of the OTHER direction's upsampled flow - each of them four low-resolution taps,
//                             so no S x S flow is ever stored - the cycle norm, the validity mask, the four taps of the source
//                             view scaled to [0, 255], and the overlay of summaries.py:42-63 in integers.
//   depth_jet_kernel          one thread per depth value: matplotlib's index arithmetic on a float32 array (jet.h), a table
//                             lookup.
//   attention_entropy_kernel  one wave per row of at_wt, 8 rows after one another per wave, 4 waves per workgroup: the row's
//                             -sum w log(w + 1e-5) by the shared wave reduction, the workgroup's 32 rows as one float
//                             (common.h's waves4_sum).
//   attention_entropy_finish_kernel   the workgroups' partials in a fixed order, in float64 (partial_sum.h's
//                             sum_partials_f64 with 256 threads) -> the mean over the rows.
// No atomics: every result is bit-reproducible, and an image's panels do not depend on the batch around it.
#include "flow_warp.h"
#include "jet.h"
#include "partial_sum.h"

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int PTW = 32, PTH = NT / PTW;                   // flow panels: the tile of one workgroup
constexpr int ENT_WAVES = NT / 64, ENT_ROWS = 8;          // entropy: rows per wave, one after another
constexpr int ENT_BLOCK_ROWS = ENT_WAVES * ENT_ROWS;

// np.asarray(float32 image, dtype=np.uint8) on values that `warp` of a [0, 255] image can produce: truncation.  Four weights
// that sum to 1 + an ulp can carry 255 slightly past 255; that and a NaN (which numpy leaves undefined) are kept in range.
__device__ __forceinline__ int to_u8(float v) { return v >= 0.f ? (v <= 255.f ? (int)v : 255) : 0; }


__global__ __launch_bounds__(NT) void flow_panels_kernel(const float* __restrict__ rgb, const float* __restrict__ flow0,
                                                         const float* __restrict__ flow1, int B, int S, int h, float fs, float rs,
                                                         float* __restrict__ warped, uint8_t* __restrict__ mask,
                                                         uint8_t* __restrict__ overlay) {
    const int tid = threadIdx.x;
    const int gx = blockIdx.x * PTW + (tid & (PTW - 1)), gy = blockIdx.y * PTH + tid / PTW;
    if (gx >= S || gy >= S) return;
    const int item = blockIdx.z, d = item / B, b = item - d * B;
    const size_t SS = (size_t)S * S;
    const float* const src = rgb + ((size_t)b * 2 + (1 - d)) * SS * 3;
    const float* const own = (d ? flow1 : flow0) + (size_t)b * 2 * h * h;
    const float* const oth = (d ? flow0 : flow1) + (size_t)b * 2 * h * h;

    float ux, uy, ix, iy;
    up_flow(own, h, h, fs, rs, gx, gy, ux, uy);
    warp_coord(S, S, gx, gy, ux, uy, ix, iy);
    const WarpTaps t = warp_taps(ix, iy, S, S);
    const float wt[4] = {t.wx0 * t.wy0, t.wx1 * t.wy0, t.wx0 * t.wy1, t.wx1 * t.wy1};
    const bool ok[4] = {t.vy0 && t.vx0, t.vy0 && t.vx1, t.vy1 && t.vx0, t.vy1 && t.vx1};
    const int tx[4] = {t.x0, t.x1, t.x0, t.x1}, ty[4] = {t.y0, t.y0, t.y1, t.y1};

    // warp(up_other, up_own): grid_sample's sum over the taps in its order, every tap value formed as F.interpolate forms it
    float cx = 0.f, cy = 0.f, v[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (ok[k]) {
            float ox, oy;
            up_flow(oth, h, h, fs, rs, tx[k], ty[k], ox, oy);
            cx += ox * wt[k];
            cy += oy * wt[k];
            const float* const p = src + ((size_t)ty[k] * S + tx[k]) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] += ((p[c] + 1.0f) * 127.5f) * wt[k];
        }
    }
    const float ex = ux + cx, ey = uy + cy;
    const float norm = sqrtf(ex * ex + ey * ey);
    const float mx = ux + (float)gx, my = uy + (float)gy, hi = (float)(S - 1);
    const bool m = norm <= 10.0f && mx >= 0.f && mx <= hi && my >= 0.f && my <= hi;

    const size_t px = (size_t)item * SS + (size_t)gy * S + gx;
    const int colour[3] = {255, 102, 51};
    mask[px] = m ? 1 : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        warped[px * 3 + c] = v[c];
        const int u = to_u8(v[c]);
        overlay[px * 3 + c] = (uint8_t)(m ? u : (u + colour[c]) >> 1);       // trunc(0.5 u + 0.5 colour), exact in integers
    }
}


__global__ __launch_bounds__(NT) void depth_jet_kernel(const float* __restrict__ depth, long long n, const float* __restrict__ table,
                                                       float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int idx = jet_index(depth[i]);
    float r = 0.f, g = 0.f, bl = 0.f;                      // NaN: the colour map's `bad` entry
    if (idx >= 0) {
        r = table[3 * idx + 0];
        g = table[3 * idx + 1];
        bl = table[3 * idx + 2];
    }
    out[3 * i + 0] = r;
    out[3 * i + 1] = g;
    out[3 * i + 2] = bl;
}


__global__ __launch_bounds__(NT) void attention_entropy_kernel(const float* __restrict__ w, long long rows, int S, int nan_to_zero,
                                                               float* __restrict__ partial) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r0 = ((long long)blockIdx.x * ENT_WAVES + wave) * ENT_ROWS;
    float acc[1] = {0.f};                                  // the wave's rows: the same in every lane
    for (int k = 0; k < ENT_ROWS; ++k) {
        const long long r = r0 + k;
        if (r >= rows) break;                              // the same for every lane of the wave
        const float* const p = w + (size_t)r * S;
        float e = 0.f;
        for (int s = lane; s < S; s += 64) {
            const float x = p[s];
            e += x * logf(x + 1e-5f);
        }
        e = -wave_sum(e);
        if (nan_to_zero && e != e) e = 0.f;                // wrapper.py:129
        acc[0] += e;
    }
    waves4_sum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc[0];
}

// one workgroup: sum_partials_f64 with 256 threads, then the four wave sums as (0 + 1) + (2 + 3)
__global__ __launch_bounds__(NT) void attention_entropy_finish_kernel(const float* __restrict__ partial, int nblk, long long rows,
                                                                      float* __restrict__ out) {
    double s[1];
    sum_partials_f64<NT>(partial, nblk, s);
    waves4_sum(s);
    if (threadIdx.x == 0) out[0] = (float)(s[0] / (double)rows);
}

}  // namespace

extern "C" int cpn_flow_panels(const float* rgb, const float* flow0, const float* flow1, int B, int S, int h, float* warped,
                               uint8_t* mask, uint8_t* overlay, void* stream) {
    CPN_REQUIRE(rgb && flow0 && flow1 && warped && mask && overlay, CPN_E_ARG, "cpn_flow_panels: null pointer");
    CPN_REQUIRE(B > 0 && h > 0 && S >= h, CPN_E_SHAPE, "cpn_flow_panels: need B > 0 and S >= h > 0 (got B %d, S %d, h %d)", B, S, h);
    CPN_REQUIRE(2 * (long long)B <= 65535 && S <= 16384, CPN_E_SHAPE, "cpn_flow_panels: %d pairs of side %d are too many for one launch",
                B, S);
    const float fs = (float)((double)S / (double)h);       // the Python float S / h, rounded when it meets the fp32 tensor
    const float rs = (float)h / (float)S;                  // ATen's area_pixel_compute_scale in fp32
    const dim3 grid(cpn_cdiv(S, PTW), cpn_cdiv(S, PTH), 2 * B);
    hipLaunchKernelGGL(flow_panels_kernel, grid, dim3(NT), 0, (hipStream_t)stream, rgb, flow0, flow1, B, S, h, fs, rs, warped, mask,
                       overlay);
    CPN_LAUNCH_CHECK("cpn_flow_panels");
    return 0;
}

extern "C" int cpn_depth_jet(const float* depth, long long n, const float* table, float* out, void* stream) {
    CPN_REQUIRE(depth && table && out, CPN_E_ARG, "cpn_depth_jet: null pointer");
    CPN_REQUIRE(n > 0 && n <= (1LL << 31) * NT - NT, CPN_E_SHAPE, "cpn_depth_jet: need 0 < n < 2^39 (got %lld)", n);
    hipLaunchKernelGGL(depth_jet_kernel, dim3(cpn_cdiv(n, NT)), dim3(NT), 0, (hipStream_t)stream, depth, n, table, out);
    CPN_LAUNCH_CHECK("cpn_depth_jet");
    return 0;
}

extern "C" int cpn_attention_entropy_blocks(long long rows) {
    if (rows <= 0 || rows > (long long)ENT_BLOCK_ROWS * 0x7fffffffLL / 2) return 0;
    return (int)cpn_cdiv(rows, ENT_BLOCK_ROWS);
}

extern "C" int cpn_attention_entropy(const float* at_wt, long long rows, int S, int nan_to_zero, float* partial, float* out,
                                     void* stream) {
    CPN_REQUIRE(at_wt && partial && out, CPN_E_ARG, "cpn_attention_entropy: null pointer");
    const int nblk = cpn_attention_entropy_blocks(rows);
    CPN_REQUIRE(nblk > 0 && S >= 1, CPN_E_SHAPE, "cpn_attention_entropy: need rows >= 1 and S >= 1 (got %lld x %d)", rows, S);
    hipLaunchKernelGGL(attention_entropy_kernel, dim3(nblk), dim3(NT), 0, (hipStream_t)stream, at_wt, rows, S, nan_to_zero, partial);
    CPN_LAUNCH_CHECK("cpn_attention_entropy");
    hipLaunchKernelGGL(attention_entropy_finish_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (const float*)partial, nblk, rows,
                       out);
    CPN_LAUNCH_CHECK("cpn_attention_entropy (finish)");
    return 0;
}
