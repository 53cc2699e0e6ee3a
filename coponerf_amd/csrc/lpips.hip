// The two memory-bound ends of LPIPS(net='vgg') as the reference's evaluation script calls it (test.py:149, 258-263; the
// `lpips` package 0.1.x with version='0.1', lpips=True, spatial=False, normalize=False).  The thirteen 3 x 3 convolutions
// between them stay library calls (coponerf_amd/lpips.py); the parts below are the ones a library serves badly.
//
//   lpips_stem_kernel    test.py:227-229, 258-259 (the clamp of the prediction and the fp32 round trip through [0, 1] that both
//                        images take), the package's ScalingLayer and conv1_1 + bias + ReLU in one launch.  As stock ops that
//                        is a clamp, four elementwise passes, a layout copy and a Cin = 3 convolution.  One workgroup per
//                        8 x 32 tile of one image: the scaled tile and a 1-pixel halo -> LDS, zeros outside the image (the
//                        padding follows the scaling: a border tap reads 0).  A thread owns 4 output channels (its 108
//                        weights live in registers) and walks 16 pixels; the 16 lanes of a pixel store its 64 channels as one
//                        256-byte row of the NHWC output.  Every sum is bias, then the 27 products in (ci, ky, kx) order, each
//                        an FMA: exact products, one rounding per term, the same bits on every run.
//   lpips_head_kernel    the package's normalize_tensor, the squared difference, the 1 x 1 `lin` layer and spatial_average
//                        for ALL tapped layers and images in one launch (about ten stock ops per layer over full-size
//                        temporaries otherwise).  16 lanes per pixel; a lane loads channels 4 (j + 16 i) .. + 3 of both maps
//                        with 16-byte loads (a pixel's row is read in 256-byte segments) and keeps them in registers while the
//                        two squared norms go round the 16 lanes, so every feature value is read once.  A workgroup owns 64
//                        consecutive pixels of one image of one layer and writes ONE float.
//   lpips_finish_kernel  one wave per image: its workgroups' floats layer by layer in a fixed order, in float64
//                        (partial_sum.h's sum_partials_f64), each layer divided by its pixel count, the layers added in order.
//   lpips_head_bwd_kernel  the head's adjoint with respect to the prediction maps, on the forward's grid and with its access
//                        pattern: a workgroup owns the same 64 pixels, a lane the same channels; both maps are read once, the
//                        two sums (sum f^2, sum u f) go round the 16 lanes, and the lane stores its channels of df with 16-byte
//                        stores.  One launch for all layers and images, no scratch buffer.  A pixel whose prediction vector is all
//                        zeros gets df = 0 (include/coponerf_hip.h: this library's rule; autograd gives NaN there).
//   lpips_stem_bwd_kernel   the stem's adjoint with respect to pred, on the forward's 8 x 32 tiles.  Phase 1 walks the tile and
//                        its 1-pixel halo with 16 lanes per pixel: a lane reads its 4 channels of dy and of the stem's output
//                        (the ReLU mask) with 16-byte loads, multiplies by its 108 weights (registers, as in the forward) and
//                        the 27 sums over the 64 channels go round the 16 lanes into LDS (27 floats per pixel, an odd stride:
//                        phase 2 reads without bank conflicts).  Phase 2, one thread per pixel: the nine taps of each input
//                        channel in (ky, kx) order, the division by the scale, the clamp's mask.
// No atomics: two runs give the same bits; an image's workgroups and their order depend only on the maps' sizes, so its value
// does not depend on N; a NaN reaches only the partials of its own image.
#include "partial_sum.h"

#include <math.h>

namespace {

// ---------------------------------------------------------------------------------------------------------------- stem
constexpr int TW = 32, TH = 8, NT = 256;
constexpr int RW = TW + 2, RH = TH + 2;
constexpr int STEM_C = 64;

// torch.clamp: a NaN stays a NaN (both comparisons are false)
__device__ __forceinline__ float clamp_unit(float v) { return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v); }

// test.py:227-229 then :258-259, then the ScalingLayer: every operation rounded to fp32 on its own.  This toolchain's
// __fadd_rn / __fmul_rn are plain operators inside inline functions, which contract once they are inlined, so the sequence is
// written with operators under the pragma: it switches contraction off for exactly these five operations, and the file needs
// no compile option.  (Contracted, the halvings and doublings would still be exact; the pragma makes that no concern.)
__device__ __forceinline__ float stem_input(float v, float shift, float scale) {
#pragma clang fp contract(off)
    const float x01 = (v + 1.0f) * 0.5f;
    const float x = (x01 - 0.5f) * 2.0f;
    return (x - shift) / scale;
}

__global__ __launch_bounds__(NT) void lpips_stem_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                        const float* __restrict__ w, const float* __restrict__ bias, int N,
                                                        int H, int W, float* __restrict__ out) {
    __shared__ float sx[3][RH * RW];
    const int tid = threadIdx.x;
    const int img = blockIdx.z;                             // 0 .. N - 1 predictions, N .. 2N - 1 targets
    const bool is_pred = img < N;
    const float* const src = (is_pred ? pred : target) + (size_t)(is_pred ? img : img - N) * H * W * 3;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;

    for (int idx = tid; idx < RH * RW; idx += NT) {
        const int ry = idx / RW, rx = idx - ry * RW;
        const int gy = ty0 + ry - 1, gx = tx0 + rx - 1;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t o = in ? ((size_t)gy * W + gx) * 3 : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float shift = c == 0 ? -0.030f : (c == 1 ? -0.088f : -0.188f);
            const float scale = c == 0 ? 0.458f : (c == 1 ? 0.448f : 0.450f);
            float v = 0.0f;
            if (in) {
                v = src[o + c];
                v = stem_input(is_pred ? clamp_unit(v) : v, shift, scale);
            }
            sx[c][idx] = v;
        }
    }

    const int cg = tid & 15, slot = tid >> 4;               // channels 4 cg .. 4 cg + 3; pixels slot, slot + 16, ..
    float wr[4][27];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < 27; ++k) wr[q][k] = w[(4 * cg + q) * 27 + k];
    const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias + 4 * cg);
    __syncthreads();

    for (int p = slot; p < TH * TW; p += NT / 16) {
        const int py = p / TW, px = p - py * TW;
        const int gy = ty0 + py, gx = tx0 + px;
        float a0 = b4[0], a1 = b4[1], a2 = b4[2], a3 = b4[3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float x = sx[c][(py + ky) * RW + px + kx];
                    const int k = (c * 3 + ky) * 3 + kx;
                    a0 = __builtin_fmaf(wr[0][k], x, a0);
                    a1 = __builtin_fmaf(wr[1][k], x, a1);
                    a2 = __builtin_fmaf(wr[2][k], x, a2);
                    a3 = __builtin_fmaf(wr[3][k], x, a3);
                }
        if (gy < H && gx < W) {
            f32x4 r;                                        // ReLU that keeps a NaN, as torch's
            r[0] = a0 < 0.0f ? 0.0f : a0;
            r[1] = a1 < 0.0f ? 0.0f : a1;
            r[2] = a2 < 0.0f ? 0.0f : a2;
            r[3] = a3 < 0.0f ? 0.0f : a3;
            *reinterpret_cast<f32x4*>(out + (((size_t)img * H + gy) * W + gx) * STEM_C + 4 * cg) = r;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- head
constexpr int HEAD_NT = 256, GROUP = 16, GROUPS = HEAD_NT / GROUP;
constexpr int HEAD_PIX = 64;                                // pixels per workgroup: 4 per 16-lane group
constexpr int MAXV = 512 / 64;                              // 16-byte loads per lane, map and pixel

struct HeadArgs {
    const float* feat[CPN_LPIPS_LAYERS];
    const float* lin[CPN_LPIPS_LAYERS];
    int C[CPN_LPIPS_LAYERS];
    int P[CPN_LPIPS_LAYERS];                                // pixels of one image
    int nblk[CPN_LPIPS_LAYERS];                             // workgroups of one image
    int off[CPN_LPIPS_LAYERS + 1];                          // first workgroup (= partial) of the layer: off[k] + n * nblk[k] + b
    int layers, N;
};

// the package's normalize_tensor adds its eps = 1e-10 to an fp32 tensor: the fp32 value of 1e-10
constexpr float LPIPS_EPS = 1e-10f;

// One pixel's vectors of both maps in the 16 lanes of its group (lane j: channels 4 (j + 16 i) .. + 3; zeros for a pixel past
// the end) and their squared norms, in every lane of the group.  Shared by the head and its adjoint: the same loads, the same sums.
template <int NV>
__device__ __forceinline__ void head_load(const float* __restrict__ fp, const float* __restrict__ ft, int C, int P, int pix, int j,
                                          f32x4 (&a)[NV], f32x4 (&b)[NV], float& sa, float& sb) {
    // zeros first, the loads over them under the guard: written as if / else over arrays that arrive by reference, the compiler
    // keeps two of the vectors in scratch memory through the pixel loop (48 bytes per lane); in this form both kernels use none
#pragma unroll
    for (int i = 0; i < NV; ++i) a[i] = b[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (pix < P) {                                          // the same in all 16 lanes of a group; the shuffles below are outside
        const float* const qa = fp + (size_t)pix * C + 4 * j;
        const float* const qb = ft + (size_t)pix * C + 4 * j;
#pragma unroll
        for (int i = 0; i < NV; ++i) a[i] = *reinterpret_cast<const f32x4*>(qa + 4 * GROUP * i);
#pragma unroll
        for (int i = 0; i < NV; ++i) b[i] = *reinterpret_cast<const f32x4*>(qb + 4 * GROUP * i);
    }
    sa = 0.0f, sb = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sa = __builtin_fmaf(a[i][e], a[i][e], sa);
            sb = __builtin_fmaf(b[i][e], b[i][e], sb);
        }
    sa = group16_sum(sa);
    sb = group16_sum(sb);
}

// sum over one pixel's channels of w (a - b)^2 for the pixels g, g + 16, .. of a workgroup's 64, in every lane of the group
template <int NV>
__device__ __forceinline__ float head_pixels(const float* __restrict__ fp, const float* __restrict__ ft,
                                             const float* __restrict__ lin, int C, int P, int pix0, int g, int j) {
    f32x4 wv[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) wv[i] = *reinterpret_cast<const f32x4*>(lin + 4 * (j + GROUP * i));
    float acc = 0.0f;
#pragma unroll 1
    for (int s = 0; s < HEAD_PIX / GROUPS; ++s) {
        const int pix = pix0 + g + GROUPS * s;
        f32x4 a[NV], b[NV];
        float sa, sb;
        head_load<NV>(fp, ft, C, P, pix, j, a, b, sa, sb);
        const float ra = 1.0f / (sqrtf(sa) + LPIPS_EPS), rb = 1.0f / (sqrtf(sb) + LPIPS_EPS);
        float v = 0.0f;                                     // a pixel past the end gives w * 0 * 0
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                // both products rounded before the subtraction: contracted into fma(a, ra, -(b rb)), identical maps would
                // leave the rounding error of one product instead of exactly 0
#pragma clang fp contract(off)
                const float d = a[i][e] * ra - b[i][e] * rb;
                v = __builtin_fmaf(wv[i][e] * d, d, v);
            }
        acc += v;
    }
    return group16_sum(acc);
}

// workgroup blk of the head's grid: layer k, image n, the image's b-th run of 64 pixels
__device__ __forceinline__ void head_block(const HeadArgs& A, int blk, int& k, int& n, int& b) {
    k = 0;
#pragma unroll
    for (int q = 1; q < CPN_LPIPS_LAYERS; ++q) k += (q < A.layers && blk >= A.off[q]) ? 1 : 0;
    const int rem = blk - A.off[k];
    n = rem / A.nblk[k];
    b = rem - n * A.nblk[k];
}

__global__ __launch_bounds__(HEAD_NT) void lpips_head_kernel(HeadArgs A, float* __restrict__ partial) {
    __shared__ float red[GROUPS];
    const int tid = threadIdx.x, g = tid >> 4, j = tid & 15;
    const int blk = blockIdx.x;
    int k, n, b;
    head_block(A, blk, k, n, b);
    const int C = A.C[k], P = A.P[k];
    const float* const fp = A.feat[k] + (size_t)n * P * C;
    const float* const ft = A.feat[k] + (size_t)(A.N + n) * P * C;
    const float* const lin = A.lin[k];
    const int pix0 = b * HEAD_PIX;
    float v;
    switch (C / 64) {                                       // the same in every lane of the workgroup
        case 1: v = head_pixels<1>(fp, ft, lin, C, P, pix0, g, j); break;
        case 2: v = head_pixels<2>(fp, ft, lin, C, P, pix0, g, j); break;
        case 3: v = head_pixels<3>(fp, ft, lin, C, P, pix0, g, j); break;
        case 4: v = head_pixels<4>(fp, ft, lin, C, P, pix0, g, j); break;
        case 5: v = head_pixels<5>(fp, ft, lin, C, P, pix0, g, j); break;
        case 6: v = head_pixels<6>(fp, ft, lin, C, P, pix0, g, j); break;
        case 7: v = head_pixels<7>(fp, ft, lin, C, P, pix0, g, j); break;
        default: v = head_pixels<MAXV>(fp, ft, lin, C, P, pix0, g, j); break;
    }
    if (j == 0) red[g] = v;
    __syncthreads();
    if (tid == 0) {
        float r[GROUPS];                                    // a fixed tree over the 16 groups
#pragma unroll
        for (int q = 0; q < GROUPS; ++q) r[q] = red[q];
#pragma unroll
        for (int h = GROUPS / 2; h > 0; h >>= 1)
#pragma unroll
            for (int q = 0; q < h; ++q) r[q] += r[q + h];
        partial[blk] = r[0];
    }
}

// one workgroup of 64 lanes per image; per layer sum_partials_f64 over the image's workgroups
__global__ __launch_bounds__(64) void lpips_finish_kernel(HeadArgs A, const float* __restrict__ partial, float* __restrict__ out,
                                                          float* __restrict__ per_layer) {
    const int n = blockIdx.x, lane = threadIdx.x;
    double total = 0.0;
    for (int k = 0; k < CPN_LPIPS_LAYERS; ++k) {
        double s[1] = {0.0};
        if (k < A.layers) {
            sum_partials_f64<64>(partial + A.off[k] + (size_t)n * A.nblk[k], A.nblk[k], s);
            s[0] /= (double)A.P[k];
        }
        total += s[0];
        if (per_layer && lane == 0) per_layer[n * CPN_LPIPS_LAYERS + k] = (float)s[0];
    }
    if (lane == 0) out[n] = (float)total;
}

// workgroups (= partial floats) of a call; 0 for sizes the head rejects
long long head_blocks(int N, int layers, const int* h, const int* w, HeadArgs* A) {
    if (N <= 0 || N > 32768 || layers < 1 || layers > CPN_LPIPS_LAYERS || !h || !w) return 0;
    long long total = 0;
    for (int k = 0; k < layers; ++k) {
        if (h[k] < 1 || w[k] < 1 || (long long)h[k] * w[k] > (1LL << 26)) return 0;
        const int P = h[k] * w[k];
        const int nb = (int)cpn_cdiv(P, HEAD_PIX);
        if (A) {
            A->P[k] = P;
            A->nblk[k] = nb;
            A->off[k] = (int)total;
        }
        total += (long long)N * nb;
        if (total >= (1LL << 31)) return 0;
    }
    if (A) A->off[layers] = (int)total;
    return total;
}

// ------------------------------------------------------------------------------------------------------- head, adjoint
struct HeadBwdArgs {
    HeadArgs A;
    float* dfeat[CPN_LPIPS_LAYERS];                         // (N, h, w, C) per layer
};

// df of the pixels g, g + 16, .. of a workgroup's 64 (include/coponerf_hip.h has the formula); coef = 2 g_n / P
template <int NV>
__device__ __forceinline__ void head_bwd_pixels(const float* __restrict__ fp, const float* __restrict__ ft,
                                                const float* __restrict__ lin, float* __restrict__ df, int C, int P, int pix0,
                                                int g, int j, float coef) {
    f32x4 wv[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) wv[i] = *reinterpret_cast<const f32x4*>(lin + 4 * (j + GROUP * i));
#pragma unroll 1
    for (int s = 0; s < HEAD_PIX / GROUPS; ++s) {
        const int pix = pix0 + g + GROUPS * s;
        f32x4 a[NV], b[NV];
        float sa, sb;
        head_load<NV>(fp, ft, C, P, pix, j, a, b, sa, sb);
        const float na = sqrtf(sa);
        const float ra = 1.0f / (na + LPIPS_EPS), rb = 1.0f / (sqrtf(sb) + LPIPS_EPS);
        float dot = 0.0f;
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma clang fp contract(off)
                const float d = a[i][e] * ra - b[i][e] * rb;                    // the forward's difference, bit for bit
                const float u = (wv[i][e] * d) * coef;
                b[i][e] = u;                                                    // the target's value is spent
                dot = __builtin_fmaf(u, a[i][e], dot);
            }
        dot = group16_sum(dot);
        const float k2 = dot * ra * ra / na;
        if (pix < P) {
            float* const q = df + (size_t)pix * C + 4 * j;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                f32x4 r;
#pragma unroll
                for (int e = 0; e < 4; ++e)                 // na == 0: every channel of the pixel is 0, and so is its gradient
                    r[e] = na == 0.0f ? 0.0f : __builtin_fmaf(-k2, a[i][e], ra * b[i][e]);
                *reinterpret_cast<f32x4*>(q + 4 * GROUP * i) = r;
            }
        }
    }
}

__global__ __launch_bounds__(HEAD_NT) void lpips_head_bwd_kernel(HeadBwdArgs B, const float* __restrict__ gout) {
    const HeadArgs& A = B.A;
    const int tid = threadIdx.x, g = tid >> 4, j = tid & 15;
    int k, n, b;
    head_block(A, blockIdx.x, k, n, b);
    const int C = A.C[k], P = A.P[k];
    const float* const fp = A.feat[k] + (size_t)n * P * C;
    const float* const ft = A.feat[k] + (size_t)(A.N + n) * P * C;
    const float* const lin = A.lin[k];
    float* const df = B.dfeat[k] + (size_t)n * P * C;
    const int pix0 = b * HEAD_PIX;
    const float coef = 2.0f * gout[n] / (float)P;
    switch (C / 64) {                                       // the same in every lane of the workgroup
        case 1: head_bwd_pixels<1>(fp, ft, lin, df, C, P, pix0, g, j, coef); break;
        case 2: head_bwd_pixels<2>(fp, ft, lin, df, C, P, pix0, g, j, coef); break;
        case 3: head_bwd_pixels<3>(fp, ft, lin, df, C, P, pix0, g, j, coef); break;
        case 4: head_bwd_pixels<4>(fp, ft, lin, df, C, P, pix0, g, j, coef); break;
        case 5: head_bwd_pixels<5>(fp, ft, lin, df, C, P, pix0, g, j, coef); break;
        case 6: head_bwd_pixels<6>(fp, ft, lin, df, C, P, pix0, g, j, coef); break;
        case 7: head_bwd_pixels<7>(fp, ft, lin, df, C, P, pix0, g, j, coef); break;
        default: head_bwd_pixels<MAXV>(fp, ft, lin, df, C, P, pix0, g, j, coef); break;
    }
}

// ------------------------------------------------------------------------------------------------------- stem, adjoint
constexpr int TAPS = 27;                                    // (ci, ky, kx); an odd LDS stride per pixel

__global__ __launch_bounds__(NT) void lpips_stem_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ yout,
                                                            const float* __restrict__ pred, const float* __restrict__ w, int H,
                                                            int W, float* __restrict__ dpred) {
    __shared__ float sv[RH * RW * TAPS];                    // per pixel of the tile + halo: sum_co w[co][k] dy'[co], k < 27
    const int tid = threadIdx.x;
    const int img = blockIdx.z;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const size_t img0 = (size_t)img * H * W;

    const int cg = tid & 15, slot = tid >> 4;               // channels 4 cg .. 4 cg + 3; pixels slot, slot + 16, ..
    float wr[4][TAPS];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < TAPS; ++k) wr[q][k] = w[(4 * cg + q) * TAPS + k];

#pragma unroll 1
    for (int idx0 = 0; idx0 < RH * RW; idx0 += NT / 16) {
        const int idx = idx0 + slot;                        // the same in all 16 lanes of a group; the shuffles are outside
        const int ry = idx / RW, rx = idx - ry * RW;
        const int gy = ty0 + ry - 1, gx = tx0 + rx - 1;
        const bool in = idx < RH * RW && gy >= 0 && gy < H && gx >= 0 && gx < W;
        f32x4 d = {0.f, 0.f, 0.f, 0.f};                     // a tap outside the image is absent
        if (in) {
            const size_t o = (img0 + (size_t)gy * W + gx) * STEM_C + 4 * cg;
            d = *reinterpret_cast<const f32x4*>(dy + o);
            const f32x4 yo = *reinterpret_cast<const f32x4*>(yout + o);
#pragma unroll
            for (int q = 0; q < 4; ++q) d[q] = yo[q] > 0.0f ? d[q] : 0.0f;     // the ReLU's mask, from its output
        }
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
            float v = wr[0][k] * d[0];
            v = __builtin_fmaf(wr[1][k], d[1], v);
            v = __builtin_fmaf(wr[2][k], d[2], v);
            v = __builtin_fmaf(wr[3][k], d[3], v);
            v = group16_sum(v);
            if (cg == (k & 15) && idx < RH * RW) sv[idx * TAPS + k] = v;
        }
    }
    __syncthreads();

    const int py = tid / TW, px = tid - py * TW;            // one thread per pixel of the tile
    const int gy = ty0 + py, gx = tx0 + px;
    if (gy >= H || gx >= W) return;
    const size_t o = (img0 + (size_t)gy * W + gx) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float scale = c == 0 ? 0.458f : (c == 1 ? 0.448f : 0.450f);
        float acc = 0.0f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)                  // output (y, x) fed input (y - ky + 1, x - kx + 1) through w[.., ky, kx]
                acc += sv[((py - ky + 2) * RW + px - kx + 2) * TAPS + (c * 3 + ky) * 3 + kx];
        const float p = pred[o + c];
        dpred[o + c] = (p >= -1.0f && p <= 1.0f) ? acc / scale : 0.0f;          // torch.clamp's mask; false for a NaN
    }
}

}  // namespace

extern "C" int cpn_lpips_stem(const float* pred, const float* target, const float* w, const float* bias, int N, int H, int W,
                              float* out, void* stream) {
    CPN_REQUIRE(pred && target && w && bias && out, CPN_E_ARG, "cpn_lpips_stem: null pointer");
    CPN_REQUIRE((((uintptr_t)bias | (uintptr_t)out) & 15) == 0, CPN_E_ARG, "cpn_lpips_stem: bias and out must be 16-byte aligned");
    CPN_REQUIRE(N > 0 && H > 0 && W > 0, CPN_E_SHAPE, "cpn_lpips_stem: need positive sizes");
    CPN_REQUIRE(H >= 16 && W >= 16, CPN_E_SHAPE,
                "cpn_lpips_stem: four 2 x 2 pools must leave a pixel: H, W >= 16 (got %d x %d)", H, W);
    CPN_REQUIRE(N <= 32767 && H <= 32768 && W <= 32768, CPN_E_SHAPE, "cpn_lpips_stem: %d images of %d x %d are too many for one launch",
                N, H, W);
    const dim3 grid(cpn_cdiv(W, TW), cpn_cdiv(H, TH), 2 * N);
    hipLaunchKernelGGL(lpips_stem_kernel, grid, dim3(NT), 0, (hipStream_t)stream, pred, target, w, bias, N, H, W, out);
    CPN_LAUNCH_CHECK("cpn_lpips_stem");
    return 0;
}

extern "C" int cpn_lpips_head_scratch(int N, int layers, const int* host_h, const int* host_w) {
    return (int)head_blocks(N, layers, host_h, host_w, nullptr);
}

extern "C" int cpn_lpips_head(const float* const* host_feat, const float* const* host_lin, const int* host_C, const int* host_h,
                              const int* host_w, int layers, int N, float* partial, float* out, float* per_layer, void* stream) {
    CPN_REQUIRE(host_feat && host_lin && host_C && host_h && host_w && partial && out, CPN_E_ARG, "cpn_lpips_head: null pointer");
    CPN_REQUIRE(layers >= 1 && layers <= CPN_LPIPS_LAYERS, CPN_E_SHAPE, "cpn_lpips_head: 1 .. %d layers, got %d", CPN_LPIPS_LAYERS,
                layers);
    HeadArgs A = {};
    const long long total = head_blocks(N, layers, host_h, host_w, &A);
    CPN_REQUIRE(total > 0, CPN_E_SHAPE, "cpn_lpips_head: %d images and these map sizes are not one launch (need N >= 1, h, w >= 1)", N);
    for (int k = 0; k < layers; ++k) {
        CPN_REQUIRE(host_feat[k] && host_lin[k], CPN_E_ARG, "cpn_lpips_head: null pointer in layer %d", k);
        CPN_REQUIRE((((uintptr_t)host_feat[k] | (uintptr_t)host_lin[k]) & 15) == 0, CPN_E_ARG,
                    "cpn_lpips_head: layer %d is not 16-byte aligned", k);
        CPN_REQUIRE(host_C[k] >= 64 && host_C[k] <= 512 && host_C[k] % 64 == 0, CPN_E_SHAPE,
                    "cpn_lpips_head: C must be a multiple of 64 up to 512, layer %d has %d", k, host_C[k]);
        A.feat[k] = host_feat[k];
        A.lin[k] = host_lin[k];
        A.C[k] = host_C[k];
    }
    A.layers = layers;
    A.N = N;
    hipLaunchKernelGGL(lpips_head_kernel, dim3((unsigned)total), dim3(HEAD_NT), 0, (hipStream_t)stream, A, partial);
    CPN_LAUNCH_CHECK("cpn_lpips_head");
    hipLaunchKernelGGL(lpips_finish_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, A, (const float*)partial, out, per_layer);
    CPN_LAUNCH_CHECK("cpn_lpips_head (finish)");
    return 0;
}

extern "C" int cpn_lpips_head_bwd(const float* const* host_feat, const float* const* host_lin, const int* host_C, const int* host_h,
                                  const int* host_w, int layers, int N, const float* g, float* const* host_dfeat, void* stream) {
    CPN_REQUIRE(host_feat && host_lin && host_C && host_h && host_w && g && host_dfeat, CPN_E_ARG, "cpn_lpips_head_bwd: null pointer");
    CPN_REQUIRE(layers >= 1 && layers <= CPN_LPIPS_LAYERS, CPN_E_SHAPE, "cpn_lpips_head_bwd: 1 .. %d layers, got %d", CPN_LPIPS_LAYERS,
                layers);
    HeadBwdArgs B = {};
    const long long total = head_blocks(N, layers, host_h, host_w, &B.A);
    CPN_REQUIRE(total > 0, CPN_E_SHAPE, "cpn_lpips_head_bwd: %d images and these map sizes are not one launch (need N >= 1, h, w >= 1)",
                N);
    for (int k = 0; k < layers; ++k) {
        CPN_REQUIRE(host_feat[k] && host_lin[k] && host_dfeat[k], CPN_E_ARG, "cpn_lpips_head_bwd: null pointer in layer %d", k);
        CPN_REQUIRE((((uintptr_t)host_feat[k] | (uintptr_t)host_lin[k] | (uintptr_t)host_dfeat[k]) & 15) == 0, CPN_E_ARG,
                    "cpn_lpips_head_bwd: layer %d is not 16-byte aligned", k);
        CPN_REQUIRE(host_C[k] >= 64 && host_C[k] <= 512 && host_C[k] % 64 == 0, CPN_E_SHAPE,
                    "cpn_lpips_head_bwd: C must be a multiple of 64 up to 512, layer %d has %d", k, host_C[k]);
        B.A.feat[k] = host_feat[k];
        B.A.lin[k] = host_lin[k];
        B.A.C[k] = host_C[k];
        B.dfeat[k] = host_dfeat[k];
    }
    B.A.layers = layers;
    B.A.N = N;
    hipLaunchKernelGGL(lpips_head_bwd_kernel, dim3((unsigned)total), dim3(HEAD_NT), 0, (hipStream_t)stream, B, g);
    CPN_LAUNCH_CHECK("cpn_lpips_head_bwd");
    return 0;
}

extern "C" int cpn_lpips_stem_bwd(const float* dy, const float* y, const float* pred, const float* w, int N, int H, int W,
                                  float* dpred, void* stream) {
    CPN_REQUIRE(dy && y && pred && w && dpred, CPN_E_ARG, "cpn_lpips_stem_bwd: null pointer");
    CPN_REQUIRE((((uintptr_t)dy | (uintptr_t)y) & 15) == 0, CPN_E_ARG, "cpn_lpips_stem_bwd: dy and y must be 16-byte aligned");
    CPN_REQUIRE(N > 0 && H >= 16 && W >= 16, CPN_E_SHAPE, "cpn_lpips_stem_bwd: N >= 1 and H, W >= 16 as in cpn_lpips_stem (got %d, %d x %d)",
                N, H, W);
    CPN_REQUIRE(N <= 65535 && H <= 32768 && W <= 32768, CPN_E_SHAPE,
                "cpn_lpips_stem_bwd: %d images of %d x %d are too many for one launch", N, H, W);
    const dim3 grid(cpn_cdiv(W, TW), cpn_cdiv(H, TH), N);
    hipLaunchKernelGGL(lpips_stem_bwd_kernel, grid, dim3(NT), 0, (hipStream_t)stream, dy, y, pred, w, H, W, dpred);
    CPN_LAUNCH_CHECK("cpn_lpips_stem_bwd");
    return 0;
}
