// Weight gradients of the convolutions of UFC's training step: one separable branch of the stride-1 Conv4d
// (cpn_conv_wgrad_planes) and the depthwise 3x3 of the feed-forward blocks, which also has its forward and data gradient
// on the token layout here (cpn_dwconv3x3_tokens).  Partial sums leave the producing kernels per workgroup and are added
// in a fixed order (partial_sum.h).
#include <algorithm>
#include "common.h"
#include "partial_sum.h"

namespace {

// ------------------------------------------------------------------------------------------------
// weight gradient of a 3x3 / stride 1 / pad 1 convolution over the LAST two dims of (B, C, G, H, W) volumes:
//   dW[o][c][i][j] = sum_{b,g,y,x} dy[b,o,g,y,x] * X[b,c,g,y+i-1,x+j-1],   db[o] = sum dy[b,o,...]
// i.e. one separable branch of Conv4d (the other branch is the same call on the volumes with the two index pairs
// swapped).  As a GEMM it is Cout x (Cin*9) with the contraction over millions of positions: MIOpen's choice for it
// ran 1.9 ms per call.  Here a workgroup walks (b,g) planes: the Cin input planes (1-pixel zero halo, so the nine
// shifted reads need no bounds logic) and the Cout gradient planes are staged in LDS; a wave owns one 16(o) x 16(c)
// output tile for all nine taps (9 accumulator tiles), dy is the MFMA A operand read once per 4 positions and reused
// by the nine v_mfma_f32_16x16x4_f32; partial sums leave once per workgroup with atomics.
// ------------------------------------------------------------------------------------------------
constexpr int WG_MAXC = 32;           // Cin, Cout <= 32
constexpr int WG_MAXP = 256;          // H * W <= 256
#ifndef CPN_WG_BLOCKS
#define CPN_WG_BLOCKS 512
#endif
constexpr int WG_BLOCKS = CPN_WG_BLOCKS;   // workgroups (= partial sums) per call
// SWAP (Cout <= 8 < Cin): the kernel is handed (dy, x, Cout, Cin) in place of (x, dy, Cin, Cout) - the gradient planes take
// the halo and the two-taps-per-column packing, since dW[o][c][tap] = sum_p dy[o][p - tap] x[c][p] is the same sum with the
// roles exchanged and the tap mirrored (8 - tap) - and writes its partial sums in the caller's (o, c, tap) order; the bias
// sum is then taken from the centre tap of the haloed operand.
template <int CI, int CO, bool SWAP = false>   // channel counts rounded up to 8 or 32: the staging registers of one plane
__global__ __launch_bounds__(256) void conv_wgrad_planes_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, int Cin, int Cout, int G, int H, int W, int nplanes,
    float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float wgl[];
    const int P = H * W, HP = (H + 2) * (W + 2);
    const int XS = HP + ((HP & 31) == 5 ? 0 : ((37 - (HP & 31)) & 31));     // plane stride = 5 (mod 32)
    const int DS = P + ((P & 31) == 4 ? 0 : ((36 - (P & 31)) & 31));        // row stride   = 4 (mod 32)
    const int CT = (Cin + 15) >> 4, MT = (Cout + 15) >> 4;
    float* xs = wgl;                                  // [CT*16][XS]   haloed input planes
    float* ds = wgl + CT * 16 * XS;                   // [MT*16][DS]   gradient planes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < CT * 16 * XS + MT * 16 * DS; i += 256) wgl[i] = 0.0f;     // halo + padding rows stay zero

    const int npairs = MT * CT;                       // 1, 2 or 4 output tiles
    const int pair = wave % npairs, kpart = wave / npairs, kparts = 4 / npairs;
    const int mt = pair % MT, ct = pair / MT;
    const int ln = lane & 15, lk = lane >> 4;
    // Cin <= 8 (CI == 8): the 16 columns of the MFMA's B operand hold 8 input channels x TWO taps (column n = channel n & 7
    // of tap 2 t + (n >> 3)), so the nine taps take five MFMAs per k step instead of nine with half of every tile empty
    // (these launches ran at twice their MFMA bound, which the padding had doubled: round 6)
    constexpr bool PACK = CI == 8;
    constexpr int NACC = PACK ? 5 : 9;
    const int tapsel = PACK ? (ln >> 3) : 0;
    f32x4 acc[NACC];
    int boff[NACC];                                   // PACK: offset of tap 2 t + tapsel in the haloed plane (the tenth slot re-reads tap 8: discarded)
#pragma unroll
    for (int t = 0; t < NACC; ++t) {
        acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int tap = min(2 * t + tapsel, 8);
        boff[t] = (tap / 3) * (W + 2) + tap % 3;
    }
    float bsum = 0.0f;
    const int ksteps = (P + 3) >> 2;
    const int k_lo = kpart * ksteps / kparts, k_hi = (kpart + 1) * ksteps / kparts;
    const float* arow = ds + (mt * 16 + ln) * DS;
    const float* brow = xs + (PACK ? (ln & 7) : ct * 16 + ln) * XS;
    // staging: P <= 256, so thread tid owns position tid of every plane
    const bool stg = tid < P;
    const int sy = stg ? tid / W : 0, sx = stg ? tid - sy * W : 0;
    const int hoff = (sy + 1) * (W + 2) + sx + 1;
    const int y0 = (k_lo * 4 + lk) / W, x0 = (k_lo * 4 + lk) - y0 * W;

    // a plane's Cin + Cout values of this thread's position travel through registers: all loads of a plane are issued
    // together, and the next plane's are in flight under the MFMA loop of the current one (the first version loaded and
    // stored channel by channel: Cin + Cout serialized HBM round trips per plane, 55 - 100 us per call for operands that
    // stream in 2 - 8 us)
    float vx[CI], vd[CO];
    const size_t cs = (size_t)G * P;
    auto load_plane = [&](int pl) {
        const int b = pl / G, g = pl - b * G;
        const float* xp = x + (((size_t)b * Cin) * G + g) * P + (stg ? tid : 0);
        const float* dp = dy + (((size_t)b * Cout) * G + g) * P + (stg ? tid : 0);
#pragma unroll
        for (int c = 0; c < CI; ++c) vx[c] = xp[(c < Cin ? c : Cin - 1) * cs];        // surplus slots repeat the last channel
#pragma unroll
        for (int o = 0; o < CO; ++o) vd[o] = dp[(o < Cout ? o : Cout - 1) * cs];
    };
    if ((int)blockIdx.x < nplanes) load_plane(blockIdx.x);
    for (int pl = blockIdx.x; pl < nplanes; pl += gridDim.x) {
        __syncthreads();                              // previous plane fully consumed (and the zero fill done)
        if (stg) {
#pragma unroll
            for (int c = 0; c < CI; ++c)
                if (c < Cin) xs[c * XS + hoff] = vx[c];
#pragma unroll
            for (int o = 0; o < CO; ++o)
                if (o < Cout) ds[o * DS + tid] = vd[o];
        }
        __syncthreads();
        if (pl + (int)gridDim.x < nplanes) load_plane(pl + gridDim.x);
        // operands of k step ks for this lane: gradient value av (rows are zero-padded past P: no predicate) and the 9
        // taps of the haloed input plane (positions past P read tap window (0,0) — finite values times av = 0).  The
        // next step's 10 LDS reads are issued before the current step's 9 MFMAs (predicated reads + a wait before every
        // MFMA ran this loop at a quarter of the MFMA rate)
        int yy = y0, xx = x0;
        bool bvalid = false;                           // SWAP: the position of the step just read lies inside the plane
        auto read_step = [&](int ks, float& av, float (&bv)[NACC]) {
            const int pos = ks * 4 + lk;
            av = arow[pos];
            if constexpr (SWAP) bvalid = pos < P;
            const float* bp = brow + (pos < P ? yy * (W + 2) + xx : 0);
            if constexpr (PACK) {
#pragma unroll
                for (int t = 0; t < 5; ++t) bv[t] = bp[boff[t]];
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) bv[i * 3 + j] = bp[i * (W + 2) + j];
            }
            xx += 4;
            const bool wrap = xx >= W;                 // W >= 4: at most one row per step
            xx -= wrap ? W : 0;
            yy += wrap ? 1 : 0;
        };
        float av, bv[NACC];
        if (k_lo < k_hi) read_step(k_lo, av, bv);
        for (int ks = k_lo; ks < k_hi; ++ks) {
            if constexpr (SWAP) bsum += (bvalid && tapsel == 0) ? bv[2] : 0.0f;     // centre tap (4 = 2 * 2 + 0) of the gradient plane
            else bsum += av;
            float an = 0.0f, bn[NACC];
#pragma unroll
            for (int t = 0; t < NACC; ++t) bn[t] = 0.0f;
            if (ks + 1 < k_hi) read_step(ks + 1, an, bn);
#pragma unroll
            for (int t = 0; t < NACC; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[t], acc[t], 0, 0, 0);
            av = an;
#pragma unroll
            for (int t = 0; t < NACC; ++t) bv[t] = bn[t];
        }
    }
    // partial sums of this workgroup: [Cout*Cin*9 weights | Cout biases]; D[m = lk*4 + e][n = ln]: m -> output
    // channel, n -> input channel.  Waves that split the positions of one tile (kparts > 1) combine with LDS atomics.
    const int nw = Cout * Cin * 9;
    const int nbias = SWAP ? Cin : Cout;              // the caller's output channels
    float* mine = partial + (size_t)blockIdx.x * (nw + nbias);
    __syncthreads();
    float* red = wgl;                                 // reuse LDS: nw + nbias floats <= 32*32*9 + 32
    for (int i = tid; i < nw + nbias; i += 256) red[i] = 0.0f;
    __syncthreads();
    const int c = PACK ? (ln & 7) : ct * 16 + ln;
#pragma unroll
    for (int t = 0; t < NACC; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o = mt * 16 + lk * 4 + e;
            const int tap = PACK ? 2 * t + tapsel : t;
            if (o < Cout && c < Cin && tap < 9) {
                // SWAP: (o, c) are (input channel, output channel) of the caller's problem, the tap is mirrored
                const size_t at = SWAP ? ((size_t)c * Cout + o) * 9 + (8 - tap) : ((size_t)o * Cin + c) * 9 + tap;
                if (kparts > 1) atomicAdd(red + at, acc[t][e]);
                else red[at] = acc[t][e];
            }
        }
    if constexpr (SWAP) {                             // bias of the caller's output channel c' = ln (tapsel 0 lanes), once per k part
        bsum += __shfl_xor(bsum, 16);
        bsum += __shfl_xor(bsum, 32);
        if (mt == 0 && lk == 0 && ln < Cin) atomicAdd(red + nw + ln, bsum);
    } else if (ct == 0) {                             // bias: lanes (ln = o, lk) hold disjoint position subsets
        bsum += __shfl_xor(bsum, 16);
        bsum += __shfl_xor(bsum, 32);
        const int o = mt * 16 + ln;
        if (lk == 0 && o < Cout) atomicAdd(red + nw + o, bsum);
    }
    __syncthreads();
    for (int i = tid; i < nw + nbias; i += 256) mine[i] = red[i];
}

__global__ __launch_bounds__(1024) void conv_wgrad_reduce_kernel(const float* __restrict__ partial, int nblocks, int nw,
                                                                 int Cout, float* __restrict__ dw,
                                                                 float* __restrict__ db) {
    // partial sums of the nblocks producers, each [nw weights | Cout biases], in the fixed order of sum_partials_16x64
    const size_t ld = (size_t)(nw + Cout);
    sum_partials_16x64(
        nw + Cout, nblocks, [&](long long b, int i) { return partial[(size_t)b * ld + i]; },
        [&](int i, float v) {
            if (i < nw) dw[i] = v;
            else if (db) db[i - nw] = v;
        });
}

// weight / bias gradient of a depthwise 3x3, stride 1, pad 1 convolution (the DWConv of the UFC feed-forward blocks,
// models/aggregation.py): dw[c][i][j] = sum_{n,y,x} dy[n,c,y,x] * X[n,c,y+i-1,x+j-1],  db[c] = sum dy[n,c].
// Ten sums over N*H*W values per channel — MIOpen's batched-GEMM weight-gradient took 1.9 ms for it.
// One workgroup per channel.
__global__ __launch_bounds__(256) void dwconv3x3_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              int N, int C, int H, int W, float* __restrict__ dw,
                                                              float* __restrict__ db) {
    const int c = blockIdx.x, P = H * W;
    float a[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int idx = threadIdx.x; idx < N * P; idx += 256) {
        const int n = idx / P, pos = idx - n * P;
        const int yy = pos / W, xx = pos - yy * W;
        const size_t base = ((size_t)n * C + c) * P;
        const float g = dy[base + pos];
        a[9] += g;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int Y = yy + i - 1, X = xx + j - 1;
                if (Y >= 0 && Y < H && X >= 0 && X < W) a[i * 3 + j] += g * x[base + (size_t)Y * W + X];
            }
    }
    __shared__ float sh[4][10];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < 10; ++t) {
        a[t] = wave_sum(a[t]);
        if (lane == 0) sh[wave][t] = a[t];
    }
    __syncthreads();
    if (threadIdx.x < 10) {
        const float v = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
        if (threadIdx.x < 9) dw[c * 9 + threadIdx.x] = v;
        else if (db) db[c] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// The same depthwise convolution directly on the TOKEN layout (B, L = H*W, C) the feed-forward blocks work in
// (aggregation.py:18-28 transposes to (B,C,H,W), runs the grouped Conv2d and transposes back).  With the channel
// innermost the reads are coalesced float4 rows: no transposed copies on either side,
// and the library's depthwise kernel (0.76 ms for 4 x 1024 x 64 x 64, 12x the streaming time) is not needed.
//   flip = 0: y = b + sum_ij w[c][i][j] * x[p + (i-1, j-1)]        (forward)
//   flip = 1: y =     sum_ij w[c][2-i][2-j] * x[p + (i-1, j-1)]    (data gradient: correlation with the flipped taps)
// ------------------------------------------------------------------------------------------------
// thread = (run of DW_RUN consecutive x positions of one image row, 4 channels): the 36 taps of its channels are loaded
// once, and the three input rows slide through registers (3 new 16-byte loads per output instead of 9)
constexpr int DW_RUN = 8;
__global__ __launch_bounds__(256) void dwconv3x3_tokens_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ bias, int H, int W, int C4,
                                                               long long total, int flip, float* __restrict__ y) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c4 = (int)(idx % C4);
    long long t = idx / C4;
    const int runs = (W + DW_RUN - 1) / DW_RUN;
    const int xr = (int)(t % runs); t /= runs;
    const int yy = (int)(t % H);
    const long long bimg = t / H;
    const int C = C4 * 4, x0 = xr * DW_RUN;
    const f32x4 b4 = bias ? *reinterpret_cast<const f32x4*>(bias + c4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 wr[9];                                              // wr[tap][channel e]
#pragma unroll
    for (int tp = 0; tp < 9; ++tp)
#pragma unroll
        for (int e = 0; e < 4; ++e) wr[tp][e] = w[(c4 * 4 + e) * 9 + ((flip & 1) ? 8 - tp : tp)];
    const float* xb = x + (bimg * H * W) * C + c4 * 4;
    auto col = [&](int X, f32x4 (&v)[3]) {                     // the three rows of column X (zeros outside the image)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int Y = yy + i - 1;
            v[i] = (X >= 0 && X < W && Y >= 0 && Y < H) ? *reinterpret_cast<const f32x4*>(xb + ((long long)Y * W + X) * C)
                                                         : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    f32x4 c0[3], c1[3], c2[3];
    col(x0 - 1, c0);
    col(x0, c1);
#pragma unroll
    for (int k = 0; k < DW_RUN; ++k) {
        const int X = x0 + k;
        if (X >= W) break;
        col(X + 1, c2);
        f32x4 acc = b4;
#pragma unroll
        for (int i = 0; i < 3; ++i) acc += wr[i * 3] * c0[i] + wr[i * 3 + 1] * c1[i] + wr[i * 3 + 2] * c2[i];
        if (flip & 2) {                                       // exact GELU of the feed-forward block (nn.GELU(), aggregation.py:180)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = 0.5f * acc[e] * (1.0f + erff(acc[e] * 0.70710678118654752440f));
        }
        *reinterpret_cast<f32x4*>(y + ((bimg * H + yy) * W + X) * C + c4 * 4) = acc;
#pragma unroll
        for (int i = 0; i < 3; ++i) { c0[i] = c1[i]; c1[i] = c2[i]; }
    }
}

// weight / bias gradient in the token layout: block = (image row, 256 consecutive channels), thread = channel; the
// 3 x 3 input window slides along the row (3 new loads per position).  Each block leaves 10 partial sums per channel
// in `partial` (rows x C x 10); a second launch reduces them in a fixed order (deterministic, no atomics).
__global__ __launch_bounds__(256) void dwconv3x3_tokens_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                     int H, int W, int C, float* __restrict__ partial) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= C) return;
    const long long rowid = blockIdx.x;                       // b * H + yy
    const int yy = (int)(rowid % H);
    const float* xr = x + (rowid - yy) * W * C + c;           // image base (+ channel)
    const float* dr = dy + rowid * W * C + c;
    float a[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto col = [&](int X, float (&v)[3]) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int Y = yy + i - 1;
            v[i] = (X >= 0 && X < W && Y >= 0 && Y < H) ? xr[((long long)Y * W + X) * C] : 0.0f;
        }
    };
    float c0[3], c1[3], c2[3];
    col(-1, c0);
    col(0, c1);
#pragma unroll 4
    for (int X = 0; X < W; ++X) {
        col(X + 1, c2);
        const float g = dr[(long long)X * C];
        a[9] += g;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            a[i * 3] += g * c0[i];
            a[i * 3 + 1] += g * c1[i];
            a[i * 3 + 2] += g * c2[i];
            c0[i] = c1[i];
            c1[i] = c2[i];
        }
    }
#pragma unroll
    for (int t = 0; t < 10; ++t) partial[(rowid * C + c) * 10 + t] = a[t];
}

__global__ __launch_bounds__(1024) void dwconv3x3_tokens_wgrad_reduce_kernel(const float* __restrict__ partial, long long rows,
                                                                             int C, float* __restrict__ dw,
                                                                             float* __restrict__ db) {
    // the rows' (channel, term) partial sums, rows x C x 10, in the fixed order of sum_partials_16x64
    const size_t ld = (size_t)C * 10;
    sum_partials_16x64(
        C * 10, rows, [&](long long r, int i) { return partial[(size_t)r * ld + i]; },
        [&](int i, float acc) {
            const int c = i / 10, t = i - c * 10;
            if (t < 9) dw[c * 9 + t] = acc;
            else if (db) db[c] = acc;
        });
}

}  // namespace

// floats of `partial`: [workgroup w < min(B*G, WG_BLOCKS)][Cout*Cin*9 weights (o, c, tap) | Cout biases], sized for WG_BLOCKS
extern "C" long long cpn_conv_wgrad_scratch(int Cin, int Cout) {
    return (long long)WG_BLOCKS * ((long long)Cout * Cin * 9 + Cout);
}

extern "C" int cpn_conv_wgrad_planes(const float* x, const float* dy, int B, int Cin, int Cout, int G, int H, int W,
                                     float* partial, float* dw, float* db, void* stream) {
    CPN_REQUIRE(x && dy && dw && partial, CPN_E_ARG, "cpn_conv_wgrad_planes: null pointer");
    CPN_REQUIRE(B > 0 && G > 0 && H > 0 && W >= 4 && Cin > 0 && Cout > 0, CPN_E_SHAPE,
                "cpn_conv_wgrad_planes: bad shape");
    CPN_REQUIRE(Cin <= WG_MAXC && Cout <= WG_MAXC && H * W <= WG_MAXP, CPN_E_SHAPE,
                "cpn_conv_wgrad_planes: supports Cin, Cout <= %d and H*W <= %d (got %d, %d, %d)", WG_MAXC, WG_MAXP, Cin,
                Cout, H * W);
    CPN_REQUIRE((long long)B * G < (1LL << 31), CPN_E_SHAPE, "cpn_conv_wgrad_planes: too many planes");
    const int P = H * W, HP = (H + 2) * (W + 2);
    const int XS = HP + ((HP & 31) == 5 ? 0 : ((37 - (HP & 31)) & 31));
    const int DS = P + ((P & 31) == 4 ? 0 : ((36 - (P & 31)) & 31));
    const bool swap = Cout <= 8 && Cin > 8;                  // conv_wgrad_planes_kernel<8, 32, true>: the operands change places
    const int CT = ((swap ? Cout : Cin) + 15) / 16, MT = ((swap ? Cin : Cout) + 15) / 16;
    const size_t lds = std::max((size_t)CT * 16 * XS + (size_t)MT * 16 * DS, (size_t)Cout * Cin * 9 + Cout) * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
        for (const void* k : {(const void*)conv_wgrad_planes_kernel<8, 8>, (const void*)conv_wgrad_planes_kernel<8, 32>,
                              (const void*)conv_wgrad_planes_kernel<8, 32, true>, (const void*)conv_wgrad_planes_kernel<32, 32>}) {
            hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
            if (e != hipSuccess) {
                cpn_set_error("cpn_conv_wgrad_planes: cannot reserve LDS: %s", hipGetErrorString(e));
                return (int)e;
            }
        }
        attr_set = true;
    }
    const int nplanes = B * G;
    const int blocks = std::min(nplanes, WG_BLOCKS);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(blocks), block(256);
    if (Cin <= 8 && Cout <= 8)
        hipLaunchKernelGGL((conv_wgrad_planes_kernel<8, 8>), grid, block, lds, st, x, dy, Cin, Cout, G, H, W, nplanes, partial);
    else if (Cin <= 8)
        hipLaunchKernelGGL((conv_wgrad_planes_kernel<8, 32>), grid, block, lds, st, x, dy, Cin, Cout, G, H, W, nplanes, partial);
    else if (Cout <= 8)                               // roles exchanged: the 8 gradient planes take the two-taps-per-column form
        hipLaunchKernelGGL((conv_wgrad_planes_kernel<8, 32, true>), grid, block, lds, st, dy, x, Cout, Cin, G, H, W, nplanes, partial);
    else
        hipLaunchKernelGGL((conv_wgrad_planes_kernel<32, 32>), grid, block, lds, st, x, dy, Cin, Cout, G, H, W, nplanes, partial);
    CPN_LAUNCH_CHECK("cpn_conv_wgrad_planes");
    const int nw = Cout * Cin * 9;
    hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3(cpn_cdiv(nw + Cout, 64)), dim3(1024), 0, st, partial, blocks, nw, Cout,
                       dw, db);
    CPN_LAUNCH_CHECK("cpn_conv_wgrad_planes(reduce)");
    return 0;
}

extern "C" int cpn_dwconv3x3_wgrad(const float* x, const float* dy, int N, int C, int H, int W, float* dw, float* db,
                                   void* stream) {
    CPN_REQUIRE(x && dy && dw, CPN_E_ARG, "cpn_dwconv3x3_wgrad: null pointer");
    CPN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && (long long)N * H * W < (1LL << 31), CPN_E_SHAPE,
                "cpn_dwconv3x3_wgrad: bad shape");
    hipLaunchKernelGGL(dwconv3x3_wgrad_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, x, dy, N, C, H, W, dw, db);
    CPN_LAUNCH_CHECK("cpn_dwconv3x3_wgrad");
    return 0;
}

extern "C" int cpn_dwconv3x3_tokens(const float* x, const float* w, const float* bias, int B, int H, int W, int C,
                                    int flip, float* y, void* stream) {
    CPN_REQUIRE(x && w && y, CPN_E_ARG, "cpn_dwconv3x3_tokens: null pointer");
    CPN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && (C % 4) == 0, CPN_E_SHAPE, "cpn_dwconv3x3_tokens: need C %% 4 == 0");
    CPN_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0 && ((uintptr_t)bias % 16) == 0, CPN_E_ARG,
                "cpn_dwconv3x3_tokens: pointers must be 16-byte aligned");
    const long long total = (long long)B * H * ((W + DW_RUN - 1) / DW_RUN) * (C / 4);
    CPN_REQUIRE(total / 256 < (1LL << 31), CPN_E_SHAPE, "cpn_dwconv3x3_tokens: too large");
    hipLaunchKernelGGL(dwconv3x3_tokens_kernel, dim3((unsigned)cpn_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, w,
                       bias, H, W, C / 4, total, flip, y);
    CPN_LAUNCH_CHECK("cpn_dwconv3x3_tokens");
    return 0;
}

// floats of `partial`: [image row r = b*H + y][channel c][10 terms: the nine taps, then the bias]
extern "C" long long cpn_dwconv3x3_tokens_wgrad_scratch(int B, int H, int C) { return (long long)B * H * C * 10; }

extern "C" int cpn_dwconv3x3_tokens_wgrad(const float* x, const float* dy, int B, int H, int W, int C, float* partial,
                                          float* dw, float* db, void* stream) {
    CPN_REQUIRE(x && dy && dw && partial, CPN_E_ARG, "cpn_dwconv3x3_tokens_wgrad: null pointer");
    CPN_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, CPN_E_SHAPE, "cpn_dwconv3x3_tokens_wgrad: bad shape");
    const long long rows = (long long)B * H;
    dim3 grid((unsigned)rows, (unsigned)cpn_cdiv(C, 256));
    hipLaunchKernelGGL(dwconv3x3_tokens_wgrad_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, dy, H, W, C, partial);
    hipLaunchKernelGGL(dwconv3x3_tokens_wgrad_reduce_kernel, dim3((unsigned)cpn_cdiv(C * 10, 64)), dim3(1024), 0,
                       (hipStream_t)stream, partial, rows, C, dw, db);
    CPN_LAUNCH_CHECK("cpn_dwconv3x3_tokens_wgrad");
    return 0;
}
