// K7 — correlation volumes of UFC (get_z path): HBM/L2-bound streaming work (up to 64^4 = 67 MB)
//   cpn_correlation          aggregation.correlation / correlation_token (models/aggregation.py:70-80)
//   cpn_resize_bilinear_ac   F.interpolate(align_corners=True) of interpolate4d / forward_attention, and its adjoint
//   cpn_corr_mean3           UFC.forward's last step: the three levels' correlations at n^4, averaged
#include <algorithm>
#include "common.h"
#include "ac_taps.h"

namespace {

// ------------------------------------------------------------------------------------------------
// correlation: tokens (B, L, C) -> x / (||x|| + eps), then C[b] = S_n[b] . T_n[b]^T with the exact-f32 MFMA
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void l2norm_rows_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          long long rows, int C, float eps) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (size_t)row * C;
    float ss = 0.f;
    for (int c = lane; c < C; c += 64) ss += xr[c] * xr[c];
    ss = wave_sum(ss);
    const float d = sqrtf(ss) + eps;
    for (int c = lane; c < C; c += 64) y[(size_t)row * C + c] = xr[c] / d;
}

// VJP of the row normalisation y = x / (|x| + eps): dx = dy / (|x| + eps) - y (y . dy) / max(|x|, tiny) — one wave per row,
// the row in registers (C <= 1024).  Ten ATen launches per call in the training step's correlation backward before.
__global__ __launch_bounds__(256) void l2norm_rows_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                              const float* __restrict__ dy, float* __restrict__ dx,
                                                              long long rows, int C, float eps) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const size_t base = (size_t)row * C;
    float xv[16], yv[16], gv[16];
    float ss = 0.f, dot = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + 64 * i;
        if (c < C) {
            xv[i] = x[base + c]; yv[i] = y[base + c]; gv[i] = dy[base + c];
            ss += xv[i] * xv[i];
            dot += yv[i] * gv[i];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { ss += __shfl_xor(ss, off); dot += __shfl_xor(dot, off); }
    const float r = sqrtf(ss);
    const float inv = 1.0f / (r + eps), k = dot / fmaxf(r, 1e-30f);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + 64 * i;
        if (c < C) dx[base + c] = gv[i] * inv - yv[i] * k;
    }
}

// C (M x N) = A (M x K) . B (N x K)^T per batch; wave = 16 rows x 16*NT cols, block = 64 rows; K % 16 == 0.
// NT = 8 for large problems (fewer re-reads of B), NT = 2 when 128-column tiles would leave most of the chip idle
// (a 256 x 256 correlation is 8 workgroups at NT = 8); the operands of k block kb+16 are requested before the MFMAs of kb.
template <int NT>
__global__ __launch_bounds__(256) void gemm_nt_f32_kernel(const float* __restrict__ A, const float* __restrict__ Bm,
                                                          float* __restrict__ Cm, int M, int N, int K) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z;
    const int m0 = (blockIdx.y * 4 + wave) * 16, n0 = blockIdx.x * 16 * NT;
    if (m0 >= M) return;
    const float* Ab = A + (size_t)b * M * K;
    const float* Bb = Bm + (size_t)b * N * K;
    float* Cb = Cm + (size_t)b * M * N;
    const int fi = lane & 15, fg = lane >> 4;
    int ar = m0 + fi;
    ar = ar < M ? ar : M - 1;
    const float* ap = Ab + (size_t)ar * K + fg * 4;
    const float* bp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = n0 + t * 16 + fi;
        bp[t] = Bb + (size_t)(n < N ? n : N - 1) * K + fg * 4;       // columns past N are computed and not stored
    }
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto load = [&](int kb, f32x4& av, f32x4 (&bv)[NT]) {
        av = *reinterpret_cast<const f32x4*>(ap + kb);
#pragma unroll
        for (int t = 0; t < NT; ++t) bv[t] = *reinterpret_cast<const f32x4*>(bp[t] + kb);
    };
    auto step = [&](const f32x4& av, const f32x4 (&bv)[NT]) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[t][e], av[e], acc[t], 0, 0, 0);
    };
    f32x4 a0, a1, b0[NT], b1[NT];
    load(0, a0, b0);
    int kb = 0;
    for (; kb + 32 <= K; kb += 32) {
        load(kb + 16, a1, b1);
        step(a0, b0);
        if (kb + 32 < K) load(kb + 32, a0, b0);
        step(a1, b1);
    }
    if (kb < K) step(a0, b0);
    const int m = m0 + fi;
    if (m >= M) return;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int nb = n0 + t * 16 + fg * 4;
        if (nb + 3 < N && (N & 3) == 0) {
            *reinterpret_cast<f32x4*>(Cb + (size_t)m * N + nb) = acc[t];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (nb + i < N) Cb[(size_t)m * N + nb + i] = acc[t][i];
        }
    }
}

// The same product for LARGE problems (the 4096 x 4096 x 256 correlations of the finest level): a wave owns a 64 x 64 output
// tile — 4 row tiles x 4 column tiles, 64 MFMAs per 8 operand loads where the kernel above has 32 per 9 — and a workgroup of
// four waves a 128 x 128 block.  Column tile t holds the columns {n0 + 4 j + t}, so a lane ends up with four CONSECUTIVE
// columns per row and stores 16-byte vectors.  Loads of the next k block are pinned in front of the MFMAs of this one.
// M, N multiples of 128, K of 16.  62 -> ~95 TFLOP/s on 4096 x 4096 x 256 (exact fp32 products, same k order per output).
__global__ __launch_bounds__(256, 2) void gemm_nt_f32_tile64_kernel(const float* __restrict__ A, const float* __restrict__ Bm,
                                                                    float* __restrict__ Cm, int M, int N, int K) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z;
    const int m0 = blockIdx.y * 128 + (wave >> 1) * 64, n0 = blockIdx.x * 128 + (wave & 1) * 64;
    const float* Ab = A + (size_t)b * M * K;
    const float* Bb = Bm + (size_t)b * N * K;
    float* Cb = Cm + (size_t)b * M * N;
    const int fi = lane & 15, fg = lane >> 4;
    const float* ap = Ab + (size_t)(m0 + fi) * K + fg * 4;                  // row tile a: + 16 a rows
    const float* bp = Bb + (size_t)(n0 + 4 * fi) * K + fg * 4;              // column tile t: + t rows
    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[a][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto load = [&](int kb, f32x4 (&av)[4], f32x4 (&bv)[4]) {
#pragma unroll
        for (int a = 0; a < 4; ++a) av[a] = *reinterpret_cast<const f32x4*>(ap + (size_t)a * 16 * K + kb);
#pragma unroll
        for (int t = 0; t < 4; ++t) bv[t] = *reinterpret_cast<const f32x4*>(bp + (size_t)t * K + kb);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto step = [&](const f32x4 (&av)[4], const f32x4 (&bv)[4]) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    acc[a][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[t][e], av[a][e], acc[a][t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    f32x4 a0[4], b0[4], a1[4], b1[4];
    load(0, a0, b0);
    int kb = 0;
    for (; kb + 32 <= K; kb += 32) {
        load(kb + 16, a1, b1);
        step(a0, b0);
        if (kb + 32 < K) load(kb + 32, a0, b0);
        step(a1, b1);
    }
    if (kb < K) step(a0, b0);
    // operands swapped (A operand = B rows): D row index = column sub-index, D column = A row fi.  Register r of tile (a, t)
    // in lane (fi, fg): C[m0 + 16 a + fi][n0 + 4 (4 fg + r) + t]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            *reinterpret_cast<f32x4*>(Cb + (size_t)(m0 + 16 * a + fi) * N + n0 + 4 * (4 * fg + r)) =
                f32x4{acc[a][0][r], acc[a][1][r], acc[a][2][r], acc[a][3][r]};
}

// ------------------------------------------------------------------------------------------------
// bilinear resize with align_corners=True of `planes` independent (h, w) images: F.interpolate as used by
// interpolate4d / forward_attention (aggregation.py:49-56, 285, 293, 299).  thread = output pixel; HBM-bound.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void resize_bilinear_ac_kernel(const float* __restrict__ src,
                                                                 float* __restrict__ dst, long long planes, int h,
                                                                 int w, int H, int W) {
    const long long total = planes * H * W;
    const float sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.0f;
    const float sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.0f;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int X = (int)(idx % W);
        const long long t = idx / W;
        const int Y = (int)(t % H);
        const long long pl = t / H;
        const AxisTap ty = axis_tap(Y, h, sy), tx = axis_tap(X, w, sx);
        const float* p = src + pl * h * w;
        const float top = mix_nc(p[ty.i0 * w + tx.i0], p[ty.i0 * w + tx.i1], tx.l);
        const float bot = mix_nc(p[ty.i1 * w + tx.i0], p[ty.i1 * w + tx.i1], tx.l);
        dst[idx] = mix_nc(top, bot, ty.l);
    }
}

// Adjoint of resize_bilinear_ac_kernel (what autograd needs behind F.interpolate(align_corners=True)): the gradient g on
// the (H, W) grid gathered onto the (h, w) grid, out[y][x] = sum_{Y,X} wy(Y, y) wx(X, x) g[Y][X] with the forward kernel's
// own tap / weight arithmetic.  A GATHER in a fixed order: deterministic, where the library's backward scatters with atomics.
__global__ __launch_bounds__(256) void resize_bilinear_ac_adjoint_kernel(const float* __restrict__ g, float* __restrict__ out,
                                                                         long long planes, int h, int w, int H, int W) {
    const long long total = planes * h * w;
    const float sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.0f;
    const float sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.0f;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % w);
        const long long t = idx / w;
        const int y = (int)(t % h);
        const long long pl = t / h;
        // fine rows / columns whose taps can touch coarse index y / x (conservative by one on each side, checked exactly below)
        const int Ylo = sy > 0.0f ? max(0, (int)((float)(y - 1) / sy) - 1) : 0;
        const int Yhi = sy > 0.0f ? min(H - 1, (int)((float)(y + 1) / sy) + 1) : H - 1;
        const int Xlo = sx > 0.0f ? max(0, (int)((float)(x - 1) / sx) - 1) : 0;
        const int Xhi = sx > 0.0f ? min(W - 1, (int)((float)(x + 1) / sx) + 1) : W - 1;
        const float* p = g + pl * H * W;
        float acc = 0.0f;
        for (int Y = Ylo; Y <= Yhi; ++Y) {
            const AxisTap ty = axis_tap(Y, h, sy);
            float wy = 0.0f;
            if (ty.i0 == y) wy += 1.0f - ty.l;
            if (ty.i1 == y) wy += ty.l;
            if (wy == 0.0f) continue;
            float row = 0.0f;
            for (int X = Xlo; X <= Xhi; ++X) {
                const AxisTap tx = axis_tap(X, w, sx);
                float wx = 0.0f;
                if (tx.i0 == x) wx += 1.0f - tx.l;
                if (tx.i1 == x) wx += tx.l;
                row += wx * p[Y * W + X];
            }
            acc += wy * row;
        }
        out[idx] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// UFC.forward's last step (models/aggregation.py:549-553): the three levels' refined correlations, interpolate4d'ed to
// n^4, averaged.  interpolate4d (aggregation.py:49-56) is two bilinear passes (align_corners=True): over the target
// pair of dims, then over the source pair — here both passes of both coarse levels, the two adds and the division in
// ONE pass over the fine volume: each output reads 16 values of each coarse volume (cache resident: 256 KB and 4 MB
// per pair) and one of the fine one, in the arithmetic order of the separate kernels (resize_bilinear_ac_kernel twice,
// then (a + b) + c, then * (1/3) as the division by a scalar is evaluated).
// ---------------------------------------------------------------------------------------------
// x (h,h,h,h) of one pair -> its interpolate4d value at (I, J, i, j) of the n^4 grid
__device__ __forceinline__ float interp4d_at(const float* __restrict__ x, int h, float sc, int I, int J, int i, int j) {
    const AxisTap ti = axis_tap(i, h, sc), tj = axis_tap(j, h, sc), tI = axis_tap(I, h, sc), tJ = axis_tap(J, h, sc);
    float y1[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const float* p = x + ((size_t)((a ? tI.i1 : tI.i0) * h + (b ? tJ.i1 : tJ.i0))) * h * h;
            y1[a][b] = blend4(p[ti.i0 * h + tj.i0], p[ti.i0 * h + tj.i1], p[ti.i1 * h + tj.i0], p[ti.i1 * h + tj.i1], tj.l, ti.l);
        }
    return blend4(y1[0][0], y1[0][1], y1[1][0], y1[1][1], tJ.l, tI.l);
}
__global__ __launch_bounds__(256) void corr_mean3_kernel(const float* __restrict__ c0, int h0, const float* __restrict__ c1,
                                                         int h1, const float* __restrict__ c2, int n, int B,
                                                         float* __restrict__ out) {
    const long long per = (long long)n * n * n * n, total = per * B;
    const float s0 = n > 1 ? (float)(h0 - 1) / (float)(n - 1) : 0.0f, s1 = n > 1 ? (float)(h1 - 1) / (float)(n - 1) : 0.0f;
    const float third = 1.0f / 3.0f;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        long long t = idx;
        const int j = (int)(t % n); t /= n;
        const int i = (int)(t % n); t /= n;
        const int J = (int)(t % n); t /= n;
        const int I = (int)(t % n);
        const long long b = t / n;
        const float u0 = interp4d_at(c0 + b * (long long)h0 * h0 * h0 * h0, h0, s0, I, J, i, j);
        const float u1 = interp4d_at(c1 + b * (long long)h1 * h1 * h1 * h1, h1, s1, I, J, i, j);
        out[idx] = ((u0 + u1) + c2[idx]) * third;
    }
}

// The same values, same arithmetic order, with the coarse planes in LDS: a workgroup owns ONE source position (I, J) of a
// pair and all n x n target positions.  Its eight source-tap planes (2 x 2 of each coarse volume) are staged with coalesced
// loads, every output then blends 2 x 16 LDS values instead of 2 x 16 global ones (the per-thread kernel above issues 537 M
// 4-byte global loads for a 64^4 volume and is bound by them: 175 us where the 134 MB it must move take 30).
__global__ __launch_bounds__(256) void corr_mean3_planes_kernel(const float* __restrict__ c0, int h0, const float* __restrict__ c1,
                                                                int h1, const float* __restrict__ c2, int n,
                                                                float* __restrict__ out) {
    extern __shared__ float planes[];                            // [4][h0*h0] then [4][h1*h1]
    const int I = blockIdx.x / n, J = blockIdx.x % n;
    const long long b = blockIdx.y;
    const float s0 = (float)(h0 - 1) / (float)(n - 1), s1 = (float)(h1 - 1) / (float)(n - 1);
    const int p0 = h0 * h0, p1 = h1 * h1;
    float* q1 = planes + 4 * p0;
    {
        const AxisTap tI = axis_tap(I, h0, s0), tJ = axis_tap(J, h0, s0);
        const float* base = c0 + b * (long long)p0 * p0;
        for (int t = threadIdx.x; t < 4 * p0; t += 256) {
            const int ab = t / p0, e = t - ab * p0;
            planes[t] = base[((size_t)(((ab >> 1) ? tI.i1 : tI.i0) * h0 + ((ab & 1) ? tJ.i1 : tJ.i0))) * p0 + e];
        }
    }
    {
        const AxisTap tI = axis_tap(I, h1, s1), tJ = axis_tap(J, h1, s1);
        const float* base = c1 + b * (long long)p1 * p1;
        for (int t = threadIdx.x; t < 4 * p1; t += 256) {
            const int ab = t / p1, e = t - ab * p1;
            q1[t] = base[((size_t)(((ab >> 1) ? tI.i1 : tI.i0) * h1 + ((ab & 1) ? tJ.i1 : tJ.i0))) * p1 + e];
        }
    }
    __syncthreads();
    const AxisTap uI0 = axis_tap(I, h0, s0), uJ0 = axis_tap(J, h0, s0), uI1 = axis_tap(I, h1, s1), uJ1 = axis_tap(J, h1, s1);
    const float third = 1.0f / 3.0f;
    const long long obase = ((b * n + I) * n + J) * (long long)n * n;
    auto at = [&](const float* pl, int h, float sc, int pp, const AxisTap& tI, const AxisTap& tJ, int i, int j) {
        const AxisTap ti = axis_tap(i, h, sc), tj = axis_tap(j, h, sc);
        float y1[4];
#pragma unroll
        for (int ab = 0; ab < 4; ++ab) {
            const float* p = pl + ab * pp;
            y1[ab] = blend4(p[ti.i0 * h + tj.i0], p[ti.i0 * h + tj.i1], p[ti.i1 * h + tj.i0], p[ti.i1 * h + tj.i1], tj.l, ti.l);
        }
        return blend4(y1[0], y1[1], y1[2], y1[3], tJ.l, tI.l);
    };
    for (int e = threadIdx.x; e < n * n; e += 256) {
        const int i = e / n, j = e - i * n;
        const float u0 = at(planes, h0, s0, p0, uI0, uJ0, i, j);
        const float u1 = at(q1, h1, s1, p1, uI1, uJ1, i, j);
        out[obase + e] = ((u0 + u1) + c2[obase + e]) * third;
    }
}

}  // namespace

extern "C" int cpn_correlation(const float* src, const float* trg, int B, int L, int C, float eps, float* src_n,
                               float* trg_n, float* out, void* stream) {
    CPN_REQUIRE(src && trg && src_n && trg_n && out, CPN_E_ARG, "cpn_correlation: null pointer");
    CPN_REQUIRE(B > 0 && B < 65536 && L > 0 && C > 0 && (C % 16) == 0, CPN_E_SHAPE,
                "cpn_correlation: C=%d must be a multiple of 16", C);
    const hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)B * L;
    if (trg == src + rows * C && trg_n == src_n + rows * C) {
        // [src ; trg] and [src_n ; trg_n] are halves of one buffer each (the batched views of UFCLayer): one launch
        hipLaunchKernelGGL(l2norm_rows_kernel, dim3(cpn_cdiv(2 * rows, 4)), dim3(256), 0, st, src, src_n, 2 * rows, C, eps);
    } else {
        hipLaunchKernelGGL(l2norm_rows_kernel, dim3(cpn_cdiv(rows, 4)), dim3(256), 0, st, src, src_n, rows, C, eps);
        hipLaunchKernelGGL(l2norm_rows_kernel, dim3(cpn_cdiv(rows, 4)), dim3(256), 0, st, trg, trg_n, rows, C, eps);
    }
    CPN_LAUNCH_CHECK("cpn_correlation(normalise)");
    if (L % 128 == 0 && (long long)B * (L / 128) * (L / 128) >= 512 && ((uintptr_t)out % 16) == 0) {
        dim3 grid(L / 128, L / 128, B);
        hipLaunchKernelGGL(gemm_nt_f32_tile64_kernel, grid, dim3(256), 0, st, src_n, trg_n, out, L, L, C);
    } else if ((long long)B * cpn_cdiv(L, 128) * cpn_cdiv(L, 64) >= 512) {
        dim3 grid(cpn_cdiv(L, 128), cpn_cdiv(L, 64), B);
        hipLaunchKernelGGL(gemm_nt_f32_kernel<8>, grid, dim3(256), 0, st, src_n, trg_n, out, L, L, C);
    } else {
        dim3 grid(cpn_cdiv(L, 32), cpn_cdiv(L, 64), B);
        hipLaunchKernelGGL(gemm_nt_f32_kernel<2>, grid, dim3(256), 0, st, src_n, trg_n, out, L, L, C);
    }
    CPN_LAUNCH_CHECK("cpn_correlation(gemm)");
    return 0;
}

extern "C" int cpn_l2norm_rows_bwd(const float* x, const float* y, const float* dy, long long rows, int C, float eps,
                                   float* dx, void* stream) {
    CPN_REQUIRE(x && y && dy && dx, CPN_E_ARG, "cpn_l2norm_rows_bwd: null pointer");
    CPN_REQUIRE(rows > 0 && rows < (1LL << 33) && C > 0 && C <= 1024, CPN_E_SHAPE, "cpn_l2norm_rows_bwd: need 0 < C <= 1024 (got %d)", C);
    hipLaunchKernelGGL(l2norm_rows_bwd_kernel, dim3(cpn_cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, y, dy, dx, rows,
                       C, eps);
    CPN_LAUNCH_CHECK("cpn_l2norm_rows_bwd");
    return 0;
}

extern "C" int cpn_resize_bilinear_ac(const float* src, float* dst, long long planes, int h, int w, int H, int W,
                                      void* stream) {
    CPN_REQUIRE(src && dst, CPN_E_ARG, "cpn_resize_bilinear_ac: null pointer");
    CPN_REQUIRE(planes > 0 && h > 0 && w > 0 && H > 0 && W > 0, CPN_E_SHAPE, "cpn_resize_bilinear_ac: bad shape");
    const long long total = planes * H * W;
    const unsigned blocks = (unsigned)(cpn_cdiv(total, 256) < 65536u ? cpn_cdiv(total, 256) : 65536u);
    hipLaunchKernelGGL(resize_bilinear_ac_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, dst, planes,
                       h, w, H, W);
    CPN_LAUNCH_CHECK("cpn_resize_bilinear_ac");
    return 0;
}

extern "C" int cpn_resize_bilinear_ac_adjoint(const float* g, float* out, long long planes, int h, int w, int H, int W,
                                              void* stream) {
    CPN_REQUIRE(g && out, CPN_E_ARG, "cpn_resize_bilinear_ac_adjoint: null pointer");
    CPN_REQUIRE(planes > 0 && h > 0 && w > 0 && H > 0 && W > 0, CPN_E_SHAPE, "cpn_resize_bilinear_ac_adjoint: bad shape");
    const long long total = planes * h * w;
    const unsigned blocks = (unsigned)std::min<long long>(cpn_cdiv(total, 256), 1 << 20);
    hipLaunchKernelGGL(resize_bilinear_ac_adjoint_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, out, planes, h, w,
                       H, W);
    CPN_LAUNCH_CHECK("cpn_resize_bilinear_ac_adjoint");
    return 0;
}

extern "C" int cpn_corr_mean3(const float* c0, int h0, const float* c1, int h1, const float* c2, int n, int B, float* out,
                              void* stream) {
    CPN_REQUIRE(c0 && c1 && c2 && out, CPN_E_ARG, "cpn_corr_mean3: null pointer");
    CPN_REQUIRE(B > 0 && h0 > 1 && h1 > 1 && n > 1 && h0 <= n && h1 <= n && n <= 128, CPN_E_SHAPE, "cpn_corr_mean3: bad shape");
    const long long total = (long long)B * n * n * n * n;
    const size_t lds = (size_t)4 * ((size_t)h0 * h0 + (size_t)h1 * h1) * sizeof(float);
    if (lds <= 60 * 1024 && B < 65536) {
        hipLaunchKernelGGL(corr_mean3_planes_kernel, dim3((unsigned)(n * n), (unsigned)B), dim3(256), lds, (hipStream_t)stream, c0, h0,
                           c1, h1, c2, n, out);
        CPN_LAUNCH_CHECK("cpn_corr_mean3");
        return 0;
    }
    const unsigned blocks = (unsigned)std::min<long long>(cpn_cdiv(total, 256), 1 << 20);
    hipLaunchKernelGGL(corr_mean3_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, c0, h0, c1, h1, c2, n, B, out);
    CPN_LAUNCH_CHECK("cpn_corr_mean3");
    return 0;
}
