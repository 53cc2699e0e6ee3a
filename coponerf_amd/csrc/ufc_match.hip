// K8 — matching on the correlation volumes of UFC (get_z path), forward and backward:
//   cpn_soft_argmax_pair aggregation.soft_argmax in both directions (models/aggregation.py:119-144, 555-560)
//   cpn_dual_softmax     the dual softmax of the cross attention (models/backbone.py:296-330)
#include <algorithm>
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// soft-argmax with temperature beta over the 4-D correlation c (B, S = h*h, T = h*h)
//   rows: for every source pixel s, softmax over t   -> expected (x, y) of the target   (t_to_s maps)
//   cols: for every target pixel t, softmax over s   -> expected (x, y) of the source   (s_to_t maps)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lin11(int i, int n) { return -1.0f + (2.0f / (float)(n - 1)) * (float)i; }

__global__ __launch_bounds__(256) void soft_argmax_rows_kernel(const float* __restrict__ c, int h, float beta,
                                                               float* __restrict__ out) {
    const int T = h * h;
    const int b = blockIdx.y, s = blockIdx.x;
    const float* row = c + ((size_t)b * T + s) * T;
    __shared__ float red[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float m = -INFINITY;
    for (int t = threadIdx.x; t < T; t += 256) m = fmaxf(m, row[t]);
    m = wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float se = 0.f, sx = 0.f, sy = 0.f;
    {   // (x, y) of the position advanced by the stride instead of t % h and t / h per element
        int x = threadIdx.x % h, y = threadIdx.x / h;
        const int dx = 256 % h, dy = 256 / h;
        for (int t = threadIdx.x; t < T; t += 256) {
            const float e = expf((row[t] - m) / beta);
            se += e;
            sx += e * lin11(x, h);
            sy += e * lin11(y, h);
            x += dx; y += dy;
            if (x >= h) { x -= h; ++y; }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        se += __shfl_xor(se, off);
        sx += __shfl_xor(sx, off);
        sy += __shfl_xor(sy, off);
    }
    if (lane == 0) { red[4 + wave] = se; red[8 + wave] = sx; red[12 + wave] = sy; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float tot = (red[4] + red[5]) + (red[6] + red[7]);
        out[((size_t)b * 2 + 0) * T + s] = ((red[8] + red[9]) + (red[10] + red[11])) / tot;
        out[((size_t)b * 2 + 1) * T + s] = ((red[12] + red[13]) + (red[14] + red[15])) / tot;
    }
}

// Column-direction reductions over a (rows x T) matrix: block = CR_COLS columns x CR_GROUPS row groups (a wave reads four
// 64-byte row segments per instruction), online softmax per thread, partials merged through LDS.  With 64 columns x 4
// groups (round 1) a 4096 x 4096 matrix was 64 workgroups whose threads each walked 1024 rows: 0.39 ms for 67 MB.
constexpr int CR_COLS = 16, CR_GROUPS = 64;
__global__ __launch_bounds__(CR_COLS * CR_GROUPS) void soft_argmax_cols_kernel(const float* __restrict__ c, int h, float beta,
                                                                               float* __restrict__ out) {
    const int T = h * h;
    const int b = blockIdx.y;
    const int l = threadIdx.x % CR_COLS, g = threadIdx.x / CR_COLS;
    const int t = blockIdx.x * CR_COLS + l;
    __shared__ float part[CR_GROUPS][4][CR_COLS];
    float m = -INFINITY, se = 0.f, sx = 0.f, sy = 0.f;
    if (t < T) {
        const float* col = c + (size_t)b * T * T + t;
        int x = g % h, y = g / h;                              // (s % h, s / h), advanced by the stride
        const int dx = CR_GROUPS % h, dy = CR_GROUPS / h;
        for (int s = g; s < T; s += CR_GROUPS) {
            const float v = col[(size_t)s * T];
            if (v > m) {
                const float r = expf((m - v) / beta);
                se *= r; sx *= r; sy *= r;
                m = v;
            }
            const float e = expf((v - m) / beta);
            se += e;
            sx += e * lin11(x, h);
            sy += e * lin11(y, h);
            x += dx; y += dy;
            if (x >= h) { x -= h; ++y; }
        }
    }
    part[g][0][l] = m; part[g][1][l] = se; part[g][2][l] = sx; part[g][3][l] = sy;
    __syncthreads();
    if (g == 0 && t < T) {
        float M = -INFINITY;
        for (int q = 0; q < CR_GROUPS; ++q) M = fmaxf(M, part[q][0][l]);
        float E = 0.f, X = 0.f, Y = 0.f;
        for (int q = 0; q < CR_GROUPS; ++q) {
            const float r = part[q][0][l] == -INFINITY ? 0.0f : expf((part[q][0][l] - M) / beta);
            E += part[q][1][l] * r; X += part[q][2][l] * r; Y += part[q][3][l] * r;
        }
        out[((size_t)b * 2 + 0) * T + t] = X / E;
        out[((size_t)b * 2 + 1) * T + t] = Y / E;
    }
}

// backward of the two soft-argmax directions: with p = softmax over the reduced index of c / beta and (ox, oy) the
// forward outputs, d c = p / beta * (gx * (x - ox) + gy * (y - oy)).  Rows first (writes dc), columns second (adds).
__global__ __launch_bounds__(256) void soft_argmax_rows_bwd_kernel(const float* __restrict__ c, int h, float beta,
                                                                   const float* __restrict__ out,
                                                                   const float* __restrict__ gout,
                                                                   float* __restrict__ dc) {
    const int T = h * h;
    const int b = blockIdx.y, s = blockIdx.x;
    const float* row = c + ((size_t)b * T + s) * T;
    float* drow = dc + ((size_t)b * T + s) * T;
    __shared__ float red[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float m = -INFINITY;
    for (int t = threadIdx.x; t < T; t += 256) m = fmaxf(m, row[t]);
    m = wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float se = 0.f;
    for (int t = threadIdx.x; t < T; t += 256) se += expf((row[t] - m) / beta);
    se = wave_sum(se);
    if (lane == 0) red[4 + wave] = se;
    __syncthreads();
    const float inv = 1.0f / (((red[4] + red[5]) + (red[6] + red[7])) * beta);
    const float ox = out[((size_t)b * 2 + 0) * T + s], oy = out[((size_t)b * 2 + 1) * T + s];
    const float gx = gout[((size_t)b * 2 + 0) * T + s], gy = gout[((size_t)b * 2 + 1) * T + s];
    for (int t = threadIdx.x; t < T; t += 256) {
        const float p = expf((row[t] - m) / beta) * inv;
        drow[t] = p * (gx * (lin11(t % h, h) - ox) + gy * (lin11(t / h, h) - oy));
    }
}

__global__ __launch_bounds__(256) void soft_argmax_cols_bwd_kernel(const float* __restrict__ c, int h, float beta,
                                                                   const float* __restrict__ out,
                                                                   const float* __restrict__ gout,
                                                                   float* __restrict__ dc) {
    const int T = h * h;
    const int b = blockIdx.y;
    const int l = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + l;
    __shared__ float part[4][2][64];
    __shared__ float fin[2][64];
    float m = -INFINITY, se = 0.f;
    const float* col = c + (size_t)b * T * T + t;
    if (t < T)
        for (int s = g; s < T; s += 4) {
            const float v = col[(size_t)s * T];
            if (v > m) { se *= expf((m - v) / beta); m = v; }
            se += expf((v - m) / beta);
        }
    part[g][0][l] = m; part[g][1][l] = se;
    __syncthreads();
    if (g == 0) {
        const float M = fmaxf(fmaxf(part[0][0][l], part[1][0][l]), fmaxf(part[2][0][l], part[3][0][l]));
        float E = 0.f;
        for (int q = 0; q < 4; ++q) E += part[q][1][l] * expf((part[q][0][l] - M) / beta);
        fin[0][l] = M; fin[1][l] = 1.0f / (E * beta);
    }
    __syncthreads();
    if (t >= T) return;
    const float M = fin[0][l], inv = fin[1][l];
    const float ox = out[((size_t)b * 2 + 0) * T + t], oy = out[((size_t)b * 2 + 1) * T + t];
    const float gx = gout[((size_t)b * 2 + 0) * T + t], gy = gout[((size_t)b * 2 + 1) * T + t];
    float* dcol = dc + (size_t)b * T * T + t;
    for (int s = g; s < T; s += 4) {
        const float q = expf((col[(size_t)s * T] - M) / beta) * inv;
        dcol[(size_t)s * T] += q * (gx * (lin11(s % h, h) - ox) + gy * (lin11(s / h, h) - oy));
    }
}

// ------------------------------------------------------------------------------------------------
// dual softmax of the "fundamental-matrix" cross attention (models/backbone.py:296-330):
//   f[b,i,j] = softmax_j(a[b,i,:])[j] * softmax_i(a[b,:,j])[i]        a: (B, L, M), up to 4096 x 4096
// torch runs two softmax kernels (the strided one at ~230 GB/s) and a product.  Here: row statistics (max, sum) with
// one wave per row, column statistics with 64 coalesced columns per workgroup and an online softmax down the rows, and
// one elementwise pass f = exp(2a - rmax_i - cmax_j) / (rsum_i * csum_j).  The statistics are kept for the backward:
//   da = 2 f df - r * Srow_i - c * Scol_j,   Srow_i = sum_j f df,  Scol_j = sum_i f df,  r / c the two softmaxes.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void row_stats_kernel(const float* __restrict__ a, const float* __restrict__ w,
                                                        long long rows, int M, float* __restrict__ stat, int mode) {
    // mode 0: stat[row] = (max, sum exp(a - max));  mode 1: stat[row] = sum a*w   (w = second operand, same shape)
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* ar = a + (size_t)row * M;
    if (mode == 0) {
        float m = -INFINITY;
        for (int j = lane; j < M; j += 64) m = fmaxf(m, ar[j]);
        m = wave_max(m);
        float se = 0.f;
        for (int j = lane; j < M; j += 64) se += expf(ar[j] - m);
        se = wave_sum(se);
        if (lane == 0) { stat[row * 2] = m; stat[row * 2 + 1] = se; }
    } else {
        const float* wr = w + (size_t)row * M;
        float sacc = 0.f;
        for (int j = lane; j < M; j += 64) sacc += ar[j] * wr[j];
        sacc = wave_sum(sacc);
        if (lane == 0) stat[row] = sacc;
    }
}

// workgroup = CR_COLS columns x CR_GROUPS row groups, partials merged through LDS (see soft_argmax_cols_kernel)
__global__ __launch_bounds__(CR_COLS * CR_GROUPS) void col_stats_kernel(const float* __restrict__ a, const float* __restrict__ w,
                                                                        int L, int M, float* __restrict__ stat, int mode) {
    const int b = blockIdx.y;
    const int l = threadIdx.x % CR_COLS, g = threadIdx.x / CR_COLS;
    const int j = blockIdx.x * CR_COLS + l;
    __shared__ float part[CR_GROUPS][2][CR_COLS];
    float m = -INFINITY, se = 0.f;
    if (j < M) {
        const float* col = a + (size_t)b * L * M + j;
        if (mode == 0) {
            for (int i = g; i < L; i += CR_GROUPS) {
                const float v = col[(size_t)i * M];
                if (v > m) { se *= expf(m - v); m = v; }
                se += expf(v - m);
            }
        } else {
            const float* wc = w + (size_t)b * L * M + j;
            for (int i = g; i < L; i += CR_GROUPS) se += col[(size_t)i * M] * wc[(size_t)i * M];
        }
    }
    part[g][0][l] = m; part[g][1][l] = se;
    __syncthreads();
    if (g == 0 && j < M) {
        if (mode == 0) {
            float Mx = -INFINITY;
            for (int q = 0; q < CR_GROUPS; ++q) Mx = fmaxf(Mx, part[q][0][l]);
            float E = 0.f;
            for (int q = 0; q < CR_GROUPS; ++q)
                E += part[q][0][l] == -INFINITY ? 0.0f : part[q][1][l] * expf(part[q][0][l] - Mx);
            stat[((size_t)b * M + j) * 2] = Mx;
            stat[((size_t)b * M + j) * 2 + 1] = E;
        } else {
            float E = 0.f;
            for (int q = 0; q < CR_GROUPS; ++q) E += part[q][1][l];
            stat[(size_t)b * M + j] = E;
        }
    }
}

__global__ __launch_bounds__(256) void dual_softmax_apply_kernel(const float* __restrict__ a,
                                                                 const float* __restrict__ rstat,
                                                                 const float* __restrict__ cstat, int L, int M,
                                                                 long long total, float* __restrict__ f) {
    // a workgroup walks whole rows (row = b*L + i): the element's (row, column, batch) came out of three 64-bit divisions
    // per element before, which cost more than its two exponentials (0.18 ms for a 268 MB matrix that streams in 0.09)
    const long long rows = total / M;
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const long long b = row / L;
        const float rm = rstat[row * 2], rs = rstat[row * 2 + 1];
        const float* cst = cstat + b * M * 2;
        const float* ar = a + row * M;
        float* fr = f + row * M;
        for (int j = threadIdx.x; j < M; j += blockDim.x) {
            const float cm = cst[j * 2], cs = cst[j * 2 + 1];
            const float v = ar[j];
            fr[j] = (expf(v - rm) / rs) * (expf(v - cm) / cs);
        }
    }
}

__global__ __launch_bounds__(256) void dual_softmax_bwd_apply_kernel(
    const float* __restrict__ a, const float* __restrict__ rstat, const float* __restrict__ cstat,
    const float* __restrict__ df, const float* __restrict__ srow, const float* __restrict__ scol, int L, int M,
    long long total, float* __restrict__ da) {
    const long long rows = total / M;
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {        // whole rows per workgroup: see dual_softmax_apply_kernel
        const long long b = row / L;
        const float rm = rstat[row * 2], rs = rstat[row * 2 + 1], sr = srow[row];
        const float* cst = cstat + b * M * 2;
        const float* scl = scol + b * M;
        const size_t off = (size_t)row * M;
        for (int j = threadIdx.x; j < M; j += blockDim.x) {
            const float v = a[off + j];
            const float r = expf(v - rm) / rs;
            const float c = expf(v - cst[j * 2]) / cst[j * 2 + 1];
            da[off + j] = 2.0f * r * c * df[off + j] - r * sr - c * scl[j];
        }
    }
}

}  // namespace

extern "C" int cpn_soft_argmax_pair(const float* c, int B, int h, float beta, float* t_to_s, float* s_to_t,
                                    void* stream) {
    CPN_REQUIRE(c && t_to_s && s_to_t, CPN_E_ARG, "cpn_soft_argmax_pair: null pointer");
    CPN_REQUIRE(B > 0 && B < 65536 && h > 1 && beta > 0.f, CPN_E_SHAPE, "cpn_soft_argmax_pair: bad shape");
    const hipStream_t st = (hipStream_t)stream;
    const int T = h * h;
    hipLaunchKernelGGL(soft_argmax_rows_kernel, dim3(T, B), dim3(256), 0, st, c, h, beta, t_to_s);
    hipLaunchKernelGGL(soft_argmax_cols_kernel, dim3(cpn_cdiv(T, CR_COLS), B), dim3(CR_COLS * CR_GROUPS), 0, st, c, h, beta,
                       s_to_t);
    CPN_LAUNCH_CHECK("cpn_soft_argmax_pair");
    return 0;
}

extern "C" int cpn_soft_argmax_pair_bwd(const float* c, int B, int h, float beta, const float* t_to_s,
                                        const float* s_to_t, const float* g_t_to_s, const float* g_s_to_t, float* dc,
                                        void* stream) {
    CPN_REQUIRE(c && t_to_s && s_to_t && g_t_to_s && g_s_to_t && dc, CPN_E_ARG, "cpn_soft_argmax_pair_bwd: null pointer");
    CPN_REQUIRE(B > 0 && B < 65536 && h > 1 && beta > 0.f, CPN_E_SHAPE, "cpn_soft_argmax_pair_bwd: bad shape");
    const hipStream_t st = (hipStream_t)stream;
    const int T = h * h;
    hipLaunchKernelGGL(soft_argmax_rows_bwd_kernel, dim3(T, B), dim3(256), 0, st, c, h, beta, t_to_s, g_t_to_s, dc);
    hipLaunchKernelGGL(soft_argmax_cols_bwd_kernel, dim3(cpn_cdiv(T, 64), B), dim3(256), 0, st, c, h, beta, s_to_t,
                       g_s_to_t, dc);
    CPN_LAUNCH_CHECK("cpn_soft_argmax_pair_bwd");
    return 0;
}

extern "C" int cpn_dual_softmax(const float* a, int B, int L, int M, float* rstat, float* cstat, float* f,
                                void* stream) {
    CPN_REQUIRE(a && rstat && cstat && f, CPN_E_ARG, "cpn_dual_softmax: null pointer");
    CPN_REQUIRE(B > 0 && B < 65536 && L > 0 && M > 0, CPN_E_SHAPE, "cpn_dual_softmax: bad shape");
    const hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)B * L, total = rows * M;
    hipLaunchKernelGGL(row_stats_kernel, dim3(cpn_cdiv(rows, 4)), dim3(256), 0, st, a, (const float*)nullptr, rows, M, rstat, 0);
    hipLaunchKernelGGL(col_stats_kernel, dim3(cpn_cdiv(M, CR_COLS), B), dim3(CR_COLS * CR_GROUPS), 0, st, a, (const float*)nullptr,
                       L, M, cstat, 0);
    const unsigned blocks = (unsigned)std::min<long long>(cpn_cdiv(total, 256), 16384);
    hipLaunchKernelGGL(dual_softmax_apply_kernel, dim3(blocks), dim3(256), 0, st, a, rstat, cstat, L, M, total, f);
    CPN_LAUNCH_CHECK("cpn_dual_softmax");
    return 0;
}

extern "C" int cpn_dual_softmax_bwd(const float* a, const float* rstat, const float* cstat, const float* f,
                                    const float* df, int B, int L, int M, float* srow, float* scol, float* da,
                                    void* stream) {
    CPN_REQUIRE(a && rstat && cstat && f && df && srow && scol && da, CPN_E_ARG, "cpn_dual_softmax_bwd: null pointer");
    CPN_REQUIRE(B > 0 && B < 65536 && L > 0 && M > 0, CPN_E_SHAPE, "cpn_dual_softmax_bwd: bad shape");
    const hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)B * L, total = rows * M;
    hipLaunchKernelGGL(row_stats_kernel, dim3(cpn_cdiv(rows, 4)), dim3(256), 0, st, f, df, rows, M, srow, 1);
    hipLaunchKernelGGL(col_stats_kernel, dim3(cpn_cdiv(M, CR_COLS), B), dim3(CR_COLS * CR_GROUPS), 0, st, f, df, L, M, scol, 1);
    const unsigned blocks = (unsigned)std::min<long long>(cpn_cdiv(total, 256), 16384);
    hipLaunchKernelGGL(dual_softmax_bwd_apply_kernel, dim3(blocks), dim3(256), 0, st, a, rstat, cstat, df, srow, scol, L, M,
                       total, da);
    CPN_LAUNCH_CHECK("cpn_dual_softmax_bwd");
    return 0;
}
