// K6 — the 4-D convolution of UFC (get_z path).
//   cpn_conv4d_gn_relu   conv4d.Conv4d (+ MaxPool4d for stride > 1) + GroupNorm(1 group) + ReLU
//                        (/root/reference models/conv4d.py:7-30, 57-163): 63 calls per get_z
//   cpn_conv4d_dgrad, cpn_gn_relu_bwd, cpn_transpose_pairs   its stride-1 data gradient, the GroupNorm + ReLU backward and
//                        the (query, support) pair swap around it
// The reference spends 44 % of get_z in einops `rearrange` copies of 6-D tensors around stock Conv2d / MaxPool2d
// calls; here both separable branches, the pooling, both biases and the GroupNorm statistics are one pass over
// the volume with direct 6-D indexing — no transposed copies.  All of it is HBM/L2-bound streaming work
// (volumes 16^4 x {8,32} ch = 2-8 MB): coalescing along the innermost support axis, one scalar-broadcast weight per
// (out-channel, in-channel, tap).
#include <algorithm>
#include <cstdlib>

#include "common.h"
#include "conv4d_geometry.h"

namespace {

// GroupNorm statistics of sample b, DETERMINISTIC (round 3; the 32-slot atomicAdd scheme of round 2 summed the workgroup
// partials in whatever order they arrived: two runs of get_z differed in the last bits).  stats layout (doubles):
//   [2b], [2b+1]        sum / sum of squares of sample b, written once by the LAST workgroup of the sample to finish
//   [2B + b]            arrival counter (zero on entry), bits of an unsigned long long
//   [3B + 2(b W + w)..] partial pair of workgroup w of sample b, W = gridDim.x * gridDim.y
// Every workgroup publishes its pair with returning exchanges (performed at the device-coherent level, like the atomic
// adds they replace; the returned values are consumed, so they have completed before the counter is bumped), the
// workgroup that draws the last ticket re-reads all W pairs with device-scope loads and sums them in a FIXED order
// (thread t takes w = t, t + 256, ...; then a fixed LDS tree).  Must be called by all 256 threads of the workgroup.
__device__ __forceinline__ void gn_publish(double s1, double s2, double* __restrict__ stats, int b) {
    __shared__ int last_flag;
    __shared__ double tree[2][256];
    const unsigned W = gridDim.x * gridDim.y, me = blockIdx.x + gridDim.x * blockIdx.y, B = gridDim.z;
    unsigned long long* part = reinterpret_cast<unsigned long long*>(stats + 3 * (size_t)B + 2 * ((size_t)b * W));
    if (threadIdx.x == 0) {
        const unsigned long long o1 = __hip_atomic_exchange(part + 2 * me, (unsigned long long)__double_as_longlong(s1),
                                                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long o2 = __hip_atomic_exchange(part + 2 * me + 1, (unsigned long long)__double_as_longlong(s2),
                                                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned zero;                                        // 0, but only known once both exchanges have returned
        asm volatile("v_and_b32 %0, 0, %1\n\tv_and_b32 %0, %0, %2" : "=&v"(zero) : "v"((unsigned)o1), "v"((unsigned)o2));
        unsigned long long* cnt = reinterpret_cast<unsigned long long*>(stats + 2 * (size_t)B + b);
        const unsigned long long ticket = __hip_atomic_fetch_add(cnt, 1ULL + zero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_flag = ticket == (unsigned long long)W - 1;
    }
    __syncthreads();
    if (!last_flag) return;
    double a1 = 0.0, a2 = 0.0;
    for (unsigned w = threadIdx.x; w < W; w += 256) {
        a1 += __longlong_as_double((long long)__hip_atomic_load(part + 2 * w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        a2 += __longlong_as_double((long long)__hip_atomic_load(part + 2 * w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    tree[0][threadIdx.x] = a1;
    tree[1][threadIdx.x] = a2;
    __syncthreads();
    for (int n = 128; n > 0; n >>= 1) {
        if ((int)threadIdx.x < n) {
            tree[0][threadIdx.x] += tree[0][threadIdx.x + n];
            tree[1][threadIdx.x] += tree[1][threadIdx.x + n];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats[2 * (size_t)b] = tree[0][0];
        stats[2 * (size_t)b + 1] = tree[1][0];
    }
}

// the end of the VALU Conv4d kernels (the MFMA one keeps its own copy: its schedule moves with it): each thread's (sum, sum of squares) over the wave (xor butterfly), the four waves in the
// order 0 .. 3, then gn_publish.  Must be called by all 256 threads of the workgroup.
__device__ __forceinline__ void gn_publish_block(double s1, double s2, double* __restrict__ stats, int b) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_xor(s1, off);
        s2 += __shfl_xor(s2, off);
    }
    __shared__ double red[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave * 2] = s1; red[wave * 2 + 1] = s2; }
    __syncthreads();
    gn_publish(red[0] + red[2] + red[4] + red[6], red[1] + red[3] + red[5] + red[7], stats, b);
}

// ------------------------------------------------------------------------------------------------
// conv4d: y[b,o,qy,qx,sy,sx] = bq[o] + bs[o]
//        + sum_{c,i,j} Wq[o,c,i,j] * Ps(x)[b,c, qy*s+i-p, qx*s+j-p, sy, sx]      (query branch, support dims pooled)
//        + sum_{c,i,j} Ws[o,c,i,j] * Pq(x)[b,c, qy, qx, sy*s+i-p, sx*s+j-p]      (support branch, query dims pooled)
// thread = one output position, blockIdx.y = output channel (uniform -> scalar weight loads), blockIdx.z = batch
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv4d_kernel(const float* __restrict__ x, const float* __restrict__ wq,
                                                     const float* __restrict__ bq, const float* __restrict__ ws,
                                                     const float* __restrict__ bs, int Cin, int Hq, int Wq, int Hs,
                                                     int Ws, int k, int s, int p, int Oq, int Pq_, int Os, int Ps_,
                                                     float* __restrict__ y, double* __restrict__ stats) {
    // Oq x Pq_ = output query dims, Os x Ps_ = output support dims
    const int o = blockIdx.y, b = blockIdx.z, Cout = gridDim.y;
    const long long npos = (long long)Oq * Pq_ * Os * Ps_;
    const long long pos = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float val = 0.0f;
    const bool active = pos < npos;
    if (active) {
        int sx = (int)(pos % Ps_);
        long long t = pos / Ps_;
        const int sy = (int)(t % Os); t /= Os;
        const int qx = (int)(t % Pq_);
        const int qy = (int)(t / Pq_);
        const size_t cstride = (size_t)Hq * Wq * Hs * Ws;
        const float* xb = x + (size_t)b * Cin * cstride;
        float acc = bq[o] + bs[o];
        for (int c = 0; c < Cin; ++c) {
            const float* xc = xb + c * cstride;
            const float* wqc = wq + ((size_t)o * Cin + c) * k * k;
            const float* wsc = ws + ((size_t)o * Cin + c) * k * k;
            for (int i = 0; i < k; ++i)
                for (int j = 0; j < k; ++j) {
                    // ---- query branch: conv over (Hq, Wq), support dims max-pooled by s (ceil mode)
                    const int Y = qy * s + i - p, X = qx * s + j - p;
                    if (Y >= 0 && Y < Hq && X >= 0 && X < Wq) {
                        const float* base = xc + ((size_t)Y * Wq + X) * Hs * Ws;
                        float m = -INFINITY;
                        for (int dy = 0; dy < s; ++dy)
                            for (int dx = 0; dx < s; ++dx) {
                                const int yy = sy * s + dy, xx = sx * s + dx;
                                if (yy < Hs && xx < Ws) m = fmaxf(m, base[(size_t)yy * Ws + xx]);
                            }
                        acc += wqc[i * k + j] * m;
                    }
                    // ---- support branch: conv over (Hs, Ws), query dims max-pooled by s
                    const int U = sy * s + i - p, Vv = sx * s + j - p;
                    if (U >= 0 && U < Hs && Vv >= 0 && Vv < Ws) {
                        float m = -INFINITY;
                        for (int dy = 0; dy < s; ++dy)
                            for (int dx = 0; dx < s; ++dx) {
                                const int yy = qy * s + dy, xx = qx * s + dx;
                                if (yy < Hq && xx < Wq) m = fmaxf(m, xc[(((size_t)yy * Wq + xx) * Hs + U) * Ws + Vv]);
                            }
                        acc += wsc[i * k + j] * m;
                    }
                }
        }
        val = acc;
        y[((size_t)b * Cout + o) * npos + pos] = acc;
    }
    // GroupNorm statistics of the whole (C, volume) slab of sample b, accumulated in double
    double s1 = active ? (double)val : 0.0, s2 = active ? (double)val * val : 0.0;
    gn_publish_block(s1, s2, stats, b);
}

// Strided layers (k3 s2 on 32^4, k5 s4 on 64^4): the kernel above re-evaluates the s x s max-pool window for every tap
// (k*k*s*s reads per output, channel and branch).  With a scratch buffer the two pooled volumes are formed once
//   Ps[b,c,Y,X,sy',sx'] = max_{dy,dx<s} x[b,c,Y,X,sy'*s+dy,sx'*s+dx]     (query branch: support dims pooled)
//   Pq[b,c,qy',qx',U,V] = max_{dy,dx<s} x[b,c,qy'*s+dy,qx'*s+dx,U,V]     (support branch: query dims pooled)
// and the convolution reads k*k values per output, channel and branch.
__global__ __launch_bounds__(256) void pool_support_kernel(const float* __restrict__ x, int Hs, int Ws, int s, int Os,
                                                           int Ps_, long long planes, float* __restrict__ out) {
    // planes = B*Cin*Hq*Wq, each an (Hs,Ws) -> (Os,Ps_) max-pool with ceil mode
    const long long total = planes * Os * Ps_;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int sx = (int)(i % Ps_);
        long long t = i / Ps_;
        const int sy = (int)(t % Os);
        const long long pl = t / Os;
        const float* base = x + pl * Hs * Ws;
        float m = -INFINITY;
        for (int dy = 0; dy < s; ++dy)
            for (int dx = 0; dx < s; ++dx) {
                const int yy = sy * s + dy, xx = sx * s + dx;
                if (yy < Hs && xx < Ws) m = fmaxf(m, base[(size_t)yy * Ws + xx]);
            }
        out[i] = m;
    }
}

__global__ __launch_bounds__(256) void pool_query_kernel(const float* __restrict__ x, int Hq, int Wq, int Hs, int Ws,
                                                         int s, int Oq, int Pq_, long long bc, float* __restrict__ out) {
    // out[bc, qy', qx', U, V]; consecutive threads walk (U,V): contiguous reads of s*s planes
    const long long P = (long long)Hs * Ws, total = bc * Oq * Pq_ * P;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long uv = i % P;
        long long t = i / P;
        const int qx = (int)(t % Pq_); t /= Pq_;
        const int qy = (int)(t % Oq);
        const long long c = t / Oq;
        const float* base = x + c * Hq * Wq * P + uv;
        float m = -INFINITY;
        for (int dy = 0; dy < s; ++dy)
            for (int dx = 0; dx < s; ++dx) {
                const int yy = qy * s + dy, xx = qx * s + dx;
                if (yy < Hq && xx < Wq) m = fmaxf(m, base[((size_t)yy * Wq + xx) * P]);
            }
        out[i] = m;
    }
}

// same contract as conv4d_kernel, reading the pooled volumes
__global__ __launch_bounds__(256) void conv4d_pooled_kernel(const float* __restrict__ ps, const float* __restrict__ pq,
                                                            const float* __restrict__ wq, const float* __restrict__ bq,
                                                            const float* __restrict__ ws, const float* __restrict__ bs,
                                                            int Cin, int Hq, int Wq, int Hs, int Ws, int k, int s, int p,
                                                            int Oq, int Pq_, int Os, int Ps_, float* __restrict__ y,
                                                            double* __restrict__ stats) {
    const int o = blockIdx.y, b = blockIdx.z, Cout = gridDim.y;
    const long long npos = (long long)Oq * Pq_ * Os * Ps_;
    const long long pos = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float val = 0.0f;
    const bool active = pos < npos;
    if (active) {
        int sx = (int)(pos % Ps_);
        long long t = pos / Ps_;
        const int sy = (int)(t % Os); t /= Os;
        const int qx = (int)(t % Pq_);
        const int qy = (int)(t / Pq_);
        const size_t ps_c = (size_t)Hq * Wq * Os * Ps_, pq_c = (size_t)Oq * Pq_ * Hs * Ws;
        const float* psb = ps + (size_t)b * Cin * ps_c;
        const float* pqb = pq + (size_t)b * Cin * pq_c;
        float acc = bq[o] + bs[o];
        for (int c = 0; c < Cin; ++c) {
            const float* wqc = wq + ((size_t)o * Cin + c) * k * k;
            const float* wsc = ws + ((size_t)o * Cin + c) * k * k;
            for (int i = 0; i < k; ++i)
                for (int j = 0; j < k; ++j) {
                    const int Y = qy * s + i - p, X = qx * s + j - p;
                    if (Y >= 0 && Y < Hq && X >= 0 && X < Wq)
                        acc += wqc[i * k + j] * psb[c * ps_c + (((size_t)Y * Wq + X) * Os + sy) * Ps_ + sx];
                    const int U = sy * s + i - p, Vv = sx * s + j - p;
                    if (U >= 0 && U < Hs && Vv >= 0 && Vv < Ws)
                        acc += wsc[i * k + j] * pqb[c * pq_c + (((size_t)qy * Pq_ + qx) * Hs + U) * Ws + Vv];
                }
        }
        val = acc;
        y[((size_t)b * Cout + o) * npos + pos] = acc;
    }
    double s1 = active ? (double)val : 0.0, s2 = active ? (double)val * val : 0.0;
    gn_publish_block(s1, s2, stats, b);
}

// conv4d_pooled_kernel with ALL eight output channels in one thread (the strided layers of UFC are 1 -> 8 channels): the
// 2 k^2 Cin taps of a position are read once instead of once per output channel (8 workgroups per position tile re-read
// them: 52 M loads per 64^4 -> 16^4 layer, 39 us for 19 MFLOP); filters in LDS as [c][tap][branch][8].  Same tap order per
// output as conv4d_pooled_kernel (bias first, then c, i, j with the query tap before the support tap).
__global__ __launch_bounds__(256) void conv4d_pooled_c8_kernel(const float* __restrict__ ps, const float* __restrict__ pq,
                                                               const float* __restrict__ wq, const float* __restrict__ bq,
                                                               const float* __restrict__ ws, const float* __restrict__ bs,
                                                               int Cin, int Hq, int Wq, int Hs, int Ws, int k, int s, int p,
                                                               int Oq, int Pq_, int Os, int Ps_, float* __restrict__ y,
                                                               double* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) float wl[];        // [Cin][k*k][2][8]
    const int b = blockIdx.z, kk = k * k;
    for (int i = threadIdx.x; i < Cin * kk * 16; i += 256) {
        const int o = i & 7, br = (i >> 3) & 1, t = i >> 4;              // t = c * kk + tap
        wl[i] = (br ? ws : wq)[(size_t)o * Cin * kk + t];
    }
    __syncthreads();
    const long long npos = (long long)Oq * Pq_ * Os * Ps_;
    const long long pos = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = pos < npos;
    double s1 = 0.0, s2 = 0.0;
    if (active) {
        const int sx = (int)(pos % Ps_);
        long long t = pos / Ps_;
        const int sy = (int)(t % Os); t /= Os;
        const int qx = (int)(t % Pq_);
        const int qy = (int)(t / Pq_);
        const size_t ps_c = (size_t)Hq * Wq * Os * Ps_, pq_c = (size_t)Oq * Pq_ * Hs * Ws;
        const float* psb = ps + (size_t)b * Cin * ps_c;
        const float* pqb = pq + (size_t)b * Cin * pq_c;
        float acc[8];
#pragma unroll
        for (int o = 0; o < 8; ++o) acc[o] = bq[o] + bs[o];
        for (int c = 0; c < Cin; ++c)
            for (int i = 0; i < k; ++i)
                for (int j = 0; j < k; ++j) {
                    const int Y = qy * s + i - p, X = qx * s + j - p;
                    const int U = sy * s + i - p, Vv = sx * s + j - p;
                    const bool okq = Y >= 0 && Y < Hq && X >= 0 && X < Wq, oks = U >= 0 && U < Hs && Vv >= 0 && Vv < Ws;
                    const float vq = okq ? psb[c * ps_c + (((size_t)Y * Wq + X) * Os + sy) * Ps_ + sx] : 0.0f;
                    const float vs = oks ? pqb[c * pq_c + (((size_t)qy * Pq_ + qx) * Hs + U) * Ws + Vv] : 0.0f;
                    const f32x4* w4 = reinterpret_cast<const f32x4*>(wl + (size_t)(c * kk + i * k + j) * 16);
                    const f32x4 a0 = w4[0], a1 = w4[1], b0 = w4[2], b1 = w4[3];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        // the per-channel kernel skips an out-of-range tap; adding w * 0 gives the same value
                        if (okq) { acc[e] += a0[e] * vq; acc[4 + e] += a1[e] * vq; }
                        if (oks) { acc[e] += b0[e] * vs; acc[4 + e] += b1[e] * vs; }
                    }
                }
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            y[((size_t)b * 8 + o) * npos + pos] = acc[o];
            s1 += (double)acc[o];
            s2 += (double)acc[o] * acc[o];
        }
    }
    gn_publish_block(s1, s2, stats, b);
}

// stride-1 3x3x3x3 fast path (57 of the 63 Conv4d calls of a get_z): one thread computes COUT output channels of
// its position (blockIdx.y = channel group), so every input value is read once per tap instead of once per (tap,
// output channel); the weights are staged in LDS as [cin][tap][branch][cout] and read as wave-uniform (broadcast)
// 16-byte vectors.  COUT = 8 (4 at B = 1 with 8 channels, where a 16^4 volume is 1 024 waves = ONE per SIMD): more
// channels per thread would read the inputs fewer times but do not fit the register budget of 4 waves per SIMD.
// DGRAD: the same kernel as the data gradient of the layer — input = dy, weights read IN PLACE as the transposed, flipped
// filters (w'[o][c][tap] = w[c][o][8 - tap], the forward layer's (cout_fwd = Cin here, cin_fwd = cout_total, 3, 3)
// tensors), no bias, no statistics.  The autograd wrapper used to build flipped copies, a zero bias and a statistics
// buffer per layer: ~450 small launches per training step.
template <int COUT, bool PF, bool DGRAD = false>
__global__ __launch_bounds__(256, PF ? 2 : 4) void conv4d_k3s1_kernel(const float* __restrict__ x, const float* __restrict__ wq,
                                                          const float* __restrict__ bq, const float* __restrict__ ws,
                                                          const float* __restrict__ bs, int Cin, int Hq, int Wq,
                                                          int Hs, int Ws, int cout_total, float* __restrict__ y,
                                                          double* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) float wl[];        // Cin * 9 * 2 * COUT floats
    const int b = blockIdx.z;
    const int o0 = blockIdx.y * COUT;
    for (int i = threadIdx.x; i < Cin * 9 * 2 * COUT; i += 256) {
        const int o = o0 + i % COUT;
        int t = i / COUT;
        const int br = t & 1; t >>= 1;
        const int tap = t % 9, c = t / 9;
        wl[i] = DGRAD ? (br ? ws : wq)[((size_t)c * cout_total + o) * 9 + (8 - tap)]
                      : (br ? ws : wq)[((size_t)o * Cin + c) * 9 + tap];
    }
    __syncthreads();
    const long long npos = (long long)Hq * Wq * Hs * Ws;
    const long long pos = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = pos < npos;
    double s1 = 0.0, s2 = 0.0;
    if (active) {
        const int sx = (int)(pos % Ws);
        long long t = pos / Ws;
        const int sy = (int)(t % Hs); t /= Hs;
        const int qx = (int)(t % Wq);
        const int qy = (int)(t / Wq);
        float acc[COUT];
#pragma unroll
        for (int o = 0; o < COUT; ++o) acc[o] = DGRAD ? 0.0f : bq[o0 + o] + bs[o0 + o];
        // The 18 taps of this position as 32-bit byte offsets into the batch element's (Cin, npos) block, read with
        // buffer loads (scalar base + per-lane offset; an out-of-range offset returns 0 = the zero padding).  Registers
        // are what limits this kernel: with 64-bit per-lane addresses it needed 512 VGPRs = one wave per SIMD.
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(x + (size_t)b * Cin * (size_t)npos), 0, (int)((size_t)Cin * npos * 4), 0x00020000);
        int off[18];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int t = i * 3 + j;
                const int Y = qy + i - 1, X = qx + j - 1, U = sy + i - 1, Vv = sx + j - 1;
                const bool okq = Y >= 0 && Y < Hq && X >= 0 && X < Wq, oks = U >= 0 && U < Hs && Vv >= 0 && Vv < Ws;
                off[2 * t] = okq ? (((Y * Wq + X) * Hs + sy) * Ws + sx) * 4 : 0x7ffffff0;
                off[2 * t + 1] = oks ? (((qy * Wq + qx) * Hs + U) * Ws + Vv) * 4 : 0x7ffffff0;
            }
        // the 18 taps of channel c+1 are requested before the FMAs of channel c (a channel is ~1 us of load latency and
        // a few hundred cycles of math: at B = 1 nothing else hides it)
        auto load_taps = [&](int c, float (&xv)[18]) {
            const int cbase = c * (int)npos * 4;              // scalar offset of the channel
#pragma unroll
            for (int t = 0; t < 18; ++t)
                xv[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off[t], cbase, 0));
        };
        auto accumulate = [&](int c, const float (&xv)[18]) {
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const f32x4* w4 = reinterpret_cast<const f32x4*>(wl + ((c * 9 + t) * 2) * COUT);
                const float vq = xv[2 * t], vs = xv[2 * t + 1];
#pragma unroll
                for (int o4 = 0; o4 < COUT / 4; ++o4) {
                    const f32x4 a = w4[o4], bb = w4[COUT / 4 + o4];
#pragma unroll
                    for (int e = 0; e < 4; ++e)              // two chained FMAs per output (v_pk_fma_f32 pairs)
                        acc[o4 * 4 + e] = __builtin_fmaf(bb[e], vs, __builtin_fmaf(a[e], vq, acc[o4 * 4 + e]));
                    if ((o4 & 1) == 1) __builtin_amdgcn_sched_barrier(0);      // <= 4 weight vectors in flight
                }
            }
        };
        if (PF) {                                             // small launches (B = 1): latency, not occupancy, is the limit
            float xa[18], xb2[18];
            load_taps(0, xa);
            int c = 0;
#pragma unroll 1
            for (; c + 2 <= Cin; c += 2) {
                load_taps(c + 1, xb2);
                accumulate(c, xa);
                if (c + 2 < Cin) load_taps(c + 2, xa);
                accumulate(c + 1, xb2);
            }
            if (c < Cin) accumulate(c, xa);
        } else {                                              // large launches: 4 waves per SIMD hide the loads
#pragma unroll 1
            for (int c = 0; c < Cin; ++c) {
                float xv[18];
                load_taps(c, xv);
                accumulate(c, xv);
            }
        }
#pragma unroll
        for (int o = 0; o < COUT; ++o) {
            y[((size_t)b * cout_total + o0 + o) * npos + pos] = acc[o];
            s1 += (double)acc[o];
            s2 += (double)acc[o] * acc[o];
        }
    }
    if (DGRAD) return;
    gn_publish_block(s1, s2, stats, b);
}

// mean / 1/std of sample b from its (sum, sum of squares) pair (gn_publish), computed ONCE per workgroup and broadcast
// through LDS.
// Must be called by all threads of the block (contains a barrier).
__device__ __forceinline__ void gn_block_stats(const double* __restrict__ stats, int b, double n, float eps, float& mean,
                                               float& rstd) {
    __shared__ float mr[2];
    if (threadIdx.x == 0) {
        const double m = stats[2 * (size_t)b] / n;
        const double var = stats[2 * (size_t)b + 1] / n - m * m;
        mr[0] = (float)m;
        mr[1] = (float)(1.0 / sqrt(var + (double)eps));
    }
    __syncthreads();
    mean = mr[0];
    rstd = mr[1];
}

__global__ __launch_bounds__(256) void gn_relu_kernel(const float* y, const double* __restrict__ stats,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ res, float eps, int Cout, long long npos,
                                                      float* out) {
    const int b = blockIdx.z, o = blockIdx.y;
    const long long pos = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float mean, rstd;
    gn_block_stats(stats, b, (double)Cout * (double)npos, eps, mean, rstd);
    if (pos >= npos) return;
    const size_t idx = ((size_t)b * Cout + o) * npos + pos;
    const float v = (y[idx] - mean) * rstd * gamma[o] + beta[o];
    // res: the residual the caller adds to the block's output (x + Encoder4D(x), aggregation.py:306,347-355) in the same pass
    out[idx] = res ? res[idx] + fmaxf(v, 0.0f) : fmaxf(v, 0.0f);
}

// ---- the stride-1 3x3x3x3 layer on the fp32 MFMA (round 4; the round-3 form fed every MFMA with its own 4-byte load) -------
// out[co, pos] = bias + sum over (branch, tap, ci) of w_branch[co, ci, tap] * x[ci, pos + tap_branch]: an implicit GEMM with
// M = output channels, N = positions, K = 2 * 9 * Cin on v_mfma_f32_16x16x4_f32 (an fmaf chain: fp32-exact products).
//   wave      64 consecutive positions x ALL output channels (MT tiles of 16, padded: Cout = 8 uses half a tile)
//   k step    four consecutive input channels of one (branch, tap): lane (j, g) holds a 16-byte vector of channel ci0 + g at
//             positions p0 + 4 j .. + 3, and ELEMENT e of that vector is the B operand of the output tile of positions
//             {p0 + 4 j + e}: one vector feeds 4 MT MFMAs
//   loads     per 4-channel group 9 aligned vectors for the query-pair taps (whole vectors in or out of the volume: the
//             buffer load's out-of-range zero is the padding) and 3 for the support-pair ROWS; the dx = -1 / +1 taps of a
//             row are the same vector shifted by one element, the element that crosses a lane coming from the neighbour
//             lane through a DPP row shift (zero at the ends of a row of Ws): 12 loads feed 72 MT MFMAs, and the loads of
//             the next group are in flight under them
//   A operand w[co][ci0 + g] from LDS ([branch][tap][ci][co], conflict-free 4-byte reads)
// The VALU version above spends 1 152 FMAs per position and 8 channels and re-reads every input once per 8 output channels;
// here the multiplies sit on the matrix pipe.  Needs Cin % 4 == 0, Ws in {4, 8, 16, 32, 64}, positions % 64 == 0.  DGRAD as above.
template <int MT, bool DGRAD>
__global__ __launch_bounds__(256, 2) void conv4d_k3s1_mfma_kernel(const float* __restrict__ x, const float* __restrict__ wq,
                                                                  const float* __restrict__ bq, const float* __restrict__ ws,
                                                                  const float* __restrict__ bs, int Cin, int Hq, int Wq, int Hs,
                                                                  int Ws, int cout_total, float* __restrict__ y,
                                                                  double* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) float wl[];        // [2][9][Cin][MT*16]
    const int b = blockIdx.z;
    constexpr int CO = MT * 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fi = lane & 15, g = lane >> 4;
    const long long npos = (long long)Hq * Wq * Hs * Ws;
    const long long pos = ((long long)blockIdx.x * 4 + wave) * 64 + 4 * fi;      // first of this lane's four positions
    const bool active = pos < npos;                                              // whole waves: npos % 64 == 0
    const long long pc = active ? pos : 0;
    const int sx = (int)(pc % Ws);
    long long t = pc / Ws;
    const int sy = (int)(t % Hs); t /= Hs;
    const int qx = (int)(t % Wq);
    const int qy = (int)(t / Wq);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(x + (size_t)b * Cin * (size_t)npos), 0, (int)((size_t)Cin * npos * 4), 0x00020000);
    const int plane = (int)npos * 4;                               // bytes of one input channel
    constexpr int kOOB = 0x7ffffff0;
    int offq[9], offs[3];                                          // with this lane's channel offset g
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int Y = qy + i - 1, X = qx + j - 1;
            const bool ok = active && Y >= 0 && Y < Hq && X >= 0 && X < Wq;
            offq[i * 3 + j] = ok ? (((Y * Wq + X) * Hs + sy) * Ws + sx) * 4 + g * plane : kOOB;
        }
        const int U = sy + i - 1;
        offs[i] = (active && U >= 0 && U < Hs) ? (((qy * Wq + qx) * Hs + U) * Ws + sx) * 4 + g * plane : kOOB;
    }
    const bool row_first = sx == 0, row_last = sx + 4 == Ws;
    f32x4 acc[MT][4];                                              // [channel tile][position subset e]
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int co = mt * 16 + g * 4 + i;
            const float bias = (DGRAD || co >= cout_total) ? 0.0f : bq[co] + bs[co];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[mt][e][i] = bias;
        }
    auto load_group = [&](int c0, f32x4 (&vq)[9], f32x4 (&vs)[3]) {
        const int so = c0 * plane;
#pragma unroll
        for (int k = 0; k < 9; ++k) vq[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, offq[k], so, 0));
#pragma unroll
        for (int k = 0; k < 3; ++k) vs[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, offs[k], so, 0));
        __builtin_amdgcn_sched_barrier(0);
    };
    auto step = [&](int c0, int k, const f32x4& v) {                // k = branch * 9 + tap
        const float* wrow = wl + ((size_t)k * Cin + c0 + g) * CO + fi;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const float a = wrow[mt * 16];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[mt][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, v[e], acc[mt][e], 0, 0, 0);
        }
    };
    auto compute_group = [&](int c0, const f32x4 (&vq)[9], const f32x4 (&vs)[3]) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const f32x4 r = vs[i];
            // neighbours' edge elements: lane j - 1's element 3 and lane j + 1's element 0 (DPP row shifts inside the 16 lanes
            // of a channel group; a row of Ws never crosses them because Ws divides 64 or is a multiple of it)
            // (written as asm: with the update_dpp builtin the compiler read element 0 of the vector for BOTH shifts here)
            float left, right;
            const float r3 = r[3], r0 = r[0];
            asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %2 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                         "v_mov_b32_dpp %1, %3 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
                         : "=&v"(left), "=&v"(right) : "v"(r3), "v"(r0));
            const f32x4 rm = {row_first ? 0.0f : left, r[0], r[1], r[2]};       // x - 1
            const f32x4 rp = {r[1], r[2], r[3], row_last ? 0.0f : right};       // x + 1
            step(c0, i * 3 + 0, vq[i * 3 + 0]);
            step(c0, 9 + i * 3 + 0, rm);
            step(c0, i * 3 + 1, vq[i * 3 + 1]);
            step(c0, 9 + i * 3 + 1, r);
            step(c0, i * 3 + 2, vq[i * 3 + 2]);
            step(c0, 9 + i * 3 + 2, rp);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    f32x4 q0[9], s0[3], q1[9], s1v[3];
    load_group(0, q0, s0);                                         // in flight while the filters are staged
    // Filters into LDS: the GLOBAL index runs with the thread index (coalesced reads, four in flight per thread), the LDS
    // index is scattered.  (Walking the LDS index instead made every thread issue up to 36 dependent 4-byte reads with a
    // stride of 9 floats: a third of the kernel's time at 32 input channels.)
    if (cout_total < CO)
        for (int i = threadIdx.x; i < 18 * Cin * CO; i += 256)
            if (i % CO >= cout_total) wl[i] = 0.0f;
    {
        const int per_branch = cout_total * Cin * 9, total = 2 * per_branch;
        for (int g0 = threadIdx.x; g0 < total; g0 += 1024) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int gi = g0 + 256 * u;
                v[u] = gi < total ? (gi < per_branch ? wq[gi] : ws[gi - per_branch]) : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int gi = g0 + 256 * u;
                if (gi >= total) continue;
                const int br = gi >= per_branch, q = gi - br * per_branch;
                const int tapg = q % 9, mid = (q / 9) % (DGRAD ? cout_total : Cin), top = q / (9 * (DGRAD ? cout_total : Cin));
                // forward tensor [o][c][tap]; data gradient reads the forward layer's [c][o][8 - tap]
                const int o = DGRAD ? mid : top, c = DGRAD ? top : mid, tap = DGRAD ? 8 - tapg : tapg;
                wl[((size_t)(br * 9 + tap) * Cin + c) * CO + o] = v[u];
            }
        }
    }
    __syncthreads();
    for (int c0 = 0; c0 < Cin; c0 += 8) {
        if (c0 + 4 < Cin) load_group(c0 + 4, q1, s1v);
        compute_group(c0, q0, s0);
        if (c0 + 4 < Cin) {
            if (c0 + 8 < Cin) load_group(c0 + 8, q0, s0);
            compute_group(c0 + 4, q1, s1v);
        }
    }
    double s1 = 0.0, s2 = 0.0;
    if (active) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int co = mt * 16 + g * 4 + i;
                if (co < cout_total) {
                    const f32x4 v = {acc[mt][0][i], acc[mt][1][i], acc[mt][2][i], acc[mt][3][i]};
                    *reinterpret_cast<f32x4*>(y + ((size_t)b * cout_total + co) * npos + pos) = v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        s1 += (double)v[e];
                        s2 += (double)v[e] * v[e];
                    }
                }
            }
    }
    if (DGRAD) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    __shared__ double red[8];
    if (lane == 0) { red[wave * 2] = s1; red[wave * 2 + 1] = s2; }
    __syncthreads();
    gn_publish(red[0] + red[2] + red[4] + red[6], red[1] + red[3] + red[5] + red[7], stats, b);
}

// ---- backward of GroupNorm(1 group) + ReLU, two passes over the volume ---------------------------------------
//   dz = dout * [out > 0],  yh = (y - mean_b) * rstd_b
//   pass 1: S1_b = sum dz*g_c, S2_b = sum dz*g_c*yh (over channels and positions);  dgamma_c = sum dz*yh, dbeta_c = sum dz
//   pass 2: dy = rstd_b * (dz*g_c - S1_b/n - yh*S2_b/n)
// red: (B*2 + C*2) doubles, zero on entry.
__global__ __launch_bounds__(256) void gn_relu_bwd_reduce_kernel(
    const float* __restrict__ y, const float* __restrict__ out, const float* __restrict__ dout,
    const double* __restrict__ stats, const float* __restrict__ gamma, float eps, int B, int Cout, long long npos,
    double* __restrict__ red) {
    const int b = blockIdx.z, o = blockIdx.y;
    float mean, rstd;
    gn_block_stats(stats, b, (double)Cout * (double)npos, eps, mean, rstd);
    const float g = gamma[o];
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    const size_t base = ((size_t)b * Cout + o) * npos;
    if ((npos & 3) == 0) {
        // 16-byte loads, fp32 partial sums over the four elements of a load (then double): the three operand streams
        // are all this kernel does
        const long long n4 = npos >> 2;
        const f32x4* o4 = reinterpret_cast<const f32x4*>(out + base);
        const f32x4* d4 = reinterpret_cast<const f32x4*>(dout + base);
        const f32x4* y4 = reinterpret_cast<const f32x4*>(y + base);
        for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += (long long)gridDim.x * blockDim.x) {
            const f32x4 ov = o4[q], dv = d4[q], yv = y4[q];
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dz = ov[e] > 0.0f ? dv[e] : 0.0f;
                s0 += dz;
                s1 += dz * ((yv[e] - mean) * rstd);
            }
            a[0] += (double)(s0 * g);
            a[1] += (double)(s1 * g);
            a[2] += (double)s1;
            a[3] += (double)s0;
        }
    } else {
        for (long long pos = (long long)blockIdx.x * blockDim.x + threadIdx.x; pos < npos;
             pos += (long long)gridDim.x * blockDim.x) {
            const float dz = out[base + pos] > 0.0f ? dout[base + pos] : 0.0f;
            const float yh = (y[base + pos] - mean) * rstd;
            a[0] += (double)(dz * g);
            a[1] += (double)(dz * g * yh);
            a[2] += (double)(dz * yh);
            a[3] += (double)dz;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a[i] += __shfl_xor(a[i], off);
    __shared__ double sh[4][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int i = 0; i < 4; ++i) sh[wave][i] = a[i];
    __syncthreads();
    if (threadIdx.x < 4) {
        const double v = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
        double* dst = threadIdx.x < 2 ? red + b * 2 + threadIdx.x : red + 2 * B + o * 2 + (threadIdx.x - 2);
        atomicAdd(dst, v);
    }
}

__global__ __launch_bounds__(256) void gn_relu_bwd_apply_kernel(
    const float* __restrict__ y, const float* __restrict__ out, const float* __restrict__ dout,
    const double* __restrict__ stats, const float* __restrict__ gamma, float eps, int B, int Cout, long long npos,
    const double* __restrict__ red, float* __restrict__ dy, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int b = blockIdx.z, o = blockIdx.y;
    const long long pos = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x == 0 && b == 0 && threadIdx.x == 0) {
        dgamma[o] = (float)red[2 * B + o * 2];
        dbeta[o] = (float)red[2 * B + o * 2 + 1];
    }
    const double n = (double)Cout * (double)npos;
    float mean, rstd;
    gn_block_stats(stats, b, n, eps, mean, rstd);           // block-wide: before the early return
    if (pos >= npos) return;
    const float m1 = (float)(red[b * 2] / n), m2 = (float)(red[b * 2 + 1] / n);
    const size_t idx = ((size_t)b * Cout + o) * npos + pos;
    const float dz = out[idx] > 0.0f ? dout[idx] : 0.0f;
    const float yh = (y[idx] - mean) * rstd;
    dy[idx] = rstd * (dz * gamma[o] - m1 - yh * m2);
}

// ------------------------------------------------------------------------------------------------
// (N, P, Q) -> (N, Q, P) batched matrix transpose = swapping the (query, support) index pairs of a 4-D correlation
// volume, x.permute(0,1,4,5,2,3).contiguous() in the reference's notation (aggregation.py:275, 349 and every
// `rearrange` around conv4d.py).  32 x 32 tiles through LDS, coalesced on both sides; ATen's strided copy for this
// permutation runs at 0.8 TB/s and there are ~170 of them in a training step.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void transpose_pairs_kernel(const float* __restrict__ x, int P, int Q, float* __restrict__ y) {
    __shared__ float tile[32][33];
    const size_t base = (size_t)blockIdx.z * P * Q;
    const int q0 = blockIdx.x * 32, p0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;              // 32 x 8
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = p0 + ty + i * 8, q = q0 + tx;
        if (p < P && q < Q) tile[ty + i * 8][tx] = x[base + (size_t)p * Q + q];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = q0 + ty + i * 8, p = p0 + tx;
        if (p < P && q < Q) y[base + (size_t)q * P + p] = tile[tx][ty + i * 8];
    }
}

// ---- host side of conv4d_k3s1_mfma_kernel, for the layer (cpn_conv4d) and its data gradient (cpn_conv4d_dgrad) -------------
inline size_t conv4d_mfma_lds(int cred, int cprod) { return (size_t)18 * cred * ((cprod + 15) / 16) * 16 * sizeof(float); }

// May the k3 s1 p1 convolution that reduces over `cred` channels of x and produces `cprod` channels of y take the MFMA form
// (64 positions per wave, 12 vector loads per 72 MT MFMAs)?  CPN_CONV4D_MFMA with a value starting with 0 keeps the VALU
// kernel.  (The round-3 MFMA form — 16 positions per wave, one 4-byte load per MFMA — measured 40 / 32 us per Cout = 8 / 32
// layer against 24 / 34 for the VALU kernel and was opt-in.)
bool conv4d_mfma_ok(int cred, int cprod, int Ws, long long npos, const void* x, const void* y) {
    static const bool off = getenv("CPN_CONV4D_MFMA") && getenv("CPN_CONV4D_MFMA")[0] == '0';
    const bool ws_ok = Ws == 4 || Ws == 8 || Ws == 16 || Ws == 32 || Ws == 64;
    return !off && cred % 4 == 0 && cprod <= 32 && conv4d_mfma_lds(cred, cprod) <= 64 * 1024 && ws_ok &&
           npos % 64 == 0 && (long long)cred * npos * 4 < 0x7ffffff0LL - 4LL * npos * 4 && ((uintptr_t)x % 16) == 0 &&
           ((uintptr_t)y % 16) == 0;
}

// launches it (conv4d_mfma_ok holds); DGRAD: x = dy, wq / ws the forward layer's filters, no bias, no statistics
template <bool DGRAD>
void launch_conv4d_mfma(hipStream_t st, const float* x, const float* wq, const float* bq, const float* ws, const float* bs, int B,
                        int cred, int cprod, int Hq, int Wq, int Hs, int Ws, float* y, double* stats) {
    // gn_publish counts gridDim.x * gridDim.y workgroups per sample: one workgroup = 256 positions, all channels
    const dim3 g2(cpn_cdiv((long long)Hq * Wq * Hs * Ws, 256), 1, B);
    auto* kernel = cprod <= 16 ? conv4d_k3s1_mfma_kernel<1, DGRAD> : conv4d_k3s1_mfma_kernel<2, DGRAD>;
    hipLaunchKernelGGL(kernel, g2, dim3(256), conv4d_mfma_lds(cred, cprod), st, x, wq, bq, ws, bs, cred, Hq, Wq, Hs, Ws, cprod, y,
                       stats);
}

}  // namespace

// doubles of the `stats` argument of cpn_conv4d / cpn_conv4d_gn_relu (layout: gn_publish); an upper bound over the
// kernel variants' grids
extern "C" long long cpn_gn_stats_doubles(int B, int Cout, long long npos) {
    // VALU kernels: one workgroup per 256 positions and output channel (group); MFMA kernel: one per 256 positions (64 in round 3)
    const long long wg = std::max<long long>((long long)cpn_cdiv(npos, 256) * Cout, (long long)cpn_cdiv(npos, 64));
    return 3LL * B + 2LL * B * wg;
}

extern "C" long long cpn_conv4d_scratch(int B, int Cin, int Hq, int Wq, int Hs, int Ws, int s) {
    if (s <= 1) return 0;
    // the two pooled volumes: Ps (n_ps floats), then Pq (n_pq)
    const SGeo g{B, Cin, 0, Hq, Wq, Hs, Ws, 0, s, 0, pooled_size(Hq, s), pooled_size(Wq, s), pooled_size(Hs, s), pooled_size(Ws, s)};
    return g.n_ps() + g.n_pq();
}

extern "C" int cpn_conv4d(const float* x, const float* wq, const float* bq, const float* ws, const float* bs, int B,
                          int Cin, int Cout, int Hq, int Wq, int Hs, int Ws, int k, int s, int p, float* y,
                          double* stats, float* scratch, void* stream) {
    CPN_REQUIRE(x && wq && bq && ws && bs && y && stats, CPN_E_ARG, "cpn_conv4d: null pointer");
    CPN_REQUIRE(B > 0 && B < 65536 && Cin > 0 && Cout > 0 && Cout < 65536 && k > 0 && s > 0 && p >= 0, CPN_E_SHAPE,
                "cpn_conv4d: bad shape");
    SGeo g;
    CPN_REQUIRE(make_geo(B, Cin, Cout, Hq, Wq, Hs, Ws, k, s, p, &g), CPN_E_SHAPE,
                "cpn_conv4d: conv output (%d) and pooled size (%d) of the two branches disagree", g.Oq, pooled_size(Hq, s));
    const int Oq = g.Oq, Pq_ = g.Pq, Os = g.Os, Ps_ = g.Ps;
    const long long npos = g.npos();
    const hipStream_t st = (hipStream_t)stream;
    dim3 grid(cpn_cdiv(npos, 256), Cout, B);
    const size_t wbytes = (size_t)Cin * 9 * 2 * Cout * sizeof(float);
    if (k == 3 && s == 1 && p == 1 && conv4d_mfma_ok(Cin, Cout, Ws, npos, x, y)) {
        launch_conv4d_mfma<false>(st, x, wq, bq, ws, bs, B, Cin, Cout, Hq, Wq, Hs, Ws, y, stats);
    } else if (k == 3 && s == 1 && p == 1 && (Cout == 8 || Cout == 32) && wbytes <= 64 * 1024 &&
        (long long)Cin * npos * 4 < 0x7ffffff0LL) {
        // channels per thread: 8 (4 when one thread per position would leave <= 2 waves per SIMD).  All 32 channels in one
        // thread read every input once instead of four times, but the compiler cannot hold 32 accumulators + a tap's
        // weights + 18 taps under 128 VGPRs (512 VGPRs = one wave per SIMD, or a kilobyte of scratch spills when
        // forced): 8 channels fit in 124 and run four waves per SIMD.
        const bool small = (long long)B * npos <= 131072;
        const int per = (Cout == 8 && small) ? 4 : 8;
        dim3 g1(cpn_cdiv(npos, 256), Cout / per, B);
        const size_t wb = wbytes / (Cout / per);
        auto* kernel = per == 4 ? conv4d_k3s1_kernel<4, true> : small ? conv4d_k3s1_kernel<8, true> : conv4d_k3s1_kernel<8, false>;
        hipLaunchKernelGGL(kernel, g1, dim3(256), wb, st, x, wq, bq, ws, bs, Cin, Hq, Wq, Hs, Ws, Cout, y, stats);
    } else if (s > 1 && scratch) {
        float* psv = scratch;
        float* pqv = scratch + (size_t)B * Cin * Hq * Wq * Os * Ps_;
        const long long planes = (long long)B * Cin * Hq * Wq;
        const long long n1 = planes * Os * Ps_, n2 = (long long)B * Cin * Oq * Pq_ * Hs * Ws;
        hipLaunchKernelGGL(pool_support_kernel, dim3((unsigned)std::min<long long>(cpn_cdiv(n1, 256), 65536)), dim3(256), 0,
                           st, x, Hs, Ws, s, Os, Ps_, planes, psv);
        hipLaunchKernelGGL(pool_query_kernel, dim3((unsigned)std::min<long long>(cpn_cdiv(n2, 256), 65536)), dim3(256), 0,
                           st, x, Hq, Wq, Hs, Ws, s, Oq, Pq_, (long long)B * Cin, pqv);
        if (Cout == 8 && (size_t)Cin * k * k * 16 * sizeof(float) <= 48 * 1024)
            hipLaunchKernelGGL(conv4d_pooled_c8_kernel, dim3(cpn_cdiv(npos, 256), 1, B), dim3(256),
                               (size_t)Cin * k * k * 16 * sizeof(float), st, psv, pqv, wq, bq, ws, bs, Cin, Hq, Wq, Hs, Ws, k, s, p,
                               Oq, Pq_, Os, Ps_, y, stats);
        else
            hipLaunchKernelGGL(conv4d_pooled_kernel, grid, dim3(256), 0, st, psv, pqv, wq, bq, ws, bs, Cin, Hq, Wq, Hs, Ws, k, s,
                               p, Oq, Pq_, Os, Ps_, y, stats);
    } else {
        hipLaunchKernelGGL(conv4d_kernel, grid, dim3(256), 0, st, x, wq, bq, ws, bs, Cin, Hq, Wq, Hs, Ws, k, s, p, Oq,
                           Pq_, Os, Ps_, y, stats);
    }
    CPN_LAUNCH_CHECK("cpn_conv4d");
    return 0;
}

extern "C" int cpn_conv4d_dgrad(const float* dy, const float* wq, const float* ws, int B, int Cout, int Cin, int Hq, int Wq,
                                int Hs, int Ws, float* dx, void* stream) {
    CPN_REQUIRE(dy && wq && ws && dx, CPN_E_ARG, "cpn_conv4d_dgrad: null pointer");
    CPN_REQUIRE(B > 0 && B < 65536 && Cin > 0 && Cout > 0 && Hq > 0 && Wq > 0 && Hs > 0 && Ws > 0, CPN_E_SHAPE,
                "cpn_conv4d_dgrad: bad shape");
    const long long npos = (long long)Hq * Wq * Hs * Ws;
    // the data gradient is a k3 s1 p1 convolution of dy (Cout channels) producing Cin channels: channel groups of 8 (4)
    CPN_REQUIRE((Cin % 4) == 0 && (long long)Cout * npos * 4 < 0x7ffffff0LL, CPN_E_SHAPE,
                "cpn_conv4d_dgrad: need Cin %% 4 == 0 and a batch element below 2 GiB (Cin=%d)", Cin);
    if (conv4d_mfma_ok(Cout, Cin, Ws, npos, dy, dx)) {                      // the gradient convolves dy (Cout channels) into Cin
        launch_conv4d_mfma<true>((hipStream_t)stream, dy, wq, nullptr, ws, nullptr, B, Cout, Cin, Hq, Wq, Hs, Ws, dx, nullptr);
        CPN_LAUNCH_CHECK("cpn_conv4d_dgrad");
        return 0;
    }
    const int per = (Cin % 8) == 0 ? 8 : 4;
    const size_t wb = (size_t)Cout * 9 * 2 * per * sizeof(float);
    CPN_REQUIRE(wb <= 64 * 1024, CPN_E_SHAPE, "cpn_conv4d_dgrad: filter slice exceeds 64 KiB of LDS (Cout=%d)", Cout);
    dim3 g1(cpn_cdiv(npos, 256), Cin / per, B);
    auto* kernel = per == 4 ? conv4d_k3s1_kernel<4, false, true> : conv4d_k3s1_kernel<8, false, true>;
    hipLaunchKernelGGL(kernel, g1, dim3(256), wb, (hipStream_t)stream, dy, wq, (const float*)nullptr, ws, (const float*)nullptr,
                       Cout, Hq, Wq, Hs, Ws, Cin, dx, (double*)nullptr);
    CPN_LAUNCH_CHECK("cpn_conv4d_dgrad");
    return 0;
}

extern "C" int cpn_transpose_pairs(const float* x, int N, int P, int Q, float* y, void* stream) {
    CPN_REQUIRE(x && y, CPN_E_ARG, "cpn_transpose_pairs: null pointer");
    CPN_REQUIRE(N > 0 && N < 65536 && P > 0 && Q > 0, CPN_E_SHAPE, "cpn_transpose_pairs: bad shape (N=%d)", N);
    hipLaunchKernelGGL(transpose_pairs_kernel, dim3(cpn_cdiv(Q, 32), cpn_cdiv(P, 32), N), dim3(256), 0, (hipStream_t)stream, x, P,
                       Q, y);
    CPN_LAUNCH_CHECK("cpn_transpose_pairs");
    return 0;
}

extern "C" int cpn_gn_relu(const float* y, const double* stats, const float* gn_w, const float* gn_b, const float* residual,
                           float eps, int B, int C, long long npos, float* out, void* stream) {
    CPN_REQUIRE(y && stats && gn_w && gn_b && out, CPN_E_ARG, "cpn_gn_relu: null pointer");
    CPN_REQUIRE(B > 0 && B < 65536 && C > 0 && C < 65536 && npos > 0, CPN_E_SHAPE, "cpn_gn_relu: bad shape");
    dim3 grid(cpn_cdiv(npos, 256), C, B);
    hipLaunchKernelGGL(gn_relu_kernel, grid, dim3(256), 0, (hipStream_t)stream, y, stats, gn_w, gn_b, residual, eps, C, npos,
                       out);
    CPN_LAUNCH_CHECK("cpn_gn_relu");
    return 0;
}

extern "C" int cpn_conv4d_gn_relu(const float* x, const float* wq, const float* bq, const float* ws, const float* bs,
                                  const float* gn_w, const float* gn_b, const float* residual, float eps, int B, int Cin,
                                  int Cout, int Hq,
                                  int Wq, int Hs, int Ws, int k, int s, int p, float* y, double* stats, float* scratch,
                                  void* stream) {
    CPN_REQUIRE(gn_w && gn_b, CPN_E_ARG, "cpn_conv4d_gn_relu: null pointer");
    int rc = cpn_conv4d(x, wq, bq, ws, bs, B, Cin, Cout, Hq, Wq, Hs, Ws, k, s, p, y, stats, scratch, stream);
    if (rc) return rc;
    SGeo g;
    make_geo(B, Cin, Cout, Hq, Wq, Hs, Ws, k, s, p, &g);                    // accepted by cpn_conv4d above
    return cpn_gn_relu(y, stats, gn_w, gn_b, residual, eps, B, Cout, g.npos(), y, stream);
}

extern "C" int cpn_gn_relu_bwd(const float* y, const float* out, const float* dout, const double* stats,
                               const float* gn_w, float eps, int B, int C, long long npos, double* red, float* dy,
                               float* dgn_w, float* dgn_b, void* stream) {
    CPN_REQUIRE(y && out && dout && stats && gn_w && red && dy && dgn_w && dgn_b, CPN_E_ARG,
                "cpn_gn_relu_bwd: null pointer");
    CPN_REQUIRE(B > 0 && B < 65536 && C > 0 && C < 65536 && npos > 0, CPN_E_SHAPE, "cpn_gn_relu_bwd: bad shape");
    const hipStream_t st = (hipStream_t)stream;
    const unsigned bx = (unsigned)std::min<long long>(cpn_cdiv(npos, 4096), 16);       // 4 x 16-byte loads per thread
    hipLaunchKernelGGL(gn_relu_bwd_reduce_kernel, dim3(bx, C, B), dim3(256), 0, st, y, out, dout, stats, gn_w, eps, B, C,
                       npos, red);
    CPN_LAUNCH_CHECK("cpn_gn_relu_bwd(reduce)");
    hipLaunchKernelGGL(gn_relu_bwd_apply_kernel, dim3(cpn_cdiv(npos, 256), C, B), dim3(256), 0, st, y, out, dout, stats,
                       gn_w, eps, B, C, npos, red, dy, dgn_w, dgn_b);
    CPN_LAUNCH_CHECK("cpn_gn_relu_bwd(apply)");
    return 0;
}
