// precision = "auto" (RenderEngine): the per-ray logit guard and the selection of the rays it flags.
//
// The fp16 default forms the attention logits <key, coords_embed> / 11.31 from fp16 operands (/root/reference
// models/CoPoNeRF.py:450-461, 475-485): each carries a relative error of ~3e-4, and a softmax weight is then off
// by ~w (1 - w) |l| 3e-4.  Under |dl_i| <= eps |l_i|,  dw_i = w_i (1 - w_i) dl_i - w_i sum_{j != i} w_j dl_j, so
//     |dw_i| <= eps (w_i (1 - w_i) |l_i| + w_i sum_{j != i} w_j |l_j|)   and, as w_i <= 1 - w_j for j != i,
//     sum_i |dw_i| <= 2 eps sum_i w_i (1 - w_i) |l_i|   and   max_i |dw_i| <= 2 eps sum_i w_i (1 - w_i) |l_i|:
// one number per ray, score = sum_i w_i (1 - w_i) |l_i|, bounds both the rgb's and the weights' exposure.  (The looser
// sum_i w_i |l_i| flagged 99.9 % of the rays from gain 24 on, sharp rays included, whose weights hardly move: DESIGN.md §2.)
// Rays whose score passes a threshold are re-rendered in the reference's arithmetic (csrc/encode_f32.hip, the _rays entries).
//
//   cpn_logit_guard   one 256-thread workgroup per ray; reads the chunk's logits (4 bytes per sample) where cpn_attend_hidden
//                     reads them and forms w with the code it uses (ray_softmax.h)
//   cpn_select_rays   ascending list of the rays with score > tau and its count: a workgroup per tile of 4096 rays counts the
//                     flags of all earlier tiles itself (no scratch, no atomics, one launch; <= 1 MB of L2-resident reads per
//                     workgroup at 262 144 rays), then scans its own tile
#include "ray_softmax.h"

namespace {

// one workgroup of 256 threads per ray of the chunk; wts: V*S floats of LDS
__global__ __launch_bounds__(256) void logit_guard_kernel(const float* __restrict__ logits, int V, int S, int ray0,
                                                          float* __restrict__ score, int accumulate) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* const wts = reinterpret_cast<float*>(smem_raw);
    __shared__ float red[12];
    const int T = V * S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the weights of cpn_attend_hidden's `logits` mode bit for bit: the same two steps of ray_softmax.h
    const float lmax = ray_logits_to_lds(logits + (size_t)blockIdx.x * T, wts, T);
    const auto [gmax, inv] = ray_softmax_stats<true>(lmax, wts, red, T);
    float acc = 0.f;
    for (int row = tid; row < T; row += 256) {
        const float l = wts[row];
        const float w = __expf(l - gmax) * inv;
        acc += (w * (1.0f - w)) * fabsf(l);
    }
    acc = wave_sum(acc);
    if (lane == 0) red[8 + wave] = acc;
    __syncthreads();
    if (tid == 0) {
        float sc = (red[8] + red[9]) + (red[10] + red[11]);
        float* const o = score + (size_t)ray0 + blockIdx.x;
        if (accumulate) sc = fmaxf(sc, *o);
        *o = sc;
    }
}

constexpr int SEL_THREADS = 256;
constexpr int SEL_PER = 16;                           // consecutive rays per thread
constexpr int SEL_TILE = SEL_THREADS * SEL_PER;       // 4096 rays per workgroup

__global__ __launch_bounds__(SEL_THREADS) void select_rays_kernel(const float* __restrict__ score, int nray, float tau,
                                                                  int* __restrict__ list, int* __restrict__ count) {
    __shared__ int wsum[SEL_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t0 = blockIdx.x * SEL_TILE;
    // flagged rays before this tile, counted here: every earlier tile is full, 16 independent coalesced loads per thread each
    int before = 0;
    for (int tb = 0; tb < t0; tb += SEL_TILE) {
        int c = 0;
#pragma unroll
        for (int k = 0; k < SEL_PER; ++k) c += score[tb + k * SEL_THREADS + tid] > tau ? 1 : 0;
        before += c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
    if (lane == 0) wsum[wave] = before;
    __syncthreads();
    const int base = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    __syncthreads();
    // this thread's SEL_PER consecutive rays
    const int i0 = t0 + tid * SEL_PER;
    unsigned flags = 0u;
#pragma unroll
    for (int k = 0; k < SEL_PER; ++k) {
        const int i = i0 + k;
        if (i < nray && score[i] > tau) flags |= 1u << k;
    }
    const int mine = __builtin_popcount(flags);
    // inclusive scan over the wave (Hillis-Steele on shuffles), then over the four waves
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wave; ++w) woff += wsum[w];
    int pos = base + woff + incl - mine;
#pragma unroll
    for (int k = 0; k < SEL_PER; ++k)
        if (flags & (1u << k)) list[pos++] = i0 + k;
    if (blockIdx.x == gridDim.x - 1 && tid == SEL_THREADS - 1) *count = base + woff + incl;   // the tile's last thread
}

}  // namespace

extern "C" int cpn_logit_guard(const float* logits, int B, int V, int R, int S, int ray0, int nrays, float* score, int accumulate,
                               void* stream) {
    CPN_REQUIRE(logits && score, CPN_E_ARG, "cpn_logit_guard: null pointer");
    CPN_REQUIRE(B > 0 && V == 2 && R > 0 && S > 0 && V * S <= 4096, CPN_E_SHAPE, "cpn_logit_guard: bad shape");
    CPN_REQUIRE(ray0 >= 0 && nrays > 0 && (long long)ray0 + nrays <= (long long)B * R, CPN_E_ARG,
                "cpn_logit_guard: ray range [%d,%d) outside B*R=%lld", ray0, ray0 + nrays, (long long)B * R);
    const size_t lds = (size_t)(V * S) * sizeof(float);
    hipLaunchKernelGGL(logit_guard_kernel, dim3(nrays), dim3(256), lds, (hipStream_t)stream, logits, V, S, ray0, score,
                       accumulate ? 1 : 0);
    CPN_LAUNCH_CHECK("cpn_logit_guard");
    return 0;
}

extern "C" int cpn_select_rays(const float* score, int nray, float tau, int* list, int* count, void* stream) {
    CPN_REQUIRE(score && list && count, CPN_E_ARG, "cpn_select_rays: null pointer");
    CPN_REQUIRE(nray > 0, CPN_E_SHAPE, "cpn_select_rays: need nray > 0 (got %d)", nray);
    hipLaunchKernelGGL(select_rays_kernel, dim3(cpn_cdiv(nray, SEL_TILE)), dim3(SEL_THREADS), 0, (hipStream_t)stream, score, nray,
                       tau, list, count);
    CPN_LAUNCH_CHECK("cpn_select_rays");
    return 0;
}
