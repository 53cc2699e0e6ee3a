// K4 — joint softmax over the V*S epipolar samples of one query ray + attention-weighted value sum.
//
// Replaces einsum('bijk,bijk->bjk') / 11.31, F.softmax over (n_context * npoints), the broadcast
// multiply-sum and the sum over views (/root/reference models/CoPoNeRF.py:450-461 and 475-485).
// The reference has NO alpha compositing: the along-ray reduction is (max, sum-exp, weighted sum), which
// maps onto wave reductions — with S = 64 each view's sample axis is exactly one 64-lane wavefront.
//
// One 256-thread workgroup per query ray: T = V*S rows; the sum runs on the HIDDEN activations (folded form below).
// (The layer-by-layer form on the 416-wide values - cpn_attend, its fp32 sibling and the "project before you store" form
// cpn_attend_value - left the library in round 6: tools/experiments/r6_pruned/attend.hip.)
//
//   cpn_attend_hidden            fp16 operands (or the logits themselves), fp16 hidden rows, hbar fp16
//   cpn_attend_hidden_f32        the reference-arithmetic mode (encode_f32.hip): fp32 operands, hidden rows as (hi, lo) fp16
//   cpn_attend_hidden_f32_rays   pairs, hbar fp32; _rays: the workgroup's ray comes from a list (precision = "auto")
// ONE kernel body, attend_hidden_ray, for both precisions; what differs is in the two traits AttendF16 / AttendF32.
#include <algorithm>

#include "hid_sum.h"
#include "ray_softmax.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Folded variant: there is no non-linearity between query_encode_latent_2 and latent_value
// (CoPoNeRF.py:387-404) and the softmax weights of a ray sum to 1, so
//     sum_s w_s (Wv [W2 h_s0 + b2 ; W2 h_s1 + b2] + bv)  =  (Wv_a W2 | Wv_b W2) . sum_s w_s [h_s0 ; h_s1]  +  const.
// This kernel therefore reduces the 2*832 = 1664 hidden activations per sample (fp16, post-ReLU) with the
// softmax weights; the 1664 -> 416 value projection then runs once per RAY instead of once per sample.
// thread = 8 hidden channels (16 B), rows streamed; per ray T x 3328 B read, fully coalesced.
// ---------------------------------------------------------------------------------------------
constexpr int HC = 1664;
// 1 = stream hid with non-temporal loads (the product; keeps the node tables of encode_hidden in L2 / Infinity Cache);
// 0 = plain loads (tools/mall_probe.py: does a second pass over a cache-sized range run faster?)
#ifndef CPN_ATTEND_NT
#define CPN_ATTEND_NT 1
#endif
// rows of hid in flight per thread (16 bytes each): 4 is enough when the kernel has the chip to itself (7 waves per SIMD)
#ifndef CPN_ATTEND_UNROLL
#define CPN_ATTEND_UNROLL 4
#endif

// What a precision supplies to attend_hidden_ray.  Every rounding is written out (__builtin_fmaf, contraction off) in the form
// the kernels have always been compiled to, so that the bits depend on no compiler's reading of `acc += a * b`.
//   row_logit   <qa[row], qb[row]> over the 128 channels, by the LANES lanes that share a row, returned in all of them
//   hid_sum     acc[e] += w[row] * hidden[row][e] for the thread's 8 channels, rows 0 .. T-1 in order
//   store       the 8 sums -> hbar
struct AttendF16 {
    using q_t = __half;
    using out_t = __half;
    static constexpr int LANES = 16;                      // 16 lanes x 8 halves per row
    static constexpr int HID_LD = HC;                     // halves per hidden row
    // 16 lanes per row, 16 bytes each: a load instruction covers 4 whole 256-byte rows of each operand (two lanes per row with 8
    // loads of 16 bytes each, 128 bytes apart, touched 64 different lines per instruction: the training step's two launches of
    // this kernel spent 42 % of their cycles with the address path stalled by the cache - TA_ADDR_STALLED_BY_TC 289 M per launch)
    // Rounding: one chain of fused multiply-adds from 0 over the lane's 8 channels, then the xor butterfly 1, 2, 4, 8.
    static __device__ __forceinline__ float row_logit(const q_t* __restrict__ qa, const q_t* __restrict__ qb, const int l) {
        const half8 a = *reinterpret_cast<const half8*>(qa + l * 8);
        const half8 b = *reinterpret_cast<const half8*>(qb + l * 8);
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = __builtin_fmaf((float)a[e], (float)b[e], acc);
        acc += __shfl_xor(acc, 1);
        acc += __shfl_xor(acc, 2);
        acc += __shfl_xor(acc, 4);
        acc += __shfl_xor(acc, 8);
        return acc;
    }
    // hid: the ray's first row + the thread's 8 channels; row stride 1664 halves.  U rows in flight (rounding: hid_sum.h).
    static __device__ __forceinline__ void hid_sum(float (&acc)[8], const float* __restrict__ wts, const __half* __restrict__ hp,
                                                   const int T) {
        constexpr int U = CPN_ATTEND_UNROLL;
        auto ld = [&](int row) {
#if CPN_ATTEND_NT
            return __builtin_nontemporal_load(reinterpret_cast<const half8*>(hp + (size_t)row * HID_LD));
#else
            return *reinterpret_cast<const half8*>(hp + (size_t)row * HID_LD);
#endif
        };
        int row = 0;
        for (; row + U <= T; row += U) {                  // U loads in flight, then their U x 8 FMAs in row order
            half8 h[U];
#pragma unroll
            for (int u = 0; u < U; ++u) h[u] = ld(row + u);
#pragma unroll
            for (int u = 0; u < U; ++u) hid_row_acc<U % HID_BLOCK_ROWS == 0>(acc, wts[row + u], h[u]);
        }
        for (; row < T; ++row) {
            const half8 h = ld(row);
            if (U != HID_BLOCK_ROWS && row < T - T % HID_BLOCK_ROWS) hid_row_acc<true>(acc, wts[row], h);
            else hid_row_acc<false>(acc, wts[row], h);
        }
    }
    static __device__ __forceinline__ void store(out_t* __restrict__ o, const float (&acc)[8]) {
        half8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (_Float16)acc[e];
        *reinterpret_cast<half8*>(o) = v;
    }
};

struct AttendF32 {
    using q_t = float;
    using out_t = float;
    static constexpr int LANES = 32;                      // 32 lanes x 4 floats per row
    static constexpr int HID_LD = 2 * HC;                 // halves per hs row: [hi | lo]
    // Rounding: the ROUNDED product of channel 1, then channels 0, 2, 3 fused onto it in that order (what the compiler made of
    // a0 b0 + a1 b1 + a2 b2 + a3 b3), then the xor butterfly 16 .. 1.
    static __device__ __forceinline__ float row_logit(const q_t* __restrict__ qa, const q_t* __restrict__ qb, const int l) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(qa + l * 4);
        const f32x4 b = *reinterpret_cast<const f32x4*>(qb + l * 4);
        float acc;
        {
#pragma clang fp contract(off)
            acc = a[1] * b[1];
        }
        acc = __builtin_fmaf(a[0], b[0], acc);
        acc = __builtin_fmaf(a[2], b[2], acc);
        acc = __builtin_fmaf(a[3], b[3], acc);
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        return acc;
    }
    // hs: hi and lo 1664 halves apart, row stride 3328.  Rounding: hi + lo rounded to fp32, then ONE fused multiply-add per
    // channel and row; 8 rows per trip.
    static __device__ __forceinline__ void hid_sum(float (&acc)[8], const float* __restrict__ wts, const __half* __restrict__ hp,
                                                   const int T) {
#pragma unroll 8
        for (int row = 0; row < T; ++row) {
            const half8 hi = __builtin_nontemporal_load(reinterpret_cast<const half8*>(hp + (size_t)row * HID_LD));
            const half8 lo = __builtin_nontemporal_load(reinterpret_cast<const half8*>(hp + (size_t)row * HID_LD + HC));
            const float w = wts[row];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = __builtin_fmaf(w, (float)hi[e] + (float)lo[e], acc[e]);
        }
    }
    static __device__ __forceinline__ void store(out_t* __restrict__ o, const float (&acc)[8]) {
        *reinterpret_cast<f32x4*>(o) = f32x4{acc[0], acc[1], acc[2], acc[3]};
        *reinterpret_cast<f32x4*>(o + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
    }
};

// One workgroup per ray, local ray = blockIdx.x: logits (given, or formed from the (rows, 128) operands), the softmax of
// ray_softmax.h, hbar = sum_rows w hidden.  LDS: T + 8 floats.
// HAVE_LOGITS: the row dot products were formed by the producing kernel.  LIST: the ray is rays[ray0 + local ray] (its at_wt
// rows are skipped if that lies outside [0, nraytot)), else ray0 + local ray.
template <class P, bool HAVE_LOGITS, bool LIST>
__device__ __forceinline__ void attend_hidden_ray(const typename P::q_t* __restrict__ qa, const typename P::q_t* __restrict__ qb,
                                                  const float* __restrict__ logits, const __half* __restrict__ hid, int V, int R,
                                                  int S, int ray0, typename P::out_t* __restrict__ hbar, float* __restrict__ at_wt,
                                                  const int* __restrict__ rays, long long nraytot) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* wts = reinterpret_cast<float*>(smem_raw);
    float* red = wts + V * S;
    const int T = V * S;
    const int tid = threadIdx.x;
    const unsigned lray = blockIdx.x;
    const size_t row0 = (size_t)lray * T;

    float lmax = -INFINITY;
    if constexpr (HAVE_LOGITS) {
        lmax = ray_logits_to_lds(logits + row0, wts, T);
    } else {
        constexpr int ROWS = 256 / P::LANES;              // rows per trip
        for (int base = 0; base < T; base += ROWS) {
            const int row = base + tid / P::LANES;
            const int rr = row < T ? row : T - 1;
            const float acc = P::row_logit(qa + (row0 + rr) * 128, qb + (row0 + rr) * 128, tid % P::LANES);
            if (row < T) {
                const float logit = acc / 11.31f;
                if (tid % P::LANES == 0) wts[row] = logit;
                lmax = fmaxf(lmax, logit);
            }
        }
    }
    const float inv = ray_softmax_stats<false>(lmax, wts, red, T).inv;
    unsigned ray = (unsigned)ray0 + lray;                 // the ray whose at_wt rows the weights go to
    bool keep = at_wt != nullptr;
    if constexpr (LIST) {
        if (keep) {
            const int lr = rays[ray0 + lray];
            keep = lr >= 0 && lr < nraytot;
            ray = (unsigned)lr;
        }
    }
    const int b = (int)(ray / (unsigned)R), r = (int)(ray % (unsigned)R);
    ray_softmax_normalise(wts, T, inv, [&](int row, float w) {
        if (keep) {
            const int v = row / S, s = row - v * S;
            at_wt[sample_index(b, V, v, R, r, S, s)] = w;
        }
    });
    __syncthreads();
    if (tid < HC / 8) {
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        P::hid_sum(acc, wts, hid + row0 * P::HID_LD + tid * 8, T);
        P::store(hbar + (size_t)lray * HC + tid * 8, acc);
    }
}

template <bool HAVE_LOGITS>
__global__ __launch_bounds__(256) void attend_hidden_kernel(const __half* __restrict__ qa,
                                                            const __half* __restrict__ qb,
                                                            const float* __restrict__ logits,
                                                            const __half* __restrict__ hid, int V, int R, int S,
                                                            int ray0, __half* __restrict__ hbar,
                                                            float* __restrict__ at_wt) {
    attend_hidden_ray<AttendF16, HAVE_LOGITS, false>(qa, qb, logits, hid, V, R, S, ray0, hbar, at_wt, nullptr, 0);
}

template <bool LIST>
__global__ __launch_bounds__(256) void attend_hidden_f32_kernel(const float* __restrict__ qa, const float* __restrict__ qb,
                                                                const __half* __restrict__ hs, int V, int R, int S, int ray0,
                                                                float* __restrict__ hbar, float* __restrict__ at_wt,
                                                                const int* __restrict__ rays, long long nraytot) {
    attend_hidden_ray<AttendF32, false, LIST>(qa, qb, nullptr, hs, V, R, S, ray0, hbar, at_wt, rays, nraytot);
}

template <bool LIST>
int attend_hidden_f32(const float* qa, const float* qb, const uint16_t* hs, int B, int V, int R, int S, const int* rays, int ray0,
                      int nrays, float* hbar, float* at_wt, void* stream) {
    CPN_REQUIRE(qa && qb && hs && hbar && (!LIST || rays), CPN_E_ARG, "cpn_attend_hidden_f32: null pointer");
    CPN_REQUIRE(B > 0 && V == 2 && R > 0 && S > 0 && V * S <= 4096, CPN_E_SHAPE, "cpn_attend_hidden_f32: bad shape");
    CPN_REQUIRE(ray0 >= 0 && nrays > 0 && (LIST || (long long)ray0 + nrays <= (long long)B * R), CPN_E_ARG,
                "cpn_attend_hidden_f32: ray range outside B*R");
    CPN_REQUIRE(((uintptr_t)qa % 16) == 0 && ((uintptr_t)qb % 16) == 0 && ((uintptr_t)hs % 16) == 0 && ((uintptr_t)hbar % 16) == 0,
                CPN_E_ARG, "cpn_attend_hidden_f32: operands must be 16-byte aligned");
    const size_t lds = (size_t)(V * S + 8) * sizeof(float);
    hipLaunchKernelGGL(attend_hidden_f32_kernel<LIST>, dim3(nrays), dim3(256), lds, (hipStream_t)stream, qa, qb, (const __half*)hs, V,
                       R, S, ray0, hbar, at_wt, rays, (long long)B * R);
    CPN_LAUNCH_CHECK("cpn_attend_hidden_f32");
    return 0;
}

}  // namespace

extern "C" int cpn_attend_hidden(const uint16_t* qa, const uint16_t* qb, const float* logits, const uint16_t* hid, int B,
                                 int V, int R, int S, int ray0, int nrays, uint16_t* hbar, float* at_wt, void* stream) {
    CPN_REQUIRE(((qa && qb) || logits) && hid && hbar, CPN_E_ARG, "cpn_attend_hidden: null pointer");
    CPN_REQUIRE(B > 0 && V == 2 && R > 0 && S > 0 && V * S <= 4096, CPN_E_SHAPE, "cpn_attend_hidden: bad shape");
    CPN_REQUIRE(ray0 >= 0 && nrays > 0 && (long long)ray0 + nrays <= (long long)B * R, CPN_E_ARG,
                "cpn_attend_hidden: ray range outside B*R");
    const size_t lds = (size_t)(V * S + 8) * sizeof(float);
    hipLaunchKernelGGL(logits ? attend_hidden_kernel<true> : attend_hidden_kernel<false>, dim3(nrays), dim3(256), lds, (hipStream_t)stream, (const __half*)qa,
                       (const __half*)qb, logits, (const __half*)hid, V, R, S, ray0, (__half*)hbar, at_wt);
    CPN_LAUNCH_CHECK("cpn_attend_hidden");
    return 0;
}

extern "C" int cpn_attend_hidden_f32(const float* qa, const float* qb, const uint16_t* hs, int B, int V, int R, int S, int ray0,
                                     int nrays, float* hbar, float* at_wt, void* stream) {
    return attend_hidden_f32<false>(qa, qb, hs, B, V, R, S, nullptr, ray0, nrays, hbar, at_wt, stream);
}

extern "C" int cpn_attend_hidden_f32_rays(const float* qa, const float* qb, const uint16_t* hs, int B, int V, int R, int S,
                                          const int* rays, int ray0, int nrays, float* hbar, float* at_wt, void* stream) {
    return attend_hidden_f32<true>(qa, qb, hs, B, V, R, S, rays, ray0, nrays, hbar, at_wt, stream);
}
