// K3b/K4 logits in UNIT order (round 5) — the per-sample query / key tails of the two attention rounds on the 16-row units the
// first-layer kernel works in (4 rays x 4 samples of one view, csrc/encode_fused.hip), so that its 128-wide key hidden layer
// reaches them as ready MFMA B fragments and the key / coords_embed matrices never exist in row-major form:
//
//   mode 0 (round 1, /root/reference models/CoPoNeRF.py:408, 446, 450):
//       ce    = query_embed_2(ReLU(query_embed(local_coords)))                         -> ce_u (unit order, for round 2)
//       key   = key_map_2(kh)            kh = cpn_encode_key's unit-order output
//       logit = <fp16(key), fp16(ce)>                                                   -> logits[row] (row order, for the sums)
//     replaces cpn_local_mlp (coords_embed) + cpn_gemm_f16_rowdot (key_map_2 + logit): one pass instead of two, kh read as
//     1 KiB fragments, 2.1 GB of coords_embed written once and read once (round 2) instead of written once and read twice.
//   mode 1 (round 2, :472-475):
//       q2    = query_repeat_embed_2(ReLU(W_l . local_coords + b + add[ray]))           add = W_z . encode_latent(z_local)
//       logit = <fp16(q2), ce_u>                                                        -> logits[row]
//     = cpn_local_mlp's logits form with the unit row map.
//   mode 2 (round 2 with coords_embed RECOMPUTED): mode 1 without its 256-byte-per-sample read of ce_u - the two query_embed
//     layers are evaluated again from the local coordinates the kernel reads anyway (56 more MFMAs per unit, the same
//     instructions in the same order as mode 0: the same bits), and mode 0 is then called with ce_u = NULL and stores nothing:
//     2.1 GB less written and 2.1 GB less read per 65 536-ray image, both kernels were bound by that traffic.
// Unit order of a (rows, 128) fp16 matrix X: [unit][32-column block p][lane = c + 16 fg][8] holds X[row(unit, c)][32 p + 8 fg .. +8],
// c = (sample & 3) * 4 + (ray & 3) — a wave's access to one block is 1 KiB of contiguous memory and IS the B operand of
// v_mfma_f32_16x16x32_f16 for the k block p.  Structure (8 waves share the layer-2 fragments in LDS, the first layer's bias on
// the unused K slot, inputs of the next unit requested before the MFMAs of the current one): cpn_local_mlp's (csrc/gather.hip).
#include <algorithm>

#include "local_units_body.h"          // the unit body: shared with cpn_attend_units (attend_units.hip), which must produce the same bits

namespace {

#ifndef CPN_LU_UNITS
#define CPN_LU_UNITS 2         // units per wave in modes 0 and 2 (mode 1 keeps one: 128 registers, four waves per SIMD)
#endif
// a wave takes the units wave_id + (it * U + u) * nwaves; past the end it walks the last unit again with nothing stored
template <int U>
struct StridedUnits {
    unsigned wave_id, nwaves, nunits;
    __device__ __forceinline__ unsigned niter() const { return wave_id < nunits ? (nunits - wave_id + U * nwaves - 1) / (U * nwaves) : 0u; }
    __device__ __forceinline__ unsigned unit(unsigned it, int u, bool& live) const {
        const unsigned x = wave_id + (it * U + (unsigned)u) * nwaves;
        live = x < nunits;
        return min(x, nunits - 1);
    }
    __device__ __forceinline__ void after(unsigned) const {}
};
struct GlobalLogits {
    float* __restrict__ logits;
    int fg;
    __device__ __forceinline__ void operator()(unsigned, int, long long srow, float d) const {
        if (srow >= 0 && fg == 0 && (!(CPN_LU_ABLATE & 8) || d == 12345.678f)) logits[srow] = d;
    }
};

template <int MODE, int U>
__global__ __launch_bounds__(512, (MODE == 2 || U > 1) ? 2 : 4) void local_units_kernel(UnitArgs args, UnitGeo geo,
                                                                                       float* __restrict__ logits) {
    __shared__ __attribute__((aligned(16))) half8 w2l[8 * 4 * 64];                       // [tile t][k block p][lane]
    __shared__ __attribute__((aligned(16))) half8 wkl[MODE != 1 ? 8 * 4 * 64 : 1];      // key_map_2 (mode 0) / query_embed_2 (mode 2), same layout
    __shared__ __attribute__((aligned(16))) float b2s[128];
    __shared__ __attribute__((aligned(16))) float bks[128];
    __shared__ __attribute__((aligned(8))) half4 w1s[(MODE == 2 ? 4 : 2) * 8 * 64];      // [set][tile][lane]
    const UnitLds L{w2l, wkl, b2s, bks, w1s};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unit_stage_weights<MODE>(L, args, (int)threadIdx.x, 512);
    __syncthreads();
    StridedUnits<U> seq{blockIdx.x * 8 + (unsigned)wave, gridDim.x * 8, (unsigned)geo.nunits};
    GlobalLogits sink{logits, lane >> 4};
    unit_walk<MODE, U>(L, args, geo, lane, seq, sink);
}

}  // namespace

extern "C" int cpn_local_units(int mode, const float* loc8, const float* coords9, const float* w1, int ldw1, const float* b1,
                               const float* add, const uint16_t* w2, int ldw2, const float* b2, const uint16_t* wk2, int ldwk2,
                               const float* bk2, const float* w1b, int ldw1b, const float* b1b, const uint16_t* kh_u, int B,
                               int V, int R, int S, int ray0, int nrays, uint16_t* ce_u, const float* lv_u, float* logits,
                               void* stream) {
    // (mode 1 - round 2 reading a STORED coords_embed - left the library in round 6: mode 2 recomputes it and is faster)
    CPN_REQUIRE(mode == 0 || mode == 2, CPN_E_ARG, "cpn_local_units: mode must be 0 or 2 (got %d)", mode);
    CPN_REQUIRE(loc8 && coords9 && w1 && b1 && w2 && b2 && logits, CPN_E_ARG, "cpn_local_units: null pointer");
    CPN_REQUIRE(mode == 0 ? (wk2 && bk2 && kh_u) : mode == 1 ? (add && ce_u) : (add && wk2 && bk2 && w1b && b1b), CPN_E_ARG,
                "cpn_local_units: null pointer for mode %d", mode);
    CPN_REQUIRE(B > 0 && V == 2 && R > 0 && S > 0 && ldw1 >= 16 && ldw2 >= 128 && (ldw2 % 8) == 0 &&
                    (mode == 1 || (ldwk2 >= 128 && (ldwk2 % 8) == 0)) && (mode != 2 || ldw1b >= 16), CPN_E_SHAPE,
                "cpn_local_units: bad shape");
    CPN_REQUIRE(ray0 >= 0 && nrays > 0 && (long long)ray0 + nrays <= (long long)B * R, CPN_E_ARG,
                "cpn_local_units: ray range outside B*R");
    CPN_REQUIRE(((uintptr_t)ce_u % 16) == 0 && ((uintptr_t)kh_u % 16) == 0 && ((uintptr_t)w2 % 16) == 0 && ((uintptr_t)wk2 % 16) == 0 &&
                    ((uintptr_t)w1 % 16) == 0 && ((uintptr_t)w1b % 16) == 0 && ((uintptr_t)lv_u % 16) == 0,
                CPN_E_ARG, "cpn_local_units: fp16 operands and first-layer weights must be 16-byte aligned");
    const UnitGeo geo = unit_geo(V, R, S, ray0, nrays);
    CPN_REQUIRE(geo.nunits * 16 < (1LL << 31), CPN_E_SHAPE, "cpn_local_units: chunk too large for 32-bit indexing");
    // lv_u covers the whole (B, R, S) problem in unit order (cpn_sample_geometry); this launch's units start at its first ray group
    const f32x4* lv_chunk = lv_u ? reinterpret_cast<const f32x4*>(lv_u) + (size_t)geo.group0 * V * geo.nsblk * 64 : nullptr;
    const unsigned blocks = (unsigned)std::min<long long>(cpn_cdiv(geo.nunits, 8), mode == 1 ? 1024 : (CPN_LU_UNITS > 1 ? 256 : 512));
    const UnitArgs args{loc8, coords9, w1, ldw1, b1, add, (const __half*)w2, ldw2, b2, (const __half*)wk2, ldwk2, bk2, w1b, ldw1b, b1b,
                        (const __half*)kh_u, (__half*)ce_u, lv_chunk};
    if (mode == 0)
        hipLaunchKernelGGL((local_units_kernel<0, CPN_LU_UNITS>), dim3(blocks), dim3(512), 0, (hipStream_t)stream, args, geo, logits);
    else
        hipLaunchKernelGGL((local_units_kernel<2, CPN_LU_UNITS>), dim3(blocks), dim3(512), 0, (hipStream_t)stream, args, geo, logits);
    CPN_LAUNCH_CHECK("cpn_local_units");
    return 0;
}
