// The tap of a bilinear resize with align_corners=True along one axis, and its blend, in ONE place for the resize kernel,
// its adjoint and corr_mean3 (ufc_corr.hip) and for the cost-volume attention (ufc_attn.hip): all of them must form the
// same fraction from the same index, or an "adjoint" is not the transpose of its forward.
#pragma once
#include "common.h"

namespace {

// a (1 - l) + b l as two multiplies and an add, never contracted into a multiply-add: the resize kernel and the two fused
// forms of the final correlation then produce the same bits whatever the compiler would have chosen in each of them
__device__ __forceinline__ float mix_nc(float a, float b, float l) {
#pragma clang fp contract(off)
    return a * (1.0f - l) + b * l;
}

// fine index I of an axis resized from h coarse points with scale = (h - 1) / (fine points - 1): the two coarse taps and
// the fraction towards the second, as torch forms them: a rounded product, then a difference
struct AxisTap {
    int i0, i1;
    float l;
};
__device__ __forceinline__ AxisTap axis_tap(int I, int h, float scale) {
#pragma clang fp contract(off)                                // (f - i0 must not become fma(scale, I, -i0): see mix_nc)
    const float f = scale * (float)I;
    AxisTap t;
    t.i0 = (int)f;
    t.i1 = t.i0 + (t.i0 < h - 1);
    t.l = f - (float)t.i0;
    return t;
}
__device__ __forceinline__ float blend4(float a, float b, float c, float d, float lx, float ly) {
    return mix_nc(mix_nc(a, b, lx), mix_nc(c, d, lx), ly);
}

}  // namespace
