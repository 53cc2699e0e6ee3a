// One row of the attention-weighted hidden sum, acc[e] += w * h[e] for the 8 channels of a 16-byte chunk - shared by
// cpn_attend_hidden (the fp16 trait of attend.hip's one body) and cpn_attend_units (attend_units.hip), which must produce the
// same bits.  (The f32 trait's row, w * (hi + lo), is fused on every channel and written out beside it in attend.hip; the
// workgroup softmax in front of both is ray_softmax.h.)
// The rounding is WRITTEN OUT rather than left to -ffp-contract: channels 0 .. 5 are fused multiply-adds; channels 6 and 7 of the
// rows below (T & ~3) - the rows cpn_attend_hidden has always taken four at a time - add a ROUNDED product (two roundings), the
// remaining T & 3 rows fuse all eight.  That is how attend_hidden_kernel has been compiled since it was written (the vectoriser
// split the last channel pair of the four-row block off the contraction), so it is what every recorded result, golden file and
// A/B dump of this project contains; stated here, it no longer depends on what a compiler makes of `acc += w * h` in one loop or
// another, and a second kernel can reproduce it.
#pragma once
#include "common.h"

constexpr int HID_BLOCK_ROWS = 4;        // rows below T - T % HID_BLOCK_ROWS take the two-rounding form on channels 6, 7

template <bool BLOCK_ROW>
__device__ __forceinline__ void hid_row_acc(float (&acc)[8], const float w, const half8& h) {
#pragma unroll
    for (int e = 0; e < (BLOCK_ROW ? 6 : 8); ++e) acc[e] = __builtin_fmaf(w, (float)h[e], acc[e]);
    if constexpr (BLOCK_ROW) {
#pragma clang fp contract(off)
        const float p6 = w * (float)h[6], p7 = w * (float)h[7];
        acc[6] = acc[6] + p6;
        acc[7] = acc[7] + p7;
    }
}
