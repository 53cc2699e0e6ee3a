// The float -> byte rule of the outputs a user writes to a file (cpn_pack_frames' frames, cpn_compact_points' colours), once.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ uint8_t to_byte(float v) {      // v in grey levels; NaN -> 0
    if (!(v == v)) return 0;
    return (uint8_t)rintf(fminf(fmaxf(v, 0.f), 255.f));
}

}  // namespace
