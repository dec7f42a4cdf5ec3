// csrc/bf16_round.h — f32 -> bf16, round to nearest even: the one copy, for the L2 screen's operands (l2_screen.hip) and for the train side a
// float view's gather writes (keypoint_select.hip). The two must agree bit for bit: the screen's error bound is stated on these values.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace apds {

__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {
    uint32_t x = __float_as_uint(f);
    if ((x & 0x7F800000u) == 0x7F800000u) return (uint16_t)(x >> 16) | ((x & 0xFFFFu) ? 0x40 : 0);   // inf / nan
    x += 0x7FFFu + ((x >> 16) & 1u);
    return (uint16_t)(x >> 16);
}

}  // namespace apds
