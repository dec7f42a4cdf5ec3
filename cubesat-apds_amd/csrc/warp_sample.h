// csrc/warp_sample.h — the sampling tail of cv::remap's INTER_LINEAR fixed-point path for u8 images, one copy: the perspective warp
// (ingest.hip) and the frame undistort (lens.hip) both end in it. (X, Y) are the source coordinates in 1/32 pixel; integer part >> 5,
// the 32 x 32 table of 15-bit weights (bilinear_tab_host), (sum + 2^14) >> 15 per channel over the 2x2 footprint; a tap outside the
// source reads `border` in every channel.
#pragma once
#include <climits>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace apds {

__device__ __forceinline__ int sat_int_rn(double v) {
    return v <= (double)INT_MIN ? INT_MIN : (v >= (double)INT_MAX ? INT_MAX : __double2int_rn(v));
}

// d[0 .. CH) = the sample. CH == 4 reads and writes whole pixels as uint32_t (src and d 4-byte aligned).
template <int CH>
__device__ __forceinline__ void sample_bilinear_u8(const uint8_t* __restrict__ src, int rows, int cols, int X, int Y, const short* __restrict__ tab,
                                                   int border, uint8_t* __restrict__ d) {
    const int sx = X >> 5, sy = Y >> 5;
    const short* w = &tab[((Y & 31) * 32 + (X & 31)) * 4];
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int xx = sx + (k & 1), yy = sy + (k >> 1);
        in[k] = xx >= 0 && xx < cols && yy >= 0 && yy < rows;
    }
    if constexpr (CH == 4) {
        const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src);
        const uint32_t border_word = (uint32_t)border * 0x01010101u;
        uint32_t p[4];
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = in[k] ? s32[(size_t)(sy + (k >> 1)) * cols + sx + (k & 1)] : border_word;
        uint32_t out = 0;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int v = (int)((p[0] >> (8 * c)) & 0xFF) * w[0] + (int)((p[1] >> (8 * c)) & 0xFF) * w[1] + (int)((p[2] >> (8 * c)) & 0xFF) * w[2] +
                          (int)((p[3] >> (8 * c)) & 0xFF) * w[3];
            out |= (uint32_t)(((v + (1 << 14)) >> 15) & 0xFF) << (8 * c);
        }
        *reinterpret_cast<uint32_t*>(d) = out;
    } else {
#pragma unroll
        for (int c = 0; c < CH; c++) {
            int v = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) v += (in[k] ? (int)src[((size_t)(sy + (k >> 1)) * cols + sx + (k & 1)) * CH + c] : border) * w[k];
            d[c] = (uint8_t)((v + (1 << 14)) >> 15);
        }
    }
}

const short* bilinear_tab_host();   // ingest.hip: the 32 x 32 x 4 table (OpenCV's BilinearTab_i restated), built on first use

}  // namespace apds
