// csrc/akaze_resize.hip — the two resizes between the octaves of the AKAZE scale space: the 2 x 2 mean and general INTER_AREA.
//
// Replaces the OpenCV work behind /root/reference/feature_extraction/src/lib.rs:64-79 (AKAZE::create(...).detect_and_compute): the
// resize(INTER_AREA) calls of Create_Nonlinear_Scale_Space. Float contract as in akaze_strip.h (one IEEE binary32 operation per
// source operation, -ffp-contract=off).
#include "akaze.h"
#include "akaze_strip.h"

namespace apds {

// ---- resize(INTER_AREA) by exactly 2: mean of 2x2 ---------------------------------------------------------
// One thread = two neighbouring output pixels of HS_ROWS consecutive rows: 16-byte loads, all of a thread's loads issued before the first
// sum (one output per thread with 8-byte loads ran at 1.5 TB/s on the 4096^2 -> 2048^2 step, which sits on the level chain's critical path).
static constexpr int HS_ROWS = 4;
__global__ __launch_bounds__(256) void half_sample_kernel(const float* __restrict__ src, int sw, float* __restrict__ dst, int dw, int dh, size_t bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    APDS_BOFS(src);
    APDS_BOFS(dst);
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 2;
    const int y0 = blockIdx.y * HS_ROWS;
    if (x >= dw) return;
    // 16-byte loads need rows that start on a 16-byte boundary; 8-byte stores an even destination width
    const bool wide = x + 1 < dw && !(sw & 3) && !(dw & 1) && !((reinterpret_cast<uintptr_t>(src) & 15) | (reinterpret_cast<uintptr_t>(dst) & 7));
    if (wide) {
        float4 a[HS_ROWS], b[HS_ROWS];
#pragma unroll
        for (int r = 0; r < HS_ROWS; r++) {
            const int y = min(y0 + r, dh - 1);
            a[r] = *reinterpret_cast<const float4*>(&src[(size_t)(2 * y) * sw + 2 * x]);
            b[r] = *reinterpret_cast<const float4*>(&src[(size_t)(2 * y + 1) * sw + 2 * x]);
        }
#pragma unroll
        for (int r = 0; r < HS_ROWS; r++) {
            const int y = y0 + r;
            if (y >= dh) break;
            float2 o;
            o.x = ((a[r].x + a[r].y) + (b[r].x + b[r].y)) * 0.25f;
            o.y = ((a[r].z + a[r].w) + (b[r].z + b[r].w)) * 0.25f;
            *reinterpret_cast<float2*>(&dst[(size_t)y * dw + x]) = o;
        }
        return;
    }
    for (int r = 0; r < HS_ROWS; r++) {
        const int y = y0 + r;
        if (y >= dh) break;
        for (int xx = x; xx < min(x + 2, dw); xx++) {
            const float* p0 = &src[(size_t)(2 * y) * sw + 2 * xx];
            const float* p1 = &src[(size_t)(2 * y + 1) * sw + 2 * xx];
            dst[(size_t)y * dw + xx] = ((p0[0] + p0[1]) + (p1[0] + p1[1])) * 0.25f;
        }
    }
}

// general INTER_AREA (odd source sizes): per destination pixel, up to 4 taps per axis from host-built tables
__global__ void area_resize_kernel(const float* __restrict__ src, int sw, float* __restrict__ dst, int dw, int dh, const int* __restrict__ xofs,
                                   const float* __restrict__ xw, const int* __restrict__ xcnt, const int* __restrict__ yofs,
                                   const float* __restrict__ yw, const int* __restrict__ ycnt, size_t bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    APDS_BOFS(src);
    APDS_BOFS(dst);
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= dw || y >= dh) return;
    float sum = 0.0f;
    const int ny = ycnt[y], nx = xcnt[x];
    for (int j = 0; j < ny; j++) {
        const float* s = &src[(size_t)yofs[y * 4 + j] * sw];
        float row = 0.0f;
        for (int k = 0; k < nx; k++) row += s[xofs[x * 4 + k]] * xw[x * 4 + k];
        if (j == 0) sum = yw[y * 4 + j] * row;
        else sum += yw[y * 4 + j] * row;
    }
    dst[(size_t)y * dw + x] = sum;
}

// ---- host launchers -------------------------------------------------------------------------------------
void launch_half_sample(const float* src, int sw, float* dst, int dw, int dh, hipStream_t s, const Batch& b) {
    hipLaunchKernelGGL(half_sample_kernel, dim3(ceil_div(dw, 512), ceil_div(dh, HS_ROWS), b.n), dim3(256), 0, s, src, sw, dst, dw, dh, b.stride);
}
void launch_area_resize(const float* src, int sw, float* dst, int dw, int dh, const int* xofs, const float* xw, const int* xcnt, const int* yofs,
                        const float* yw, const int* ycnt, hipStream_t s, const Batch& b) {
    hipLaunchKernelGGL(area_resize_kernel, dim3(ceil_div(dw, 256), dh, b.n), dim3(256), 0, s, src, sw, dst, dw, dh, xofs, xw, xcnt, yofs, yw, ycnt, b.stride);
}

}  // namespace apds
