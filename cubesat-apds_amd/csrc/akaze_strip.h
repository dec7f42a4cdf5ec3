// csrc/akaze_strip.h — device-only helpers of the AKAZE filter files: border indexing, the batch offset, the lane shifts and the
// arithmetic of the register-strip kernels (a wave owns 64 columns, one per lane, and keeps its rows in registers), one copy each.
//
// Everything here is under the float contract with oracle/akaze_oracle.cpp: one IEEE binary32 operation per source operation, in
// this order, no FMA contraction (-ffp-contract=off); symmetric taps as  acc = k0*c; acc += k1*(lo1+hi1); ...  antisymmetric taps
// as  hi - lo. A change to one of these formulas is made here - and in the two places that could not take them without their kernels
// compiling differently (profiles/filters_split/README.md): level_stream_rows (akaze_level_stream.hip) keeps stages A - D written out,
// and the FED step loop stands in nld_strip (akaze_fed.hip) and again at the end of level_strip (akaze_level_strips.hip).
#pragma once
#include "akaze.h"

namespace apds {

__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }   // BORDER_REPLICATE
__device__ __forceinline__ int reflect101(int i, int n) {                                          // BORDER_REFLECT_101
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

// APDS_BOFS(p): the plane of image blockIdx.z of a batched launch (akaze.h: bofs)
#define APDS_BOFS(p) p = bofs(p, bstride)

// ---- lane shifts ---------------------------------------------------------------------------------------------------------------
// lane_next: lane i <- lane i + 1 (DPP wave_shl:1); lane_prev: lane i <- lane i - 1 (wave_shr:1). The lane without a source (63 /
// 0) receives a value nothing may rely on (zero here, its old content with the _any forms below). That is harmless: a strip's outermost lanes are halo lanes - every shift moves the frontier of
// unspecified values one lane inwards, a kernel that shifts k times finishes lanes [k, 64 - k) and stores no others.
__device__ __forceinline__ float lane_next(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}
__device__ __forceinline__ float lane_prev(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
// The same shifts without the zero that update_dpp(0, ...) names for the lane that has no source: that lane keeps whatever its register
// held. The two streaming kernels (akaze_level_stream.hip, akaze_doh_strips.hip) were written and tuned with this spelling and compile to
// different code with the other one (and the strip kernels likewise, the other way round), so both stay, each where it was.
__device__ __forceinline__ float lane_next_any(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}
__device__ __forceinline__ float lane_prev_any(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}

// ---- Gaussian, 5 taps ----------------------------------------------------------------------------------------------------------
// the symmetric combination of a centre and its neighbours at distance 1 (a1, b1) and 2 (a2, b2): the column pass takes them from the
// lane's own rows
__device__ __forceinline__ float gauss5(const GaussTaps& taps, float c, float a1, float b1, float a2, float b2) {
    float acc = taps.k[0] * c;
    acc += taps.k[1] * (a1 + b1);
    acc += taps.k[2] * (a2 + b2);
    return acc;
}
// the row pass of one value: its neighbours at x -+ 1, 2 through lane shifts
__device__ __forceinline__ float gauss5_row(const GaussTaps& taps, float v) {
    const float l1 = lane_prev(v), r1 = lane_next(v);
    const float l2 = lane_prev(l1), r2 = lane_next(r1);
    return gauss5(taps, v, l1, r1, l2, r2);
}

// ---- Scharr (unnormalised: 3, 10, 3) and the Perona-Malik g2 conductivity ------------------------------------------------------------
// Row terms of one Lsmooth value: rd = L[x+1] - L[x-1], rs = 10 L[x] + 3 (L[x-1] + L[x+1]). REFLECT (the waves on the image border):
// reflect-101 in x - at x = 0 the left neighbour is the right one, at x = w - 1 the right neighbour is the left one.
template <bool REFLECT>
__device__ __forceinline__ void scharr_row_terms(float sm, int gx, int w, float& rd, float& rs) {
    float l = lane_prev(sm), r = lane_next(sm);
    if (REFLECT) {
        const float l0 = l;
        l = gx == 0 ? r : l;
        r = gx == w - 1 ? l0 : r;
    }
    rd = r - l;
    float a = 10.0f * sm;
    a += 3.0f * (l + r);
    rs = a;
}
// Lx = 10 rd(y) + 3 (rd(y-1) + rd(y+1)), Ly = rs(y+1) - rs(y-1) from the row terms of three rows (reflect-101 in y: the caller passes
// the other row for the missing one)
__device__ __forceinline__ void scharr_xy(float rd_up, float rd_mid, float rd_dn, float rs_up, float rs_dn, float& ax, float& ay) {
    ax = 10.0f * rd_mid;
    ax += 3.0f * (rd_up + rd_dn);
    ay = rs_dn - rs_up;
}
// g2 = 1 / (1 + |grad|^2 / k^2), k2inv = 1 / (k * k)
__device__ __forceinline__ float pm_g2_strip(float rd_up, float rd_mid, float rd_dn, float rs_up, float rs_dn, float k2inv) {
    float ax, ay;
    scharr_xy(rd_up, rd_mid, rd_dn, rs_up, rs_dn, ax, ay);
    return 1.0f / (1.0f + ((ax * ax + ay * ay) * k2inv));
}

}  // namespace apds
