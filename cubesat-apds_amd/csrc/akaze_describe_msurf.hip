// csrc/akaze_describe_msurf.hip — AKAZE's float descriptor (DESCRIPTOR_KAZE: M-SURF, 64 x f32, unit length, compared with NORM_L2) on gfx950,
// one wave per keypoint.
//
// Restates OpenCV 4.8 AKAZEFeatures.cpp MSURF_Descriptor_64_Invoker::Get_MSURF_Descriptor_64 (from memory: DESIGN.md section 2). The reference
// crate never asks for it (feature_extraction/src/lib.rs:64-73 fixes DESCRIPTOR_MLDB); it is what fills the input of the float L2 matcher
// (l2_match.hip). orientation_kernel (akaze_describe.hip) runs unchanged in front of it.
#include "akaze.h"
#include "akaze_describe.h"
#include "config.h"

namespace apds {

// g1 of a cell's 9 x 9 samples: the sample (k, l) of the cell with centre (ky, kx) = (i + 5, j + 5) lies scale * ((k - ky), (l - kx)) from the
// centre in the rotated frame whatever the angle, so exp(-((xs - sample_x)^2 + (ys - sample_y)^2) / (2 (2.5 scale)^2)) is
// exp(-((a - 5)^2 + (b - 5)^2) / 12.5) with a = k - i, b = l - j in 0 .. 8: one table for every keypoint. The factors are e(t) = exp(-t^2 / 12.5)
// for t = 0 .. 5, multiplied in double and rounded once.
struct MsurfG1 {
    float v[81];
};
constexpr MsurfG1 make_msurf_g1() {
    constexpr double e[6] = {1.0,
                             0.92311634638663576,     // exp(-1 / 12.5)
                             0.72614903707369094,     // exp(-4 / 12.5)
                             0.48675225595997168,     // exp(-9 / 12.5)
                             0.27803730045319414,     // exp(-16 / 12.5)
                             0.13533528323661270};    // exp(-25 / 12.5)
    MsurfG1 t{};
    for (int a = 0; a < 9; a++)
        for (int b = 0; b < 9; b++) t.v[a * 9 + b] = (float)(e[a < 5 ? 5 - a : a - 5] * e[b < 5 ? 5 - b : b - 5]);
    return t;
}
__constant__ MsurfG1 c_msurf_g1 = make_msurf_g1();

__device__ __forceinline__ int clampi_ms(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// One wave per keypoint, four keypoints per block (the shape of mldb_kernel). The 16 cells (origins -12, -7, -2, 3 in both directions, 9 x 9
// samples each) overlap and draw on ONE lattice of offsets (k, l) in [-12, 12)^2, and a sample's bilinear (rx, ry) depends on (k, l) only. So:
//   phase 1: the 64 lanes gather the 576 lattice points, nine each - the four corners of a point are four float2 loads of the interleaved
//            (Lx, Ly) plane, all 36 of a lane in flight before the first LDS store - blend, rotate once, and store the two unweighted values
//            (-rx si + ry co, rx co + ry si) to two per-wave LDS planes;
//   phase 2: the 64 lanes ARE the 64 outputs, lane = cell * 4 + component: each sums its cell's 81 terms g1 * value (|.| for components 2, 3)
//            k-major, l-minor, scales by the cell's g2;
//   the norm is a wave reduction and the row one coalesced 256-byte store.
// LDS: a lane of phase 2 reads word 24 * (5 ci + a) + 5 cj + b of plane (component & 1): the 16 cells' words fall into 16 different banks
// (120 ci + 5 cj mod 64, and mod 32), components 0 / 2 and 1 / 3 read the same word (a broadcast), and the plane pitch 580 = 4 mod 32 puts
// the second plane's 16 words into 16 banks the first leaves free: no conflict. Phase 1 stores consecutive words.
// plane_level >= 0: every keypoint is described on level `plane_level` whatever its class_id (apds_dev_akaze_describe_float: the caller's
// plane is the level).
__global__ __launch_bounds__(256) void msurf_kernel(LevelTable T, const apds_keypoint* __restrict__ kps, const int* __restrict__ range, int n_cap, size_t kp_bstride,
                                                    float* __restrict__ desc, size_t desc_bstride, int xcd_ranges, int plane_level) {
    APDS_RAISE_WAVE_PRIORITY();
    const int begin = range ? bofs(range, T.bstride)[0] : 0;
    const int n = range ? min(bofs(range, T.bstride)[1], n_cap) : n_cap;
    kps = bofs(kps, kp_bstride);
    desc = bofs(desc, desc_bstride);
    constexpr int LW = 24;                  // lattice width: offsets -12 .. 11
    constexpr int NP = LW * LW;             // 576 = 9 x 64 points
    constexpr int PL = NP + 4;              // plane pitch (see above)
    constexpr int NS = NP / 64;             // points per lane
    __shared__ float s_rot[4][2 * PL];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // phase 2's view of the lane: output `lane` is component `comp` of cell (ci, cj)
    const int comp = lane & 3, ci = lane >> 4, cj = (lane >> 2) & 3;
    const float* const cell = &s_rot[wv][(comp & 1) * PL + (5 * ci) * LW + 5 * cj];
    const float g2 = expf(-(((float)ci - 1.5f) * ((float)ci - 1.5f) + ((float)cj - 1.5f) * ((float)cj - 1.5f)) / 4.5f);
    KP_GROUP_LOOP(kb, begin, n, xcd_ranges) {   // block-uniform trip count
    const int ki = kb + wv;
    const bool live = ki < n;
    const apds_keypoint kp = kps[live ? ki : kb];
    const int lvl = clampi_ms(plane_level >= 0 ? plane_level : kp.class_id, T.n);
    const int w = T.w[lvl], h = T.h[lvl];
    const float2* __restrict__ Lxy = bofs(T.Lxy[lvl], T.bstride);
    const float ratio = (float)(1 << kp.octave);
    const float scale = (float)__float2int_rn(0.5f * kp.size / ratio);
    const float xf = kp.x / ratio, yf = kp.y / ratio;
    const float angle = kp.angle * (float)(3.14159265358979323846 / 180.f);
    double sd, cd;
    det_sincos((double)angle, sd, cd);
    const float co = (float)cd, si = (float)sd;
    {
        float2 d[NS][4];
        float fx[NS], fy[NS];
#pragma unroll
        for (int j = 0; j < NS; j++) {
            const int sidx = lane + 64 * j;
            const int k = -12 + sidx / LW, l = -12 + sidx % LW;
            const float sample_y = yf + (l * scale * co + k * scale * si);
            const float sample_x = xf + (-l * scale * si + k * scale * co);
            // floor, then the clamp to the plane: every index below is inside [0, w) x [0, h) whatever the keypoint holds
            const int xa = (int)floorf(sample_x), ya = (int)floorf(sample_y);
            const int x1 = clampi_ms(xa, w), y1 = clampi_ms(ya, h);
            const int x2 = clampi_ms(min(xa, w - 1) + 1, w), y2 = clampi_ms(min(ya, h - 1) + 1, h);
            fx[j] = sample_x - (float)x1;
            fy[j] = sample_y - (float)y1;
            d[j][0] = Lxy[(size_t)y1 * w + x1];
            d[j][1] = Lxy[(size_t)y1 * w + x2];
            d[j][2] = Lxy[(size_t)y2 * w + x1];
            d[j][3] = Lxy[(size_t)y2 * w + x2];
        }
#pragma unroll
        for (int j = 0; j < NS; j++) {
            const float w11 = (1.0f - fx[j]) * (1.0f - fy[j]), w21 = fx[j] * (1.0f - fy[j]), w12 = (1.0f - fx[j]) * fy[j], w22 = fx[j] * fy[j];
            const float rx = w11 * d[j][0].x + w21 * d[j][1].x + w12 * d[j][2].x + w22 * d[j][3].x;
            const float ry = w11 * d[j][0].y + w21 * d[j][1].y + w12 * d[j][2].y + w22 * d[j][3].y;
            s_rot[wv][lane + 64 * j] = -rx * si + ry * co;        // rrx / g1
            s_rot[wv][PL + lane + 64 * j] = rx * co + ry * si;    // rry / g1
        }
    }
    wave_lds_phase();
    float acc = 0.0f;
#pragma unroll 1
    for (int a = 0; a < 9; a++) {   // (a row at a time, as mldb_kernel: fully unrolled, the 81 loads are hoisted together)
        const float* row = cell + a * LW;
#pragma unroll
        for (int b = 0; b < 9; b++) {
            const float t = c_msurf_g1.v[a * 9 + b] * row[b];
            acc += comp >= 2 ? fabsf(t) : t;
        }
    }
    const float val = acc * g2;
    float len_sq = val * val;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) len_sq += __shfl_xor(len_sq, off);   // (xor butterfly: every lane ends with the same sum)
    // OpenCV divides by sqrt(len_sq) unconditionally: a flat patch would be 64 NaNs and poison every distance of the matcher - it is 64 zeros here
    const float inv = len_sq > 0.0f ? 1.0f / sqrtf(len_sq) : 0.0f;
    if (live) desc[(size_t)ki * 64 + lane] = val * inv;
    wave_lds_phase();   // the next keypoint reuses the wave's LDS slices
    }
}

void launch_msurf(const LevelTable& T, const apds_keypoint* kps, const int* range, int n_cap, size_t kp_bstride, float* desc, size_t desc_bstride, int blocks,
                  int batch, int xcd_ranges, int plane_level, hipStream_t s) {
    hipLaunchKernelGGL(msurf_kernel, dim3(blocks, 1, batch), dim3(256), 0, s, T, kps, range, n_cap, kp_bstride, desc, desc_bstride, xcd_ranges, plane_level);
}

// apds_dev_akaze_describe_float: the describe stage alone on one caller-supplied plane
void msurf_describe_plane_device(const float2* lxy, int w, int h, const apds_keypoint* kps, int n, float* desc, hipStream_t s) {
    if (n <= 0) return;
    LevelTable T{};
    T.n = 1;
    T.bstride = 0;
    T.w[0] = w;
    T.h[0] = h;
    T.Lxy[0] = lxy;
    launch_msurf(T, kps, nullptr, n, 0, desc, 0, ceil_div(n, 4), 1, 0, 0, s);
    HIP_CHECK(hipGetLastError());
}

}  // namespace apds
