// csrc/akaze_smooth_flow.hip — per level: Lsmooth and the Perona-Malik g2 conductivity in one pass, on LDS tiles and on register strips.
//
// Replaces the OpenCV work behind /root/reference/feature_extraction/src/lib.rs:64-79 (AKAZE::create(...).detect_and_compute): the
// Gaussian smoothing and the conductivity of Create_Nonlinear_Scale_Space. Float contract as in akaze_strip.h (one IEEE binary32
// operation per source operation, -ffp-contract=off).
#include "akaze.h"
#include "akaze_strip.h"

namespace apds {

// ---- per level: Lsmooth = Gaussian(5 taps, replicate) of the level's start image, and the PM-g2 conductivity from the
// Scharr gradient of Lsmooth (reflect-101), in one pass: the start image is read once, Lsmooth never comes back from HBM
// (16 -> 12 B/pixel and one launch less per level). Lsmooth is evaluated on the tile + 1 ring at in-image positions; a ring
// position outside the image is, under reflect-101, an in-image position at most one pixel inside the border, i.e. part of
// the same region, so the gradient stencil simply indexes it through the reflected coordinate. Arithmetic per value is
// that of gauss_kernel<2> followed by deriv_pair_kernel<1> (akaze_base.hip).
#ifndef APDS_SF_THREADS
#define APDS_SF_THREADS 1024
#endif
static constexpr int FW = SF_TILE_W, FH = SF_TILE_H, FNT = APDS_SF_THREADS;

// Persistent blocks: each block walks a strided list of tiles of its XCD's band and issues the loads of its NEXT tile (into
// registers) before it computes the current one, so the HBM latency of a tile hides behind the three LDS passes of the previous
// tile instead of being paid once per tile per block.
__global__ __launch_bounds__(FNT) void smooth_flow_kernel(const float* __restrict__ src, float* __restrict__ smooth, float* __restrict__ flow, int w, int h,
                                                          GaussTaps taps, const float* __restrict__ kptr, int tiles_x, int ntiles, int txi, int tyi, size_t bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    APDS_BOFS(src);
    APDS_BOFS(smooth);
    APDS_BOFS(flow);
    APDS_BOFS(kptr);
    constexpr int SW = FW + 6, SH = FH + 6;      // start image, halo 3 (= ring 1 + Gaussian radius 2), replicate on load
    constexpr int TWD = FW + 2;                  // row-pass / Lsmooth width: tile + ring 1
    constexpr int MH = FH + 2;
    constexpr int NL = (SW * SH + FNT - 1) / FNT;
    __shared__ float s_src[SH * SW];
    __shared__ float s_tmp[SH * TWD];
    __shared__ float s_sm[MH * TWD];
    // Item i of this block -> tile. Whole level: blocks go round-robin over the XCDs (gridDim.x is a multiple of 8) and each XCD
    // walks its own band of tiles. Frame only (txi > 0: tiles [1, txi) x [1, tyi) belong to smooth_flow_strip_kernel): the frame's
    // tiles are enumerated compactly — top rows, then (left column + right columns) of the middle rows, then the bottom rows — and
    // dealt out one per block, so that no block gets a whole column of them.
    const int tiles_y = ntiles / tiles_x;
    const int n_top = tiles_x, per_mid = 1 + (tiles_x - txi), n_mid = (tyi - 1) * per_mid;
    const int n_frame = n_top + n_mid + (tiles_y - tyi) * tiles_x;
    const int xcd = blockIdx.x & 7, per = txi > 0 ? (int)gridDim.x : (int)(gridDim.x >> 3);
    const int band = (ntiles + 7) >> 3;
    const int t_end = txi > 0 ? n_frame : min(ntiles, (xcd + 1) * band);
    int t = txi > 0 ? (int)blockIdx.x : xcd * band + (int)(blockIdx.x >> 3);
    auto tile_of = [&](int i) {
        if (txi <= 0) return i;
        if (i < n_top) return i;
        i -= n_top;
        if (i < n_mid) {
            const int row = i / per_mid, c = i - row * per_mid;
            return (1 + row) * tiles_x + (c == 0 ? 0 : txi + c - 1);
        }
        return tyi * tiles_x + (i - n_mid);
    };
    float v[NL];
    auto issue_loads = [&](int item) {
        const int tile = tile_of(item);
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int x0 = tx * FW, y0 = ty * FH;
        const bool inside = x0 >= 3 && y0 >= 3 && x0 + FW + 3 <= w && y0 + FH + 3 <= h;
#pragma unroll
        for (int k = 0; k < NL; k++) {
            const int i = min((int)threadIdx.x + k * FNT, SW * SH - 1);
            const int ly = i / SW, lx = i - ly * SW;
            v[k] = inside ? src[(size_t)(y0 - 3 + ly) * w + (x0 - 3 + lx)] : src[(size_t)clampi(y0 - 3 + ly, h) * w + clampi(x0 - 3 + lx, w)];
        }
    };
    if (t < t_end) issue_loads(t);
    const float k = *kptr;
    const float k2inv = 1.0f / (k * k);
    const float kside = 3.0f, kmid = 10.0f;      // unnormalised Scharr, as launch_flow passes them
    for (int tn; t < t_end; t = tn) {
        tn = t + per;
        const int tile = tile_of(t);
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int x0 = tx * FW, y0 = ty * FH;
        // the tile and its halo inside the image (all but the outermost tiles): no bounds tests, no reflected coordinates
        const bool inside = x0 >= 3 && y0 >= 3 && x0 + FW + 3 <= w && y0 + FH + 3 <= h;
#pragma unroll
        for (int kk = 0; kk < NL; kk++) {
            const int i = threadIdx.x + kk * FNT;
            if (i < SW * SH) s_src[i] = v[kk];
        }
        __syncthreads();
        if (tn < t_end) issue_loads(tn);
        for (int i = threadIdx.x; i < SH * TWD; i += FNT) {
            const int ly = i / TWD, lx = i - ly * TWD;
            const float* p = &s_src[ly * SW + lx + 2];
            float acc = taps.k[0] * p[0];
            acc += taps.k[1] * (p[-1] + p[1]);
            acc += taps.k[2] * (p[-2] + p[2]);
            s_tmp[i] = acc;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < MH * TWD; i += FNT) {
            const int ly = i / TWD, lx = i - ly * TWD;
            const float* p = &s_tmp[(ly + 2) * TWD + lx];
            float acc = taps.k[0] * p[0];
            acc += taps.k[1] * (p[-TWD] + p[TWD]);
            acc += taps.k[2] * (p[-2 * TWD] + p[2 * TWD]);
            s_sm[i] = acc;
            const int gx = x0 - 1 + lx, gy = y0 - 1 + ly;
            if (lx >= 1 && lx <= FW && ly >= 1 && ly <= FH && (inside || (gx < w && gy < h))) smooth[(size_t)gy * w + gx] = acc;
        }
        __syncthreads();
        auto flow_point = [&](const float* r0, const float* r1, const float* r2, int cxm, int cx, int cxp) {
            const float rd0 = r0[cxp] - r0[cxm], rd1 = r1[cxp] - r1[cxm], rd2 = r2[cxp] - r2[cxm];
            float ax = kmid * rd1;
            ax += kside * (rd0 + rd2);
            float rs0 = kmid * r0[cx];
            rs0 += kside * (r0[cxm] + r0[cxp]);
            float rs2 = kmid * r2[cx];
            rs2 += kside * (r2[cxm] + r2[cxp]);
            const float ay = rs2 - rs0;
            return 1.0f / (1.0f + ((ax * ax + ay * ay) * k2inv));
        };
        if (inside) {
            for (int i = threadIdx.x; i < FW * FH; i += FNT) {
                const int ly = i / FW, lx = i - ly * FW;
                const float* r1 = &s_sm[(ly + 1) * TWD];
                flow[(size_t)(y0 + ly) * w + (x0 + lx)] = flow_point(r1 - TWD, r1, r1 + TWD, lx, lx + 1, lx + 2);
            }
        } else {
            for (int i = threadIdx.x; i < FW * FH; i += FNT) {
                const int ly = i / FW, lx = i - ly * FW;
                const int gx = x0 + lx, gy = y0 + ly;
                if (gx >= w || gy >= h) continue;
                const float* r1 = &s_sm[(ly + 1) * TWD];
                if (gx >= 1 && gx <= w - 2 && gy >= 1 && gy <= h - 2) {   // only the image's outermost pixels need reflected coordinates
                    flow[(size_t)gy * w + gx] = flow_point(r1 - TWD, r1, r1 + TWD, lx, lx + 1, lx + 2);
                    continue;
                }
                const int cxm = reflect101(gx - 1, w) - (x0 - 1), cxp = reflect101(gx + 1, w) - (x0 - 1);
                flow[(size_t)gy * w + gx] = flow_point(&s_sm[(reflect101(gy - 1, h) - (y0 - 1)) * TWD], r1,
                                                       &s_sm[(reflect101(gy + 1, h) - (y0 - 1)) * TWD], cxm, lx + 1, cxp);
            }
        }
        // the next iteration's s_src stores are ordered after this iteration's row pass by the two barriers above; its row pass
        // (s_tmp) and column pass (s_sm) are each a barrier away from this iteration's readers of those planes
    }
}

// The same pass on register strips, for the tiles that lie inside the image together with their halo (no clamping, no reflection):
// a wave owns 64 columns x (RB + 6) rows, one column per lane; the 5-tap row pass takes its neighbours through lane shifts, the
// column pass and the Scharr rows come out of the lane's own registers (the formulas of akaze_strip.h). Every value is produced by
// the same operations in the same order as in smooth_flow_kernel. Lanes [3, 61) and strip rows [3, 3 + RB) are final.
static constexpr int SF_RB = 16, SF_VW = 58;

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8)))
void smooth_flow_strip_kernel(const float* __restrict__ src, float* __restrict__ smooth, float* __restrict__ flow, int w, int h, GaussTaps taps,
                              const float* __restrict__ kptr, int rx0, int ry0, int rx1, int ry1, int strips, int nwaves, size_t bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    APDS_BOFS(src);
    APDS_BOFS(smooth);
    APDS_BOFS(flow);
    APDS_BOFS(kptr);
    constexpr int RB = SF_RB, R = RB + 6;
    const int id = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (id >= nwaves) return;                   // wave-uniform; no barriers in this kernel
    const int band = __builtin_amdgcn_readfirstlane(id / strips);
    const int strip = id - band * strips;
    const int lane = threadIdx.x & 63;
    const int gx = rx0 + strip * SF_VW - 3 + lane;
    const int y0 = ry0 + band * RB, ys = y0 - 3;
    const int plane_bytes = w * h * 4;
    const __amdgpu_buffer_rsrc_t rs_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src), 0, plane_bytes, 0x00020000);
    float s[R];
#pragma unroll
    for (int r = 0; r < R; r++) s[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_src, 4 * gx, (ys + r) * w * 4, 0));
    const float k = *kptr;
    const float k2inv = 1.0f / (k * k);
#pragma unroll
    for (int r = 0; r < R; r++) s[r] = gauss5_row(taps, s[r]);   // row pass, in place
    float sm[RB + 2];                           // Lsmooth rows y0 - 1 .. y0 + RB
#pragma unroll
    for (int q = 0; q < RB + 2; q++) {
        const int r = q + 2;
        sm[q] = gauss5(taps, s[r], s[r - 1], s[r + 1], s[r - 2], s[r + 2]);
    }
    const bool mine = lane >= 3 && lane < 61 && gx < rx1;
    float rd[RB + 2], rs[RB + 2];
#pragma unroll
    for (int q = 0; q < RB + 2; q++) scharr_row_terms<false>(sm[q], gx, w, rd[q], rs[q]);
    if (mine) {
        const __amdgpu_buffer_rsrc_t rs_sm = __builtin_amdgcn_make_buffer_rsrc(smooth, 0, plane_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rs_fl = __builtin_amdgcn_make_buffer_rsrc(flow, 0, plane_bytes, 0x00020000);
#pragma unroll
        for (int q = 1; q <= RB; q++) {
            const int gy = y0 + q - 1;
            if (gy < ry1) {
                const float fl = pm_g2_strip(rd[q - 1], rd[q], rd[q + 1], rs[q - 1], rs[q + 1], k2inv);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, sm[q]), rs_sm, 4 * gx, gy * w * 4, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, fl), rs_fl, 4 * gx, gy * w * 4, 0);
            }
        }
    }
}

// ---- host launcher --------------------------------------------------------------------------------------
// grid of a persistent tile kernel with two 1024-thread blocks per CU: a multiple of 8 (one slice per XCD), at most 2 x 256 blocks
static int persistent_grid(int ntiles) {
    return std::min((ntiles + 7) & ~7, 512);
}

void launch_smooth_flow(const float* src, float* smooth, float* flow, int w, int h, const GaussTaps& taps, const float* kptr, hipStream_t s, const Batch& b,
                        bool strips_on) {
    const int tiles_x = ceil_div(w, FW), tiles_y = ceil_div(h, FH), ntiles = tiles_x * tiles_y;
    // tiles [1, txi) x [1, tyi) lie inside the image with their 3-pixel halo: register strips; the frame around them: LDS tiles
    int txi, tyi;
    smooth_flow_interior(w, h, txi, tyi);
    if (strips_on) {
        APDS_REQUIRE(txi > 1 && tyi > 1 && fits_32bit_offsets(w, h), APDS_ERR_INTERNAL, "smooth_flow strips: an interior tile, 32-bit offsets");
        const int rx0 = FW, ry0 = FH, rx1 = txi * FW, ry1 = tyi * FH;
        const int strips = ceil_div(rx1 - rx0, SF_VW), nwaves = strips * ceil_div(ry1 - ry0, SF_RB);
        hipLaunchKernelGGL(smooth_flow_strip_kernel, dim3(ceil_div(nwaves, 4), 1, b.n), dim3(256), 0, s, src, smooth, flow, w, h, taps, kptr, rx0, ry0, rx1, ry1,
                           strips, nwaves, b.stride);
    }
    if (strips_on) {   // the frame: one tile per block
        const int n_frame = tiles_x + (tyi - 1) * (1 + tiles_x - txi) + (tiles_y - tyi) * tiles_x;
        hipLaunchKernelGGL(smooth_flow_kernel, dim3(n_frame, 1, b.n), dim3(FNT), 0, s, src, smooth, flow, w, h, taps, kptr, tiles_x, ntiles, txi, tyi, b.stride);
    } else {
        hipLaunchKernelGGL(smooth_flow_kernel, dim3(persistent_grid(ntiles), 1, b.n), dim3(FNT), 0, s, src, smooth, flow, w, h, taps, kptr, tiles_x, ntiles, 0, 0,
                           b.stride);
    }
}

}  // namespace apds
