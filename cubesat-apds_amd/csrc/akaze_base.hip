// csrc/akaze_base.hip — the base stage of the AKAZE scale space on gfx950: gray conversion, the two Gaussians, the Scharr pair, the
// fused register-strip form of all of them, and the contrast factor from the gradient histogram.
//
// Replaces the OpenCV work behind /root/reference/feature_extraction/src/lib.rs:64-79 (AKAZE::create(...)
// .detect_and_compute). The other stages of the scale space: akaze_smooth_flow.hip (smoothing + conductivity), akaze_fed.hip (FED
// steps), akaze_level_fused.hip / akaze_level_strips.hip / akaze_level_stream.hip (a whole level step), akaze_resize.hip,
// akaze_doh_tiles.hip / akaze_doh_strips.hip (determinant of the Hessian).
//
// All planes are f32, row-major, pitch == width, resident in HBM. These kernels are HBM-bandwidth bound:
// every stencil stages its input tile (+halo, border already applied) in LDS once, so each plane is read
// from HBM once per pass and written once; rows are read as contiguous 256-byte wave accesses.
//
// Float contract (identical to oracle/akaze_oracle.cpp, and what makes keypoint sets bit-equal): one IEEE
// binary32 operation per source operation, no FMA contraction (-ffp-contract=off), correctly rounded
// division; symmetric taps as  acc = k0*c; acc += k1*(lo1+hi1); ...  antisymmetric taps as  hi - lo.
#include "akaze.h"
#include "akaze_strip.h"

namespace apds {

// ---- a1.1: BGR(A)/gray u8 -> f32 in [0,1] ----------------------------------------------------------
__global__ void gray_kernel(const uint8_t* __restrict__ img, int rows, int cols, int channels, size_t stride, float* __restrict__ out, size_t img_bstride,
                            size_t bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    img += (size_t)blockIdx.z * img_bstride;
    APDS_BOFS(out);
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= cols) return;
    const uint8_t* p = img + (size_t)y * stride;
    int g;
    if (channels == 1) {
        g = p[x];
    } else if (channels == 4) {
        const uint32_t v = reinterpret_cast<const uint32_t*>(p)[x];   // B,G,R,A little endian (rows are 4-byte aligned)
        g = (int)((v & 0xFF) * 3735u + ((v >> 8) & 0xFF) * 19235u + ((v >> 16) & 0xFF) * 9798u + (1u << 14)) >> 15;
    } else {
        const uint8_t* q = p + (size_t)x * 3;
        g = (q[0] * 3735 + q[1] * 19235 + q[2] * 9798 + (1 << 14)) >> 15;
    }
    out[(size_t)y * cols + x] = (float)g * (float)(1.0 / 255.0);
}

// ---- separable symmetric blur, BORDER_REPLICATE (GaussianBlur) --------------------------------------
static constexpr int TW = 64, TH = 16;   // output tile, 256 threads

template <int R>
__global__ __launch_bounds__(256) void gauss_kernel(const float* __restrict__ src, float* __restrict__ dst, int w, int h, GaussTaps taps, size_t bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    APDS_BOFS(src);
    APDS_BOFS(dst);
    __shared__ float s_src[(TH + 2 * R) * (TW + 2 * R)];
    __shared__ float s_tmp[(TH + 2 * R) * TW];
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    constexpr int SW = TW + 2 * R, SH = TH + 2 * R;
    for (int i = threadIdx.x; i < SW * SH; i += 256) {
        const int ly = i / SW, lx = i - ly * SW;
        const int gx = clampi(x0 - R + lx, w), gy = clampi(y0 - R + ly, h);
        s_src[i] = src[(size_t)gy * w + gx];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SH * TW; i += 256) {
        const int ly = i / TW, lx = i - ly * TW;
        const float* p = &s_src[ly * SW + lx + R];
        float acc = taps.k[0] * p[0];
#pragma unroll
        for (int j = 1; j <= R; j++) acc += taps.k[j] * (p[-j] + p[j]);
        s_tmp[i] = acc;
    }
    __syncthreads();
    const int lx = threadIdx.x & 63;
    for (int ly = threadIdx.x >> 6; ly < TH; ly += 4) {
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx < w && gy < h) {
            const float* p = &s_tmp[(ly + R) * TW + lx];
            float acc = taps.k[0] * p[0];
#pragma unroll
            for (int j = 1; j <= R; j++) acc += taps.k[j] * (p[-j * TW] + p[j * TW]);
            dst[(size_t)gy * w + gx] = acc;
        }
    }
}

// ---- dilated 3x3 derivative pair, BORDER_REFLECT_101 ------------------------------------------------
// Lx = colsmooth(row: hi - lo), Ly = coldiff(row: smooth); taps at -s, 0, +s; smooth = {kside, kmid, kside}.
// MODE 0: write Lx, Ly.  MODE 1: write flow = 1/(1 + (Lx^2+Ly^2)/k^2)  (k read from device memory).
// MODE 2: write |grad| and atomically track its maximum over interior pixels (contrast factor pass).
template <int MODE>
__global__ __launch_bounds__(256) void deriv_pair_kernel(const float* __restrict__ src, float* __restrict__ outA, float* __restrict__ outB,
                                                         int w, int h, int s, float kside, float kmid, const float* __restrict__ kptr,
                                                         unsigned int* __restrict__ hmax_bits, size_t bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    APDS_BOFS(src);
    APDS_BOFS(outA);
    APDS_BOFS(outB);
    APDS_BOFS(kptr);
    APDS_BOFS(hmax_bits);
    extern __shared__ float smem[];
    const int SW = TW + 2 * s, SH = TH + 2 * s;
    float* s_src = smem;                 // SH x SW
    float* s_rd = s_src + SH * SW;       // SH x TW   row pass, derivative
    float* s_rs = s_rd + SH * TW;        // SH x TW   row pass, smooth
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    for (int i = threadIdx.x; i < SW * SH; i += 256) {
        const int ly = i / SW, lx = i - ly * SW;
        const int gx = reflect101(x0 - s + lx, w), gy = reflect101(y0 - s + ly, h);
        s_src[i] = src[(size_t)gy * w + gx];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SH * TW; i += 256) {
        const int ly = i / TW, lx = i - ly * TW;
        const float* p = &s_src[ly * SW + lx + s];
        const float lo = p[-s], hi = p[s];
        s_rd[i] = hi - lo;
        float acc = kmid * p[0];
        acc += kside * (lo + hi);
        s_rs[i] = acc;
    }
    __syncthreads();
    float k2inv = 0.f;
    if (MODE == 1) {
        const float k = *kptr;
        k2inv = 1.0f / (k * k);
    }
    float local_max = 0.f;
    const int lx = threadIdx.x & 63;
    for (int ly = threadIdx.x >> 6; ly < TH; ly += 4) {
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx < w && gy < h) {
            const int c = (ly + s) * TW + lx;
            float ax = kmid * s_rd[c];
            ax += kside * (s_rd[c - s * TW] + s_rd[c + s * TW]);
            const float ay = s_rs[c + s * TW] - s_rs[c - s * TW];
            const size_t o = (size_t)gy * w + gx;
            if (MODE == 0) {
                outA[o] = ax;
                outB[o] = ay;
            } else if (MODE == 1) {
                outA[o] = 1.0f / (1.0f + ((ax * ax + ay * ay) * k2inv));
            } else {
                const float m = sqrtf(ax * ax + ay * ay);
                outA[o] = m;
                if (gx >= 1 && gx < w - 1 && gy >= 1 && gy < h - 1) local_max = fmaxf(local_max, m);
            }
        }
    }
    if (MODE == 2) {
        // non-negative floats order like their bit patterns. One atomic per BLOCK, and only if it can raise the maximum
        // (a stale read of *hmax_bits is never larger than the truth, so no update is lost).
        __shared__ unsigned int s_wmax[4];
        unsigned int bits = __float_as_uint(local_max);
        for (int off = 32; off > 0; off >>= 1) bits = max(bits, (unsigned int)__shfl_xor((int)bits, off));
        if ((threadIdx.x & 63) == 0) s_wmax[threadIdx.x >> 6] = bits;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned int b = max(max(s_wmax[0], s_wmax[1]), max(s_wmax[2], s_wmax[3]));
            if (b > *reinterpret_cast<volatile unsigned int*>(hmax_bits)) atomicMax(hmax_bits, b);
        }
    }
}

// ---- a1.1 + a1.2 + the gradient pass of a1.3 on register strips (large images) ---------------------------------------------------
// image -> gray (registers) -> { 9-tap Gaussian -> Lt[0] } and { 5-tap Gaussian -> unnormalised Scharr -> |grad| + its maximum over
// the interior }: one read of the image instead of gray_kernel, gauss_kernel<4>, gauss_kernel<2> and deriv_pair_kernel<2> with
// their three f32 round trips. A wave owns 64 columns x (RB + 8) rows, one column per lane; x +- 1 .. 4 come through chained lane
// shifts (the same shifted values serve both Gaussians). Borders: both Gaussians replicate THE GRAY IMAGE, which clamped
// loads give for free; the Scharr pass reflects (101) its input, the 5-tap result, so at the image edge the missing neighbour is
// the opposite one (lane x + 1 for x - 1 at x = 0, row 1 for row -1, ...): selects in the BORDER waves only. Same operations in
// the same order as the four kernels it replaces. Lanes [4, 60) and strip rows [4, 4 + RB) are final.
#ifndef APDS_BS_RB
#define APDS_BS_RB 8
#endif
#ifndef APDS_BS_WAVES
#define APDS_BS_WAVES 4
#endif
static constexpr int BS_RB = APDS_BS_RB, BS_VW = 56;

template <int CH, bool BORDER>
__device__ __forceinline__ void base_strip(const uint8_t* __restrict__ img, int w, int h, int stride, const GaussTaps& g16, const GaussTaps& g10,
                                           float* __restrict__ Lt0, float* __restrict__ modg, unsigned int* __restrict__ hmax_bits, int want_modg, int gx0,
                                           int y0) {
    constexpr int RB = BS_RB, R = RB + 8;
    const int lane = threadIdx.x & 63;
    const int gx = gx0 + lane, ys = y0 - 4;
    const int cx = BORDER ? clampi(gx, w) : gx;
    const __amdgpu_buffer_rsrc_t r_img = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(img), 0, h * stride, 0x00020000);
    float h9[R], h5[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int row = (BORDER ? clampi(ys + r, h) : ys + r) * stride;   // scalar
        int gi;
        if (CH == 4) {
            const uint32_t v = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(r_img, 4 * cx, row, 0);   // B,G,R,A little endian
            gi = (int)((v & 0xFF) * 3735u + ((v >> 8) & 0xFF) * 19235u + ((v >> 16) & 0xFF) * 9798u + (1u << 14)) >> 15;
        } else if (CH == 3) {
            const int b = __builtin_amdgcn_raw_buffer_load_b8(r_img, 3 * cx, row, 0), g = __builtin_amdgcn_raw_buffer_load_b8(r_img, 3 * cx + 1, row, 0),
                      rr = __builtin_amdgcn_raw_buffer_load_b8(r_img, 3 * cx + 2, row, 0);
            gi = (b * 3735 + g * 19235 + rr * 9798 + (1 << 14)) >> 15;
        } else {
            gi = __builtin_amdgcn_raw_buffer_load_b8(r_img, cx, row, 0);
        }
        // (the 9-tap and the 5-tap row pass share the shifted values and the pair sums p1, p2: written out, not gauss5_row)
        const float v = (float)gi * (float)(1.0 / 255.0);
        const float l1 = lane_prev(v), r1 = lane_next(v);
        const float l2 = lane_prev(l1), r2 = lane_next(r1);
        const float l3 = lane_prev(l2), r3 = lane_next(r2);
        const float l4 = lane_prev(l3), r4 = lane_next(r3);
        const float p1 = l1 + r1, p2 = l2 + r2;
        float a = g16.k[0] * v;
        a += g16.k[1] * p1;
        a += g16.k[2] * p2;
        a += g16.k[3] * (l3 + r3);
        a += g16.k[4] * (l4 + r4);
        h9[r] = a;
        float b5 = g10.k[0] * v;
        b5 += g10.k[1] * p1;
        b5 += g10.k[2] * p2;
        h5[r] = b5;
    }
    const bool mine = lane >= 4 && lane < 60 && gx < w;
    const int plane_bytes = w * h * 4;
    {
        const __amdgpu_buffer_rsrc_t r_lt = __builtin_amdgcn_make_buffer_rsrc(Lt0, 0, plane_bytes, 0x00020000);
#pragma unroll
        for (int q = 0; q < RB; q++) {
            const int r = q + 4;
            float a = g16.k[0] * h9[r];
#pragma unroll
            for (int j = 1; j <= 4; j++) a += g16.k[j] * (h9[r - j] + h9[r + j]);
            if (mine && (!BORDER || y0 + q < h)) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, a), r_lt, 4 * gx, (y0 + q) * w * 4, 0);
        }
    }
    if (!want_modg) return;                     // uniform
    float rd[RB + 2], rs[RB + 2];               // image rows y0 - 1 .. y0 + RB
#pragma unroll
    for (int q = 0; q < RB + 2; q++) {
        const int r = q + 3;
        const float sm = gauss5(g10, h5[r], h5[r - 1], h5[r + 1], h5[r - 2], h5[r + 2]);
        scharr_row_terms<BORDER>(sm, gx, w, rd[q], rs[q]);   // reflect-101 of the Gaussian's output
    }
    float local_max = 0.f;
    const __amdgpu_buffer_rsrc_t r_mg = __builtin_amdgcn_make_buffer_rsrc(modg, 0, plane_bytes, 0x00020000);
#pragma unroll
    for (int q = 1; q <= RB; q++) {
        const int gy = y0 + q - 1;
        float rd_up = rd[q - 1], rd_dn = rd[q + 1], rs_up = rs[q - 1], rs_dn = rs[q + 1];
        if (BORDER) {
            if (gy == 0) {
                rd_up = rd[q + 1];
                rs_up = rs[q + 1];
            }
            if (gy == h - 1) {
                rd_dn = rd[q - 1];
                rs_dn = rs[q - 1];
            }
        }
        float ax, ay;
        scharr_xy(rd_up, rd[q], rd_dn, rs_up, rs_dn, ax, ay);
        const float m = sqrtf(ax * ax + ay * ay);
        if (mine && (!BORDER || gy < h)) {
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, m), r_mg, 4 * gx, gy * w * 4, 0);
            if (!BORDER || (gx >= 1 && gx < w - 1 && gy >= 1 && gy < h - 1)) local_max = fmaxf(local_max, m);
        }
    }
    // non-negative floats order like their bit patterns; one atomic per wave, and only if it can raise the maximum
    unsigned int bits = __float_as_uint(local_max);
    for (int off = 32; off > 0; off >>= 1) bits = max(bits, (unsigned int)__shfl_xor((int)bits, off));
    if (lane == 0 && bits > *reinterpret_cast<volatile unsigned int*>(hmax_bits)) atomicMax(hmax_bits, bits);
}

template <int CH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(APDS_BS_WAVES, 8)))
void base_strip_kernel(const uint8_t* __restrict__ img, int w, int h, int stride, GaussTaps g16, GaussTaps g10, float* __restrict__ Lt0,
                       float* __restrict__ modg, unsigned int* __restrict__ hmax_bits, int want_modg, int strips, int nwaves, size_t img_bstride, size_t bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    img += (size_t)blockIdx.z * img_bstride;
    APDS_BOFS(Lt0);
    APDS_BOFS(modg);
    APDS_BOFS(hmax_bits);
    const int id = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (id >= nwaves) return;                   // wave-uniform; no barriers in this kernel
    const int band = __builtin_amdgcn_readfirstlane(id / strips);
    const int strip = id - band * strips;
    const int gx0 = strip * BS_VW - 4, y0 = band * BS_RB;
    const bool border = gx0 < 0 || gx0 + 64 > w || y0 - 4 < 0 || y0 + BS_RB + 4 > h;
    if (border) base_strip<CH, true>(img, w, h, stride, g16, g10, Lt0, modg, hmax_bits, want_modg, gx0, y0);
    else base_strip<CH, false>(img, w, h, stride, g16, g10, Lt0, modg, hmax_bits, want_modg, gx0, y0);
}

// ---- contrast factor: 300-bin histogram of |grad|/hmax over interior pixels, 70th percentile -----------
// SUB sub-histograms per block (lane & (SUB - 1) picks one): gradient magnitudes crowd the low bins, so with one histogram most of a
// wave's 64 LDS atomics hit a handful of addresses and serialise; each thread reads four consecutive pixels of a row per step.
template <int SUB>
__global__ __launch_bounds__(256) void kcontrast_hist_kernel(const float* __restrict__ modg, int w, int h, const unsigned int* __restrict__ hmax_bits,
                                                              int* __restrict__ hist, size_t bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    APDS_BOFS(modg);
    APDS_BOFS(hmax_bits);
    APDS_BOFS(hist);
    constexpr int PITCH = 301;                          // odd pitch: the copies of a bin sit in different banks
    __shared__ int s_hist[SUB * PITCH];
    for (int i = threadIdx.x; i < SUB * PITCH; i += 256) s_hist[i] = 0;
    __syncthreads();
    const float hmax = __uint_as_float(*hmax_bits);
    if (hmax != 0.0f) {
        const float scale = 299.0f / hmax;
        const int cw = w - 2, ch = h - 2;
        int* mine = s_hist + (threadIdx.x & (SUB - 1)) * PITCH;
        const int groups = (cw + 3) >> 2;               // 4-pixel groups per interior row
        const long long total = (long long)groups * ch;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
            const int y = (int)(i / groups), x = (int)(i - (long long)y * groups) * 4;
            const float* p = modg + (size_t)(y + 1) * w + (x + 1);
            const int n = min(4, cw - x);
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = k < n ? p[k] : 0.0f;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < n) atomicAdd(&mine[(int)(v[k] * scale)], 1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 300; i += 256) {
        int sum = 0;
#pragma unroll
        for (int sidx = 0; sidx < SUB; sidx++) sum += s_hist[sidx * PITCH + i];
        if (sum) atomicAdd(&hist[i], sum);
    }
}
// histogram -> kcontrast and its per-octave values k, k*0.75, (k*0.75)*0.75, ... One wave: lane l owns bins [5l, 5l + 5), a wave scan gives
// every bin the count of the bins in front of it, and the first bin b >= 1 with (bins 1 .. b-1) >= the 70 % threshold names k - the value the
// sequential loop of the reference (nldiffusion_functions.cpp compute_k_percentile) stops at. (Round 4 measured this inside the histogram
// kernel, done by the block that draws the last of gridDim.x tickets: 1024 same-address device-scope atomics behind 1024 fences took the
// histogram kernel from 43 to 81 us - 139 beside a Hessian kernel. A launch of its own, 300 loads wide instead of 300 loads deep, is cheaper.)
__global__ __launch_bounds__(64) void kcontrast_finish_kernel(const int* __restrict__ hist, const unsigned int* __restrict__ hmax_bits, int w, int h,
                                                               float* __restrict__ k_oct, int n_oct, size_t bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    APDS_BOFS(hist);
    APDS_BOFS(hmax_bits);
    APDS_BOFS(k_oct);
    const int lane = threadIdx.x;
    const float hmax = __uint_as_float(*hmax_bits);
    constexpr int nbins = 300;
    int v[5], mine = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int bin = lane * 5 + j;
        v[j] = bin < nbins ? hist[bin] : 0;
        if (bin >= 1) mine += v[j];
    }
    const int h0 = __shfl(v[0], 0);
    int incl = mine;    // inclusive scan over lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    float k = 0.03f;
    if (hmax != 0.0f && w > 2 && h > 2) {
        const int total = (w - 2) * (h - 2);
        const int nthreshold = (int)((total - h0) * 0.7f);
        int before = incl - mine;   // bins 1 .. 5 * lane - 1
        int hit = nbins;
#pragma unroll
        for (int j = 0; j < 5; j++) {
            const int bin = lane * 5 + j;
            if (bin >= 1 && bin < nbins && before >= nthreshold && hit == nbins) hit = bin;
            if (bin >= 1) before += v[j];
        }
        const unsigned long long any = __ballot(hit < nbins);
        if (any) {
            const int b = __shfl(hit, __ffsll((long long)any) - 1);
            k = hmax * b / nbins;
        }
    }
    if (lane == 0)
        for (int o = 0; o < n_oct; o++) {
            k_oct[o] = k;
            k *= 0.75f;
        }
}

// ---- host launchers -------------------------------------------------------------------------------------
void launch_gray(const void* img, int rows, int cols, int channels, size_t stride, float* out, hipStream_t s, const Batch& b) {
    hipLaunchKernelGGL(gray_kernel, dim3(ceil_div(cols, 256), rows, b.n), dim3(256), 0, s, static_cast<const uint8_t*>(img), rows, cols, channels, stride, out,
                       b.img_stride, b.stride);
}

void launch_gauss(const float* src, float* dst, int w, int h, const GaussTaps& taps, int radius, hipStream_t s, const Batch& b) {
    dim3 grid(ceil_div(w, TW), ceil_div(h, TH), b.n);
    if (radius == 4) hipLaunchKernelGGL((gauss_kernel<4>), grid, dim3(256), 0, s, src, dst, w, h, taps, b.stride);
    else hipLaunchKernelGGL((gauss_kernel<2>), grid, dim3(256), 0, s, src, dst, w, h, taps, b.stride);
}

static size_t deriv_lds_bytes(int s) { return (size_t)((TH + 2 * s) * (TW + 2 * s) + 2 * (TH + 2 * s) * TW) * sizeof(float); }

void launch_kcontrast(const float* smooth, float* modg_tmp, int w, int h, unsigned int* hmax_bits, int* hist, float* k_oct, int n_oct, hipStream_t s,
                      const Batch& b, bool gradient_done) {
    // hmax_bits and hist are zeroed by the caller (one clear of the per-image counter block for the whole batch)
    if (!gradient_done)    // otherwise launch_base_strips has written |grad| to modg_tmp and its maximum to hmax_bits
        hipLaunchKernelGGL((deriv_pair_kernel<2>), dim3(ceil_div(w, TW), ceil_div(h, TH), b.n), dim3(256), deriv_lds_bytes(1), s, smooth, modg_tmp,
                           (float*)nullptr, w, h, 1, 3.0f, 10.0f, (const float*)nullptr, hmax_bits, b.stride);
    // the histogram's grid shrinks with the image: 1024 blocks for one large frame, a share of that for each image of a batch
    const int hist_blocks = std::max(8, std::min(1024, ceil_div((long long)w * h, 4096)));
    // 16 sub-histograms per block (8: 1.755, 16: 1.739, 32: 1.763 ms per 4096^2 extraction, profiles/r03/half_sample_ab.txt)
    hipLaunchKernelGGL(kcontrast_hist_kernel<16>, dim3(hist_blocks, 1, b.n), dim3(256), 0, s, modg_tmp, w, h, hmax_bits, hist, b.stride);
    hipLaunchKernelGGL(kcontrast_finish_kernel, dim3(1, 1, b.n), dim3(64), 0, s, hist, hmax_bits, w, h, k_oct, n_oct, b.stride);
}
// image -> Lt[0] (and, if want_modg, |grad| of the sigma = 1 image + its interior maximum) in one pass on register strips
void launch_base_strips(const void* img, int rows, int cols, int channels, size_t stride, const GaussTaps& g16, const GaussTaps& g10, float* Lt0, float* modg,
                        unsigned int* hmax_bits, bool want_modg, hipStream_t s, const Batch& b) {
    APDS_REQUIRE((size_t)rows * cols < ((size_t)1 << 29) && (size_t)rows * stride < ((size_t)1 << 31), APDS_ERR_INTERNAL, "base_strips: 32-bit offsets");
    APDS_REQUIRE(channels != 4 || ((reinterpret_cast<uintptr_t>(img) | stride | b.img_stride) & 3) == 0, APDS_ERR_INTERNAL, "base_strips: dword loads of the BGRA pixels");
    const int strips = ceil_div(cols, BS_VW), nwaves = strips * ceil_div(rows, BS_RB);
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(ceil_div(nwaves, 4), 1, b.n), dim3(256), 0, s, static_cast<const uint8_t*>(img), cols, rows, (int)stride, g16, g10, Lt0,
                           modg, hmax_bits, want_modg ? 1 : 0, strips, nwaves, b.img_stride, b.stride);
    };
    if (channels == 4) go(&base_strip_kernel<4>);
    else if (channels == 3) go(&base_strip_kernel<3>);
    else go(&base_strip_kernel<1>);
}

}  // namespace apds
