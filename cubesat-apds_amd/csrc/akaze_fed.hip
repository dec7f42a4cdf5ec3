// csrc/akaze_fed.hip — the explicit FED diffusion steps of the AKAZE scale space, on LDS tiles and on register strips.
//
// Replaces the OpenCV work behind /root/reference/feature_extraction/src/lib.rs:64-79 (AKAZE::create(...).detect_and_compute): the
// nld_step_scalar calls of Create_Nonlinear_Scale_Space. Float contract as in akaze_strip.h (one IEEE binary32 operation per source
// operation, -ffp-contract=off).
#include "akaze.h"
#include "akaze_strip.h"

namespace apds {

// ---- explicit FED diffusion steps: Lnew = Lt + step_size * div(c grad Lt), several steps per pass (temporal blocking) ----
// Every intermediate value is exactly what a one-step-per-launch formulation produces (same expression, same inputs), so
// results do not depend on how the steps are grouped; HBM traffic and the launch count of the latency-bound small octaves
// drop with the group size.
static constexpr int T2W = 64, T2H = 32;

__device__ __forceinline__ float nld_point(const float* __restrict__ st, const float* __restrict__ sf, int c, int pitch, int x, int y, int w, int h,
                                           float step_size) {
    const float tc = st[c], fc = sf[c];
    const bool top = y == 0, bot = y == h - 1, left = x == 0, right = x == w - 1;
    const float xp = (fc + sf[c + 1]) * (st[c + 1] - tc);
    const float xm = (fc + sf[c - 1]) * (st[c - 1] - tc);
    const float yp = (fc + sf[c + pitch]) * (st[c + pitch] - tc);
    const float ym = (fc + sf[c - pitch]) * (st[c - pitch] - tc);
    float step_r;
    if ((top || bot) && (left || right)) step_r = 0.0f;
    else if (top) step_r = xp + xm + yp;
    else if (bot) step_r = xp + xm + ym;
    else if (left) step_r = xp + yp + ym;
    else if (right) step_r = xm + yp + ym;
    else step_r = xp + xm + yp + ym;
    return tc + step_r * step_size;
}

// S FED steps in one pass: inputs are loaded with an S-pixel halo; step j is evaluated on the tile + (S - j) rings, ping-ponging
// between two LDS planes; the last step writes the tile. Only positions inside the image are evaluated; a border pixel's
// out-of-image neighbour is read (whatever LDS holds) but never used, exactly as in the single-step kernel.

// a point with all four neighbours inside the image: nld_point without the border cases (same expression, same order)
__device__ __forceinline__ float nld_point_interior(const float* __restrict__ st, const float* __restrict__ sf, int c, int pitch, float step_size) {
    const float tc = st[c], fc = sf[c];
    const float xp = (fc + sf[c + 1]) * (st[c + 1] - tc);
    const float xm = (fc + sf[c - 1]) * (st[c - 1] - tc);
    const float yp = (fc + sf[c + pitch]) * (st[c + pitch] - tc);
    const float ym = (fc + sf[c - pitch]) * (st[c - pitch] - tc);
    return tc + (xp + xm + yp + ym) * step_size;
}

// two horizontally adjacent interior points at once: the same IEEE operations per point, issued as packed-f32 instructions
// (v_pk_add_f32 / v_pk_mul_f32 work on register pairs), so the per-item index arithmetic is also paid once per two points
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 lds_pair(const float* p) { return f32x2{p[0], p[1]}; }
__device__ __forceinline__ f32x2 nld_pair_interior(const float* __restrict__ st, const float* __restrict__ sf, int c, int pitch, float step_size) {
    const f32x2 t = lds_pair(st + c), f = lds_pair(sf + c);
    const f32x2 xp = (f + lds_pair(sf + c + 1)) * (lds_pair(st + c + 1) - t);
    const f32x2 xm = (f + lds_pair(sf + c - 1)) * (lds_pair(st + c - 1) - t);
    const f32x2 yp = (f + lds_pair(sf + c + pitch)) * (lds_pair(st + c + pitch) - t);
    const f32x2 ym = (f + lds_pair(sf + c - pitch)) * (lds_pair(st + c - pitch) - t);
    return t + (xp + xm + yp + ym) * step_size;
}

// INTERIOR: the tile with its halo lies inside the image and touches no image border (block-uniform; all but the outermost
// tiles): no clamping, no in-image tests, no border cases — a third of the instructions of the general path.
template <int S, int NT, bool INTERIOR>
__device__ __forceinline__ void nld_multi_tile(const float* __restrict__ Lt, const float* __restrict__ Lf, float* __restrict__ Lnew, int w, int h,
                                               const NldSteps& steps, float* s_f, float* s_a, float* s_b, int x0, int y0) {
    constexpr int SW = T2W + 2 * S, SH = T2H + 2 * S;
    {
        constexpr int NL = (SW * SH + NT - 1) / NT;
        float va[NL], vf[NL];
#pragma unroll
        for (int k = 0; k < NL; k++) {   // every load of both tiles in flight before the first LDS store
            const int i = min((int)threadIdx.x + k * NT, SW * SH - 1);
            const int ly = i / SW, lx = i - ly * SW;
            const size_t o = INTERIOR ? (size_t)(y0 + ly) * w + (x0 + lx) : (size_t)clampi(y0 + ly, h) * w + clampi(x0 + lx, w);
            va[k] = Lt[o];
            vf[k] = Lf[o];
        }
#pragma unroll
        for (int k = 0; k < NL; k++) {
            const int i = threadIdx.x + k * NT;
            if (i < SW * SH) {
                s_a[i] = va[k];
                s_f[i] = vf[k];
            }
        }
    }
    __syncthreads();
    const float* src = s_a;
    float* dst = s_b;
#pragma unroll
    for (int j = 1; j < S; j++) {
        const int rw = SW - 2 * j, rh = SH - 2 * j;   // region of this step: local [j, SW - j) x [j, SH - j)
        if constexpr (INTERIOR) {
            const int hw = rw / 2;   // the region's width is even: two points per item
            for (int i = threadIdx.x; i < hw * rh; i += NT) {
                const int ry = i / hw, rx = i - ry * hw;
                const int c = (ry + j) * SW + 2 * rx + j;
                const f32x2 v = nld_pair_interior(src, s_f, c, SW, steps.v[j - 1]);
                dst[c] = v.x;
                dst[c + 1] = v.y;
            }
        } else {
            for (int i = threadIdx.x; i < rw * rh; i += NT) {
                const int ry = i / rw, rx = i - ry * rw;
                const int lx = rx + j, ly = ry + j;
                const int gx = x0 + lx, gy = y0 + ly;
                if (gx >= 0 && gx < w && gy >= 0 && gy < h) dst[ly * SW + lx] = nld_point(src, s_f, ly * SW + lx, SW, gx, gy, w, h, steps.v[j - 1]);
            }
        }
        __syncthreads();
        const float* t = src;
        src = dst;
        dst = const_cast<float*>(t);
    }
    if constexpr (INTERIOR) {
        for (int i = threadIdx.x; i < (T2W / 2) * T2H; i += NT) {
            const int ly = i / (T2W / 2), lx = 2 * (i - ly * (T2W / 2));
            const f32x2 v = nld_pair_interior(src, s_f, (ly + S) * SW + lx + S, SW, steps.v[S - 1]);
            float* o = &Lnew[(size_t)(y0 + S + ly) * w + (x0 + S + lx)];
            o[0] = v.x;
            o[1] = v.y;
        }
    } else {
        for (int i = threadIdx.x; i < T2W * T2H; i += NT) {
            const int ly = i / T2W, lx = i - ly * T2W;
            const int gx = x0 + S + lx, gy = y0 + S + ly;
            if (gx < w && gy < h) Lnew[(size_t)gy * w + gx] = nld_point(src, s_f, (ly + S) * SW + lx + S, SW, gx, gy, w, h, steps.v[S - 1]);
        }
    }
}

template <int S, int NT>
__global__ __launch_bounds__(NT) void nld_multi_kernel(const float* __restrict__ Lt, const float* __restrict__ Lf, float* __restrict__ Lnew, int w, int h,
                                                        NldSteps steps, size_t bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    APDS_BOFS(Lt);
    APDS_BOFS(Lf);
    APDS_BOFS(Lnew);
    constexpr int SW = T2W + 2 * S, SH = T2H + 2 * S;
    __shared__ float s_f[SH * SW];
    __shared__ float s_a[SH * SW];
    __shared__ float s_b[SH * SW];
    const int x0 = blockIdx.x * T2W - S, y0 = blockIdx.y * T2H - S;   // global coordinate of local (0, 0)
    // every evaluated point (local [1, SW-1) x [1, SH-1) at the first step) has its four neighbours inside the image
    if (x0 >= 0 && y0 >= 0 && x0 + SW <= w && y0 + SH <= h) nld_multi_tile<S, NT, true>(Lt, Lf, Lnew, w, h, steps, s_f, s_a, s_b, x0, y0);
    else nld_multi_tile<S, NT, false>(Lt, Lf, Lnew, w, h, steps, s_f, s_a, s_b, x0, y0);
}

// ---- FED steps on register strips (the large levels) -------------------------------------------------------------
// One wave owns a strip of 64 columns x (RB + 2S) rows of Lt and of the conductivity, one column per lane, all rows in registers
// (fully unrolled, static register indices): no LDS, no barriers. Horizontal neighbours come through lane shifts. With
//   P[x] = (f[x] + f[x+1]) * (t[x+1] - t[x])        Q[r] = (f[r] + f[r+1]) * (t[r+1] - t[r])
// the four flux terms of nld_point are xp = P[x], xm = -P[x-1], yp = Q[r], ym = -Q[r-1] EXACTLY: float addition commutes,
// a - b == -(b - a) and (-a) * b == -(a * b) in IEEE arithmetic, and x + (-y) is x - y. So a step costs one P and one Q per point
// (11 instructions) instead of four products. Step j is valid on rows [j, R - j) and lanes [j, 64 - j): the same shrinking halo as
// the LDS kernel. Border handling (BORDER waves only): a flux across the image edge is forced to +0 — exactly the reference's
// dropped term, because the sum's first operand is never -0 (a difference of equal floats is +0 and conductivities are positive),
// so adding +-0 changes nothing — and the four corner pixels, whose step is 0 in the reference, keep their value.
// (The step loop stands here and, line for line, at the end of level_strip in akaze_level_strips.hip: as a shared function over
// the callers' arrays it compiled to different kernel bodies - profiles/filters_split/README.md - so it was not shared.)
template <int S, int RB, bool BORDER, bool HALF>
__device__ __forceinline__ void nld_strip(const float* __restrict__ Lt, const float* __restrict__ Lf, float* __restrict__ Lnew, int w, int h,
                                          const NldSteps& steps, int gx0, int y0, float* __restrict__ half) {
    constexpr int R = RB + 2 * S;
    const int lane = threadIdx.x & 63;
    const int gx = gx0 + lane;
    const int ys = y0 - S;                      // image row of strip row 0
    float t[R], f[R];
    {
        // buffer loads: (descriptor, one lane-offset VGPR shared by every row, the row's byte offset in a scalar register) — plain
        // global loads would keep a 64-bit address pair per row in vector registers
        const int plane_bytes = w * h * 4;
        const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Lt), 0, plane_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rf = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Lf), 0, plane_bytes, 0x00020000);
        const int cx4 = 4 * (BORDER ? clampi(gx, w) : gx);
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int row4 = (BORDER ? clampi(ys + r, h) : ys + r) * w * 4;
            t[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rt, cx4, row4, 0));
            f[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rf, cx4, row4, 0));
        }
    }
    const bool flux_x_inside = gx >= 0 && gx + 1 <= w - 1;   // the edge between columns gx and gx + 1
    const bool edge_col = gx == 0 || gx == w - 1;
#pragma unroll
    for (int j = 1; j <= S; j++) {
        const float tau = steps.v[j - 1];
        float qprev = (f[j - 1] + f[j]) * (t[j] - t[j - 1]);
        if (BORDER && !(ys + j - 1 >= 0 && ys + j <= h - 1)) qprev = 0.0f;
#pragma unroll
        for (int r = j; r < R - j; r++) {
            const float tc = t[r];
            const float d = lane_next(tc) - tc;
            float P = (f[r] + lane_next(f[r])) * d;
            if (BORDER && !flux_x_inside) P = 0.0f;
            float q = (f[r] + f[r + 1]) * (t[r + 1] - tc);   // t[r + 1] is still this step's input
            if (BORDER && !(ys + r >= 0 && ys + r + 1 <= h - 1)) q = 0.0f;
            float sr = P - lane_prev(P);                      // xp + xm
            sr = sr + q;                                      // + yp
            sr = sr - qprev;                                  // + ym
            float out = tc + sr * tau;
            if (BORDER && edge_col && (ys + r == 0 || ys + r == h - 1)) out = tc;
            qprev = q;
            t[r] = out;
        }
    }
    if (lane >= S && lane < 64 - S && gx < w) {
        const __amdgpu_buffer_rsrc_t rn = __builtin_amdgcn_make_buffer_rsrc(Lnew, 0, w * h * 4, 0x00020000);
#pragma unroll
        for (int r = S; r < S + RB; r++)
            if (!BORDER || ys + r < h) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, t[r]), rn, 4 * gx, (ys + r) * w * 4, 0);
    }
    if (HALF) {
        // the last level of an octave: the next octave's start image, ((a + b) + (c + d)) * 0.25 as half_sample_kernel forms it, from the
        // rows in registers (bands start on even rows, strips on even columns: pairs never straddle waves). A template parameter, so that the
        // plain instantiations keep their register allocation.
        static_assert((RB & 1) == 0, "row pairs must stay inside a band");
        const int hw = w >> 1;
        const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(half, 0, hw * (h >> 1) * 4, 0x00020000);
        const bool col_ok = lane >= S && lane < 64 - S && !(gx & 1) && gx + 1 < w;
#pragma unroll
        for (int r = S; r < S + RB; r += 2) {
            const float top = t[r] + lane_next(t[r]);
            const float bot = t[r + 1] + lane_next(t[r + 1]);
            if (col_ok && (!BORDER || ys + r + 1 < h))
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, (top + bot) * 0.25f), rh, 2 * gx, ((ys + r) >> 1) * hw * 4, 0);
        }
    }
}

template <int S, int RB, bool HALF = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(APDS_STRIP_WAVES, 8))) void nld_strip_kernel(const float* __restrict__ Lt, const float* __restrict__ Lf, float* __restrict__ Lnew, int w, int h,
                                                         NldSteps steps, int strips, int nwaves, size_t bstride, float* __restrict__ half) {
    APDS_RAISE_WAVE_PRIORITY();
    APDS_BOFS(Lt);
    APDS_BOFS(Lf);
    APDS_BOFS(Lnew);
    if (HALF) APDS_BOFS(half);
    constexpr int VW = 64 - 2 * S;              // columns a wave finishes
    // wave-uniform by construction; readfirstlane tells the compiler, so that row bases and row conditions live in scalar registers
    const int id = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (id >= nwaves) return;                   // the kernel has no barriers
    const int band = __builtin_amdgcn_readfirstlane(id / strips);   // (the division itself runs on the vector ALU)
    const int strip = id - band * strips;
    const int gx0 = strip * VW - S, y0 = band * RB;
    const bool border = gx0 < 0 || gx0 + 64 > w || y0 - S < 0 || y0 + RB + S > h;
    if (border) nld_strip<S, RB, true, HALF>(Lt, Lf, Lnew, w, h, steps, gx0, y0, half);
    else nld_strip<S, RB, false, HALF>(Lt, Lf, Lnew, w, h, steps, gx0, y0, half);
}

// ---- host launchers -------------------------------------------------------------------------------------
template <int S>
static void nld_multi_launch(const float* Lt, const float* Lf, float* Lnew, int w, int h, const NldSteps& st, hipStream_t s, const Batch& b) {
    // 1024 threads per 64x32 tile: each step is ~3 short dependent LDS passes, so what matters is waves in flight per CU
    const dim3 grid(ceil_div(w, T2W), ceil_div(h, T2H), b.n);
    hipLaunchKernelGGL((nld_multi_kernel<S, 1024>), grid, dim3(1024), 0, s, Lt, Lf, Lnew, w, h, st, b.stride);
}
template <int S>
static void nld_strip_launch(const float* Lt, const float* Lf, float* Lnew, int w, int h, const NldSteps& st, hipStream_t s, const Batch& b, float* half) {
    constexpr int RB = APDS_STRIP_RB;
    const int strips = ceil_div(w, 64 - 2 * S), nwaves = strips * ceil_div(h, RB);
    if (half)
        hipLaunchKernelGGL((nld_strip_kernel<S, RB, true>), dim3(ceil_div(nwaves, 4), 1, b.n), dim3(256), 0, s, Lt, Lf, Lnew, w, h, st, strips, nwaves, b.stride, half);
    else
        hipLaunchKernelGGL((nld_strip_kernel<S, RB, false>), dim3(ceil_div(nwaves, 4), 1, b.n), dim3(256), 0, s, Lt, Lf, Lnew, w, h, st, strips, nwaves, b.stride, (float*)nullptr);
}
void launch_nld_strips(const float* Lt, const float* Lf, float* Lnew, int w, int h, const float* step_sizes, int nsteps, hipStream_t s, const Batch& b,
                       float* half_out) {
    APDS_REQUIRE(nsteps >= 1 && nsteps <= 4 && fits_32bit_offsets(w, h), APDS_ERR_INTERNAL, "nld_strips: 1..4 steps per launch, 32-bit offsets");
    NldSteps st{};
    for (int i = 0; i < nsteps; i++) st.v[i] = step_sizes[i];
    switch (nsteps) {
        case 1: nld_strip_launch<1>(Lt, Lf, Lnew, w, h, st, s, b, half_out); break;
        case 2: nld_strip_launch<2>(Lt, Lf, Lnew, w, h, st, s, b, half_out); break;
        case 3: nld_strip_launch<3>(Lt, Lf, Lnew, w, h, st, s, b, half_out); break;
        default: nld_strip_launch<4>(Lt, Lf, Lnew, w, h, st, s, b, half_out); break;
    }
}
void launch_nld_tiles(const float* Lt, const float* Lf, float* Lnew, int w, int h, const float* step_sizes, int nsteps, hipStream_t s, const Batch& b) {
    APDS_REQUIRE(nsteps >= 1 && nsteps <= 8, APDS_ERR_INTERNAL, "nld_multi: 1..8 steps per launch");
    NldSteps st{};
    for (int i = 0; i < nsteps; i++) st.v[i] = step_sizes[i];
    switch (nsteps) {
        case 1: nld_multi_launch<1>(Lt, Lf, Lnew, w, h, st, s, b); break;
        case 2: nld_multi_launch<2>(Lt, Lf, Lnew, w, h, st, s, b); break;
        case 3: nld_multi_launch<3>(Lt, Lf, Lnew, w, h, st, s, b); break;
        case 4: nld_multi_launch<4>(Lt, Lf, Lnew, w, h, st, s, b); break;
        case 5: nld_multi_launch<5>(Lt, Lf, Lnew, w, h, st, s, b); break;
        case 6: nld_multi_launch<6>(Lt, Lf, Lnew, w, h, st, s, b); break;
        case 7: nld_multi_launch<7>(Lt, Lf, Lnew, w, h, st, s, b); break;
        default: nld_multi_launch<8>(Lt, Lf, Lnew, w, h, st, s, b); break;
    }
}

}  // namespace apds
