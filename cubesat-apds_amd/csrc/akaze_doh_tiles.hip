// csrc/akaze_doh_tiles.hip — a1.5 + a1.6 (determinant of the Hessian + 3x3 extrema) on LDS tiles; akaze_doh_strips.hip is the
// streaming form of the same stage for the large levels.
//
// Replaces the OpenCV work behind /root/reference/feature_extraction/src/lib.rs:64-79 (AKAZE::create(...).detect_and_compute):
// Compute_Determinant_Hessian_Response and the first pass of Find_Scale_Space_Extrema. Float contract as in akaze_strip.h (one IEEE
// binary32 operation per source operation, -ffp-contract=off).
#include "akaze.h"
#include "akaze_strip.h"

namespace apds {

// ---- a1.5 + a1.6 fused: Lsmooth -> Lx, Ly (dilated Scharr pair at scale s) -> Lxx, Lxy, Lyy -> Ldet -> 3x3 extrema, one pass ----
// The reference applies sepFilter2D twice (derivatives of derivatives), each with BORDER_REFLECT_101 on ITS input. Fused,
// that means: the Lx/Ly values a tile needs within s pixels beyond the image are the values AT the reflected positions
// (Lx(reflect(p)), not a stencil evaluated on a reflected Lsmooth). So: Lsmooth tile with a 2s+1 halo (reflect on load),
// then Lx/Ly on the tile + (s+1) ring evaluated at the reflected coordinate of every ring position, then the second
// derivatives and the determinant on the tile + 1 ring (kept in LDS), then the strict 3x3 maxima of the tile above the
// threshold and inside the level's border -> keypoint mask + candidate list (block-aggregated append). Lsmooth is read once,
// Ldet is not read back for the extrema test, and two launches per level disappear.
static constexpr int DH = 32;             // tile height (the width is the kernel's TW parameter)
// (candidates of a tile: strict 3x3 maxima are never adjacent, so at most a quarter of the tile pixels — the room behind the determinant plane)

// S = sigma_size as a compile-time constant (2, 3, 4 are all the reference's AKAZE parameters produce): constant LDS strides turn
// the index divisions into multiplies and let the tile loads be issued together; S = 0 takes it at run time.
template <int S, int NT, int TW>
__device__ __forceinline__ void doh_tile_generic(const float* __restrict__ Lsmooth, float2* __restrict__ Lxy, float* __restrict__ Ldet, int w, int h, int s_rt,
                                                 float kside, float kmid, float sq, int border, float thr, uint8_t* __restrict__ mask,
                                                 uint32_t* __restrict__ list, int* __restrict__ list_count) {
    extern __shared__ float smem[];
    __shared__ int s_n, s_base;
    const int s = S ? S : s_rt;
    const int SW = TW + 4 * s + 2, SH = DH + 4 * s + 2;   // Lsmooth tile, halo 2s + 1
    const int MW = TW + 2 * s + 2, MH = DH + 2 * s + 2;   // first derivatives, halo s + 1
    constexpr int EW = TW + 2, EH = DH + 2;               // determinant, halo 1
    float* s_src = smem;
    float* s_mx = s_src + SW * SH;
    float* s_my = s_mx + MW * MH;
    float* s_det = s_src;                                 // reuses the Lsmooth tile once the first derivatives exist
    uint32_t* s_cand = reinterpret_cast<uint32_t*>(s_src + EW * EH);
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * DH;
    const int ox = x0 - 2 * s - 1, oy = y0 - 2 * s - 1;   // global coordinate of s_src[0]
    if (threadIdx.x == 0) s_n = 0;
    // the tile with its 2s+1 halo inside the image (all but the outermost tiles, block-uniform): no reflected coordinates, no tests
    const bool inside = ox >= 0 && oy >= 0 && ox + SW <= w && oy + SH <= h;
    if constexpr (S > 0) {
        constexpr int CSW = TW + 4 * S + 2, CSH = DH + 4 * S + 2, NL = (CSW * CSH + NT - 1) / NT;
        float v[NL];
#pragma unroll
        for (int k = 0; k < NL; k++) {   // all of the tile's loads in flight before the first LDS store
            const int i = min((int)threadIdx.x + k * NT, CSW * CSH - 1);
            const int ly = i / CSW, lx = i - ly * CSW;
            v[k] = inside ? Lsmooth[(size_t)(oy + ly) * w + (ox + lx)] : Lsmooth[(size_t)reflect101(oy + ly, h) * w + reflect101(ox + lx, w)];
        }
#pragma unroll
        for (int k = 0; k < NL; k++) {
            const int i = threadIdx.x + k * NT;
            if (i < CSW * CSH) s_src[i] = v[k];
        }
    } else {
        for (int i = threadIdx.x; i < SW * SH; i += NT) {
            const int ly = i / SW, lx = i - ly * SW;
            s_src[i] = Lsmooth[(size_t)reflect101(oy + ly, h) * w + reflect101(ox + lx, w)];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < MW * MH; i += NT) {
        const int my = i / MW, mx = i - my * MW;
        // the first-derivative value this ring position stands for lives at the reflected coordinate
        const int cx = inside ? mx + s : reflect101(x0 - s - 1 + mx, w) - ox, cy = inside ? my + s : reflect101(y0 - s - 1 + my, h) - oy;
        const float* r0 = &s_src[(cy - s) * SW + cx];
        const float* r1 = &s_src[cy * SW + cx];
        const float* r2 = &s_src[(cy + s) * SW + cx];
        const float rd0 = r0[s] - r0[-s], rd1 = r1[s] - r1[-s], rd2 = r2[s] - r2[-s];
        float ax = kmid * rd1;
        ax += kside * (rd0 + rd2);
        float rs0 = kmid * r0[0];
        rs0 += kside * (r0[-s] + r0[s]);
        float rs2 = kmid * r2[0];
        rs2 += kside * (r2[-s] + r2[s]);
        s_mx[i] = ax;
        s_my[i] = rs2 - rs0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < EW * EH; i += NT) {
        const int ey = i / EW, ex = i - ey * EW;
        const int gx = x0 - 1 + ex, gy = y0 - 1 + ey;
        if (!inside && (gx < 0 || gy < 0 || gx >= w || gy >= h)) continue;   // never compared: tested pixels are >= border away from the edge
        const int c = (ey + s) * MW + ex + s;
        const float* x0r = &s_mx[c - s * MW];
        const float* x1r = &s_mx[c];
        const float* x2r = &s_mx[c + s * MW];
        const float rd0 = x0r[s] - x0r[-s], rd1 = x1r[s] - x1r[-s], rd2 = x2r[s] - x2r[-s];
        float lxx = kmid * rd1;
        lxx += kside * (rd0 + rd2);
        float rsx0 = kmid * x0r[0];
        rsx0 += kside * (x0r[-s] + x0r[s]);
        float rsx2 = kmid * x2r[0];
        rsx2 += kside * (x2r[-s] + x2r[s]);
        const float lxy = rsx2 - rsx0;
        const float* y0r = &s_my[c - s * MW];
        const float* y2r = &s_my[c + s * MW];
        float rsy0 = kmid * y0r[0];
        rsy0 += kside * (y0r[-s] + y0r[s]);
        float rsy2 = kmid * y2r[0];
        rsy2 += kside * (y2r[-s] + y2r[s]);
        const float lyy = rsy2 - rsy0;
        const float det = (lxx * lyy - lxy * lxy) * sq;
        s_det[i] = det;
        if (ex >= 1 && ex <= TW && ey >= 1 && ey <= DH) {   // the tile itself
            const size_t o = (size_t)gy * w + gx;
            Lxy[o] = make_float2(s_mx[c], s_my[c]);   // interleaved: orientation and M-LDB gather both with one 8-byte load
            Ldet[o] = det;
        }
    }
    __syncthreads();
    if (border < 0) return;   // level too small for any extremum (block-uniform)
    const unsigned span_x = (unsigned)(w - 2 * border), span_y = (unsigned)(h - 2 * border);   // (positive: checked by the launcher)
    for (int i = threadIdx.x; i < TW * DH; i += NT) {
        const int ly = i / TW, lx = i - ly * TW;
        const int gx = x0 + lx, gy = y0 + ly;
        const float* p = &s_det[(ly + 1) * EW + lx + 1];
        const float v = p[0];
        // all nine tests evaluated (no short-circuit branches: a strict maximum is rare, the branches were most of this loop);
        // "reject if v <= neighbour" exactly as written in the reference, hence the negated comparisons
        // "v <= x for some neighbour x" is "v <= the largest neighbour": fmaxf ignores a NaN operand exactly as the comparison v <= NaN
        // is false, and !(v <= m) keeps a NaN v as the reference's chain of comparisons does (three v_max3_f32 instead of eight compares)
        const float m = fmaxf(fmaxf(fmaxf(fmaxf(p[-EW - 1], p[-EW]), p[-EW + 1]), fmaxf(p[-1], p[1])), fmaxf(fmaxf(p[EW - 1], p[EW]), p[EW + 1]));
        const bool keep = ((unsigned)(gx - border) < span_x) & ((unsigned)(gy - border) < span_y) & !(v <= thr) & !(v <= m);
        if (keep) {
            mask[(size_t)gy * w + gx] = 1;
            s_cand[atomicAdd(&s_n, 1)] = (uint32_t)gx | ((uint32_t)gy << 16);
        }
    }
    __syncthreads();
    const int n = s_n;
    if (n == 0) return;
    if (threadIdx.x == 0) s_base = atomicAdd(list_count, n);   // list order is irrelevant (only used to enumerate candidates)
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += NT) list[s_base + i] = s_cand[i];
}

template <int S, int NT, int TW>
__global__ __launch_bounds__(NT) void doh_fused_kernel(const float* __restrict__ Lsmooth, float2* __restrict__ Lxy, float* __restrict__ Ldet, int w, int h,
                                                       int s_rt, float kside, float kmid, float sq, int border, float thr, uint8_t* __restrict__ mask,
                                                       uint32_t* __restrict__ list, int* __restrict__ list_count, size_t bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    APDS_BOFS(Lsmooth);
    APDS_BOFS(Lxy);
    APDS_BOFS(Ldet);
    APDS_BOFS(mask);
    APDS_BOFS(list);
    APDS_BOFS(list_count);
    doh_tile_generic<S, NT, TW>(Lsmooth, Lxy, Ldet, w, h, s_rt, kside, kmid, sq, border, thr, mask, list, list_count);
}

// (Measured and not adopted, round 2: "column runs" — a thread owns a column of a stage and walks K consecutive rows, so that the row
// terms rd(r) = L[r][x+s] - L[r][x-s], rs(r) = kmid L[r][x] + kside (L[r][x-s] + L[r][x+s]) are computed once per row and shared by
// the outputs that use the row as their upper, middle or lower one. Bit-identical, ~12 % fewer instructions, and slower: K = 10 on
// 576 threads ran one block per CU (4096^2 extraction 2.26 ms against 1.93), K = 6 on 1024 threads at 64 registers 1.98 - 2.12 ms.
// Two horizontally adjacent outputs per item with packed-f32 arithmetic (v_pk_add_f32 / v_pk_mul_f32, pairs read with one LDS
// instruction) was tried again on the 64 x 32 tiles: bit-identical, 1.824 against 1.782 ms — v_pk_add / v_pk_mul issue at half the rate
// of their scalar forms (tools/valu_calib.py), so they save index arithmetic only, and the unaligned pair reads cost more than that.)

// ---- host launcher --------------------------------------------------------------------------------------
void launch_doh_fused(const float* Lsmooth, float2* Lxy, float* Ldet, int w, int h, int sc, float kside, float kmid, int border, float thr, uint8_t* mask,
                      uint32_t* list, int* list_count, hipStream_t s, const Batch& b) {
    // 64 x 32 tiles on 512 threads (halo 1.75x, four blocks per CU: the kernel is four barrier-separated phases, and more independent
    // blocks per CU hide their latencies better than the 128 x 32 / 1024-thread tiles of round 1 or 32-pixel tiles on 256 threads did:
    // 1.82 against 1.91 and 1.98 ms per 4096^2 extraction; those variants are gone)
    constexpr int tw = 64;
    const size_t lds = (size_t)((tw + 4 * sc + 2) * (DH + 4 * sc + 2) + 2 * (tw + 2 * sc + 2) * (DH + 2 * sc + 2)) * sizeof(float);
    APDS_REQUIRE((size_t)(tw + 2) * (DH + 2) + (size_t)tw * DH / 4 <= (size_t)(tw + 4 * sc + 2) * (DH + 4 * sc + 2), APDS_ERR_INTERNAL, "doh_fused: LDS aliasing needs sigma_size >= 2");
    // the extrema test of a level that is too small for its border is skipped (border < 0 in the kernel)
    const bool none = border + 1 >= h || w - 2 * border <= 0 || h - 2 * border <= 0;
    auto go = [&](auto kernel, int nt) {
        if (lds > 64 * 1024)   // above the default dynamic-LDS limit: opt in (idempotent)
            HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
        hipLaunchKernelGGL(kernel, dim3(ceil_div(w, tw), ceil_div(h, DH), b.n), dim3(nt), lds, s, Lsmooth, Lxy, Ldet, w, h, sc, kside, kmid,
                           (float)(sc * sc * sc * sc), none ? -1 : border, thr, mask, list, list_count, b.stride);
    };
    switch (sc) {
        case 2: go(&doh_fused_kernel<2, 512, 64>, 512); break;
        case 3: go(&doh_fused_kernel<3, 512, 64>, 512); break;
        case 4: go(&doh_fused_kernel<4, 512, 64>, 512); break;
        default: go(&doh_fused_kernel<0, 512, 64>, 512); break;
    }
}

}  // namespace apds
