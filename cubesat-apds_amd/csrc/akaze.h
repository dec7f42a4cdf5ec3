// csrc/akaze.h — shared declarations of the AKAZE pipeline: the launchers of the filter, suppression, compaction and descriptor files and the
// extraction driver's hooks, grouped by the file that implements them. The host arithmetic (levels, slab layout, and which kernel family
// serves the base stage and every level): akaze_plan.h. The filter launchers decide nothing: each launches the kernel the plan named and
// APDS_REQUIREs what that kernel cannot do; band heights, grids, LDS sizes and template dispatch are theirs.
#pragma once
#include "akaze_plan.h"
#include "common.h"

namespace apds {

// Batched launches (gridDim.z = images): every image of a batch owns an identical workspace slab `bstride` bytes after the previous
// one, so a plane of image blockIdx.z is the plane of image 0 shifted by blockIdx.z * bstride (akaze_plan.h lays the slab
// out). A single image is a batch of one (blockIdx.z = 0).
#ifdef __HIPCC__
template <class T>
__device__ __forceinline__ T* bofs(T* p, size_t bstride) {
    return p ? reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + (size_t)blockIdx.z * bstride) : p;
}
#endif

// step sizes of one FED pass, by value to nld_multi_kernel, nld_strip_kernel and level_strip_kernel
struct NldSteps {
    float v[8];
};
// the register-strip FED kernels (nld_strip_kernel, level_strip_kernel): waves per SIMD the compiler is asked for, rows a wave finishes
#ifndef APDS_STRIP_WAVES
#define APDS_STRIP_WAVES 4
#endif
#ifndef APDS_STRIP_RB
#define APDS_STRIP_RB 16
#endif

// level table handed to keypoint kernels by value (pointers: image 0 of the batch)
struct LevelTable {
    int n;
    size_t bstride;
    int w[AKAZE_MAX_LEVELS], h[AKAZE_MAX_LEVELS], octave[AKAZE_MAX_LEVELS], sigma_size[AKAZE_MAX_LEVELS], border[AKAZE_MAX_LEVELS];
    float esigma[AKAZE_MAX_LEVELS], ratio[AKAZE_MAX_LEVELS];
    long long pix_offset[AKAZE_MAX_LEVELS + 1];
    const float* Lt[AKAZE_MAX_LEVELS];
    const float2* Lxy[AKAZE_MAX_LEVELS];   // (Lx, Ly) interleaved
    const float* Ldet[AKAZE_MAX_LEVELS];
    uint8_t* mask[AKAZE_MAX_LEVELS];
    const uint32_t* list[AKAZE_MAX_LEVELS];   // the level's candidate list (unordered), counts in list_count[level]
    float* ref[AKAZE_MAX_LEVELS];             // three floats per list entry: the refined (x, y, response) of a surviving candidate
};

// The mask support of an extraction, by value to the kernels that apply the detection mask: the zero-count summed-area table of the mask
// (akaze_mask_sat.hip: (rows + 1) x (cols + 1) u32 per image) and every level's radius in full-resolution pixels, decided by the plan.
// A null table: the mask is consulted at the keypoint's own pixel alone.
struct MaskSupport {
    const uint32_t* sat = nullptr;
    size_t img_stride = 0;              // elements between the tables of consecutive images; 0: one table (one mask) for all
    int radius[AKAZE_MAX_LEVELS] = {};
};

// A batched launch: `n` images of one size through one grid (gridDim.z = n). Every image owns an identical workspace slab, `stride`
// bytes apart (so a plane of image i is the plane of image 0 + i * stride); the input images are `img_stride` bytes apart.
struct Batch {
    int n = 1;
    size_t stride = 0, img_stride = 0;
};

// (akaze_strip.h: the device-only helpers the filter files share - border indexing, lane shifts, the register-strip formulas)

// akaze_base.hip: gray conversion, Gaussians, the contrast factor, and all of them in one pass on register strips
void launch_gray(const void* img, int rows, int cols, int channels, size_t stride, float* out, hipStream_t s, const Batch& b);
void launch_gauss(const float* src, float* dst, int w, int h, const GaussTaps& taps, int radius, hipStream_t s, const Batch& b);
void launch_kcontrast(const float* smooth, float* modg_tmp, int w, int h, unsigned int* hmax_bits, int* hist, float* k_oct, int n_oct, hipStream_t s,
                      const Batch& b, bool gradient_done = false);
void launch_base_strips(const void* img, int rows, int cols, int channels, size_t stride, const GaussTaps& g16, const GaussTaps& g10, float* Lt0, float* modg,
                        unsigned int* hmax_bits, bool want_modg, hipStream_t s, const Batch& b);

// akaze_smooth_flow.hip
// strips: the interior on register strips and the frame around it on LDS tiles (two launches), else LDS tiles throughout
void launch_smooth_flow(const float* src, float* smooth, float* flow, int w, int h, const GaussTaps& taps, const float* kptr, hipStream_t s, const Batch& b,
                        bool strips);

// akaze_fed.hip
// `nsteps` FED steps in one pass: register strips (1 .. 4 steps; half_out, optional: the 2 x 2 area means of Lnew as well, the next
// octave's start image) or LDS tiles (1 .. 8 steps)
void launch_nld_strips(const float* Lt, const float* Lf, float* Lnew, int w, int h, const float* step_sizes, int nsteps, hipStream_t s, const Batch& b,
                       float* half_out = nullptr);
void launch_nld_tiles(const float* Lt, const float* Lf, float* Lnew, int w, int h, const float* step_sizes, int nsteps, hipStream_t s, const Batch& b);

// akaze_level_strips.hip, akaze_level_stream.hip, akaze_level_fused.hip: a whole level step (smoothing, conductivity, FED steps) in one launch
void launch_level_strips(const float* src, float* smooth, float* flow_out, float* Lnew, int w, int h, const GaussTaps& taps, const float* kptr,
                         const float* step_sizes, int nsteps, hipStream_t s, const Batch& b);
void launch_level_stream(const float* src, float* smooth, float* flow_out, float* Lnew, int w, int h, const GaussTaps& taps, const float* kptr,
                         const float* step_sizes, int nsteps, hipStream_t s, const Batch& b, float* half_out = nullptr);
void launch_level_fused(const float* src, float* smooth, float* flow_out, const float* flow_in, float* Lnew, int w, int h, const GaussTaps& taps,
                        const float* kptr, const float* step_sizes, int nsteps, hipStream_t s, const Batch& b, float* half_out = nullptr);

// akaze_resize.hip
void launch_half_sample(const float* src, int sw, float* dst, int dw, int dh, hipStream_t s, const Batch& b);
void launch_area_resize(const float* src, int sw, float* dst, int dw, int dh, const int* xofs, const float* xw, const int* xcnt, const int* yofs,
                        const float* yw, const int* ycnt, hipStream_t s, const Batch& b);

// akaze_doh_tiles.hip: determinant of the Hessian and 3x3 extrema on LDS tiles
void launch_doh_fused(const float* Lsmooth, float2* Lxy, float* Ldet, int w, int h, int sc, float kside, float kmid, int border, float thr, uint8_t* mask,
                      uint32_t* list, int* list_count, hipStream_t s, const Batch& b);

// akaze_doh_strips.hip: the streaming form of the same stage for the large levels; it also writes the mask and the suppression status of
// every pixel of the level (so neither needs clearing).
void launch_doh_strips(const float* Lsmooth, float2* Lxy, float* Ldet, int w, int h, int sc, float kside, float kmid, int border, float thr, uint8_t* mask,
                       uint8_t* status, uint32_t* list, int* list_count, hipStream_t s, const Batch& b, bool dense_det);

// Band height of a streaming kernel (a wave walks a band of rows of one 64-column strip; 256-thread blocks = four waves): the waves of a
// launch should fill the resident wave slots a WHOLE number of times - 5248 waves on 5120 slots run as two rounds, the second one 2.5 %
// full (the first measurements of both streaming kernels had exactly that). Asks the runtime how many blocks of `kernel` fit a CU, takes
// bands of about `want_rows` rows and then stretches them so that the last round is (just) full.
long long stream_wave_slots(const void* kernel, int dynamic_lds = 0);   // resident waves of a 256-thread-block kernel on the current device (cached)
template <class K>
inline int stream_band_rows(K kernel, int strips, int h, int batch, int want_rows, int min_rows, int dynamic_lds = 0) {
    const long long slots = stream_wave_slots(reinterpret_cast<const void*>(kernel), dynamic_lds);
    const long long lanes = (long long)strips * batch;                              // waves per band row
    long long bands = (h + want_rows - 1) / want_rows;
    const long long rounds = std::max<long long>(1, (lanes * bands + slots / 2) / slots);
    bands = std::max<long long>(1, rounds * slots / lanes);                          // as many bands as fill `rounds` rounds, not one more
    const int rb = (int)((h + bands - 1) / bands);
    return std::max(rb, min_rows);
}

// akaze_suppress.hip: cross-level suppression. Makes the keypoint masks of ALL levels final (every level's Hessian kernel is done).
void suppress_all_levels(const std::vector<LevelDesc>& ev, const SlabLayout& sl, hipStream_t s, const Batch& b);

// akaze_compact.hip: sub-pixel refinement and ordered compaction (level-major, row-major).
// All levels of every image of the batch: keypoints to kps + image * capacity (at most `capacity` each), the image's count to kp_base[1] of
// its slab. APDS_KP_RANKED: the candidates place themselves; 0: two passes over the masks. pmask (common.h): the detection mask, applied to
// the refined positions where the refinement's own drop is - what it removes never counts, so the max_points cut comes after it.
// support: a table makes the mask's rule "any zero byte in the square of the level's radius around that position" (four table reads).
void compact_all_levels(const LevelTable& T, const SlabLayout& sl, const PixelMask& pmask, const MaskSupport& support, apds_keypoint* kps, int capacity,
                        hipStream_t s, const Batch& b);

// akaze_mask_sat.hip: S[y][x] = the zero bytes of the mask in rows < y, columns < x; `n_tables` masks M.img_stride bytes apart to tables
// sat_img_stride elements apart (two launches on s; deterministic)
size_t mask_zero_sat_elems(int rows, int cols);
void mask_zero_sat_device(const PixelMask& M, int n_tables, uint32_t* sat, size_t sat_img_stride, hipStream_t s);
// The keypoints of image `bi` (Tb: its level table, bstride 0), all n_all of them, then the `keep` strongest (response descending, ties by
// detection order) to `out`. The masks are final and filtered: compact_all_levels has run.
void compact_strongest(const LevelTable& Tb, const SlabLayout& sl, size_t slab_bytes, int bi, int n_all, int keep, apds_keypoint* out, hipStream_t s);

// akaze_describe.hip: main orientation + M-LDB descriptor of keypoints [range[0], min(range[1], n_cap)) of every image (range: two ints of
// image 0's slab) or, range == nullptr, of keypoints [0, n_cap). `blocks`: grid width (the kernels stride over the keypoints).
// descriptor: APDS_AKAZE_DESCRIPTOR_MLDB - rows of 64 bytes at desc; APDS_AKAZE_DESCRIPTOR_KAZE - rows of 64 floats (akaze_describe_msurf.hip runs
// behind the orientation kernel instead of the M-LDB kernel). desc_bstride: bytes between the images' row blocks.
void describe_keypoints(const LevelTable& T, apds_keypoint* kps, const int* range, int n_cap, size_t kp_bstride, uint8_t* desc, size_t desc_bstride,
                        int blocks, int batch, int xcd_ranges, hipStream_t s, int descriptor = APDS_AKAZE_DESCRIPTOR_MLDB);
void pack_desc61_device(const uint8_t* d64, int n, uint8_t* d61, hipStream_t s);

// akaze_describe_msurf.hip: the 64-float M-SURF descriptor of the same keypoint ranges (their angles are final: the orientation kernel has run).
// plane_level >= 0: all keypoints are described on that level of T whatever their class_id.
void launch_msurf(const LevelTable& T, const apds_keypoint* kps, const int* range, int n_cap, size_t kp_bstride, float* desc, size_t desc_bstride, int blocks,
                  int batch, int xcd_ranges, int plane_level, hipStream_t s);
// ... of n keypoints [0, n) on one h x w plane of interleaved (Lx, Ly)
void msurf_describe_plane_device(const float2* lxy, int w, int h, const apds_keypoint* kps, int n, float* desc, hipStream_t s);

// akaze_extract.hip (host driver: kernels.h declares akaze_extract_device)
// Test hook: when armed (per thread) the next akaze_extract_device copies one intermediate plane to the host.
// which: 0 Lt, 2 Lx, 3 Ly, 4 Ldet (f32), 7 keypoint mask after cross-level suppression (u8), 8 kcontrast (1 float)
struct AkazeDebugRequest {
    bool armed = false;
    int level = 0, which = 0;
    void* host_out = nullptr;
};
AkazeDebugRequest& akaze_debug_request();

}  // namespace apds
