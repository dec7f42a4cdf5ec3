// csrc/akaze_compact.hip — AKAZE sub-pixel refinement and the ordered compaction of the keypoint masks into the keypoint list on gfx950,
// and the selection of the strongest keypoints when an image has more than max_points.
//
// Replaces OpenCV AKAZEFeatures::Do_Subpixel_Refinement, the order in which Find_Scale_Space_Extrema leaves its keypoints, and
// KeyPointsFilter::retainBest behind feature_extraction/src/lib.rs:79.
//
// Output order is the reference's: level-major, then row-major (ordered compaction by prefix sums, no atomics in anything that decides an
// index).
#include "akaze.h"
#include "config.h"

namespace apds {

// ---- a1.7 sub-pixel refinement ---------------------------------------------------------------------------------
struct Refined {
    float x, y, response;
    bool ok;
};

__device__ __forceinline__ Refined refine(const float* __restrict__ ldet, int cols, int x, int y, float ratio) {
    const size_t c = (size_t)y * cols + x;
    const float Dx = 0.5f * (ldet[c + 1] - ldet[c - 1]);
    const float Dy = 0.5f * (ldet[c + cols] - ldet[c - cols]);
    const float Dxx = ldet[c + 1] + ldet[c - 1] - 2.0f * ldet[c];
    const float Dyy = ldet[c + cols] + ldet[c - cols] - 2.0f * ldet[c];
    const float Dxy = 0.25f * (ldet[c + cols + 1] + ldet[c - cols - 1] - ldet[c - cols + 1] - ldet[c + cols - 1]);
    // cv::solve(Matx22f, Vec2f, dst, DECOMP_LU): lapack.cpp's 2 x 2 CV_32F branch - determinant (`det2`) and both numerators in
    // double (products of two floats are exact there), one rounding to float per unknown
    float dx = 0.0f, dy = 0.0f;
    double det = (double)Dxx * (double)Dyy - (double)Dxy * (double)Dxy;
    if (det != 0.) {
        det = 1. / det;
        const float b0 = -Dx, b1 = -Dy;
        dx = (float)(((double)b0 * (double)Dyy - (double)b1 * (double)Dxy) * det);
        dy = (float)(((double)b1 * (double)Dxx - (double)b0 * (double)Dxy) * det);
    }
    Refined r;
    r.ok = !(fabsf(dx) > 1.0f || fabsf(dy) > 1.0f);
    r.x = x * ratio + (dx * ratio + .5f * (ratio - 1.f));
    r.y = y * ratio + (dy * ratio + .5f * (ratio - 1.f));
    r.response = ldet[c];
    return r;
}

// The detection mask (KeyPointsFilter::runByPixelsMask behind detectAndCompute's `mask`): a refined keypoint goes iff the mask byte under
// its rounded position - (int)(pt + 0.5f) per axis, f32 addition, truncation; pt in full-resolution pixels whatever the level - is zero.
// By construction the rounded position lies inside the image (border >= 1 at every level, pt.x <= W - ratio / 2 - 1 / 2): the clamp is for
// memory safety alone. A null base is uniform over the launch: no access, no divergence.
// With a mask support (S.sat, uniform over the launch as well) the keypoint goes iff ANY byte is zero in the square of the level's radius
// around that pixel, clipped to the image (outside the image nothing is masked): the zero count of the square from four reads of the
// mask's summed-area table, in u32 arithmetic modulo 2^32 (the count itself is exact). Radius 0 is the byte rule.
__device__ __forceinline__ bool masked_out(const PixelMask& M, const MaskSupport& S, int lvl, float x, float y) {
    if (!M.base) return false;
    const int mx = min(max((int)(x + 0.5f), 0), M.cols - 1);
    const int my = min(max((int)(y + 0.5f), 0), M.rows - 1);
    if (!S.sat) return M.base[(size_t)blockIdx.z * M.img_stride + (size_t)my * M.row_stride + (size_t)mx * M.pix_stride] == 0;
    const int R = S.radius[lvl];
    const size_t x0 = max(mx - R, 0), x1 = min(mx + R, M.cols - 1) + 1, y0 = max(my - R, 0), y1 = min(my + R, M.rows - 1) + 1;
    const size_t pitch = (size_t)M.cols + 1;
    const uint32_t* __restrict__ t = S.sat + (size_t)blockIdx.z * S.img_stride;
    return t[y1 * pitch + x1] - t[y0 * pitch + x1] - t[y1 * pitch + x0] + t[y0 * pitch + x0] != 0;
}

// drop candidates whose refinement is unstable or whose refined position the detection mask excludes, so bit 0 of the concatenated masks becomes the final keypoint flag (the levels of a
// stage are final by now: no suppression pass reads their masks as victims any more)
__global__ void subpixel_filter_kernel(LevelTable T, PixelMask M, MaskSupport S, const int* __restrict__ list_count, int lvl0) {
    APDS_RAISE_WAVE_PRIORITY();
    const int lvl = lvl0 + blockIdx.y;
    const int cnt = bofs(list_count, T.bstride)[lvl];
    const uint32_t* __restrict__ list = bofs(T.list[lvl], T.bstride);
    uint8_t* __restrict__ mask = bofs(T.mask[lvl], T.bstride);
    const float* __restrict__ ldet = bofs(T.Ldet[lvl], T.bstride);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x) {
        const uint32_t e = list[i];
        const int x = e & 0xFFFF, y = e >> 16;
        const size_t p = (size_t)y * T.w[lvl] + x;
        if (!mask[p]) continue;
        const Refined r = refine(ldet, T.w[lvl], x, y, T.ratio[lvl]);
        // survived the suppression, dropped by the refinement or the detection mask: bit 0 (= "is a keypoint") clear, byte non-zero
        if (!r.ok || masked_out(M, S, lvl, r.x, r.y)) mask[p] = 2;
    }
}

// ---- ordered compaction without passes over the masks ------------------------------------------------------------------------------
// Output order is level-major, row-major: a keypoint's position is the number of keypoints before it in the concatenated masks.
// The mask-scan path below (kp_block_counts / kp_scan_offsets / emit_keypoints) reads all the masks twice (85 MB at 4096^2) to place
// ~35 000 keypoints. Here the candidates place themselves: (1) subpixel_count_kernel, one thread per list entry: a survivor of the
// suppression is refined; if it stays it keeps its refined values next to its list entry and counts itself in the 128-byte chunk
// (`fine`) and the 128 KiB block (`coarse`, one counter per 128-byte line: same-line atomics serialise) of the masks it lies in;
// (2) kp_scan_fine_kernel, one block per coarse block: exclusive prefix of the fine counts (+ the coarse blocks before it);
// (3) emit_ranked_kernel, one thread per list entry: position = prefix of its chunk + the set flags before it inside the chunk
// (one cache line of the mask). Same keypoints, same order, same values as the mask-scan path.
static constexpr uint32_t REF_DEAD = 0xFFFFFFFFu;

__global__ void subpixel_count_kernel(LevelTable T, PixelMask M, MaskSupport S, const int* __restrict__ list_count, int lvl0, int* __restrict__ fine,
                                      int* __restrict__ coarse) {
    APDS_RAISE_WAVE_PRIORITY();
    const int lvl = lvl0 + blockIdx.y;
    const int cnt = bofs(list_count, T.bstride)[lvl];
    const uint32_t* __restrict__ list = bofs(T.list[lvl], T.bstride);
    uint8_t* __restrict__ mask = bofs(T.mask[lvl], T.bstride);
    const float* __restrict__ ldet = bofs(T.Ldet[lvl], T.bstride);
    float* __restrict__ ref = bofs(T.ref[lvl], T.bstride);
    fine = bofs(fine, T.bstride);
    coarse = bofs(coarse, T.bstride);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x) {
        const uint32_t e = list[i];
        const int x = e & 0xFFFF, y = e >> 16;
        const size_t p = (size_t)y * T.w[lvl] + x;
        bool keep = mask[p] & 1;
        Refined r{};
        if (keep) {
            r = refine(ldet, T.w[lvl], x, y, T.ratio[lvl]);
            if (!r.ok || masked_out(M, S, lvl, r.x, r.y)) {
                mask[p] = 2;   // survived the suppression, dropped by the refinement or the detection mask: bit 0 (= "is a keypoint") clear, byte non-zero
                keep = false;
            }
        }
        if (!keep) {
            reinterpret_cast<uint32_t*>(ref)[3 * (size_t)i] = REF_DEAD;
            continue;
        }
        ref[3 * (size_t)i] = r.x;
        ref[3 * (size_t)i + 1] = r.y;
        ref[3 * (size_t)i + 2] = r.response;
        const long long eg = T.pix_offset[lvl] + (long long)p;
        atomicAdd(&fine[eg >> FINE_SHIFT], 1);
        atomicAdd(&coarse[(eg >> COARSE_SHIFT) * COARSE_PITCH], 1);
    }
}

// fine[i] <- kp_base[0] + (number of keypoints in the chunks before chunk i); kp_base[1] <- kp_base[0] + all keypoints
__global__ __launch_bounds__(1024) void kp_scan_fine_kernel(int* __restrict__ fine, const int* __restrict__ coarse, int n_fine, int* __restrict__ kp_base,
                                                            size_t bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    fine = bofs(fine, bstride);
    coarse = bofs(coarse, bstride);
    kp_base = bofs(kp_base, bstride);
    __shared__ int wsum[16];
    __shared__ int s_prefix;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int part = 0;
    for (int cb = tid; cb < b; cb += 1024) part += coarse[(size_t)cb * COARSE_PITCH];
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    if (lane == 0) wsum[wv] = part;
    __syncthreads();
    if (tid == 0) {
        int t = kp_base[0];
        for (int k = 0; k < 16; k++) t += wsum[k];
        s_prefix = t;
    }
    __syncthreads();
    const int prefix = s_prefix;
    const int idx = b * 1024 + tid;
    const int v = idx < n_fine ? fine[idx] : 0;
    int incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    __syncthreads();   // wsum is reused
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < wv; k++) before += wsum[k];
    if (idx < n_fine) fine[idx] = prefix + before + incl - v;
    if (b == (int)gridDim.x - 1 && tid == 1023) kp_base[1] = prefix + before + incl;
}

__global__ void emit_ranked_kernel(LevelTable T, const int* __restrict__ list_count, int lvl0, const uint8_t* __restrict__ flags,
                                   const int* __restrict__ fine_excl, apds_keypoint* __restrict__ kps, int capacity, size_t kp_bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    const int lvl = lvl0 + blockIdx.y;
    const int cnt = bofs(list_count, T.bstride)[lvl];
    const uint32_t* __restrict__ list = bofs(T.list[lvl], T.bstride);
    const float* __restrict__ ref = bofs(T.ref[lvl], T.bstride);
    flags = bofs(flags, T.bstride);
    fine_excl = bofs(fine_excl, T.bstride);
    kps = bofs(kps, kp_bstride);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x) {
        const uint32_t rx = reinterpret_cast<const uint32_t*>(ref)[3 * (size_t)i];
        if (rx == REF_DEAD) continue;
        const uint32_t e = list[i];
        const int x = e & 0xFFFF, y = e >> 16;
        const long long eg = T.pix_offset[lvl] + (long long)y * T.w[lvl] + x;
        // set flags (bit 0) in [chunk, eg): the chunk is one 128-byte line of the masks
        const uint4* __restrict__ line = reinterpret_cast<const uint4*>(flags + (eg & ~127ll));
        const int nb = (int)(eg & 127);
        int pos = fine_excl[eg >> FINE_SHIFT];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint4 v = line[j];
            const int r = nb - 16 * j;   // bytes of this word group that lie before eg
            if (r <= 0) continue;
            unsigned long long lo = ((unsigned long long)v.y << 32 | v.x) & 0x0101010101010101ull;
            unsigned long long hi = ((unsigned long long)v.w << 32 | v.z) & 0x0101010101010101ull;
            if (r < 8) {
                lo &= (1ull << (8 * r)) - 1;
                hi = 0;
            } else if (r < 16) {
                hi &= r == 8 ? 0ull : (1ull << (8 * (r - 8))) - 1;
            }
            pos += __popcll(lo) + __popcll(hi);
        }
        if (pos >= capacity) continue;
        apds_keypoint kp;
        kp.x = __uint_as_float(rx);
        kp.y = ref[3 * (size_t)i + 1];
        kp.size = (T.esigma[lvl] * 1.5f) * 2.0f;
        kp.angle = 0.0f;
        kp.response = ref[3 * (size_t)i + 2];
        kp.octave = T.octave[lvl];
        kp.class_id = lvl;
        kps[pos] = kp;
    }
}

// flags[lo, hi) = the masks of a run of consecutive levels (a stage); block b covers the 16 KiB from (lo & ~15) + b * 16 KiB. Bytes
// outside [lo, hi) belong to other stages and read as zero.
__device__ __forceinline__ uint4 load_flags16_range(const uint8_t* __restrict__ flags, long long base, long long lo, long long hi) {
    if (base >= lo && base + 16 <= hi) return *reinterpret_cast<const uint4*>(flags + base);
    uint32_t w[4] = {0, 0, 0, 0};
    for (int b = 0; b < 16; b++)
        if (base + b >= lo && base + b < hi && (flags[base + b] & 1)) w[b >> 2] |= 1u << (8 * (b & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// kp_base[0] = index of the stage's first keypoint in the image's output (the keypoints of the earlier stages come first: output
// order is level-major), written by the stage's scan; kp_base == nullptr: 0.
__global__ __launch_bounds__(SCAN_BLOCK) void emit_keypoints_kernel(LevelTable T, const uint8_t* __restrict__ flags, long long lo, long long hi,
                                                                    const int* __restrict__ block_offsets, const int* __restrict__ kp_base,
                                                                    apds_keypoint* __restrict__ kps, int capacity, size_t kp_bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    flags = bofs(flags, T.bstride);
    block_offsets = bofs(block_offsets, T.bstride);
    kps = bofs(kps, kp_bstride);
    const int first = kp_base ? bofs(kp_base, T.bstride)[0] : 0;
    __shared__ int wsum[SCAN_BLOCK / 64];
    const long long base = (lo & ~15ll) + ((long long)blockIdx.x * SCAN_BLOCK + threadIdx.x) * 16;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (base < hi) v = load_flags16_range(flags, base, lo, hi);
    const int mine = __popc(v.x & 0x01010101u) + __popc(v.y & 0x01010101u) + __popc(v.z & 0x01010101u) + __popc(v.w & 0x01010101u);
    // exclusive position of this thread's first keypoint inside the block: wave prefix (shuffles) + earlier waves
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    if (!mine) return;
    int before = 0;
    for (int k = 0; k < wv; k++) before += wsum[k];
    int pos = first + block_offsets[blockIdx.x] + before + incl - mine;
    const uint32_t words[4] = {v.x, v.y, v.z, v.w};
    for (int b = 0; b < 16; b++) {
        if (!((words[b >> 2] >> (8 * (b & 3))) & 1)) continue;
        if (pos >= capacity) return;
        const long long e = base + b;
        int lvl = 0;
        while (lvl + 1 < T.n && e >= T.pix_offset[lvl + 1]) lvl++;
        const long long pix = e - T.pix_offset[lvl];
        const int y = (int)(pix / T.w[lvl]), x = (int)(pix - (long long)y * T.w[lvl]);
        const Refined r = refine(bofs(T.Ldet[lvl], T.bstride), T.w[lvl], x, y, T.ratio[lvl]);
        apds_keypoint kp;
        kp.x = r.x;
        kp.y = r.y;
        kp.size = (T.esigma[lvl] * 1.5f) * 2.0f;
        kp.angle = 0.0f;
        kp.response = r.response;
        kp.octave = T.octave[lvl];
        kp.class_id = lvl;
        kps[pos++] = kp;
    }
}

// Ordered compaction over the concatenated level masks: every thread owns 16 consecutive mask bytes (one 16-byte load),
// a block 16 KiB; per-block counts -> exclusive offsets (single block) -> emit.
__device__ __forceinline__ int nonzero_bytes(uint32_t w) {
    // bit 0 of a mask byte = keypoint (2 = dropped by the sub-pixel refinement)
    return __popc(w & 0x01010101u);
}

__global__ __launch_bounds__(SCAN_BLOCK) void kp_block_counts_kernel(const uint8_t* __restrict__ flags, long long lo, long long hi, int* __restrict__ block_counts,
                                                                     size_t bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    flags = bofs(flags, bstride);
    block_counts = bofs(block_counts, bstride);
    __shared__ int wsum[SCAN_BLOCK / 64];
    const long long base = (lo & ~15ll) + ((long long)blockIdx.x * SCAN_BLOCK + threadIdx.x) * 16;
    int c = 0;
    if (base < hi) {
        const uint4 v = load_flags16_range(flags, base, lo, hi);
        c = nonzero_bytes(v.x) + nonzero_bytes(v.y) + nonzero_bytes(v.z) + nonzero_bytes(v.w);
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
        for (int w = 0; w < SCAN_BLOCK / 64; w++) sum += wsum[w];
        block_counts[blockIdx.x] = sum;
    }
}

// block counts -> exclusive offsets inside the stage; kp_base[1] = kp_base[0] + the stage's keypoint count (kp_base[0]: the count of
// the stages before it, 0 for the first: the array starts zeroed)
__global__ __launch_bounds__(1024) void kp_scan_offsets_kernel(int* __restrict__ block_counts, int nblocks, int* __restrict__ kp_base, size_t bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    block_counts = bofs(block_counts, bstride);
    kp_base = bofs(kp_base, bstride);
    __shared__ int buf[1024];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nblocks; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < nblocks ? block_counts[i] : 0;
        buf[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const int add = threadIdx.x >= off ? buf[threadIdx.x - off] : 0;
            __syncthreads();
            buf[threadIdx.x] += add;
            __syncthreads();
        }
        const int incl = buf[threadIdx.x];
        if (i < nblocks) block_counts[i] = carry + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) kp_base[1] = kp_base[0] + carry;
}

// ---- max_points: keep the `keep` strongest (response desc, ties by detection order), in that order -------------
__global__ __launch_bounds__(256) void rank_select_kernel(const apds_keypoint* __restrict__ in, int n, int keep, apds_keypoint* __restrict__ out) {
    APDS_RAISE_WAVE_PRIORITY();
    __shared__ float s_resp[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const float mine = i < n ? in[i].response : 0.f;
    int rank = 0;
    for (int base = 0; base < n; base += 256) {
        const int j = base + threadIdx.x;
        s_resp[threadIdx.x] = j < n ? in[j].response : -1.f;
        __syncthreads();
        const int lim = min(256, n - base);
        for (int k = 0; k < lim; k++) {
            const float r = s_resp[k];
            rank += (r > mine) || (r == mine && base + k < i);
        }
        __syncthreads();
    }
    if (i < n && rank < keep) out[rank] = in[i];
}

// ---- host side ---------------------------------------------------------------------------------------------------
void compact_all_levels(const LevelTable& T, const SlabLayout& sl, const PixelMask& pmask, const MaskSupport& support, apds_keypoint* kps, int capacity,
                        hipStream_t s, const Batch& b) {
    const int B = b.n;
    const size_t kp_bstride = (size_t)capacity * sizeof(apds_keypoint);
    if (config().kp_ranked) {
        // the candidates count and place themselves (no pass over the masks)
        const dim3 cgrid(B > 1 ? 16 : 128, T.n, B);
        hipLaunchKernelGGL(subpixel_count_kernel, cgrid, dim3(256), 0, s, T, pmask, support, (const int*)sl.list_count, 0, sl.fine_counts, sl.coarse_counts);
        hipLaunchKernelGGL(kp_scan_fine_kernel, dim3(ceil_div(sl.n_fine, 1024), 1, B), dim3(1024), 0, s, sl.fine_counts, (const int*)sl.coarse_counts, sl.n_fine, sl.kp_base, b.stride);
        hipLaunchKernelGGL(emit_ranked_kernel, cgrid, dim3(256), 0, s, T, (const int*)sl.list_count, 0, (const uint8_t*)sl.mask_all,
                           (const int*)sl.fine_counts, kps, capacity, kp_bstride);
    } else {
        hipLaunchKernelGGL(subpixel_filter_kernel, dim3(B > 1 ? 16 : 64, T.n, B), dim3(256), 0, s, T, pmask, support, (const int*)sl.list_count, 0);
        const long long lo = 0, hi = sl.total_pix;
        hipLaunchKernelGGL(kp_block_counts_kernel, dim3(sl.nblocks, 1, B), dim3(SCAN_BLOCK), 0, s, (const uint8_t*)sl.mask_all, lo, hi, sl.block_counts, b.stride);
        hipLaunchKernelGGL(kp_scan_offsets_kernel, dim3(1, 1, B), dim3(1024), 0, s, sl.block_counts, sl.nblocks, sl.kp_base, b.stride);
        hipLaunchKernelGGL(emit_keypoints_kernel, dim3(sl.nblocks, 1, B), dim3(SCAN_BLOCK), 0, s, T, (const uint8_t*)sl.mask_all, lo, hi,
                           (const int*)sl.block_counts, (const int*)sl.kp_base, kps, capacity, kp_bstride);
    }
}

void compact_strongest(const LevelTable& Tb, const SlabLayout& sl, size_t slab_bytes, int bi, int n_all, int keep, apds_keypoint* out, hipStream_t s) {
    apds_keypoint* kps_all = ctx().alloc_n<apds_keypoint>(n_all);
    const uint8_t* masks = sl.mask_all + (size_t)bi * slab_bytes;
    int* bc = reinterpret_cast<int*>(reinterpret_cast<char*>(sl.block_counts) + (size_t)bi * slab_bytes);
    int* base2 = bc + sl.nblocks;   // two ints behind the block counts: {0, total}
    HIP_CHECK(hipMemsetAsync(base2, 0, 2 * sizeof(int), s));
    hipLaunchKernelGGL(kp_block_counts_kernel, dim3(sl.nblocks), dim3(SCAN_BLOCK), 0, s, masks, 0ll, sl.total_pix, bc, (size_t)0);
    hipLaunchKernelGGL(kp_scan_offsets_kernel, dim3(1), dim3(1024), 0, s, bc, sl.nblocks, base2, (size_t)0);
    hipLaunchKernelGGL(emit_keypoints_kernel, dim3(sl.nblocks), dim3(SCAN_BLOCK), 0, s, Tb, masks, 0ll, sl.total_pix, (const int*)bc, (const int*)nullptr, kps_all, n_all, (size_t)0);
    hipLaunchKernelGGL(rank_select_kernel, dim3(ceil_div(n_all, 256)), dim3(256), 0, s, (const apds_keypoint*)kps_all, n_all, keep, out);
}
}  // namespace apds
