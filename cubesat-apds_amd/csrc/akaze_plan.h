// csrc/akaze_plan.h — the host arithmetic of an AKAZE extraction: what is decided before the first launch. Plain C++17 without a GPU
// (tests/cpp/akaze_plan_host.cpp compiles it with g++): the evolution list, the FED step sizes, the Gaussian and INTER_AREA tap tables, the
// derivative weights, which kernel family serves the base stage and every level (plan_extraction: the table the driver executes), how many
// launches a level's FED steps take and where each pass lands, and the layout of one image's workspace slab.
//
// Replaces OpenCV AKAZEFeatures::Allocate_Memory_Evolution, fed_tau_by_process_time, getGaussianKernel, the tap tables of resize(INTER_AREA)
// and compute_derivative_kernels (the Scharr weights of a scaled 3 x 3 stencil).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <type_traits>
#include <vector>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

namespace apds {

#ifdef __HIPCC__
using Float2 = float2;
#else
struct Float2 {   // (only its size matters to the host: the (Lx, Ly) plane holds one per pixel)
    float x, y;
};
#endif

struct GaussTaps {
    float k[5];   // k[0] centre, k[j] the two taps at distance j
};

static constexpr int AKAZE_MAX_LEVELS = 16;
static constexpr float AKAZE_SOFFSET = 1.6f, AKAZE_DERIVATIVE_FACTOR = 1.5f, AKAZE_DTHRESHOLD = 0.001f;

// One evolution level (mirrors OpenCV's MEvolution / the oracle's Level)
struct LevelDesc {
    int w, h, octave, sigma_size, border;
    float esigma, etime, ratio;
    int nsteps;
    float tau[64];
    long long pix_offset;   // offset of this level in the level-major concatenated pixel index space
};

inline bool fed_is_prime(int n) {
    if (n <= 1) return false;
    if (n == 2 || n == 3 || n == 5 || n == 7) return true;
    if (n % 2 == 0 || n % 3 == 0 || n % 5 == 0 || n % 7 == 0) return false;
    const int upper = (int)std::sqrt((double)n + 1.0);
    for (int d = 11; d <= upper; d += 2)
        if (n % d == 0) return false;
    return true;
}

// fed_tau_by_process_time(T, 1, 0.25, reordering = true): FED step sizes for one evolution level
inline int fed_tau(float T, float tau_max, float* tau) {
    const int n = (int)std::ceil(sqrtf(3.0f * T / tau_max + 0.25f) - 0.5f - 1.0e-8f);
    if (n <= 0) return 0;
    if (n > 64) throw std::logic_error("FED cycle longer than expected");
    const float scale = 3.0f * T / (tau_max * (float)(n * (n + 1)));
    float tauh[64];
    const float c = 1.0f / (4.0f * (float)n + 2.0f);
    const float d = scale * tau_max / 2.0f;
    for (int k = 0; k < n; ++k) {
        const float hc = cosf((float)M_PI * (2.0f * (float)k + 1.0f) * c);
        tauh[k] = d / (hc * hc);
    }
    const int kappa = n / 2;
    int prime = n + 1;
    while (!fed_is_prime(prime)) prime++;
    for (int k = 0, l = 0; l < n; ++k, ++l) {
        int index = 0;
        while ((index = ((k + 1) * kappa) % prime - 1) >= n) k++;
        tau[l] = tauh[index];
    }
    return n;
}

// Allocate_Memory_Evolution: four octaves of four sublevels, ended early when the next octave would be narrower than 80 or lower than 40
inline std::vector<LevelDesc> akaze_levels(int W, int H) {
    std::vector<LevelDesc> ev;
    const int omax = 4, nsub = 4;
    const float smax = 10.0f * sqrtf(2.0f);
    int lw = W, lh = H, power = 1;
    long long total_pix = 0;
    for (int i = 0; i < omax; i++) {
        for (int j = 0; j < nsub; j++) {
            LevelDesc d{};
            d.w = lw;
            d.h = lh;
            d.esigma = AKAZE_SOFFSET * powf(2.f, (float)j / (float)nsub + i);
            d.sigma_size = (int)lrintf(d.esigma * AKAZE_DERIVATIVE_FACTOR / power);
            d.etime = 0.5f * (d.esigma * d.esigma);
            d.octave = i;
            d.ratio = (float)power;
            d.border = (int)lrintf(smax * d.sigma_size) + 1;
            d.pix_offset = total_pix;
            total_pix += (long long)lw * lh;
            ev.push_back(d);
        }
        power <<= 1;
        lh >>= 1;
        lw >>= 1;
        if (lw < 80 || lh < 40) break;
    }
    for (size_t i = 1; i < ev.size(); i++) ev[i].nsteps = fed_tau(ev[i].etime - ev[i - 1].etime, 0.25f, ev[i].tau);
    return ev;
}

inline GaussTaps gauss_taps(int n, double sigma) {
    double k[9], sum = 0;
    const double s2 = -0.5 / (sigma * sigma);
    for (int i = 0; i < n; i++) {
        const double x = i - (n - 1) * 0.5;
        k[i] = std::exp(s2 * x * x);
        sum += k[i];
    }
    GaussTaps t{};
    const int r = n / 2;
    for (int j = 0; j <= r; j++) t.k[j] = (float)(k[r + j] / sum);
    return t;
}

// INTER_AREA tap tables for one axis (<= 4 taps per destination pixel)
inline void area_tables(int ssize, int dsize, std::vector<int>& ofs, std::vector<float>& wgt, std::vector<int>& cnt) {
    const double scale = (double)ssize / dsize;
    ofs.assign((size_t)dsize * 4, 0);
    wgt.assign((size_t)dsize * 4, 0.f);
    cnt.assign(dsize, 0);
    for (int d = 0; d < dsize; d++) {
        const double f1 = d * scale, f2 = f1 + scale;
        const double cell = std::min(scale, ssize - f1);
        int s1 = (int)std::ceil(f1), s2 = (int)std::floor(f2);
        s2 = std::min(s2, ssize);
        s1 = std::min(s1, s2);
        auto push = [&](int sidx, double a) {
            if (cnt[d] >= 4) throw std::logic_error("area resize tap overflow");
            ofs[(size_t)d * 4 + cnt[d]] = sidx;
            wgt[(size_t)d * 4 + cnt[d]] = (float)a;
            cnt[d]++;
        };
        if (s1 - f1 > 1e-3) push(s1 - 1, (s1 - f1) / cell);
        for (int sx = s1; sx < s2; sx++) push(sx, 1.0 / cell);
        if (f2 - s2 > 1e-3) push(s2, std::min(std::min(f2 - s2, 1.0), cell) / cell);
    }
}

// side and middle weight of the scaled Scharr stencil of a level (sc = its sigma_size)
inline void deriv_weights(int sc, float& kside, float& kmid) {
    if (sc == 1) {
        kside = 3.0f / 32.0f;
        kmid = 10.0f / 32.0f;
    } else {
        const float wgt = 10.0f / 3.0f;
        const float norm = 1.0f / (2.0f * sc * (wgt + 2.0f));
        kside = norm;
        kmid = wgt * norm;
    }
}

// ---- which kernels serve an extraction ---------------------------------------------------------------------------------------------------
// Everything that picks a kernel family is decided here, before the first launch: plan_extraction (per level: Hessian kernel, start image,
// smoothing pass, head, FED passes, who writes the next octave's start image) and plan_base (the base stage). The driver
// (akaze_extract.hip) executes the table; a launcher launches what it is told and APDS_REQUIREs what its kernel cannot do.
//
// FED steps are issued in fused groups of up to `fuse` steps (temporal blocking in LDS): `launches` passes ping-pong between the level's Lt
// and a scratch plane and must end in Lt. Deeper fusion for the small octaves, whose launches are latency-bound. Small levels do Lsmooth,
// the conductivity and the first (usually all) steps in ONE launch (level_fused_kernel, up to LEVEL_FUSED_MAX_STEPS steps: pass 0); large
// levels may do the smoothing pass and pass 0 in one pass over register strips (level_stream_kernel / level_strip_kernel, up to 4 steps).
// Such a pass 0 is the level's HEAD. The steps are spread evenly over the passes that follow (e.g. 11 steps, fuse 8 -> 6 + 5).

// The values of the switches (config.h) that the plan depends on - 0 never, 1 by size, 2 always - and whether the Hessian kernels fork.
struct PlanSwitches {
    int nld_strip = 1, sf_strip = 1, base_strip = 1, level_strip = 1, level_fuse = 1, level_stream = 1, doh_strip = 1, half_fuse = 1;
    bool fork = false;
};

static constexpr int LEVEL_FUSED_MAX_STEPS = 29;      // level_fused_kernel's capacity (akaze_level_fused.hip asserts its LF_MAX_STEPS against it)
static constexpr int SF_TILE_W = 64, SF_TILE_H = 32;  // smooth_flow_kernel's tile

enum class Head { None, Stream, Strips, Fused };      // pass 0 with the smoothing in it: level_stream / level_strip / level_fused_kernel
enum class Smooth { None, Tiles, Strips };            // a separate smooth_flow pass: LDS tiles, or register strips + a frame of tiles
enum class Start { PrevLt, Written, HalfSample, AreaResize };   // Written: by the launch that finished the previous level (into tmpH)
enum class BaseStage { Strips, Separate };            // base_strip_kernel, or gray + two Gaussians + the gradient kernel

struct LevelPlan {
    static constexpr int MAX_PASSES = 18;   // <= 64 steps in groups of >= 4, + the fused head
    int fuse = 0;               // most steps of a pass (of pass 0 of a fused level: fused_max_steps)
    bool fused_level = false;   // pass 0 is level_fused_kernel's
    bool try_strips = false;    // pass 0 goes to a register-strip head if one can take the level
    int launches = 0;
    int first[MAX_PASSES] = {}, steps[MAX_PASSES] = {};   // pass p runs FED steps [first[p], first[p] + steps[p])
    bool lands_in_lt(int pass) const { return (launches - 1 - pass) % 2 == 0; }
    bool start_in_lt() const { return launches % 2 == 0; }   // where a resampled start image goes, so that the last pass lands in Lt
    // filled by plan_extraction
    bool doh_strips = false;    // the Hessian kernel: doh_strip_kernel, else doh_fused_kernel
    Start start = Start::PrevLt;
    Smooth smooth = Smooth::None;
    Head head = Head::None;
    bool strip_pass[MAX_PASSES] = {};   // a pass that is not the head: nld_strip_kernel, else nld_multi_kernel (LDS tiles)
    int half_pass = -1;         // the pass that also writes the next octave's start image (the last one), or -1: the next level resamples
    int support_unit = 0;       // mask_support_unit of the level: a mask support of n reaches n * support_unit full-resolution pixels
    int first_fed_pass() const { return head == Head::None ? 0 : 1; }
};

// The unit of a keypoint's descriptor support in full-resolution pixels, constant per level: scale * ratio, where scale is what
// akaze_describe.hip rounds from the keypoint's size, rint(0.5f * size / ratio) to nearest even with size = (esigma * 1.5f) * 2.0f (the
// M-LDB lattice and the orientation samples are laid out in steps of `scale` level pixels), and ratio = 2^octave. The mask support of an
// extraction (apds_akaze_extract_masked_support) is a whole number of these units per side of the keypoint's square.
inline int mask_support_unit(const LevelDesc& e) {
    const float size = (e.esigma * AKAZE_DERIVATIVE_FACTOR) * 2.0f;
    return (int)lrintf(0.5f * size / e.ratio) * (int)e.ratio;
}
// The radius a support of `support` units gives a level; past the largest image side every square is the whole image
inline int mask_support_radius(int support, int support_unit) { return (int)std::min<long long>((long long)support * support_unit, 65536); }

inline bool fits_32bit_offsets(int w, int h) { return (size_t)w * h < (size_t)1 << 29; }   // byte offsets into a float plane (buffer loads)

// smooth_flow's tiles [1, txi) x [1, tyi) lie inside the image with their 3-pixel halo (the strips' region; the frame around them: LDS tiles)
inline void smooth_flow_interior(int w, int h, int& txi, int& tyi) {
    txi = w >= SF_TILE_W + 67 ? (w - 67) / SF_TILE_W + 1 : 1;
    tyi = h >= SF_TILE_H + 35 ? (h - 35) / SF_TILE_H + 1 : 1;
}

// The pass arithmetic of one level. level_fuse, level_strip: the values of APDS_LEVEL_FUSE and APDS_LEVEL_STRIP
inline LevelPlan plan_level(const LevelDesc& e, int batch, int level_fuse, int level_strip, int fused_max_steps) {
    LevelPlan p;
    const size_t lpx = (size_t)e.w * e.h * batch;
    const bool small = lpx <= (size_t)1 << 20;
    p.fuse = small ? 8 : 4;
    p.fused_level = e.nsteps > 0 && level_fuse && (small || level_fuse == 2);
    const int head = p.fused_level ? std::min(e.nsteps, fused_max_steps) : 0;
    p.launches = (e.nsteps - head + p.fuse - 1) / p.fuse + (p.fused_level ? 1 : 0);
    if (p.launches > LevelPlan::MAX_PASSES) throw std::logic_error("more FED passes than expected");
    int pass = 0, k = 0;
    if (p.fused_level) {
        p.steps[0] = head;
        pass = 1;
        k = head;
    }
    for (; k < e.nsteps; pass++) {
        const int g = (e.nsteps - k + (p.launches - pass) - 1) / (p.launches - pass);
        p.first[pass] = k;
        p.steps[pass] = g;
        k += g;
    }
    if (pass != p.launches) throw std::logic_error("FED passes do not add up");
    // (every level of at least 1 Mpx. On the 16 Mpx levels of a 4096^2 frame the gain is within the box-to-box noise: the Hessian
    // kernel beside them is VALU-bound and the strips' recomputed halos cost issue slots — 1.89 against 1.93 ms in one run, 1.85
    // against 1.83 in another; 2048^2: 0.79 against 0.82. APDS_LEVEL_STRIP=2: every level whatever its size, 0: never)
    p.try_strips = !p.fused_level && e.nsteps > 0 && level_strip && (level_strip == 2 || lpx >= (size_t)1 << 20) && p.steps[0] <= 4;
    return p;
}

struct ExtractionPlan {
    std::vector<LevelPlan> level;   // level[0]: only doh_strips (Lt[0] comes from the base stage)
    int n_strip_levels = 0;         // the levels, a prefix of the list, whose Hessian kernel is the streaming one
};

// The thresholds (a batch counts as a whole: the strip and streaming kernels pay once a LAUNCH has enough pixels to be throughput-bound):
// streaming kernels from 8 Mpx (below that a level has too few 64-column strips to fill the chip with bands of a useful height - 2048^2: 41
// strips; bands of 16 rows spend half their walk on the warm-up rows - and the LDS tiles are quicker), FED strips from 1 Mpx (the LDS
// tiles keep the deeply fused launches of the small, latency-bound octaves: their unrolled strip code would not fit the instruction
// cache), smooth_flow's strips from 2 Mpx.
inline ExtractionPlan plan_extraction(const std::vector<LevelDesc>& ev, int batch, const PlanSwitches& sw) {
    const int L = (int)ev.size();
    ExtractionPlan plan;
    plan.level.resize(L);
    bool strip_prefix = true;
    for (int i = 0; i < L; i++) {
        const LevelDesc& e = ev[i];
        const size_t bpx = (size_t)e.w * e.h * batch;
        const bool fits = fits_32bit_offsets(e.w, e.h);
        LevelPlan& p = plan.level[i];
        if (i > 0) p = plan_level(e, batch, sw.level_fuse, sw.level_strip, LEVEL_FUSED_MAX_STEPS);
        // doh_strip_kernel writes the mask and status bytes of its whole level, and zero_slab_heads skips a PREFIX of the levels
        strip_prefix = strip_prefix && sw.doh_strip && e.sigma_size >= 2 && e.sigma_size <= 4 && e.w >= 64 && e.h >= 64 &&
                       (sw.doh_strip == 2 || bpx >= (size_t)1 << 23);
        p.doh_strips = strip_prefix;
        p.support_unit = mask_support_unit(e);
        plan.n_strip_levels += strip_prefix ? 1 : 0;
        if (i == 0) continue;

        const LevelDesc& prev = ev[i - 1];
        if (e.octave == prev.octave) p.start = Start::PrevLt;
        else if (plan.level[i - 1].half_pass >= 0) p.start = Start::Written;
        else p.start = prev.w == 2 * e.w && prev.h == 2 * e.h ? Start::HalfSample : Start::AreaResize;   // (odd sizes: the general area resize)

        if (p.fused_level) {
            p.head = Head::Fused;
        } else if (p.try_strips && p.steps[0] >= 1 && p.steps[0] <= 4 && fits) {
            if (sw.level_stream && e.w >= 64 && e.h >= 32 && (sw.level_stream == 2 || bpx >= (size_t)1 << 23)) p.head = Head::Stream;
            else if (e.w >= 2 && e.h >= 2) p.head = Head::Strips;
        }
        // the last level's Hessian kernel is on the critical path (nothing follows to hide it): when it forks, its Lsmooth comes from a
        // separate smoothing pass, so that it runs beside the level's FED steps
        if (p.head != Head::Stream && p.head != Head::Strips && (!p.fused_level || (sw.fork && i == L - 1))) {
            int txi, tyi;
            smooth_flow_interior(e.w, e.h, txi, tyi);
            const bool strips = sw.sf_strip && txi > 1 && tyi > 1 && fits && (bpx >= (size_t)1 << 21 || sw.sf_strip == 2);
            p.smooth = strips ? Smooth::Strips : Smooth::Tiles;
        }
        for (int q = p.first_fed_pass(); q < p.launches; q++)
            p.strip_pass[q] = sw.nld_strip && p.steps[q] <= 4 && (bpx >= (size_t)1 << 20 || sw.nld_strip == 2) && fits;
        // does the NEXT level start an octave from exactly half this level's size (the 2 x 2 mean)? Then the pass that finishes this
        // level writes that image too, if its kernel can: not level_strip_kernel, not the LDS tiles
        const bool want_half = sw.half_fuse && i + 1 < L && ev[i + 1].octave > e.octave && e.w == 2 * ev[i + 1].w && e.h == 2 * ev[i + 1].h;
        const int last = p.launches - 1;
        if (want_half && last >= 0 && (last < p.first_fed_pass() ? p.head == Head::Stream || p.head == Head::Fused : p.strip_pass[last])) p.half_pass = last;
    }
    return plan;
}

// The base stage: one fused pass on register strips for large images (the launch-bound small tiles keep the separate kernels), if the
// image fits 32-bit offsets and, with four channels, dword loads of the BGRA pixels. img: the address of the first image.
inline BaseStage plan_base(int rows, int cols, int channels, size_t stride, uintptr_t img, size_t img_stride, int batch, const PlanSwitches& sw) {
    const size_t px = (size_t)rows * cols;
    const bool strips = sw.base_strip && (px * batch >= (size_t)1 << 21 || sw.base_strip == 2) && px < (size_t)1 << 29 &&
                        (size_t)rows * stride < (size_t)1 << 31 && (channels != 4 || ((img | stride | img_stride) & 3) == 0);
    return strips ? BaseStage::Strips : BaseStage::Separate;
}

// ---- one image's workspace slab -------------------------------------------------------------------------------------------------------
// Constants of the layout that the kernels share: the pitch of the suppression's pending counters (same-line atomics serialise in L2, ~12 ns
// each, measured: one 128-byte line per counter), the ranked compaction's chunk (128 bytes of masks) and block (128 KiB, one counter per
// line), and the 16 KiB of masks a block of the mask-pass compaction covers.
static constexpr int PEND_PITCH = 32;
static constexpr int FINE_SHIFT = 7, COARSE_SHIFT = 17, COARSE_PITCH = 32;
static constexpr int SCAN_BLOCK = 1024, KP_BYTES_PER_BLOCK = SCAN_BLOCK * 16;

// Bump layout of one image's slab (all images of a batch: the same layout, `bytes` apart): lay_out(nullptr, ...) sizes it, lay_out(base, ...)
// once more places the planes. Every plane starts on a 256-byte boundary. The head up to `zero_bytes` starts zeroed: counters, then the
// keypoint masks and the suppression statuses of all levels, level-major.
struct SlabLayout {
    long long total_pix = 0;
    int nblocks = 0, n_fine = 0, n_coarse = 0;
    size_t mask_off = 0, status_off = 0, zero_bytes = 0, bytes = 0;
    int *list_count, *hist, *pend_count, *block_counts, *kp_base, *fine_counts, *coarse_counts;
    unsigned int* hmax_bits;
    float *k_oct, *gray, *tmpS, *tmpF, *tmpP, *tmpH;
    uint8_t *mask_all, *status_all;
    float *Lt[AKAZE_MAX_LEVELS], *Ldet[AKAZE_MAX_LEVELS], *lsm[AKAZE_MAX_LEVELS];
    Float2* Lxy[AKAZE_MAX_LEVELS];   // (Lx, Ly) interleaved
    uint32_t *list[AKAZE_MAX_LEVELS], *pend[AKAZE_MAX_LEVELS];
    int pend_cap[AKAZE_MAX_LEVELS];  // strict 3x3 maxima are never adjacent: a level has at most ceil(w / 2) * ceil(h / 2) candidates

    // lsm_per_level: a Lsmooth plane per level (the Hessian kernels run on a side stream), else one shared plane
    void lay_out(char* base, const std::vector<LevelDesc>& ev, bool lsm_per_level) {
        if (ev.empty() || ev.size() > (size_t)AKAZE_MAX_LEVELS) throw std::logic_error("level count out of range");
        size_t off = 0;
        auto take = [&](auto*& p, size_t n) {
            using T = std::remove_reference_t<decltype(*p)>;
            p = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + off);
            off += (n * sizeof(T) + 255) & ~(size_t)255;
        };
        const size_t n0 = (size_t)ev[0].w * ev[0].h;
        total_pix = ev.back().pix_offset + (long long)ev.back().w * ev.back().h;
        nblocks = (int)((total_pix + KP_BYTES_PER_BLOCK - 1) / KP_BYTES_PER_BLOCK);
        n_fine = (int)((total_pix >> FINE_SHIFT) + 1);
        n_coarse = (int)((total_pix >> COARSE_SHIFT) + 1);
        take(list_count, AKAZE_MAX_LEVELS);
        take(hmax_bits, 1);
        take(hist, 304);                      // 300 bins + the ticket counter of kcontrast_hist_kernel's last block
        take(pend_count, 3 * AKAZE_MAX_LEVELS * PEND_PITCH);
        take(kp_base, 8);                     // kp_base[0] stays 0, kp_base[1] = the image's keypoint count
        take(fine_counts, n_fine + 1024);     // ranked compaction: keypoints per 128-byte chunk of the masks (then their prefix)
        take(coarse_counts, (size_t)n_coarse * COARSE_PITCH);
        mask_off = off;
        take(mask_all, (size_t)total_pix + 128);   // (+ a line: the last chunk is read whole)
        status_off = off;
        take(status_all, (size_t)total_pix);
        zero_bytes = off;
        take(k_oct, 8);
        take(block_counts, nblocks + 4);
        take(gray, n0);
        take(tmpS, n0);
        take(tmpF, n0);
        take(tmpP, n0);
        take(tmpH, n0 / 4 + 64);              // the next octave's start image when the last level of an octave writes it itself
        for (size_t i = 0; i < ev.size(); i++) {
            const size_t n = (size_t)ev[i].w * ev[i].h;
            take(Lt[i], n);
            take(Lxy[i], n);
            take(Ldet[i], n);
            pend_cap[i] = ((ev[i].w + 1) / 2) * ((ev[i].h + 1) / 2);
            take(list[i], (size_t)pend_cap[i]);
            take(pend[i], 3 * (size_t)pend_cap[i]);   // three rotating buffers; idle once the suppression is done: then the refined keypoints
            if (lsm_per_level && i > 0) take(lsm[i], n);
            else lsm[i] = tmpS;
        }
        bytes = (off + 4095) & ~(size_t)4095;
    }
};

}  // namespace apds
