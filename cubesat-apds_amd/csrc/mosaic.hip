// csrc/mosaic.hip — the mosaic resident in HBM and the window read of the preprocessor on it
// (/root/reference/geotiff_extractor/src/image_extractor/mod.rs:332-343: read_as::<f32>(window, window_size, size, Lanczos);
// preprocessor/src/main.rs:197-277 cuts every level of detail into tiles with it):
//   * a NaN-ignoring min/max reduction over the three bands (mod.rs:200-229 datasets_min_max);
//   * the nearest-neighbour gather (the rule of geotiff_extractor.py's host mirror, bit for bit);
//   * the separable Lanczos pair: a row pass that stages source rows in LDS and a column pass over the row-filtered strip. The weights
//     are computed in double on the host (apds_resample_weights), rounded once to f32 and read as per-output (start, count, weights)
//     tables; taps are clamped to the RASTER, so a tile's footprint reaches into its neighbours. One launch per pass covers every tile
//     and band of a batch. The rule itself (GDAL's convolution resampler restated) is in DESIGN.md section 2;
//   * the overview pyramid a COG carries beside the raster (levels of factor 2, 4, 8, ..., each resampled from the one below with
//     Keys' cubic): one fused launch per level, and the window read of a handle that has them served from the level GDAL would pick.
#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "kernels.h"

namespace apds {

struct MosaicLevel {
    int rows = 0, cols = 0;
    float* data = nullptr;   // [3][rows][cols]
};

struct Mosaic {
    int device = 0;
    int rows = 0, cols = 0;
    float* data = nullptr;   // [3][rows][cols]
    std::mutex m;            // the min/max cache and the one build of the overviews are the only state that changes after create
    bool mm_valid = false;
    double mm[6] = {0, 0, 0, 0, 0, 0};
    int ov_min_size = 0;                  // the argument the overviews were built with; 0: not built
    std::vector<MosaicLevel> overviews;   // level k >= 1 at [k - 1]: ceil(rows / 2^k) x ceil(cols / 2^k)
    int n_levels() const { return (int)overviews.size(); }
    MosaicLevel level(int k) const { return k == 0 ? MosaicLevel{rows, cols, data} : overviews[(size_t)k - 1]; }
};

// one tile of a batch: window origin, its x / y weight table (tap starts in a table are relative to the window origin), and the source
// rows [ylo, ylo + nr) its column taps reach
struct MosaicTile {
    int x0, y0, xt, yt, ylo, nr;
};

constexpr int kRowsPerBlock = 4;     // source rows a row-pass block filters with one read of the weights
constexpr int kSegCap = 2304;        // floats of one staged source-row segment: 8 * (256 + 6) + 2 = 2098 serves ratio 8 at 256 outputs a block
constexpr int kColsPerThread = 4;    // output rows a column-pass thread produces from one walk over the strip
// one cascade step of the overviews: ratio = n / ceil(n / 2) <= 2, so the cubic's radius 2 * ratio <= 4 and an output has at most 9 taps
constexpr int kOvTaps = 9;
constexpr int kOvTx = 64, kOvTy = 16;   // outputs of one block: a wave is one output row wide
constexpr int kOvSrcW = 144;            // source columns under 64 outputs: 63 * 2 + 9 = 135, 3 in front and 3 behind for 16-byte loads
constexpr int kOvSrcH = 40;             // source rows under 16 outputs: 15 * 2 + 9 = 39
constexpr int kOvRowsPerWave = kOvTy / 4;

// NaN is the identity of both folds: a band without a number reduces to NaN, as numpy's nanmin / nanmax give it
__device__ __forceinline__ float nan_min(float a, float v) { return (v < a || a != a) ? v : a; }
__device__ __forceinline__ float nan_max(float a, float v) { return (v > a || a != a) ? v : a; }

// grid (blocks, bands): band b of `lo_src` is folded by min into out_lo[b * gridDim.x + block], of `hi_src` by max into out_hi. The first
// pass gives the mosaic for both; the second pass (one block per band) gives the first pass's partial results.
__global__ __launch_bounds__(256) void mosaic_minmax_kernel(const float* __restrict__ lo_src, const float* __restrict__ hi_src, size_t n, float* __restrict__ out_lo,
                                                            float* __restrict__ out_hi) {
    APDS_RAISE_WAVE_PRIORITY();
    const float* lo = lo_src + (size_t)blockIdx.y * n;
    const float* hi = hi_src + (size_t)blockIdx.y * n;
    const float qnan = __int_as_float(0x7FC00000);
    float mn = qnan, mx = qnan;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if (lo == hi && (n & 3) == 0) {   // the mosaic itself: 16 bytes a lane (a band starts 16-byte aligned when n is a multiple of four)
        const float4* v4 = reinterpret_cast<const float4*>(lo);
        for (size_t i = tid; i < n / 4; i += stride) {
            const float4 v = v4[i];
            mn = nan_min(nan_min(nan_min(nan_min(mn, v.x), v.y), v.z), v.w);
            mx = nan_max(nan_max(nan_max(nan_max(mx, v.x), v.y), v.z), v.w);
        }
    } else {
        for (size_t i = tid; i < n; i += stride) {
            mn = nan_min(mn, lo[i]);
            mx = nan_max(mx, hi[i]);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        mn = nan_min(mn, __shfl_down(mn, off));
        mx = nan_max(mx, __shfl_down(mx, off));
    }
    __shared__ float smn[4], smx[4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        smn[wave] = mn;
        smx[wave] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) {
            mn = nan_min(mn, smn[w]);
            mx = nan_max(mx, smx[w]);
        }
        out_lo[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = mn;
        out_hi[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = mx;
    }
}

// grid (ceil(out_w / 256), out_h, 3 * n_tiles): out[band][tile][oy][ox] = src[band][y0 + ys[oy]][x0 + xs[ox]]
__global__ __launch_bounds__(256) void mosaic_nearest_kernel(const float* __restrict__ src, int rows, int cols, const MosaicTile* __restrict__ tiles, int n_tiles,
                                                             const int* __restrict__ xs, const int* __restrict__ ys, int out_w, int out_h, float* __restrict__ out) {
    APDS_RAISE_WAVE_PRIORITY();
    const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y, z = blockIdx.z;
    if (ox >= out_w) return;
    const int band = z / n_tiles;
    const MosaicTile t = tiles[z - band * n_tiles];
    const int sx = min(max(t.x0 + xs[ox], 0), cols - 1), sy = min(max(t.y0 + ys[oy], 0), rows - 1);   // the host has checked the window: never clamps
    out[((size_t)z * out_h + oy) * out_w + ox] = src[((size_t)band * rows + sy) * cols + sx];
}

// Row pass. grid (ceil(out_w / oxb), ceil(nr_max / kRowsPerBlock), 3 * n_tiles), 256 threads: a block filters kRowsPerBlock source rows
// of one tile and band for `oxb` (<= 256) neighbouring outputs. Their taps cover one contiguous piece of each row (start and start + count
// grow with the output index), which is read once, coalesced, into LDS; thread i then walks output i's taps with its weights from the
// tap-major table (lanes read neighbouring floats), one weight read serving the four rows. f32 accumulation in tap order.
__global__ __launch_bounds__(256) void mosaic_lanczos_rows_kernel(const float* __restrict__ src, int rows, int cols, const MosaicTile* __restrict__ tiles, int n_tiles,
                                                                  const int* __restrict__ xstart, const int* __restrict__ xcount, const float* __restrict__ xw,
                                                                  int taps_x, int out_w, int oxb, int nr_max, float* __restrict__ tmp) {
    APDS_RAISE_WAVE_PRIORITY();
    __shared__ float seg[kRowsPerBlock][kSegCap];
    const int z = blockIdx.z, band = z / n_tiles;
    const MosaicTile t = tiles[z - band * n_tiles];
    const int r0 = blockIdx.y * kRowsPerBlock;
    if (r0 >= t.nr) return;   // block-uniform: in front of the barrier
    const int nrow = min(kRowsPerBlock, t.nr - r0);
    const int ox0 = blockIdx.x * oxb, oxn = min(oxb, out_w - ox0);
    const int* st = xstart + (size_t)t.xt * out_w;
    const int* cn = xcount + (size_t)t.xt * out_w;
    const int seg0 = max(t.x0 + st[ox0], 0);
    const int len = min(min(t.x0 + st[ox0 + oxn - 1] + cn[ox0 + oxn - 1], cols) - seg0, kSegCap);
    const int tid = threadIdx.x;
    for (int r = 0; r < kRowsPerBlock; r++) {
        const int y = min(t.ylo + r0 + min(r, nrow - 1), rows - 1);   // rows past the tile's strip repeat its last one (computed, not stored)
        const float* row = src + ((size_t)band * rows + y) * cols + seg0;
        for (int i = tid; i < len; i += 256) seg[r][i] = row[i];
    }
    __syncthreads();
    if (tid >= oxn) return;
    const int ox = ox0 + tid;
    const int s = max(t.x0 + st[ox] - seg0, 0);
    const int c = min(cn[ox], len - s);
    const float* w = xw + (size_t)t.xt * taps_x * out_w + ox;
    float acc[kRowsPerBlock] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < c; k++) {
        const float wk = w[(size_t)k * out_w];
#pragma unroll
        for (int r = 0; r < kRowsPerBlock; r++) acc[r] = __builtin_fmaf(seg[r][s + k], wk, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < kRowsPerBlock; r++)
        if (r < nrow) tmp[((size_t)z * nr_max + r0 + r) * out_w + ox] = acc[r];
}

// Column pass. grid (ceil(out_w / 256), ceil(out_h / kColsPerThread), 3 * n_tiles): a thread owns one output column and kColsPerThread
// neighbouring output rows; it walks the union of their taps down the row-filtered strip once (lanes read neighbouring floats of one strip
// row), the weights are the same for the whole block (scalar loads). f32 accumulation in tap order per output.
__global__ __launch_bounds__(256) void mosaic_lanczos_cols_kernel(const float* __restrict__ tmp, const MosaicTile* __restrict__ tiles, int n_tiles,
                                                                  const int* __restrict__ ystart, const int* __restrict__ ycount, const float* __restrict__ yw,
                                                                  int taps_y, int out_w, int out_h, int nr_max, float* __restrict__ out) {
    APDS_RAISE_WAVE_PRIORITY();
    const int z = blockIdx.z, band = z / n_tiles;
    const MosaicTile t = tiles[z - band * n_tiles];
    const int oy0 = blockIdx.y * kColsPerThread, ox = blockIdx.x * 256 + threadIdx.x;
    if (ox >= out_w) return;
    const int* st = ystart + (size_t)t.yt * out_h;
    const int* cn = ycount + (size_t)t.yt * out_h;
    int s[kColsPerThread], c[kColsPerThread];
    const float* w[kColsPerThread];
    int rlo = 0, rhi = 0;
#pragma unroll
    for (int o = 0; o < kColsPerThread; o++) {
        const int oy = min(oy0 + o, out_h - 1);
        s[o] = t.y0 + st[oy];
        c[o] = oy0 + o < out_h ? cn[oy] : 0;
        w[o] = yw + ((size_t)t.yt * out_h + oy) * taps_y;
        if (o == 0) rlo = s[o];
        rhi = max(rhi, s[o] + c[o]);
    }
    rlo = max(rlo, t.ylo);
    rhi = min(rhi, t.ylo + t.nr);
    const float* col = tmp + (size_t)z * nr_max * out_w + ox;
    float acc[kColsPerThread] = {0.f, 0.f, 0.f, 0.f};
    for (int r = rlo; r < rhi; r++) {
        const float v = col[(size_t)(r - t.ylo) * out_w];
#pragma unroll
        for (int o = 0; o < kColsPerThread; o++) {
            const int k = r - s[o];
            if (k >= 0 && k < c[o]) acc[o] = __builtin_fmaf(v, w[o][k], acc[o]);
        }
    }
#pragma unroll
    for (int o = 0; o < kColsPerThread; o++)
        if (oy0 + o < out_h) out[((size_t)z * out_h + oy0 + o) * out_w + ox] = acc[o];
}

// One cascade step of the overviews, level k - 1 -> level k, fused. grid (ceil(out_w / 64), ceil(out_h / 16), 3), 256 threads: a block owns
// 64 x 16 outputs of one band. It reads the source rectangle under them once into LDS (16 bytes a lane when rows start 16-byte aligned,
// i.e. cols is a multiple of four), filters rows (along x) into a second LDS array - lane i owns output column i with its weights in
// registers, a wave walks the source rows - and filters columns from that: lane i reads float i of a row (no bank conflict), the weights
// are the same for a wave (scalar loads). Per-output (start, count, weights[9]) tables, xw tap-major: odd sizes and the clamped edges are
// in the tables. f32, fused multiply-adds in tap order; NaN propagates. Nothing goes through the workspace.
__global__ __launch_bounds__(256) void mosaic_overview_kernel(const float* __restrict__ src, int rows, int cols, const int* __restrict__ xstart,
                                                              const int* __restrict__ xcount, const float* __restrict__ xw, const int* __restrict__ ystart,
                                                              const int* __restrict__ ycount, const float* __restrict__ yw, int out_w, int out_h,
                                                              float* __restrict__ out) {
    APDS_RAISE_WAVE_PRIORITY();
    __shared__ __attribute__((aligned(16))) float tile[kOvSrcH][kOvSrcW];
    __shared__ float filt[kOvSrcH][kOvTx];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int band = blockIdx.z;
    const int ox0 = blockIdx.x * kOvTx, oy0 = blockIdx.y * kOvTy;
    const int oxl = min(ox0 + kOvTx, out_w) - 1, oyl = min(oy0 + kOvTy, out_h) - 1;
    const int xs0 = xstart[ox0], xs1 = xstart[oxl] + xcount[oxl];   // starts and ends grow with the output index: one contiguous rectangle
    const int ys0 = ystart[oy0], ys1 = ystart[oyl] + ycount[oyl];
    const bool vec = (cols & 3) == 0;
    const int xa = vec ? xs0 & ~3 : xs0;
    const int w = min((vec ? (xs1 + 3) & ~3 : xs1) - xa, kOvSrcW);   // the host has checked that the rectangle fits: never clamps
    const int nr = min(ys1 - ys0, kOvSrcH);
    const float* base = src + ((size_t)band * rows + ys0) * cols + xa;
    if (vec) {
        const int nch = w >> 2;
        for (int i = tid; i < nr * nch; i += 256) {
            const int r = i / nch, ch = i - r * nch;
            *reinterpret_cast<float4*>(&tile[r][4 * ch]) = *reinterpret_cast<const float4*>(base + (size_t)r * cols + 4 * ch);
        }
    } else {
        for (int i = tid; i < nr * w; i += 256) {
            const int r = i / w, x = i - r * w;
            tile[r][x] = base[(size_t)r * cols + x];
        }
    }
    __syncthreads();
    const int ox = min(ox0 + lane, out_w - 1);   // lanes past the raster repeat its last column (computed, not stored)
    const int sx = max(xstart[ox] - xa, 0);
    const int cx = min(xcount[ox], w - sx);
    float wx[kOvTaps];
#pragma unroll
    for (int k = 0; k < kOvTaps; k++) wx[k] = xw[(size_t)k * out_w + ox];
    for (int r = wave; r < nr; r += 4) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < kOvTaps; k++)
            if (k < cx) acc = __builtin_fmaf(tile[r][sx + k], wx[k], acc);
        filt[r][lane] = acc;
    }
    __syncthreads();
    if (ox0 + lane >= out_w) return;
    for (int o = 0; o < kOvRowsPerWave; o++) {
        const int oy = oy0 + wave * kOvRowsPerWave + o;   // the same for a wave
        if (oy >= out_h) break;
        const int sy = max(ystart[oy] - ys0, 0);
        const int cy = min(ycount[oy], nr - sy);
        const float* wy = yw + (size_t)oy * kOvTaps;
        float acc = 0.f;
        for (int k = 0; k < cy; k++) acc = __builtin_fmaf(filt[sy + k][lane], wy[k], acc);
        out[((size_t)band * out_h + oy) * out_w + ox] = acc;
    }
}

namespace {

// L(0) = 1, L(x) = sin(pi x) sin(pi x / 3) / (pi^2 x^2 / 3) for 0 < |x| < 3, 0 otherwise
double lanczos3(double x) {
    if (x == 0.0) return 1.0;
    if (!(std::fabs(x) < 3.0)) return 0.0;
    const double a = M_PI * x;
    return std::sin(a) * std::sin(a / 3.0) / (a * a / 3.0);
}

// Keys' cubic with a = -0.5 (the overviews' kernel): support 2
double cubic(double x) {
    const double a = std::fabs(x);
    if (a <= 1.0) return 1.5 * a * a * a - 2.5 * a * a + 1.0;
    if (a < 2.0) return -0.5 * a * a * a + 2.5 * a * a - 4.0 * a + 2.0;
    return 0.0;
}

// a convolution kernel of the resampling rule: its function and the support it has at scale 1
struct ConvKernel {
    double (*f)(double);
    double support;
};
constexpr ConvKernel kLanczos3{lanczos3, 3.0}, kCubic{cubic, 2.0};

int nearest_index(int i, int win, int n_out) {
    return (int)std::min<int64_t>((int64_t)((i + 0.5) * ((double)win / n_out)), (int64_t)win - 1);
}

// taps [first, last) of output i, clamped to the raster (n_src <= 0: no raster, the footprint as it is)
void conv_taps(int n_src, double offset, double ratio, double radius, int i, int* first, int* last, double* centre) {
    const double c = (i + 0.5) * ratio + offset;
    const double lo = std::floor(c - radius + 0.5), hi = c + radius + 0.5;
    *first = (int)(n_src > 0 ? std::max(lo, 0.0) : lo);
    *last = (int)(n_src > 0 ? std::min(hi, (double)n_src) : hi);   // (int) truncates, as the rule's cast does
    *centre = c;
}

// the table of one axis under kernel `kern`: start / count / weights[max_taps] per output, and the widest footprint (start null: only that)
int conv_table(const ConvKernel& kern, int n_src, double offset, double ratio, int n_out, int max_taps, int32_t* start, int32_t* count, float* weights) {
    const double sw = std::min(1.0, 1.0 / ratio), radius = kern.support / sw;
    int need = 1;
    std::vector<double> w;
    for (int i = 0; i < n_out; i++) {
        int a, b;
        double c;
        conv_taps(n_src, offset, ratio, radius, i, &a, &b, &c);
        need = std::max(need, b - a);
        if (!start) continue;
        w.resize((size_t)std::max(b - a, 1));
        double sum = 0.0;
        for (int j = a; j < b; j++) {
            w[j - a] = kern.f((j + 0.5 - c) * sw);
            sum += w[j - a];
        }
        start[i] = a;
        count[i] = b - a;
        for (int j = a; j < b; j++) weights[(size_t)i * max_taps + (j - a)] = (float)(w[j - a] / sum);
    }
    return need;
}

// the (start, count, weights[max_taps]) table of one axis; max_taps = 0: only *taps_needed is computed. Throws on bad arguments.
void resample_table(int n_src, double offset, double span, int n_out, int resample, int max_taps, int32_t* start, int32_t* count, float* weights,
                    int* taps_needed) {
    APDS_REQUIRE(n_src > 0 && n_out > 0 && span > 0, APDS_ERR_ASSERT, "empty raster, window or output");
    APDS_REQUIRE(resample == APDS_RESAMPLE_NEAREST || resample == APDS_RESAMPLE_LANCZOS, APDS_ERR_BAD_ARG, "unknown resampling mode");
    APDS_REQUIRE(offset >= 0 && offset + span <= (double)n_src, APDS_ERR_OUT_OF_RANGE, "window outside the raster");
    const double ratio = span / n_out;
    APDS_REQUIRE(ratio <= 64.0, APDS_ERR_BAD_ARG, "window / output above 64 (385 taps) is not served");
    const int need = resample == APDS_RESAMPLE_LANCZOS ? conv_table(kLanczos3, n_src, offset, ratio, n_out, 0, nullptr, nullptr, nullptr) : 1;
    if (taps_needed) *taps_needed = need;
    if (max_taps == 0 && !start) return;
    APDS_REQUIRE(start && count && weights, APDS_ERR_BAD_ARG, "null output");
    APDS_REQUIRE(max_taps >= need, APDS_ERR_BAD_ARG, "max_taps is smaller than the widest footprint");
    std::fill(weights, weights + (size_t)n_out * max_taps, 0.0f);
    if (resample == APDS_RESAMPLE_NEAREST) {
        for (int i = 0; i < n_out; i++) {
            start[i] = (int)offset + nearest_index(i, (int)span, n_out);
            count[i] = 1;
            weights[(size_t)i * max_taps] = 1.0f;
        }
        return;
    }
    conv_table(kLanczos3, n_src, offset, ratio, n_out, max_taps, start, count, weights);
}

// The tables of one axis of a batch. A window origin moves the taps with it and changes nothing else, unless the raster's edge cuts a
// footprint: every window whose footprints lie inside the raster shares ONE table, computed at origin 0 without the clamp (so its
// weights do not depend on which windows are batched together); a window that touches an edge gets the table of its own origin
// (apds_resample_weights' arithmetic). Tap starts are stored relative to the window origin.
struct AxisTables {
    std::vector<int> keys;        // -1: the shared interior table; otherwise the origin of an edge window
    std::vector<int32_t> start, count, in_start, in_count;
    std::vector<float> weights, in_weights;   // [table][n_out][taps]
    int taps = 1, n_src = 0, win = 0, n_out = 0;
    void prepare(int n_src_, int win_, int n_out_) {
        n_src = n_src_, win = win_, n_out = n_out_;
        const double ratio = (double)win / n_out;
        taps = conv_table(kLanczos3, 0, 0.0, ratio, n_out, 0, nullptr, nullptr, nullptr);   // the clamp only shortens a footprint
        in_start.resize((size_t)n_out);
        in_count.resize((size_t)n_out);
        in_weights.assign((size_t)n_out * taps, 0.0f);
        conv_table(kLanczos3, 0, 0.0, ratio, n_out, taps, in_start.data(), in_count.data(), in_weights.data());
    }
    int index_of(int origin) {
        const bool interior = origin + in_start[0] >= 0 && origin + in_start[n_out - 1] + in_count[n_out - 1] <= n_src;
        const int key = interior ? -1 : origin;
        for (size_t i = 0; i < keys.size(); i++)
            if (keys[i] == key) return (int)i;
        keys.push_back(key);
        return (int)keys.size() - 1;
    }
    void build() {
        const size_t n = keys.size();
        for (int key : keys)
            if (key >= 0) {
                int need = 1;
                resample_table(n_src, key, win, n_out, APDS_RESAMPLE_LANCZOS, 0, nullptr, nullptr, nullptr, &need);
                taps = std::max(taps, need);
            }
        start.resize(n * n_out);
        count.resize(n * n_out);
        weights.resize(n * n_out * taps);
        for (size_t i = 0; i < n; i++) {
            if (keys[i] < 0) {
                std::copy(in_start.begin(), in_start.end(), start.begin() + i * n_out);
                std::copy(in_count.begin(), in_count.end(), count.begin() + i * n_out);
                const int in_taps = (int)(in_weights.size() / n_out);
                for (int k = 0; k < n_out; k++)
                    for (int j = 0; j < taps; j++) weights[(i * n_out + k) * taps + j] = j < in_taps ? in_weights[(size_t)k * in_taps + j] : 0.0f;
                continue;
            }
            resample_table(n_src, keys[i], win, n_out, APDS_RESAMPLE_LANCZOS, taps, &start[i * n_out], &count[i * n_out], &weights[i * n_out * taps], nullptr);
            for (int k = 0; k < n_out; k++) start[i * n_out + k] -= keys[i];
        }
    }
};

template <class T>
T* upload(ThreadCtx& c, const std::vector<T>& v, hipStream_t s) {
    T* d = c.alloc_n<T>(std::max<size_t>(v.size(), 1));
    if (!v.empty()) HIP_CHECK(hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return d;
}

}  // namespace

int mosaic_device(const Mosaic* m) {
    APDS_REQUIRE(m, APDS_ERR_BAD_ARG, "null argument");
    return m->device;
}

void mosaic_check_window(const Mosaic* m, int level, const int32_t* xy0, int n_tiles, int win_w, int win_h, int out_w, int out_h, int resample) {
    APDS_REQUIRE(m && xy0, APDS_ERR_BAD_ARG, "null argument");
    APDS_REQUIRE(level >= 0 && level <= m->n_levels(), APDS_ERR_OUT_OF_RANGE, "the mosaic has no such overview level");
    const MosaicLevel lv = m->level(level);
    APDS_REQUIRE(n_tiles >= 1 && n_tiles <= 4096, APDS_ERR_BAD_ARG, "batch must hold 1 .. 4096 tiles");
    APDS_REQUIRE(win_w > 0 && win_h > 0 && out_w > 0 && out_h > 0, APDS_ERR_ASSERT, "empty window or output");
    APDS_REQUIRE(resample == APDS_RESAMPLE_NEAREST || resample == APDS_RESAMPLE_LANCZOS, APDS_ERR_BAD_ARG, "unknown resampling mode");
    for (int i = 0; i < n_tiles; i++) {
        const int64_t x0 = xy0[2 * i], y0 = xy0[2 * i + 1];
        APDS_REQUIRE(x0 >= 0 && y0 >= 0 && x0 + win_w <= lv.cols && y0 + win_h <= lv.rows, APDS_ERR_OUT_OF_RANGE, "window outside the raster");
    }
    APDS_REQUIRE((int64_t)win_w <= 64ll * out_w && (int64_t)win_h <= 64ll * out_h, APDS_ERR_BAD_ARG, "window / output above 64 (385 taps) is not served");
    APDS_REQUIRE(m->device == ctx().device, APDS_ERR_BAD_ARG, "the mosaic lives on another device than the calling thread's");
}

// The windows of n_tiles origins (xy0: x, y pairs, in the pixels of `level`) of that level's raster resampled to out_w x out_h, band-major
// on the device: out[band][tile][out_h][out_w]. The tables and the row-filtered strip live in the calling thread's workspace; returns when
// the kernels are done. The arguments have been checked.
void mosaic_window_device(const Mosaic* m, int level, const int32_t* xy0, int n_tiles, int win_w, int win_h, int out_w, int out_h, int resample, float* out,
                          hipStream_t s) {
    const MosaicLevel lv = m->level(level);
    ThreadCtx& c = ctx();
    std::vector<MosaicTile> tiles((size_t)n_tiles);
    for (int i = 0; i < n_tiles; i++) tiles[i] = MosaicTile{xy0[2 * i], xy0[2 * i + 1], 0, 0, 0, 0};
    const dim3 block(256);
    if (resample == APDS_RESAMPLE_NEAREST || (win_w == out_w && win_h == out_h)) {   // equal sizes copy the window under both modes
        std::vector<int> xs((size_t)out_w), ys((size_t)out_h);
        for (int i = 0; i < out_w; i++) xs[i] = nearest_index(i, win_w, out_w);
        for (int i = 0; i < out_h; i++) ys[i] = nearest_index(i, win_h, out_h);
        const MosaicTile* dt = upload(c, tiles, s);
        const int* dxs = upload(c, xs, s);
        const int* dys = upload(c, ys, s);
        {
            KernelTimer timer("mosaic_resample", s);
            for (int y = 0; y < out_h; y += 65535) {   // grid.y is a 16-bit quantity
                hipLaunchKernelGGL(mosaic_nearest_kernel, dim3(ceil_div(out_w, 256), std::min(out_h - y, 65535), 3 * n_tiles), block, 0, s, (const float*)lv.data,
                                   lv.rows, lv.cols, dt, n_tiles, dxs, dys + y, out_w, out_h, out + (size_t)y * out_w);
                HIP_CHECK(hipGetLastError());
            }
        }
        HIP_CHECK(hipStreamSynchronize(s));   // the host tables are this call's locals
        return;
    }
    AxisTables X, Y;
    X.prepare(lv.cols, win_w, out_w);
    Y.prepare(lv.rows, win_h, out_h);
    for (int i = 0; i < n_tiles; i++) {
        tiles[i].xt = X.index_of(tiles[i].x0);
        tiles[i].yt = Y.index_of(tiles[i].y0);
    }
    X.build();
    Y.build();
    int nr_max = 1;
    for (int i = 0; i < n_tiles; i++) {
        const size_t base = (size_t)tiles[i].yt * out_h;
        tiles[i].ylo = tiles[i].y0 + Y.start[base];
        tiles[i].nr = Y.start[base + out_h - 1] + Y.count[base + out_h - 1] - Y.start[base];
        nr_max = std::max(nr_max, tiles[i].nr);
    }
    // outputs per row-pass block: the largest power of two whose every group's source piece fits the LDS segment (one output always does: <= 385 taps)
    auto fits = [&](int per_block) {
        for (size_t tb = 0; tb < X.keys.size(); tb++)
            for (int g = 0; g < out_w; g += per_block) {
                const size_t a = tb * out_w + g, b = tb * out_w + std::min(g + per_block, out_w) - 1;
                if (X.start[b] + X.count[b] - X.start[a] > kSegCap) return false;
            }
        return true;
    };
    int oxb = 256;
    while (oxb > 1 && !fits(oxb)) oxb /= 2;
    std::vector<float> xw_t(X.weights.size());   // tap-major for the row pass: [table][tap][output]
    for (size_t tb = 0; tb < X.keys.size(); tb++)
        for (int i = 0; i < out_w; i++)
            for (int k = 0; k < X.taps; k++) xw_t[(tb * X.taps + k) * out_w + i] = X.weights[(tb * out_w + i) * X.taps + k];
    const MosaicTile* dt = upload(c, tiles, s);
    const int* dxs = upload(c, X.start, s);
    const int* dxc = upload(c, X.count, s);
    const float* dxw = upload(c, xw_t, s);
    const int* dys = upload(c, Y.start, s);
    const int* dyc = upload(c, Y.count, s);
    const float* dyw = upload(c, Y.weights, s);
    float* tmp = c.alloc_n<float>((size_t)3 * n_tiles * nr_max * out_w);
    APDS_REQUIRE(ceil_div(nr_max, kRowsPerBlock) <= 65535 && ceil_div(out_h, kColsPerThread) <= 65535, APDS_ERR_BAD_ARG, "window too tall for one launch");
    {
        KernelTimer timer("mosaic_resample", s);
        hipLaunchKernelGGL(mosaic_lanczos_rows_kernel, dim3(ceil_div(out_w, oxb), ceil_div(nr_max, kRowsPerBlock), 3 * n_tiles), block, 0, s, (const float*)lv.data, lv.rows,
                           lv.cols, dt, n_tiles, dxs, dxc, dxw, X.taps, out_w, oxb, nr_max, tmp);
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(mosaic_lanczos_cols_kernel, dim3(ceil_div(out_w, 256), ceil_div(out_h, kColsPerThread), 3 * n_tiles), block, 0, s, (const float*)tmp, dt, n_tiles,
                           dys, dyc, dyw, Y.taps, out_w, out_h, nr_max, out);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(s));   // the host tables are this call's locals
}

// GDAL's choice of overview for a read of win -> out, restated: the largest level whose factor does not exceed the
// read's own downsampling; 0 without overviews or below a factor of 2
int mosaic_best_level(const Mosaic* m, int win_w, int win_h, int out_w, int out_h) {
    const double desired = std::min((double)win_w / out_w, (double)win_h / out_h);
    if (desired < 2.0) return 0;
    int best = 0;
    for (int k = 1; k <= m->n_levels(); k++) {
        const MosaicLevel lv = m->level(k);
        if (std::min((double)m->cols / lv.cols, (double)m->rows / lv.rows) <= desired) best = k;
    }
    return best;
}

// a base-raster window on one axis of a level, as GDAL's overview read maps an integer window: origin and extent rounded to the nearest
// pixel of the level, the extent at least 1 and shortened to the level's edge
static void map_to_level(int n_base, int n_level, int x0, int win, int32_t* ox, int* ow) {
    const double f = (double)n_base / n_level;
    *ox = std::min(n_level - 1, (int)(x0 / f + 0.5));
    *ow = std::min(std::max(1, (int)(win / f + 0.5)), n_level - *ox);
}

// What apds_mosaic_window and apds_mosaic_tile_extract* read: without overviews the window itself; with them the window mapped onto the
// level mosaic_best_level picks, read there with the caller's mode (for windows a power of two times the output that is a copy of the
// overview). The windows have been checked against the base raster. out as mosaic_window_device.
void mosaic_read_device(const Mosaic* m, const int32_t* xy0, int n_tiles, int win_w, int win_h, int out_w, int out_h, int resample, float* out, hipStream_t s) {
    const int level = mosaic_best_level(m, win_w, win_h, out_w, out_h);
    if (level == 0) return mosaic_window_device(m, 0, xy0, n_tiles, win_w, win_h, out_w, out_h, resample, out, s);
    const MosaicLevel lv = m->level(level);
    std::vector<int32_t> xy((size_t)2 * n_tiles);
    std::vector<int> wh((size_t)2 * n_tiles);
    bool one_shape = true;
    for (int i = 0; i < n_tiles; i++) {
        map_to_level(m->cols, lv.cols, xy0[2 * i], win_w, &xy[2 * i], &wh[2 * i]);
        map_to_level(m->rows, lv.rows, xy0[2 * i + 1], win_h, &xy[2 * i + 1], &wh[2 * i + 1]);
        one_shape = one_shape && wh[2 * i] == wh[0] && wh[2 * i + 1] == wh[1];
    }
    if (one_shape) {
        mosaic_check_window(m, level, xy.data(), n_tiles, wh[0], wh[1], out_w, out_h, resample);
        return mosaic_window_device(m, level, xy.data(), n_tiles, wh[0], wh[1], out_w, out_h, resample, out, s);
    }
    // a window that the level's edge shortened has tables of its own: tile by tile, each moved to its place in the band-major batch
    const size_t px = (size_t)out_w * out_h;
    float* one = ctx().alloc_n<float>(3 * px);
    for (int i = 0; i < n_tiles; i++) {
        mosaic_check_window(m, level, &xy[2 * i], 1, wh[2 * i], wh[2 * i + 1], out_w, out_h, resample);
        mosaic_window_device(m, level, &xy[2 * i], 1, wh[2 * i], wh[2 * i + 1], out_w, out_h, resample, one, s);
        for (int b = 0; b < 3; b++)
            HIP_CHECK(hipMemcpyAsync(out + ((size_t)b * n_tiles + i) * px, one + b * px, px * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));
}

namespace {

struct OverviewStep {
    MosaicLevel dst;
    std::vector<int32_t> xs, xc, ys, yc;
    std::vector<float> xw, yw;   // xw tap-major [9][cols], yw [rows][9]
};

// the tables of one axis of one cascade step; the source pieces a block of `per_block` outputs reads must fit `cap`
void overview_axis(int n_src, int n_out, int per_block, int cap, std::vector<int32_t>& start, std::vector<int32_t>& count, std::vector<float>& weights) {
    start.resize((size_t)n_out);
    count.resize((size_t)n_out);
    weights.assign((size_t)n_out * kOvTaps, 0.0f);
    const double ratio = (double)n_src / n_out;
    const int need = conv_table(kCubic, n_src, 0.0, ratio, n_out, kOvTaps, start.data(), count.data(), weights.data());
    APDS_REQUIRE(need <= kOvTaps, APDS_ERR_INTERNAL, "an overview footprint above 9 taps");
    for (int g = 0; g < n_out; g += per_block) {
        const int l = std::min(g + per_block, n_out) - 1;
        APDS_REQUIRE(start[g] >= 0 && start[l] + count[l] <= n_src && start[l] + count[l] - start[g] <= cap, APDS_ERR_INTERNAL, "an overview block's source piece does not fit");
    }
}

}  // namespace

// Builds the overviews (once; under the handle's mutex): levels of factor 2, 4, ... while the level below exceeds min_size on either axis,
// each from the one below, one fused launch per level. Returns the number of levels.
int mosaic_build_overviews(Mosaic* m, int min_size) {
    if (min_size <= 0) min_size = 512;   // the COG driver's block size
    std::lock_guard<std::mutex> g(m->m);
    if (m->ov_min_size) {
        APDS_REQUIRE(m->ov_min_size == min_size, APDS_ERR_BAD_ARG, "the overviews have been built with another min_size");
        return m->n_levels();
    }
    ThreadCtx& c = ctx();
    APDS_REQUIRE(m->device == c.device, APDS_ERR_BAD_ARG, "the mosaic lives on another device than the calling thread's");
    c.ws_reset();
    hipStream_t s = c.stream;
    std::vector<OverviewStep> steps;
    try {
        MosaicLevel prev = m->level(0);
        while (prev.rows > min_size || prev.cols > min_size) {
            steps.emplace_back();
            OverviewStep& st = steps.back();
            st.dst.rows = (prev.rows + 1) / 2;
            st.dst.cols = (prev.cols + 1) / 2;
            APDS_REQUIRE(ceil_div(st.dst.rows, kOvTy) <= 65535, APDS_ERR_BAD_ARG, "raster too tall for one launch");
            overview_axis(prev.cols, st.dst.cols, kOvTx, kOvSrcW - 6, st.xs, st.xc, st.xw);
            overview_axis(prev.rows, st.dst.rows, kOvTy, kOvSrcH, st.ys, st.yc, st.yw);
            std::vector<float> t(st.xw.size());   // tap-major for the row pass
            for (int i = 0; i < st.dst.cols; i++)
                for (int k = 0; k < kOvTaps; k++) t[(size_t)k * st.dst.cols + i] = st.xw[(size_t)i * kOvTaps + k];
            st.xw.swap(t);
            HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&st.dst.data), (size_t)3 * st.dst.rows * st.dst.cols * sizeof(float)));
            prev = st.dst;
        }
        struct Dev {
            const int *xs, *xc, *ys, *yc;
            const float *xw, *yw;
        };
        std::vector<Dev> dev;
        for (const OverviewStep& st : steps) dev.push_back(Dev{upload(c, st.xs, s), upload(c, st.xc, s), upload(c, st.ys, s), upload(c, st.yc, s), upload(c, st.xw, s), upload(c, st.yw, s)});
        {
            KernelTimer timer("mosaic_overviews", s);
            prev = m->level(0);
            for (size_t k = 0; k < steps.size(); k++) {
                const MosaicLevel& d = steps[k].dst;
                hipLaunchKernelGGL(mosaic_overview_kernel, dim3(ceil_div(d.cols, kOvTx), ceil_div(d.rows, kOvTy), 3), dim3(256), 0, s, (const float*)prev.data, prev.rows,
                                   prev.cols, dev[k].xs, dev[k].xc, dev[k].xw, dev[k].ys, dev[k].yc, dev[k].yw, d.cols, d.rows, d.data);
                HIP_CHECK(hipGetLastError());
                prev = d;
            }
        }
        HIP_CHECK(hipStreamSynchronize(s));   // the host tables are this call's locals
    } catch (...) {
        for (OverviewStep& st : steps)
            if (st.dst.data) (void)hipFree(st.dst.data);
        throw;
    }
    for (const OverviewStep& st : steps) m->overviews.push_back(st.dst);
    m->ov_min_size = min_size;
    return m->n_levels();
}

// per-band minimum and maximum, NaN ignored (a band of NaN only: NaN), computed once per handle
void mosaic_min_max(Mosaic* m, double* minmax6) {
    std::lock_guard<std::mutex> g(m->m);
    if (!m->mm_valid) {
        ThreadCtx& c = ctx();
        APDS_REQUIRE(m->device == c.device, APDS_ERR_BAD_ARG, "the mosaic lives on another device than the calling thread's");
        c.ws_reset();
        hipStream_t s = c.stream;
        const size_t n = (size_t)m->rows * m->cols;
        const int blocks = (int)std::min<size_t>((n + 1023) / 1024, 2048);
        float* part = c.alloc_n<float>((size_t)6 * blocks + 6);
        float* plo = part, *phi = part + 3 * blocks, *res = part + 6 * blocks;
        {
            KernelTimer timer("mosaic_minmax", s);
            hipLaunchKernelGGL(mosaic_minmax_kernel, dim3(blocks, 3), dim3(256), 0, s, (const float*)m->data, (const float*)m->data, n, plo, phi);
            HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(mosaic_minmax_kernel, dim3(1, 3), dim3(256), 0, s, (const float*)plo, (const float*)phi, (size_t)blocks, res, res + 3);
            HIP_CHECK(hipGetLastError());
        }
        float h[6];
        HIP_CHECK(hipMemcpyAsync(h, res, sizeof h, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        for (int b = 0; b < 3; b++) {
            m->mm[2 * b] = h[b];
            m->mm[2 * b + 1] = h[3 + b];
        }
        m->mm_valid = true;
    }
    for (int i = 0; i < 6; i++) minmax6[i] = m->mm[i];
}

}  // namespace apds

using namespace apds;

extern "C" {

int apds_mosaic_create(void** mosaic, const void* red, const void* green, const void* blue, int rows, int cols, size_t row_stride, int on_device) {
    return guarded([&] {
        APDS_REQUIRE(mosaic, APDS_ERR_BAD_ARG, "null output");
        *mosaic = nullptr;
        APDS_REQUIRE(red && green && blue, APDS_ERR_BAD_ARG, "null argument");
        APDS_REQUIRE(rows > 0 && cols > 0, APDS_ERR_ASSERT, "empty raster");
        APDS_REQUIRE(row_stride >= (size_t)cols, APDS_ERR_ASSERT, "row stride smaller than a row");
        ThreadCtx& c = ctx();
        Mosaic* m = new Mosaic();
        m->device = c.device;
        m->rows = rows;
        m->cols = cols;
        try {
            const size_t n = (size_t)rows * cols;
            HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&m->data), 3 * n * sizeof(float)));
            const void* src[3] = {red, green, blue};
            for (int b = 0; b < 3; b++)
                HIP_CHECK(hipMemcpy2DAsync(m->data + b * n, (size_t)cols * 4, src[b], row_stride * 4, (size_t)cols * 4, rows,
                                           on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c.stream));
            HIP_CHECK(hipStreamSynchronize(c.stream));
        } catch (...) {
            if (m->data) (void)hipFree(m->data);
            delete m;
            throw;
        }
        *mosaic = m;
    });
}

int apds_mosaic_destroy(void* mosaic) {
    return guarded([&] {
        Mosaic* m = static_cast<Mosaic*>(mosaic);
        if (!m) return;
        if (m->data) {
            (void)hipSetDevice(m->device);
            (void)hipDeviceSynchronize();   // another thread's window read may still be queued
            (void)hipFree(m->data);
            for (const MosaicLevel& lv : m->overviews) (void)hipFree(lv.data);
            (void)hipSetDevice(ctx().device);
        }
        delete m;
    });
}

int apds_mosaic_info(const void* mosaic, int* rows, int* cols) {
    return guarded([&] {
        const Mosaic* m = static_cast<const Mosaic*>(mosaic);
        APDS_REQUIRE(m, APDS_ERR_BAD_ARG, "null mosaic");
        if (rows) *rows = m->rows;
        if (cols) *cols = m->cols;
    });
}

int apds_mosaic_min_max(void* mosaic, double* minmax6) {
    return guarded([&] {
        APDS_REQUIRE(mosaic && minmax6, APDS_ERR_BAD_ARG, "null argument");
        mosaic_min_max(static_cast<Mosaic*>(mosaic), minmax6);
    });
}

// host arithmetic only: no device is touched
int apds_resample_weights(int n_src, double offset, double span, int n_out, int resample, int max_taps, int32_t* start, int32_t* count, float* weights) {
    return guarded([&] {
        APDS_REQUIRE(start && count && weights, APDS_ERR_BAD_ARG, "null output");
        APDS_REQUIRE(max_taps >= 1, APDS_ERR_BAD_ARG, "max_taps must be positive");
        resample_table(n_src, offset, span, n_out, resample, max_taps, start, count, weights, nullptr);
    });
}

// host arithmetic only: no device is touched
int apds_overview_weights(int n_src, int n_out, int max_taps, int32_t* start, int32_t* count, float* weights) {
    int need = 0;
    const int rc = guarded([&] {
        APDS_REQUIRE(n_src > 0 && n_out > 0, APDS_ERR_ASSERT, "empty raster or output");
        APDS_REQUIRE(n_out <= n_src, APDS_ERR_BAD_ARG, "an overview is not larger than its source");
        const double ratio = (double)n_src / n_out;
        APDS_REQUIRE(ratio <= 64.0, APDS_ERR_BAD_ARG, "n_src / n_out above 64 is not served");
        need = conv_table(kCubic, n_src, 0.0, ratio, n_out, 0, nullptr, nullptr, nullptr);
        if (max_taps == 0 && !start && !count && !weights) return;
        APDS_REQUIRE(start && count && weights, APDS_ERR_BAD_ARG, "null output");
        APDS_REQUIRE(max_taps >= need, APDS_ERR_BAD_ARG, "max_taps is smaller than the widest footprint");
        std::fill(weights, weights + (size_t)n_out * max_taps, 0.0f);
        conv_table(kCubic, n_src, 0.0, ratio, n_out, max_taps, start, count, weights);
    });
    return rc == APDS_OK ? need : rc;
}

int apds_mosaic_build_overviews(void* mosaic, int min_size, int* n_levels) {
    APDS_RANGE("apds_mosaic_build_overviews");
    return guarded([&] {
        APDS_REQUIRE(mosaic, APDS_ERR_BAD_ARG, "null mosaic");
        const int n = mosaic_build_overviews(static_cast<Mosaic*>(mosaic), min_size);
        if (n_levels) *n_levels = n;
    });
}

int apds_mosaic_level_info(const void* mosaic, int level, int* rows, int* cols) {
    return guarded([&] {
        const Mosaic* m = static_cast<const Mosaic*>(mosaic);
        APDS_REQUIRE(m, APDS_ERR_BAD_ARG, "null mosaic");
        APDS_REQUIRE(level >= 0 && level <= m->n_levels(), APDS_ERR_OUT_OF_RANGE, "the mosaic has no such overview level");
        const MosaicLevel lv = m->level(level);
        if (rows) *rows = lv.rows;
        if (cols) *cols = lv.cols;
    });
}

int apds_mosaic_best_level(const void* mosaic, int win_w, int win_h, int out_w, int out_h, int* level) {
    return guarded([&] {
        const Mosaic* m = static_cast<const Mosaic*>(mosaic);
        APDS_REQUIRE(m && level, APDS_ERR_BAD_ARG, "null argument");
        APDS_REQUIRE(win_w > 0 && win_h > 0 && out_w > 0 && out_h > 0, APDS_ERR_ASSERT, "empty window or output");
        *level = mosaic_best_level(m, win_w, win_h, out_w, out_h);
    });
}

namespace {

// the window read of both entry points: `level` < 0 is the read of a base-raster window (mosaic_read_device)
void window_to_host(const Mosaic* m, int level, int x0, int y0, int win_w, int win_h, int out_w, int out_h, int resample, float* out3) {
    APDS_REQUIRE(out3, APDS_ERR_BAD_ARG, "null output");
    const int32_t xy0[2] = {x0, y0};
    mosaic_check_window(m, std::max(level, 0), xy0, 1, win_w, win_h, out_w, out_h, resample);
    ThreadCtx& c = ctx();
    c.ws_reset();
    hipStream_t s = c.stream;
    const size_t n = (size_t)3 * out_w * out_h;
    float* d = c.alloc_n<float>(n);
    if (level < 0)
        mosaic_read_device(m, xy0, 1, win_w, win_h, out_w, out_h, resample, d, s);
    else
        mosaic_window_device(m, level, xy0, 1, win_w, win_h, out_w, out_h, resample, d, s);
    HIP_CHECK(hipMemcpyAsync(out3, d, n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace

int apds_mosaic_window(void* mosaic, int x0, int y0, int win_w, int win_h, int out_w, int out_h, int resample, float* out3) {
    APDS_RANGE("apds_mosaic_window");
    return guarded([&] { window_to_host(static_cast<const Mosaic*>(mosaic), -1, x0, y0, win_w, win_h, out_w, out_h, resample, out3); });
}

int apds_mosaic_window_level(void* mosaic, int level, int x0, int y0, int win_w, int win_h, int out_w, int out_h, int resample, float* out3) {
    APDS_RANGE("apds_mosaic_window_level");
    return guarded([&] {
        APDS_REQUIRE(mosaic, APDS_ERR_BAD_ARG, "null argument");
        APDS_REQUIRE(level >= 0, APDS_ERR_OUT_OF_RANGE, "the mosaic has no such overview level");
        window_to_host(static_cast<const Mosaic*>(mosaic), level, x0, y0, win_w, win_h, out_w, out_h, resample, out3);
    });
}

}  // extern "C"
