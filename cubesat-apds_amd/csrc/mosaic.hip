// csrc/mosaic.hip — the mosaic resident in HBM and the window read of the preprocessor on it
// (/root/reference/geotiff_extractor/src/image_extractor/mod.rs:332-343: read_as::<f32>(window, window_size, size, Lanczos);
// preprocessor/src/main.rs:197-277 cuts every level of detail into tiles with it):
//   * a NaN-ignoring min/max reduction over the three bands (mod.rs:200-229 datasets_min_max);
//   * the nearest-neighbour gather (the rule of geotiff_extractor.py's host mirror, bit for bit);
//   * the separable Lanczos pair: a row pass that stages source rows in LDS and a column pass over the row-filtered strip. The weights
//     are computed in double on the host (apds_resample_weights), rounded once to f32 and read as per-output (start, count, weights)
//     tables; taps are clamped to the RASTER, so a tile's footprint reaches into its neighbours. One launch per pass covers every tile
//     and band of a batch. The rule itself (GDAL's convolution resampler restated) is in DESIGN.md section 2.
#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "kernels.h"

namespace apds {

struct Mosaic {
    int device = 0;
    int rows = 0, cols = 0;
    float* data = nullptr;   // [3][rows][cols]
    std::mutex m;            // the min/max cache is the only state that changes after create
    bool mm_valid = false;
    double mm[6] = {0, 0, 0, 0, 0, 0};
};

// one tile of a batch: window origin, its x / y weight table (tap starts in a table are relative to the window origin), and the source
// rows [ylo, ylo + nr) its column taps reach
struct MosaicTile {
    int x0, y0, xt, yt, ylo, nr;
};

constexpr int kRowsPerBlock = 4;     // source rows a row-pass block filters with one read of the weights
constexpr int kSegCap = 2304;        // floats of one staged source-row segment: 8 * (256 + 6) + 2 = 2098 serves ratio 8 at 256 outputs a block
constexpr int kColsPerThread = 4;    // output rows a column-pass thread produces from one walk over the strip

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

namespace {

// L(0) = 1, L(x) = sin(pi x) sin(pi x / 3) / (pi^2 x^2 / 3) for 0 < |x| < 3, 0 otherwise
double lanczos3(double x) {
    if (x == 0.0) return 1.0;
    if (!(std::fabs(x) < 3.0)) return 0.0;
    const double a = M_PI * x;
    return std::sin(a) * std::sin(a / 3.0) / (a * a / 3.0);
}

int nearest_index(int i, int win, int n_out) {
    return (int)std::min<int64_t>((int64_t)((i + 0.5) * ((double)win / n_out)), (int64_t)win - 1);
}

// taps [first, last) of output i, clamped to the raster (n_src <= 0: no raster, the footprint as it is)
void lanczos_taps(int n_src, double offset, double ratio, double radius, int i, int* first, int* last, double* centre) {
    const double c = (i + 0.5) * ratio + offset;
    const double lo = std::floor(c - radius + 0.5), hi = c + radius + 0.5;
    *first = (int)(n_src > 0 ? std::max(lo, 0.0) : lo);
    *last = (int)(n_src > 0 ? std::min(hi, (double)n_src) : hi);   // (int) truncates, as the rule's cast does
    *centre = c;
}

// the Lanczos table of one axis: start / count / weights[max_taps] per output, and the widest footprint (start null: only that)
int lanczos_table(int n_src, double offset, double ratio, int n_out, int max_taps, int32_t* start, int32_t* count, float* weights) {
    const double sw = std::min(1.0, 1.0 / ratio), radius = 3.0 / sw;
    int need = 1;
    std::vector<double> w;
    for (int i = 0; i < n_out; i++) {
        int a, b;
        double c;
        lanczos_taps(n_src, offset, ratio, radius, i, &a, &b, &c);
        need = std::max(need, b - a);
        if (!start) continue;
        w.resize((size_t)std::max(b - a, 1));
        double sum = 0.0;
        for (int j = a; j < b; j++) {
            w[j - a] = lanczos3((j + 0.5 - c) * sw);
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
    const int need = resample == APDS_RESAMPLE_LANCZOS ? lanczos_table(n_src, offset, ratio, n_out, 0, nullptr, nullptr, nullptr) : 1;
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
    lanczos_table(n_src, offset, ratio, n_out, max_taps, start, count, weights);
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
        taps = lanczos_table(0, 0.0, ratio, n_out, 0, nullptr, nullptr, nullptr);   // the clamp only shortens a footprint
        in_start.resize((size_t)n_out);
        in_count.resize((size_t)n_out);
        in_weights.assign((size_t)n_out * taps, 0.0f);
        lanczos_table(0, 0.0, ratio, n_out, taps, in_start.data(), in_count.data(), in_weights.data());
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

void mosaic_check_window(const Mosaic* m, const int32_t* xy0, int n_tiles, int win_w, int win_h, int out_w, int out_h, int resample) {
    APDS_REQUIRE(m && xy0, APDS_ERR_BAD_ARG, "null argument");
    APDS_REQUIRE(n_tiles >= 1 && n_tiles <= 4096, APDS_ERR_BAD_ARG, "batch must hold 1 .. 4096 tiles");
    APDS_REQUIRE(win_w > 0 && win_h > 0 && out_w > 0 && out_h > 0, APDS_ERR_ASSERT, "empty window or output");
    APDS_REQUIRE(resample == APDS_RESAMPLE_NEAREST || resample == APDS_RESAMPLE_LANCZOS, APDS_ERR_BAD_ARG, "unknown resampling mode");
    for (int i = 0; i < n_tiles; i++) {
        const int64_t x0 = xy0[2 * i], y0 = xy0[2 * i + 1];
        APDS_REQUIRE(x0 >= 0 && y0 >= 0 && x0 + win_w <= m->cols && y0 + win_h <= m->rows, APDS_ERR_OUT_OF_RANGE, "window outside the raster");
    }
    APDS_REQUIRE((int64_t)win_w <= 64ll * out_w && (int64_t)win_h <= 64ll * out_h, APDS_ERR_BAD_ARG, "window / output above 64 (385 taps) is not served");
    APDS_REQUIRE(m->device == ctx().device, APDS_ERR_BAD_ARG, "the mosaic lives on another device than the calling thread's");
}

// The windows of n_tiles origins (xy0: x, y pairs) resampled to out_w x out_h, band-major on the device: out[band][tile][out_h][out_w].
// Asynchronous on s; the tables and the row-filtered strip live in the calling thread's workspace. The arguments have been checked.
void mosaic_window_device(const Mosaic* m, const int32_t* xy0, int n_tiles, int win_w, int win_h, int out_w, int out_h, int resample, float* out, hipStream_t s) {
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
                hipLaunchKernelGGL(mosaic_nearest_kernel, dim3(ceil_div(out_w, 256), std::min(out_h - y, 65535), 3 * n_tiles), block, 0, s, (const float*)m->data,
                                   m->rows, m->cols, dt, n_tiles, dxs, dys + y, out_w, out_h, out + (size_t)y * out_w);
                HIP_CHECK(hipGetLastError());
            }
        }
        HIP_CHECK(hipStreamSynchronize(s));   // the host tables are this call's locals
        return;
    }
    AxisTables X, Y;
    X.prepare(m->cols, win_w, out_w);
    Y.prepare(m->rows, win_h, out_h);
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
        hipLaunchKernelGGL(mosaic_lanczos_rows_kernel, dim3(ceil_div(out_w, oxb), ceil_div(nr_max, kRowsPerBlock), 3 * n_tiles), block, 0, s, (const float*)m->data, m->rows,
                           m->cols, dt, n_tiles, dxs, dxc, dxw, X.taps, out_w, oxb, nr_max, tmp);
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(mosaic_lanczos_cols_kernel, dim3(ceil_div(out_w, 256), ceil_div(out_h, kColsPerThread), 3 * n_tiles), block, 0, s, (const float*)tmp, dt, n_tiles,
                           dys, dyc, dyw, Y.taps, out_w, out_h, nr_max, out);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(s));   // the host tables are this call's locals
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

int apds_mosaic_window(void* mosaic, int x0, int y0, int win_w, int win_h, int out_w, int out_h, int resample, float* out3) {
    APDS_RANGE("apds_mosaic_window");
    return guarded([&] {
        APDS_REQUIRE(out3, APDS_ERR_BAD_ARG, "null output");
        const int32_t xy0[2] = {x0, y0};
        const Mosaic* m = static_cast<const Mosaic*>(mosaic);
        mosaic_check_window(m, xy0, 1, win_w, win_h, out_w, out_h, resample);
        ThreadCtx& c = ctx();
        c.ws_reset();
        hipStream_t s = c.stream;
        const size_t n = (size_t)3 * out_w * out_h;
        float* d = c.alloc_n<float>(n);
        mosaic_window_device(m, xy0, 1, win_w, win_h, out_w, out_h, resample, d, s);
        HIP_CHECK(hipMemcpyAsync(out3, d, n * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

}  // extern "C"
