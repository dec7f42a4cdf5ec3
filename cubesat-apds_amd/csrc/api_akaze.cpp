// csrc/api_akaze.cpp — C-ABI entry points of the extraction step (feature_extraction/src/lib.rs:61-92).
#include <cstdlib>
#include <cstring>

#include "akaze.h"
#include "kernels.h"

using namespace apds;

extern "C" {

// APDS_TILE_MASK_ALPHA: the alpha bytes of `n_img` packed BGRA images band_merger has just written are the detection mask - no buffer,
// no pass; APDS_TILE_MASK_NONE: none
static PixelMask tile_mask(int mask_mode, const uint8_t* bgra, int rows, int cols) {
    PixelMask m;
    if (mask_mode == APDS_TILE_MASK_ALPHA || mask_mode == APDS_TILE_MASK_ALPHA_SUPPORT) {
        m.base = bgra + 3;
        m.pix_stride = 4;
        m.row_stride = (size_t)cols * 4;
        m.img_stride = (size_t)rows * cols * 4;
        m.rows = rows;
        m.cols = cols;
    }
    return m;
}
static void check_mask_mode(int mask_mode) {
    APDS_REQUIRE(mask_mode == APDS_TILE_MASK_NONE || mask_mode == APDS_TILE_MASK_ALPHA || mask_mode == APDS_TILE_MASK_ALPHA_SUPPORT, APDS_ERR_BAD_ARG,
                 "unknown mask_mode");
}
// APDS_TILE_MASK_ALPHA_SUPPORT: the alpha mask reaches over the descriptor's support
static int tile_mask_support(int mask_mode) { return mask_mode == APDS_TILE_MASK_ALPHA_SUPPORT ? APDS_MASK_SUPPORT_DESCRIPTOR : 0; }
static void check_mask_support(int mask_support) { APDS_REQUIRE(mask_support >= 0, APDS_ERR_BAD_ARG, "mask_support must be >= 0"); }

// a mask plane of the caller's on the device (rows x cols bytes, any strides)
static PixelMask plane_mask(const void* mask_dev, size_t row_stride, size_t img_stride, int rows, int cols) {
    PixelMask m;
    if (mask_dev) {
        APDS_REQUIRE(row_stride >= (size_t)cols, APDS_ERR_ASSERT, "mask row stride smaller than a row");   // CV_Assert(mask.size() == image.size())
        m.base = static_cast<const uint8_t*>(mask_dev);
        m.row_stride = row_stride;
        m.img_stride = img_stride;
        m.rows = rows;
        m.cols = cols;
    }
    return m;
}

// bytes of a descriptor row on the device / in the host arrays the calls hand out: M-LDB 64 (one line) / 61 packed; float 256 / 256
static size_t device_row_bytes(int descriptor) { return descriptor == APDS_AKAZE_DESCRIPTOR_KAZE ? APDS_DESC_FLOAT_DIM * sizeof(float) : APDS_DESC_STRIDE; }
static size_t host_row_bytes(int descriptor) { return descriptor == APDS_AKAZE_DESCRIPTOR_KAZE ? APDS_DESC_FLOAT_DIM * sizeof(float) : APDS_DESC_BYTES; }

// device image -> host keypoints + 61-byte descriptors, or rows of 64 floats (malloc'ed, the caller frees them with apds_free)
static void extract_to_host(ThreadCtx& c, hipStream_t s, const uint8_t* dimg, int rows, int cols, int channels, size_t dstride, const PixelMask& pmask,
                            int mask_support, int max_points, apds_keypoint** kps, uint8_t** desc, int* n, int descriptor = APDS_AKAZE_DESCRIPTOR_MLDB) {
    // strict 3x3 maxima are never adjacent: at most ceil(w/2)*ceil(h/2) per level, and the cap is max_points
    const int capacity = max_points;
    const size_t row_dev = device_row_bytes(descriptor), row_host = host_row_bytes(descriptor);
    apds_keypoint* dk = c.alloc_n<apds_keypoint>(capacity);
    uint8_t* dd = c.alloc_n<uint8_t>((size_t)capacity * row_dev);
    const int K = akaze_extract_device(dimg, rows, cols, channels, dstride, pmask, mask_support, max_points, dk, dd, capacity, s, descriptor);
    apds_keypoint* hk = static_cast<apds_keypoint*>(std::malloc(std::max<size_t>(1, (size_t)K * sizeof(apds_keypoint))));
    uint8_t* hd = static_cast<uint8_t*>(std::malloc(std::max<size_t>(1, (size_t)K * row_host)));
    if (!hk || !hd) {
        std::free(hk);
        std::free(hd);
        throw std::bad_alloc();
    }
    try {
        if (K) {
            const uint8_t* rows_dev = dd;   // float rows are packed as they are
            if (descriptor == APDS_AKAZE_DESCRIPTOR_MLDB) {
                uint8_t* d61 = c.alloc_n<uint8_t>((size_t)K * APDS_DESC_BYTES);
                pack_desc61_device(dd, K, d61, s);
                rows_dev = d61;
            }
            HIP_CHECK(hipMemcpyAsync(hk, dk, (size_t)K * sizeof(apds_keypoint), hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(hd, rows_dev, (size_t)K * row_host, hipMemcpyDeviceToHost, s));
        }
        HIP_CHECK(hipStreamSynchronize(s));
    } catch (...) {
        std::free(hk);
        std::free(hd);
        throw;
    }
    *kps = hk;
    *desc = hd;
    *n = K;
}

static int akaze_extract_host(const uint8_t* img, int rows, int cols, int channels, size_t stride, const uint8_t* mask, size_t mask_stride, int mask_support,
                              int max_points, apds_keypoint** kps, uint8_t** desc, int* n, int* desc_bytes, int descriptor = APDS_AKAZE_DESCRIPTOR_MLDB) {
    return guarded([&] {
        APDS_REQUIRE(kps && desc && n && desc_bytes, APDS_ERR_BAD_ARG, "null output");
        check_mask_support(mask_support);
        *kps = nullptr;
        *desc = nullptr;
        *n = 0;
        *desc_bytes = descriptor == APDS_AKAZE_DESCRIPTOR_KAZE ? APDS_DESC_FLOAT_DIM : APDS_DESC_BYTES;   // (the float calls: floats per row)
        APDS_REQUIRE(img != nullptr && rows > 0 && cols > 0, APDS_ERR_ASSERT, "empty image");   // CV_Assert(!image.empty())
        APDS_REQUIRE(channels == 1 || channels == 3 || channels == 4, APDS_ERR_ASSERT, "image must have 1, 3 or 4 channels");
        APDS_REQUIRE(stride >= (size_t)cols * channels, APDS_ERR_ASSERT, "row stride smaller than a row");
        APDS_REQUIRE(!mask || mask_stride >= (size_t)cols, APDS_ERR_ASSERT, "mask row stride smaller than a row");   // CV_Assert(mask.size() == image.size())
        if (max_points <= 0) max_points = APDS_MAX_POINTS;
        ThreadCtx& c = ctx();
        c.ws_reset();
        hipStream_t s = c.stream;
        const size_t row_bytes = (size_t)cols * channels;
        const size_t dstride = (row_bytes + 3) & ~size_t(3);
        uint8_t* dimg = c.alloc_n<uint8_t>(dstride * rows);
        HIP_CHECK(hipMemcpy2DAsync(dimg, dstride, img, stride, row_bytes, rows, hipMemcpyHostToDevice, s));
        uint8_t* dmask = nullptr;
        if (mask) {
            dmask = c.alloc_n<uint8_t>((size_t)rows * cols);
            HIP_CHECK(hipMemcpy2DAsync(dmask, cols, mask, mask_stride, cols, rows, hipMemcpyHostToDevice, s));
        }
        extract_to_host(c, s, dimg, rows, cols, channels, dstride, plane_mask(dmask, cols, 0, rows, cols), mask_support, max_points, kps, desc, n, descriptor);
    });
}

int apds_akaze_extract(const uint8_t* img, int rows, int cols, int channels, size_t stride, int max_points, apds_keypoint** kps, uint8_t** desc,
                       int* n, int* desc_bytes) {
    APDS_RANGE("apds_akaze_extract");
    return akaze_extract_host(img, rows, cols, channels, stride, nullptr, 0, 0, max_points, kps, desc, n, desc_bytes);
}

// cv::Feature2D::detectAndCompute(img, mask, ..): the call above passes Mat::default() (feature_extraction/src/lib.rs:75-79)
int apds_akaze_extract_masked(const uint8_t* img, int rows, int cols, int channels, size_t stride, const uint8_t* mask, size_t mask_stride, int max_points,
                              apds_keypoint** kps, uint8_t** desc, int* n, int* desc_bytes) {
    APDS_RANGE("apds_akaze_extract_masked");
    return akaze_extract_host(img, rows, cols, channels, stride, mask, mask_stride, 0, max_points, kps, desc, n, desc_bytes);
}

// the mask consulted on the square of mask_support descriptor units around the keypoint (0: the call above)
int apds_akaze_extract_masked_support(const uint8_t* img, int rows, int cols, int channels, size_t stride, const uint8_t* mask, size_t mask_stride,
                                      int mask_support, int max_points, apds_keypoint** kps, uint8_t** desc, int* n, int* desc_bytes) {
    APDS_RANGE("apds_akaze_extract_masked_support");
    return akaze_extract_host(img, rows, cols, channels, stride, mask, mask_stride, mask_support, max_points, kps, desc, n, desc_bytes);
}

// One tile of the preprocessor in one call (preprocessor/src/main.rs:258-277): the three f32 band windows go up once, band_merger
// writes BGRA (geotiff_extractor mod.rs:346-378 fused with homographier raster_to_mat mod.rs:183-197) and AKAZE reads it on the device.
int apds_tile_extract_ex(const float* red, const float* green, const float* blue, int rows, int cols, size_t row_stride, const double* minmax6,
                         int max_points, int mask_mode, apds_keypoint** kps, uint8_t** desc, int* n, int* desc_bytes) {
    APDS_RANGE("apds_tile_extract");
    return guarded([&] {
        APDS_REQUIRE(kps && desc && n && desc_bytes, APDS_ERR_BAD_ARG, "null output");
        *kps = nullptr;
        *desc = nullptr;
        *n = 0;
        *desc_bytes = APDS_DESC_BYTES;
        APDS_REQUIRE(red && green && blue && minmax6, APDS_ERR_BAD_ARG, "null argument");
        check_mask_mode(mask_mode);
        APDS_REQUIRE(rows > 0 && cols > 0, APDS_ERR_ASSERT, "empty tile");
        APDS_REQUIRE(row_stride >= (size_t)cols, APDS_ERR_ASSERT, "row stride smaller than a row");
        if (max_points <= 0) max_points = APDS_MAX_POINTS;
        ThreadCtx& c = ctx();
        c.ws_reset();
        hipStream_t s = c.stream;
        const size_t px = (size_t)rows * cols;
        float* bands = c.alloc_n<float>(3 * px);
        const float* src[3] = {red, green, blue};
        for (int b = 0; b < 3; b++)
            HIP_CHECK(hipMemcpy2DAsync(bands + b * px, (size_t)cols * 4, src[b], row_stride * 4, (size_t)cols * 4, rows, hipMemcpyHostToDevice, s));
        uint8_t* dimg = c.alloc_n<uint8_t>(px * 4);
        band_merger_device(bands, bands + px, bands + 2 * px, px, minmax6, /*bgra=*/1, dimg, s);
        extract_to_host(c, s, dimg, rows, cols, 4, (size_t)cols * 4, tile_mask(mask_mode, dimg, rows, cols), tile_mask_support(mask_mode), max_points, kps, desc, n);
    });
}

int apds_tile_extract(const float* red, const float* green, const float* blue, int rows, int cols, size_t row_stride, const double* minmax6,
                      int max_points, apds_keypoint** kps, uint8_t** desc, int* n, int* desc_bytes) {
    return apds_tile_extract_ex(red, green, blue, rows, cols, row_stride, minmax6, max_points, APDS_TILE_MASK_NONE, kps, desc, n, desc_bytes);
}

// Test hook (tests/test_akaze_gpu.py): run the extraction and copy one intermediate plane of `level` to out_plane.
int apds_akaze_debug_plane(const uint8_t* img, int rows, int cols, int channels, size_t stride, int level, int which, void* out_plane) {
    AkazeDebugRequest& r = akaze_debug_request();
    r.armed = true;
    r.level = level;
    r.which = which;
    r.host_out = out_plane;
    apds_keypoint* k = nullptr;
    uint8_t* d = nullptr;
    int n = 0, nb = 0;
    const int rc = apds_akaze_extract(img, rows, cols, channels, stride, 0, &k, &d, &n, &nb);
    r.armed = false;
    apds_free(k);
    apds_free(d);
    return rc;
}

// Output rows per image of a batched extraction: the rule of the single-image call (capacity = max_points) unless the image cannot hold
// that many. Strict 3x3 maxima are never adjacent, so a level of w x h pixels has at most ceil(w/2) * ceil(h/2) of them; summed over every
// level of every octave (four levels per octave; octaves as the detector builds them: halved until width < 80 or height < 40). A bound
// below the true ceiling would fail a whole batch on a dense image that extracts fine alone.
static int batch_capacity(int rows, int cols, int max_points) {
    long long bound = 0;
    for (int o = 0, w = cols, h = rows; o < 4 && (o == 0 || (w >= 80 && h >= 40)); o++, w >>= 1, h >>= 1)
        bound += 4LL * ((w + 1) / 2) * ((h + 1) / 2);
    return (int)std::min<long long>(max_points, std::max<long long>(bound, 64));
}

// device results of a batch (capacity rows per image) -> malloc'ed host arrays holding the images' rows back to back
static void batch_results_to_host(ThreadCtx& c, hipStream_t s, const apds_keypoint* dk, const uint8_t* dd, int capacity, int n_images, const int* counts,
                                  apds_keypoint** kps, uint8_t** desc, int descriptor = APDS_AKAZE_DESCRIPTOR_MLDB) {
    size_t total = 0;
    for (int i = 0; i < n_images; i++) total += (size_t)counts[i];
    const size_t row_dev = device_row_bytes(descriptor), row_host = host_row_bytes(descriptor);
    apds_keypoint* hk = static_cast<apds_keypoint*>(std::malloc(std::max<size_t>(1, total * sizeof(apds_keypoint))));
    uint8_t* hd = static_cast<uint8_t*>(std::malloc(std::max<size_t>(1, total * row_host)));
    if (!hk || !hd) {
        std::free(hk);
        std::free(hd);
        throw std::bad_alloc();
    }
    try {
        const bool pack = descriptor == APDS_AKAZE_DESCRIPTOR_MLDB;   // float rows are packed as they are: straight from the images' blocks
        uint8_t* d61 = pack ? c.alloc_n<uint8_t>(std::max<size_t>(1, total * APDS_DESC_BYTES)) : nullptr;
        size_t off = 0;
        for (int i = 0; i < n_images; i++) {
            const int K = counts[i];
            if (!K) continue;
            if (pack) pack_desc61_device(dd + (size_t)i * capacity * row_dev, K, d61 + off * APDS_DESC_BYTES, s);
            else HIP_CHECK(hipMemcpyAsync(hd + off * row_host, dd + (size_t)i * capacity * row_dev, (size_t)K * row_host, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(hk + off, dk + (size_t)i * capacity, (size_t)K * sizeof(apds_keypoint), hipMemcpyDeviceToHost, s));
            off += (size_t)K;
        }
        if (total && pack) HIP_CHECK(hipMemcpyAsync(hd, d61, total * APDS_DESC_BYTES, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    } catch (...) {
        std::free(hk);
        std::free(hd);
        throw;
    }
    *kps = hk;
    *desc = hd;
}

// B tiles of the preprocessor in one call (preprocessor/src/main.rs:227-245 spawns one task per tile; 258-277 is the per-tile chain): the
// band windows of all tiles go up (3 B strided copies), ONE band_merger pass writes the B BGRA images and the batched extraction runs
// every kernel once for all of them. red / green / blue: n_tiles pointers each (windows of one size, row_stride elements between rows).
int apds_tile_extract_batch_ex(const float* const* red, const float* const* green, const float* const* blue, int n_tiles, int rows, int cols, size_t row_stride,
                               const double* minmax6, int max_points, int mask_mode, apds_keypoint** kps, uint8_t** desc, int* counts, int* desc_bytes) {
    APDS_RANGE("apds_tile_extract_batch");
    return guarded([&] {
        APDS_REQUIRE(kps && desc && counts && desc_bytes, APDS_ERR_BAD_ARG, "null output");
        *kps = nullptr;
        *desc = nullptr;
        *desc_bytes = APDS_DESC_BYTES;
        APDS_REQUIRE(red && green && blue && minmax6, APDS_ERR_BAD_ARG, "null argument");
        check_mask_mode(mask_mode);
        APDS_REQUIRE(n_tiles >= 1 && n_tiles <= 4096, APDS_ERR_BAD_ARG, "batch must hold 1 .. 4096 tiles");
        APDS_REQUIRE(rows > 0 && cols > 0, APDS_ERR_ASSERT, "empty tile");
        APDS_REQUIRE(row_stride >= (size_t)cols, APDS_ERR_ASSERT, "row stride smaller than a row");
        if (max_points <= 0) max_points = APDS_MAX_POINTS;
        for (int i = 0; i < n_tiles; i++) counts[i] = 0;
        ThreadCtx& c = ctx();
        c.ws_reset();
        hipStream_t s = c.stream;
        const size_t px = (size_t)rows * cols, all = px * n_tiles;
        float* bands = c.alloc_n<float>(3 * all);   // band-major: all tiles' red, then green, then blue
        const float* const* src[3] = {red, green, blue};
        for (int b = 0; b < 3; b++)
            for (int i = 0; i < n_tiles; i++) {
                APDS_REQUIRE(src[b][i] != nullptr, APDS_ERR_BAD_ARG, "null band window");
                HIP_CHECK(hipMemcpy2DAsync(bands + b * all + i * px, (size_t)cols * 4, src[b][i], row_stride * 4, (size_t)cols * 4, rows, hipMemcpyHostToDevice, s));
            }
        uint8_t* dimg = c.alloc_n<uint8_t>(all * 4);
        band_merger_device(bands, bands + all, bands + 2 * all, all, minmax6, /*bgra=*/1, dimg, s);
        const int capacity = batch_capacity(rows, cols, max_points);
        apds_keypoint* dk = c.alloc_n<apds_keypoint>((size_t)capacity * n_tiles);
        uint8_t* dd = c.alloc_n<uint8_t>((size_t)capacity * 64 * n_tiles);
        akaze_extract_batch_device(dimg, n_tiles, px * 4, rows, cols, 4, (size_t)cols * 4, tile_mask(mask_mode, dimg, rows, cols),
                                   tile_mask_support(mask_mode), max_points, dk, dd, capacity, counts, s);
        batch_results_to_host(c, s, dk, dd, capacity, n_tiles, counts, kps, desc);
    });
}

int apds_tile_extract_batch(const float* const* red, const float* const* green, const float* const* blue, int n_tiles, int rows, int cols, size_t row_stride,
                            const double* minmax6, int max_points, apds_keypoint** kps, uint8_t** desc, int* counts, int* desc_bytes) {
    return apds_tile_extract_batch_ex(red, green, blue, n_tiles, rows, cols, row_stride, minmax6, max_points, APDS_TILE_MASK_NONE, kps, desc, counts, desc_bytes);
}

// apds_tile_extract on a window of the resident mosaic (geotiff_extractor mod.rs:332-343 read_as(.., Lanczos) in front of the chain): the
// resampled bands, the BGRA image and the extraction all stay on the device.
int apds_mosaic_tile_extract_ex(void* mosaic, int x0, int y0, int win_w, int win_h, int out_w, int out_h, int resample, const double* minmax6, int max_points,
                                int mask_mode, apds_keypoint** kps, uint8_t** desc, int* n, int* desc_bytes) {
    APDS_RANGE("apds_mosaic_tile_extract");
    return guarded([&] {
        APDS_REQUIRE(kps && desc && n && desc_bytes, APDS_ERR_BAD_ARG, "null output");
        *kps = nullptr;
        *desc = nullptr;
        *n = 0;
        *desc_bytes = APDS_DESC_BYTES;
        check_mask_mode(mask_mode);
        Mosaic* m = static_cast<Mosaic*>(mosaic);
        const int32_t xy0[2] = {x0, y0};
        mosaic_check_window(m, 0, xy0, 1, win_w, win_h, out_w, out_h, resample);
        if (max_points <= 0) max_points = APDS_MAX_POINTS;
        double own[6];
        if (!minmax6) {
            mosaic_min_max(m, own);
            minmax6 = own;
        }
        ThreadCtx& c = ctx();
        c.ws_reset();
        hipStream_t s = c.stream;
        const size_t px = (size_t)out_w * out_h;
        float* bands = c.alloc_n<float>(3 * px);
        uint8_t* dimg = c.alloc_n<uint8_t>(px * 4);
        mosaic_read_device(m, xy0, 1, win_w, win_h, out_w, out_h, resample, bands, s);
        band_merger_device(bands, bands + px, bands + 2 * px, px, minmax6, /*bgra=*/1, dimg, s);
        extract_to_host(c, s, dimg, out_h, out_w, 4, (size_t)out_w * 4, tile_mask(mask_mode, dimg, out_h, out_w), tile_mask_support(mask_mode), max_points, kps, desc, n);
    });
}

int apds_mosaic_tile_extract(void* mosaic, int x0, int y0, int win_w, int win_h, int out_w, int out_h, int resample, const double* minmax6, int max_points,
                             apds_keypoint** kps, uint8_t** desc, int* n, int* desc_bytes) {
    return apds_mosaic_tile_extract_ex(mosaic, x0, y0, win_w, win_h, out_w, out_h, resample, minmax6, max_points, APDS_TILE_MASK_NONE, kps, desc, n, desc_bytes);
}

// The front of the two calls below: the checks of the batch call, then window read -> band_merger -> batched extraction of n_tiles windows
// of the resident mosaic on the calling thread's stream, in its (reset) workspace. counts[] is final on return; the rows stay on the device
// (tile i at i * capacity rows; 64-byte rows, or rows of 64 floats with APDS_AKAZE_DESCRIPTOR_KAZE) with the descriptor kernels still queued on `s`.
struct MosaicBatchRows {
    apds_keypoint* kps;
    uint8_t* desc64;
    int capacity;
    hipStream_t s;
};
static MosaicBatchRows mosaic_tiles_extract_device(ThreadCtx& c, Mosaic* m, const int32_t* xy0, int n_tiles, int win_w, int win_h, int out_w, int out_h, int resample,
                                                   const double* minmax6, int max_points, int mask_mode, int* counts,
                                                   int descriptor = APDS_AKAZE_DESCRIPTOR_MLDB) {
    check_mask_mode(mask_mode);
    mosaic_check_window(m, 0, xy0, n_tiles, win_w, win_h, out_w, out_h, resample);
    if (max_points <= 0) max_points = APDS_MAX_POINTS;
    for (int i = 0; i < n_tiles; i++) counts[i] = 0;
    double own[6];
    if (!minmax6) {
        mosaic_min_max(m, own);
        minmax6 = own;
    }
    c.ws_reset();
    hipStream_t s = c.stream;
    const size_t px = (size_t)out_w * out_h, all = px * n_tiles;
    float* bands = c.alloc_n<float>(3 * all);   // band-major: all tiles' red, then green, then blue
    uint8_t* dimg = c.alloc_n<uint8_t>(all * 4);
    const int capacity = batch_capacity(out_h, out_w, max_points);
    apds_keypoint* dk = c.alloc_n<apds_keypoint>((size_t)capacity * n_tiles);
    uint8_t* dd = c.alloc_n<uint8_t>((size_t)capacity * device_row_bytes(descriptor) * n_tiles);
    mosaic_read_device(m, xy0, n_tiles, win_w, win_h, out_w, out_h, resample, bands, s);
    band_merger_device(bands, bands + all, bands + 2 * all, all, minmax6, /*bgra=*/1, dimg, s);
    akaze_extract_batch_device(dimg, n_tiles, px * 4, out_h, out_w, 4, (size_t)out_w * 4, tile_mask(mask_mode, dimg, out_h, out_w), tile_mask_support(mask_mode),
                               max_points, dk, dd, capacity, counts, s, descriptor);
    return MosaicBatchRows{dk, dd, capacity, s};
}

// apds_tile_extract_batch on n_tiles windows of the resident mosaic: ONE resampling launch per pass, ONE band_merger pass and ONE batched
// extraction serve all tiles.
int apds_mosaic_tile_extract_batch_ex(void* mosaic, const int32_t* xy0, int n_tiles, int win_w, int win_h, int out_w, int out_h, int resample,
                                      const double* minmax6, int max_points, int mask_mode, apds_keypoint** kps, uint8_t** desc, int* counts, int* desc_bytes) {
    APDS_RANGE("apds_mosaic_tile_extract_batch");
    return guarded([&] {
        APDS_REQUIRE(kps && desc && counts && desc_bytes, APDS_ERR_BAD_ARG, "null output");
        *kps = nullptr;
        *desc = nullptr;
        *desc_bytes = APDS_DESC_BYTES;
        ThreadCtx& c = ctx();
        const MosaicBatchRows r = mosaic_tiles_extract_device(c, static_cast<Mosaic*>(mosaic), xy0, n_tiles, win_w, win_h, out_w, out_h, resample, minmax6, max_points,
                                                              mask_mode, counts);
        batch_results_to_host(c, r.s, r.kps, r.desc64, r.capacity, n_tiles, counts, kps, desc);
    });
}

// The DB build of a group of tiles in one call (preprocessor/src/main.rs:197-327): the call above up to the extraction, then the rows go
// from the extraction's buffers into the keypoint table on the same stream. Only counts[] reaches the host.
int apds_mosaic_tiles_to_db(void* mosaic, void* db, const int32_t* xy0, int n_tiles, int win_w, int win_h, int out_w, int out_h, int resample,
                            const double* minmax6, int max_points, int mask_mode, int first_image_id, int level_of_detail, const uint32_t* columns_rows,
                            int* counts) {
    APDS_RANGE("apds_mosaic_tiles_to_db");
    return guarded([&] {
        APDS_REQUIRE(mosaic && db && counts && columns_rows, APDS_ERR_BAD_ARG, "null argument");
        APDS_REQUIRE(level_of_detail >= 0 && level_of_detail < 31, APDS_ERR_BAD_ARG, "bad level of detail");
        Mosaic* m = static_cast<Mosaic*>(mosaic);
        APDS_REQUIRE(mosaic_device(m) == table_device(db), APDS_ERR_BAD_ARG, "the mosaic and the keypoint table live on different devices");
        ThreadCtx& c = ctx();
        // (the rows are of the table's kind: a float table gets the M-SURF extraction of the same keypoints)
        const MosaicBatchRows r = mosaic_tiles_extract_device(c, m, xy0, n_tiles, win_w, win_h, out_w, out_h, resample, minmax6, max_points, mask_mode, counts,
                                                              table_descriptor(db));
        table_insert_batch_device(db, r.kps, r.desc64, n_tiles, r.capacity, counts, first_image_id, level_of_detail, columns_rows, (uint64_t)out_w, (uint64_t)out_h,
                                  r.s);
    });
}

int apds_mosaic_tile_extract_batch(void* mosaic, const int32_t* xy0, int n_tiles, int win_w, int win_h, int out_w, int out_h, int resample, const double* minmax6,
                                   int max_points, apds_keypoint** kps, uint8_t** desc, int* counts, int* desc_bytes) {
    return apds_mosaic_tile_extract_batch_ex(mosaic, xy0, n_tiles, win_w, win_h, out_w, out_h, resample, minmax6, max_points, APDS_TILE_MASK_NONE, kps, desc, counts,
                                             desc_bytes);
}

// n_images equal-sized host images in one call: one upload, one batched extraction (every kernel's grid covers all images), one download.
// Outputs: concatenated keypoints / 61-byte descriptors (image 0's rows first), counts[i] rows per image.
static int akaze_extract_batch_host(const uint8_t* imgs, int n_images, size_t image_stride, int rows, int cols, int channels, size_t stride,
                                    const uint8_t* const* masks, size_t mask_stride, int mask_support, int max_points, apds_keypoint** kps, uint8_t** desc,
                                    int* counts, int* desc_bytes, int descriptor = APDS_AKAZE_DESCRIPTOR_MLDB) {
    return guarded([&] {
        APDS_REQUIRE(kps && desc && counts && desc_bytes, APDS_ERR_BAD_ARG, "null output");
        check_mask_support(mask_support);
        *kps = nullptr;
        *desc = nullptr;
        *desc_bytes = descriptor == APDS_AKAZE_DESCRIPTOR_KAZE ? APDS_DESC_FLOAT_DIM : APDS_DESC_BYTES;
        APDS_REQUIRE(imgs != nullptr && rows > 0 && cols > 0, APDS_ERR_ASSERT, "empty image");
        APDS_REQUIRE(n_images >= 1 && n_images <= 4096, APDS_ERR_BAD_ARG, "batch must hold 1 .. 4096 images");
        APDS_REQUIRE(channels == 1 || channels == 3 || channels == 4, APDS_ERR_ASSERT, "image must have 1, 3 or 4 channels");
        APDS_REQUIRE(stride >= (size_t)cols * channels && image_stride >= stride * rows, APDS_ERR_ASSERT, "strides smaller than a row / an image");
        if (max_points <= 0) max_points = APDS_MAX_POINTS;
        for (int i = 0; i < n_images; i++) counts[i] = 0;
        ThreadCtx& c = ctx();
        c.ws_reset();
        hipStream_t s = c.stream;
        const size_t row_bytes = (size_t)cols * channels;
        const size_t dstride = (row_bytes + 3) & ~size_t(3), dimg_bytes = dstride * rows;
        uint8_t* dimg = c.alloc_n<uint8_t>(dimg_bytes * n_images);
        if (stride == dstride && image_stride == dimg_bytes) {
            HIP_CHECK(hipMemcpyAsync(dimg, imgs, dimg_bytes * n_images, hipMemcpyHostToDevice, s));
        } else {
            for (int i = 0; i < n_images; i++)
                HIP_CHECK(hipMemcpy2DAsync(dimg + i * dimg_bytes, dstride, imgs + i * image_stride, stride, row_bytes, rows, hipMemcpyHostToDevice, s));
        }
        const int capacity = batch_capacity(rows, cols, max_points);
        apds_keypoint* dk = c.alloc_n<apds_keypoint>((size_t)capacity * n_images);
        uint8_t* dd = c.alloc_n<uint8_t>((size_t)capacity * device_row_bytes(descriptor) * n_images);
        // the masks go into one device buffer, a plane per image; an image without one gets all ones
        uint8_t* dmask = nullptr;
        const size_t mpx = (size_t)rows * cols;
        bool any = false;
        for (int i = 0; masks && i < n_images; i++) any |= masks[i] != nullptr;
        if (any) {
            APDS_REQUIRE(mask_stride >= (size_t)cols, APDS_ERR_ASSERT, "mask row stride smaller than a row");   // CV_Assert(mask.size() == image.size())
            dmask = c.alloc_n<uint8_t>(mpx * n_images);
            for (int i = 0; i < n_images; i++) {
                if (masks[i]) HIP_CHECK(hipMemcpy2DAsync(dmask + i * mpx, cols, masks[i], mask_stride, cols, rows, hipMemcpyHostToDevice, s));
                else HIP_CHECK(hipMemsetAsync(dmask + i * mpx, 0xFF, mpx, s));
            }
        }
        akaze_extract_batch_device(dimg, n_images, dimg_bytes, rows, cols, channels, dstride, plane_mask(dmask, cols, mpx, rows, cols), mask_support, max_points, dk, dd,
                                   capacity, counts, s, descriptor);
        batch_results_to_host(c, s, dk, dd, capacity, n_images, counts, kps, desc, descriptor);
    });
}

int apds_akaze_extract_batch(const uint8_t* imgs, int n_images, size_t image_stride, int rows, int cols, int channels, size_t stride, int max_points,
                             apds_keypoint** kps, uint8_t** desc, int* counts, int* desc_bytes) {
    APDS_RANGE("apds_akaze_extract_batch");
    return akaze_extract_batch_host(imgs, n_images, image_stride, rows, cols, channels, stride, nullptr, 0, 0, max_points, kps, desc, counts, desc_bytes);
}

int apds_akaze_extract_batch_masked(const uint8_t* imgs, int n_images, size_t image_stride, int rows, int cols, int channels, size_t stride,
                                    const uint8_t* const* masks, size_t mask_stride, int max_points, apds_keypoint** kps, uint8_t** desc, int* counts,
                                    int* desc_bytes) {
    APDS_RANGE("apds_akaze_extract_batch_masked");
    return akaze_extract_batch_host(imgs, n_images, image_stride, rows, cols, channels, stride, masks, mask_stride, 0, max_points, kps, desc, counts, desc_bytes);
}

int apds_akaze_extract_batch_masked_support(const uint8_t* imgs, int n_images, size_t image_stride, int rows, int cols, int channels, size_t stride,
                                            const uint8_t* const* masks, size_t mask_stride, int mask_support, int max_points, apds_keypoint** kps, uint8_t** desc,
                                            int* counts, int* desc_bytes) {
    APDS_RANGE("apds_akaze_extract_batch_masked_support");
    return akaze_extract_batch_host(imgs, n_images, image_stride, rows, cols, channels, stride, masks, mask_stride, mask_support, max_points, kps, desc, counts,
                                    desc_bytes);
}

int apds_dev_akaze_extract_batch_masked_support(const void* imgs, int n_images, size_t image_stride, int rows, int cols, int channels, size_t stride,
                                                const void* mask_dev, size_t mask_stride, size_t mask_image_stride, int mask_support, int max_points, void* kps,
                                                void* desc64, int capacity, int* counts, void* stream) {
    APDS_RANGE("apds_dev_akaze_extract_batch");
    return guarded([&] {
        APDS_REQUIRE(counts && kps && desc64, APDS_ERR_BAD_ARG, "null output");
        check_mask_support(mask_support);
        ctx().ws_reset(pick_stream(stream));
        akaze_extract_batch_device(imgs, n_images, image_stride, rows, cols, channels, stride, plane_mask(mask_dev, mask_stride, mask_image_stride, rows, cols),
                                   mask_support, max_points, static_cast<apds_keypoint*>(kps), static_cast<uint8_t*>(desc64), capacity, counts,
                                   pick_stream(stream));
    });
}

int apds_dev_akaze_extract_batch_masked(const void* imgs, int n_images, size_t image_stride, int rows, int cols, int channels, size_t stride, const void* mask_dev,
                                        size_t mask_stride, size_t mask_image_stride, int max_points, void* kps, void* desc64, int capacity, int* counts,
                                        void* stream) {
    return apds_dev_akaze_extract_batch_masked_support(imgs, n_images, image_stride, rows, cols, channels, stride, mask_dev, mask_stride, mask_image_stride, 0,
                                                       max_points, kps, desc64, capacity, counts, stream);
}

int apds_dev_akaze_extract_batch(const void* imgs, int n_images, size_t image_stride, int rows, int cols, int channels, size_t stride, int max_points,
                                 void* kps, void* desc64, int capacity, int* counts, void* stream) {
    return apds_dev_akaze_extract_batch_masked(imgs, n_images, image_stride, rows, cols, channels, stride, nullptr, 0, 0, max_points, kps, desc64, capacity, counts,
                                               stream);
}

int apds_dev_akaze_extract_masked_support(const void* img, int rows, int cols, int channels, size_t stride, const void* mask_dev, size_t mask_stride,
                                          int mask_support, int max_points, void* kps, void* desc64, int capacity, int* n, void* stream) {
    APDS_RANGE("apds_dev_akaze_extract");
    return guarded([&] {
        APDS_REQUIRE(n && kps && desc64, APDS_ERR_BAD_ARG, "null output");
        check_mask_support(mask_support);
        ctx().ws_reset(pick_stream(stream));
        *n = akaze_extract_device(img, rows, cols, channels, stride, plane_mask(mask_dev, mask_stride, 0, rows, cols), mask_support, max_points,
                                  static_cast<apds_keypoint*>(kps), static_cast<uint8_t*>(desc64), capacity, pick_stream(stream));
    });
}

int apds_dev_akaze_extract_masked(const void* img, int rows, int cols, int channels, size_t stride, const void* mask_dev, size_t mask_stride, int max_points,
                                  void* kps, void* desc64, int capacity, int* n, void* stream) {
    return apds_dev_akaze_extract_masked_support(img, rows, cols, channels, stride, mask_dev, mask_stride, 0, max_points, kps, desc64, capacity, n, stream);
}

// ---- AKAZE's float descriptor (APDS_AKAZE_DESCRIPTOR_KAZE: akaze_describe_msurf.hip); not in the reference, the producer of the L2 matcher's input
int apds_akaze_extract_float(const uint8_t* img, int rows, int cols, int channels, size_t stride, const uint8_t* mask, size_t mask_stride, int mask_support,
                             int max_points, apds_keypoint** kps, float** desc, int* n, int* desc_dim) {
    APDS_RANGE("apds_akaze_extract_float");
    return akaze_extract_host(img, rows, cols, channels, stride, mask, mask_stride, mask_support, max_points, kps, reinterpret_cast<uint8_t**>(desc), n, desc_dim,
                              APDS_AKAZE_DESCRIPTOR_KAZE);
}

int apds_akaze_extract_float_batch(const uint8_t* imgs, int n_images, size_t image_stride, int rows, int cols, int channels, size_t stride,
                                   const uint8_t* const* masks, size_t mask_stride, int mask_support, int max_points, apds_keypoint** kps, float** desc, int* counts,
                                   int* desc_dim) {
    APDS_RANGE("apds_akaze_extract_float_batch");
    return akaze_extract_batch_host(imgs, n_images, image_stride, rows, cols, channels, stride, masks, mask_stride, mask_support, max_points, kps,
                                    reinterpret_cast<uint8_t**>(desc), counts, desc_dim, APDS_AKAZE_DESCRIPTOR_KAZE);
}

int apds_dev_akaze_extract_float(const void* img, int rows, int cols, int channels, size_t stride, const void* mask_dev, size_t mask_stride, int mask_support,
                                 int max_points, void* kps, void* desc_f32, int capacity, int* n, void* stream) {
    APDS_RANGE("apds_dev_akaze_extract_float");
    return guarded([&] {
        APDS_REQUIRE(n && kps && desc_f32, APDS_ERR_BAD_ARG, "null output");
        check_mask_support(mask_support);
        ctx().ws_reset(pick_stream(stream));
        *n = akaze_extract_device(img, rows, cols, channels, stride, plane_mask(mask_dev, mask_stride, 0, rows, cols), mask_support, max_points,
                                  static_cast<apds_keypoint*>(kps), static_cast<uint8_t*>(desc_f32), capacity, pick_stream(stream), APDS_AKAZE_DESCRIPTOR_KAZE);
    });
}

int apds_dev_akaze_extract_float_batch(const void* imgs, int n_images, size_t image_stride, int rows, int cols, int channels, size_t stride, const void* mask_dev,
                                       size_t mask_stride, size_t mask_image_stride, int mask_support, int max_points, void* kps, void* desc_f32, int capacity,
                                       int* counts, void* stream) {
    APDS_RANGE("apds_dev_akaze_extract_float_batch");
    return guarded([&] {
        APDS_REQUIRE(counts && kps && desc_f32, APDS_ERR_BAD_ARG, "null output");
        check_mask_support(mask_support);
        ctx().ws_reset(pick_stream(stream));
        akaze_extract_batch_device(imgs, n_images, image_stride, rows, cols, channels, stride, plane_mask(mask_dev, mask_stride, mask_image_stride, rows, cols),
                                   mask_support, max_points, static_cast<apds_keypoint*>(kps), static_cast<uint8_t*>(desc_f32), capacity, counts,
                                   pick_stream(stream), APDS_AKAZE_DESCRIPTOR_KAZE);
    });
}

// the float describe stage alone on one plane of the caller's (the hook the kernel's tests stand on)
int apds_dev_akaze_describe_float(const void* lxy_dev, int w, int h, const void* kps_dev, int n, void* desc_f32_dev, void* stream) {
    APDS_RANGE("apds_dev_akaze_describe_float");
    return guarded([&] {
        APDS_REQUIRE(n >= 0, APDS_ERR_BAD_ARG, "negative keypoint count");
        if (n == 0) return;
        APDS_REQUIRE(lxy_dev && kps_dev && desc_f32_dev, APDS_ERR_BAD_ARG, "null argument");
        APDS_REQUIRE(w >= 1 && h >= 1 && w < 65536 && h < 65536, APDS_ERR_ASSERT, "plane sides must be 1 .. 65535");
        msurf_describe_plane_device(static_cast<const float2*>(lxy_dev), w, h, static_cast<const apds_keypoint*>(kps_dev), n, static_cast<float*>(desc_f32_dev),
                                    pick_stream(stream));
    });
}

// The zero-count summed-area table of a device mask on its own (what the mask support builds in its workspace): out[y][x], (rows + 1) x
// (cols + 1) u32, = the zero bytes in rows < y and columns < x.
int apds_dev_mask_zero_sat(const void* mask_dev, int rows, int cols, size_t row_stride, size_t pix_stride, void* out_u32_dev, void* stream) {
    APDS_RANGE("apds_dev_mask_zero_sat");
    return guarded([&] {
        APDS_REQUIRE(mask_dev && out_u32_dev, APDS_ERR_BAD_ARG, "null argument");
        PixelMask m;
        m.base = static_cast<const uint8_t*>(mask_dev);
        m.row_stride = row_stride;
        m.pix_stride = pix_stride;
        m.rows = rows;
        m.cols = cols;
        mask_zero_sat_device(m, 1, static_cast<uint32_t*>(out_u32_dev), 0, pick_stream(stream));
    });
}

int apds_dev_akaze_extract(const void* img, int rows, int cols, int channels, size_t stride, int max_points, void* kps, void* desc64, int capacity,
                           int* n, void* stream) {
    return apds_dev_akaze_extract_masked(img, rows, cols, channels, stride, nullptr, 0, max_points, kps, desc64, capacity, n, stream);
}

}  // extern "C"
