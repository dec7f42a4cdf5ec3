/*
 * include/apds.h — C ABI of libapds_hip.so, the MI355X (gfx950) implementation of the cubesat-APDS
 * hot path: AKAZE feature extraction -> Hamming brute-force match -> RANSAC homography.
 *
 * Every entry point replaces one public item of the reference's Rust crates `feature_extraction`
 * and `homographier` (cited per function as /root/reference/<file>:<line>). The Rust shim that keeps
 * the crates' signatures and forwards here is in INTEGRATION.md / rust_shim/.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ / torch types cross this boundary;
 *   - return 0 on success, a negative OpenCV-style status otherwise (the reference surfaces
 *     opencv::Error{code,..}): APDS_ERR_* below; text via apds_last_error() (thread local);
 *   - inputs are borrowed for the duration of the call; variable-length outputs are allocated by
 *     the library and released with apds_free(); fixed-size outputs are caller allocated;
 *   - every function is re-entrant and may be called concurrently from many host threads (the
 *     reference calls extraction from a rayon pool with no lock: preprocessor/src/main.rs:227-245,277);
 *     each host thread gets its own HIP stream and device workspace;
 *   - there is NO CPU fallback: without a usable HIP device every compute call fails with
 *     APDS_ERR_NO_DEVICE.
 *
 * The "_dev" functions are the same operations on buffers already resident in HBM (device
 * pointers + an optional hipStream_t passed as void*); they are what bench.py times and what the
 * multi-GPU sharded matcher is built from.
 */
#ifndef APDS_H
#define APDS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APDS_OK 0
#define APDS_ERR_INTERNAL (-2)      /* cv::Error::StsError  (HIP runtime failure, unsupported method) */
#define APDS_ERR_NOMEM (-4)         /* cv::Error::StsNoMem */
#define APDS_ERR_BAD_ARG (-5)       /* cv::Error::StsBadArg */
#define APDS_ERR_NO_DEVICE (-216)   /* cv::Error::GpuNotSupported: no HIP device / kernels not loadable */
#define APDS_ERR_OUT_OF_RANGE (-211)/* cv::Error::StsOutOfRange */
#define APDS_ERR_ASSERT (-215)      /* cv::Error::StsAssert (bad shapes, k < 1, too few points) */
#define APDS_ERR_NOT_IMPLEMENTED (-213) /* cv::Error::StsNotImplemented (a method of the reference surface that is not built) */
#define APDS_ERR_EMPTY (-1000)      /* no model found: the shim maps it to MatError::Empty (mod.rs:114-119,258) */

/* feature_extraction/src/lib.rs:12-13  MAX_POINTS_SHIFT / MAX_POINTS (twin: feature_database/src/keypointdb.rs:12) */
#define APDS_MAX_POINTS_SHIFT 18
#define APDS_MAX_POINTS ((1 << APDS_MAX_POINTS_SHIFT) - 1)
#define APDS_DESC_BYTES 61          /* 486-bit M-LDB */
#define APDS_DESC_STRIDE 64         /* device row pitch (one 64-byte line per descriptor) */

/* cv::KeyPoint, 28 bytes (fields read back by to_db_type, lib.rs:34-58) */
typedef struct apds_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} apds_keypoint;

/* cv::DMatch, 16 bytes */
typedef struct apds_dmatch {
    int32_t query_idx, train_idx, img_idx;
    float distance;
} apds_dmatch;

/* homographier/src/homographier/mod.rs:25-31  enum HomographyMethod */
enum { APDS_HOMOGRAPHY_DEFAULT = 0, APDS_HOMOGRAPHY_LMEDS = 4, APDS_HOMOGRAPHY_RANSAC = 8, APDS_HOMOGRAPHY_RHO = 16 };

/* ---- library ------------------------------------------------------------------------------ */
const char* apds_last_error(void);
void apds_free(void* p);
int apds_device_count(void);
int apds_set_device(int ordinal);             /* device used by the calling thread (default 0) */
const char* apds_build_info(void);            /* "gfx950 ..." */

/* ---- feature_extraction ------------------------------------------------------------------- */

/* lib.rs:61-92  akaze_keypoint_descriptor_extraction_def(img:&Mat, max_points:Option<i32>) -> ExtractedKeyPoint
 * img: rows x cols x channels u8 (channels 1 gray, 3 BGR, 4 BGRA), row pitch stride_bytes.
 * max_points <= 0 means None (-> APDS_MAX_POINTS). Outputs: *kps (n x 28 B), *desc (n x 61 B, rows packed),
 * both owned by the caller afterwards (apds_free). */
int apds_akaze_extract(const uint8_t* img, int rows, int cols, int channels, size_t stride_bytes, int max_points,
                       apds_keypoint** kps, uint8_t** desc, int* n, int* desc_bytes);
/* The same for n_images images of ONE size in one call (image i starts image_stride_bytes after image i-1): the batch goes through every
 * kernel's grid together, which is what makes small tiles cheap (a single small tile is launch-latency-bound). This is how a caller
 * that extracts one tile per task (preprocessor/src/main.rs:227-245,277) should hand its tiles over. Per-image results are exactly those
 * of apds_akaze_extract. Outputs: *kps / *desc hold the images' rows back to back (image 0 first), counts[i] = rows of image i. */
int apds_akaze_extract_batch(const uint8_t* imgs, int n_images, size_t image_stride_bytes, int rows, int cols, int channels, size_t stride_bytes,
                             int max_points, apds_keypoint** kps, uint8_t** desc, int* counts, int* desc_bytes);
/* The same two calls with detectAndCompute's `mask` argument, which lib.rs:75-79 leaves empty (OpenCV 4.8 AKAZE_Impl::detectAndCompute ->
 * KeyPointsFilter::runByPixelsMask, restated from memory: DESIGN.md section 2). Detection runs unmasked; then a keypoint is removed iff
 * mask[(int)(pt.y + 0.5f)][(int)(pt.x + 0.5f)] == 0 - pt the refined position in full-resolution pixels whatever its level, f32 additions,
 * truncation. The survivors keep their order and every field and descriptor byte of the unmasked call; the max_points cut (strongest
 * responses, ties by detection order) comes AFTER the mask. mask: rows x cols u8, mask_stride_bytes between rows, any non-zero value keeps.
 * A NULL mask is the unmasked call; mask_stride_bytes < cols is APDS_ERR_ASSERT (OpenCV asserts mask.size() == image.size()).
 * Batch form: masks = n_images pointers (or NULL: no mask at all), any of them NULL = that image unmasked; one mask_stride_bytes for all.
 * These two consult the mask at that one pixel, as OpenCV does; the _support forms below widen the test to the keypoint's descriptor support. */
int apds_akaze_extract_masked(const uint8_t* img, int rows, int cols, int channels, size_t stride_bytes, const uint8_t* mask, size_t mask_stride_bytes,
                              int max_points, apds_keypoint** kps, uint8_t** desc, int* n, int* desc_bytes);
int apds_akaze_extract_batch_masked(const uint8_t* imgs, int n_images, size_t image_stride_bytes, int rows, int cols, int channels, size_t stride_bytes,
                                    const uint8_t* const* masks, size_t mask_stride_bytes, int max_points, apds_keypoint** kps, uint8_t** desc, int* counts,
                                    int* desc_bytes);
/* The masked calls with a mask support: one more argument, int mask_support >= 0 (negative: APDS_ERR_BAD_ARG). A keypoint of level l in
 * octave o has ratio = 2^o and scale = rint(0.5f * size / ratio) (f32, half to even: the unit in which the descriptor's lattice is laid out,
 * constant per level), and radius R = mask_support * scale * ratio full-resolution pixels. Its centre is the pixel of the rule above,
 * cx = (int)(pt.x + 0.5f), cy = (int)(pt.y + 0.5f). It is removed iff at least one mask byte is zero in the square [cx - R, cx + R] x
 * [cy - R, cy + R] clipped to the image: pixels outside the image are not masked (the descriptor skips its samples there). Everything else
 * is as above: detection unmasked, the survivors keep order, fields and descriptor bytes, max_points cuts after the mask.
 * mask_support 0 is exactly the call without _support; a NULL mask is the unmasked call whatever mask_support is.
 * APDS_MASK_SUPPORT_DESCRIPTOR covers the M-LDB lattice at any orientation: its offsets reach 10 * scale per rotated axis, 10 * sqrt(2) < 15
 * (the orientation is not yet known where the mask is applied, so the square is the axis-aligned one that holds every rotation).
 * Cost: the device answers the square from a zero-count summed-area table of the mask, built in the workspace by two launches per call
 * (4 bytes per pixel and image; one table for a mask that a batch shares); mask_support 0 builds none. */
#define APDS_MASK_SUPPORT_DESCRIPTOR 15
int apds_akaze_extract_masked_support(const uint8_t* img, int rows, int cols, int channels, size_t stride_bytes, const uint8_t* mask, size_t mask_stride_bytes,
                                      int mask_support, int max_points, apds_keypoint** kps, uint8_t** desc, int* n, int* desc_bytes);
int apds_akaze_extract_batch_masked_support(const uint8_t* imgs, int n_images, size_t image_stride_bytes, int rows, int cols, int channels, size_t stride_bytes,
                                            const uint8_t* const* masks, size_t mask_stride_bytes, int mask_support, int max_points, apds_keypoint** kps,
                                            uint8_t** desc, int* counts, int* desc_bytes);

/* AKAZE's float descriptor. NOT in the reference, which fixes DESCRIPTOR_MLDB (lib.rs:64-73): cv::AKAZE::DESCRIPTOR_KAZE, the 64-float M-SURF
 * descriptor of OpenCV 4.8 MSURF_Descriptor_64_Invoker (restated from memory: DESIGN.md section 2), unit length, compared with NORM_L2 - the
 * input of apds_l2_knn_match and apds_dev_l2_topk. Same detector, same keypoints, same orientation: the keypoints of a float extraction are
 * those of the M-LDB call with the same arguments, field for field and bit for bit; only the describe kernel differs. Per keypoint, on the
 * (Lx, Ly) planes of its level (class_id): ratio = 2^octave, scale = rint(0.5f * size / ratio) (f32, half to even), 4 x 4 cells of 9 x 9
 * samples scale apart on a lattice rotated by the keypoint's angle, every sample the bilinear blend of the four pixels around it (indices
 * clamped to the plane), rotated into the keypoint's frame and weighted by a Gaussian around its cell's centre; a cell gives (sum dx, sum dy,
 * sum |dx|, sum |dy|) times a Gaussian over the cells; the 64 values are divided by their Euclidean length.
 * One deliberate departure from OpenCV: a row whose length is 0 (a flat patch) is 64 zeros - OpenCV divides by zero and writes NaN, which
 * would poison every distance of the L2 matcher.
 * The values are OpenCV's enum values; MLDB is what every other extraction call of this header computes. */
enum { APDS_AKAZE_DESCRIPTOR_KAZE = 3, APDS_AKAZE_DESCRIPTOR_MLDB = 5 };
#define APDS_DESC_FLOAT_DIM 64       /* floats per row, packed: 256 bytes */
/* The masked_support calls with float rows: *desc = n x 64 f32 (apds_free), *desc_dim = 64. A NULL mask with mask_support 0 is the plain
 * call; the argument rules and error codes are those of the masked_support calls above. */
int apds_akaze_extract_float(const uint8_t* img, int rows, int cols, int channels, size_t stride_bytes, const uint8_t* mask, size_t mask_stride_bytes,
                             int mask_support, int max_points, apds_keypoint** kps, float** desc, int* n, int* desc_dim);
int apds_akaze_extract_float_batch(const uint8_t* imgs, int n_images, size_t image_stride_bytes, int rows, int cols, int channels, size_t stride_bytes,
                                   const uint8_t* const* masks, size_t mask_stride_bytes, int mask_support, int max_points, apds_keypoint** kps, float** desc,
                                   int* counts, int* desc_dim);

/* lib.rs:94-114  get_knn_matches(origin_desc, target_desc, k, filter_strength) -> Vector<DMatch>
 * Hamming k-NN of each origin (query) row over the target (train) rows, then keep m[0] iff
 * m[0].distance < m[1].distance * filter_strength. Returns APDS_ERR_OUT_OF_RANGE when a query has fewer
 * than two neighbours (k < 2 or n_target < 2), like the reference's `i.get(1)?`. Rows are desc_bytes long, packed. */
int apds_get_knn_matches(const uint8_t* origin_desc, int n_origin, const uint8_t* target_desc, int n_target,
                         int desc_bytes, int k, float filter_strength, apds_dmatch** matches, int* n_matches);

/* lib.rs:116-126  get_bruteforce_matches(origin_desc, target_desc) -> Vector<DMatch>  (crossCheck = true) */
int apds_get_bruteforce_matches(const uint8_t* origin_desc, int n_origin, const uint8_t* target_desc, int n_target,
                                int desc_bytes, apds_dmatch** matches, int* n_matches);

/* BFMatcher::knnMatch itself (lib.rs:103), any k >= 1 (k <= 2 is the tuned path; k <= APDS_MATCH_MFMA_KMAX runs on the matrix cores like it,
 * see apds_dev_hamming_topk; above 16 the scan runs once per 16 neighbours): idx/dist are n_query*k, -1 / INT32_MAX where fewer than k exist. */
int apds_knn_match(const uint8_t* query_desc, int n_query, const uint8_t* train_desc, int n_train, int desc_bytes,
                   int k, int32_t* idx, int32_t* dist);

/* lib.rs:161-180  get_points_from_matches. bug_compatible = 1 reproduces the reference exactly (img1 index taken
 * from img_idx, both outputs from img1); 0 is the intended gather (query_idx -> img1, train_idx -> img2).
 * pts1/pts2: n_matches x 2 floats, caller allocated. */
int apds_get_points_from_matches(const apds_keypoint* img1_kp, int n1, const apds_keypoint* img2_kp, int n2,
                                 const apds_dmatch* matches, int n_matches, int bug_compatible, float* pts1, float* pts2);

/* ---- homographier -------------------------------------------------------------------------- */

/* mod.rs:231-259  find_homography_mat(input, reference, method, reproj_threshold) -> (Cmat<f64>, Option<Cmat<u8>>)
 * method: APDS_HOMOGRAPHY_*; reproj_threshold <= 0 -> 3.0. H: 9 doubles row major (H[8] == 1). mask: n bytes or
 * NULL (the shim passes it for RANSAC / LMEDS only, mod.rs:253-257). APDS_ERR_EMPTY when no model is found. */
int apds_find_homography(const float* input_xy, const float* reference_xy, int n, int method, double reproj_threshold,
                         double* H, uint8_t* mask);
/* same with OpenCV's two defaulted arguments exposed (maxIters 2000, confidence 0.995) */
int apds_find_homography_ex(const float* input_xy, const float* reference_xy, int n, int method, double reproj_threshold,
                            int max_iters, double confidence, double* H, uint8_t* mask);

/* mod.rs:183-220  raster_to_mat(pixels:&[RGBA8], w, h) -> Cmat<Vec4b>: RGBA -> BGRA rows.
 * APDS_ERR_BAD_ARG (MatError::Unknown) when n_pixels != w*h. bgra: w*h*4 bytes, caller allocated. */
int apds_raster_to_mat(const uint8_t* rgba, size_t n_pixels, int w, int h, uint8_t* bgra);

/* ---- "next" rows either side of the path ------------------------------------------ */

/* geotiff_extractor/src/image_extractor/mod.rs:346-378 band_merger (f32_to_u8 :410-422, gamma_correction :402-408): three f32 bands
 * + min/max {red_min, red_max, green_min, green_max, blue_min, blue_max} -> n pixels of RGBA8 (bgra = 0, what band_merger returns) or
 * BGRA8 (bgra = 1: raster_to_mat, mod.rs:183-220, fused). NaN / out-of-range -> 0; alpha 0 only if all three bands are NaN. */
int apds_band_merger(const float* red, const float* green, const float* blue, size_t n, const double* minmax6, int bgra, uint8_t* out);
int apds_dev_band_merger(const void* red, const void* green, const void* blue, size_t n, const double* minmax6, int bgra, void* out, void* stream);
/* One preprocessor tile in one call: `to_rgb` of an equal-size window (geotiff_extractor/src/image_extractor/mod.rs:241-269, band_merger
 * :346-378) -> `raster_to_mat` (homographier/src/homographier/mod.rs:183-197) -> `akaze_keypoint_descriptor_extraction_def`
 * (feature_extraction/src/lib.rs:61-92), as preprocessor/src/main.rs:258-277 chains them. red/green/blue: rows x cols f32 windows with
 * `row_stride` elements between rows (they may point into the mosaic); the RGBA / BGRA image exists on the device only. Outputs as apds_akaze_extract. */
int apds_tile_extract(const float* red, const float* green, const float* blue, int rows, int cols, size_t row_stride, const double* minmax6,
                      int max_points, apds_keypoint** kps, uint8_t** desc, int* n, int* desc_bytes);
/* The same for n_tiles equal-sized tiles in one call (the reference spawns one task per tile, main.rs:227-245): red / green / blue are arrays
 * of n_tiles window pointers (one row_stride for all); ONE band_merger pass and ONE batched extraction (apds_akaze_extract_batch) serve all
 * tiles. Per-tile results are exactly those of apds_tile_extract. Outputs as apds_akaze_extract_batch. */
int apds_tile_extract_batch(const float* const* red, const float* const* green, const float* const* blue, int n_tiles, int rows, int cols, size_t row_stride,
                            const double* minmax6, int max_points, apds_keypoint** kps, uint8_t** desc, int* counts, int* desc_bytes);
/* The tile calls (these two and the two apds_mosaic_tile_extract calls below) with a detection mask made of the tile's own nodata: the _ex
 * forms take one more argument, mask_mode. APDS_TILE_MASK_NONE is exactly the call without _ex. APDS_TILE_MASK_ALPHA masks the extraction
 * (the rule of apds_akaze_extract_masked) with the alpha byte of the BGRA image band_merger has just written on the device: a keypoint whose
 * refined position rounds onto a pixel of alpha 0 is removed. No mask buffer is allocated and no pass is added: the kernels read the
 * image's own fourth byte. The alpha rule is band_merger's and unchanged: alpha 0 only where ALL three bands are NaN (a pixel that lost one
 * or two bands keeps alpha 255 and masks nothing). Under APDS_RESAMPLE_LANCZOS a NaN propagates through every tap that touches it, so the
 * masked area is the nodata area widened by the filter footprint (three source pixels times max(1, win / out) on every side). Any other
 * mask_mode is APDS_ERR_BAD_ARG. Results equal apds_akaze_extract_masked on the BGRA tile with mask = its alpha plane.
 * APDS_TILE_MASK_ALPHA_SUPPORT is the alpha mask with the mask support APDS_MASK_SUPPORT_DESCRIPTOR (apds_akaze_extract_masked_support on
 * the BGRA tile with its alpha plane): a keypoint whose descriptor could sample a nodata pixel is removed, not only one that lies on one.
 * The modes are two bits: 1 = the alpha is the mask, 2 = with the descriptor support; 2 alone names no mask and stays APDS_ERR_BAD_ARG. */
#define APDS_TILE_MASK_NONE 0
#define APDS_TILE_MASK_ALPHA 1
#define APDS_TILE_MASK_ALPHA_SUPPORT 3
int apds_tile_extract_ex(const float* red, const float* green, const float* blue, int rows, int cols, size_t row_stride, const double* minmax6,
                         int max_points, int mask_mode, apds_keypoint** kps, uint8_t** desc, int* n, int* desc_bytes);
int apds_tile_extract_batch_ex(const float* const* red, const float* const* green, const float* const* blue, int n_tiles, int rows, int cols, size_t row_stride,
                               const double* minmax6, int max_points, int mask_mode, apds_keypoint** kps, uint8_t** desc, int* counts, int* desc_bytes);

/* The mosaic resident in HBM and the preprocessor's window read on it: geotiff_extractor/src/image_extractor/mod.rs:332-343
 * read_as::<f32>(window, window_size, size, Some(ResampleAlg::Lanczos)), which preprocessor/src/main.rs:197-277 cuts every level of detail
 * into tiles with. apds_tile_extract* take host windows of ONE size (no resampling); these calls keep the three bands on the device and
 * resample there, so a level > 0 tile is filtered (its footprint reaching into the neighbouring tiles) instead of decimated.
 * resample: APDS_RESAMPLE_NEAREST = index min((int64)((i + 0.5) * (win / out)), win - 1) per axis in double (the host mirror's rule, bit for
 * bit); APDS_RESAMPLE_LANCZOS = GDAL's convolution resampler restated (per axis ratio = win / out, sw = min(1, 1 / ratio),
 * radius = 3 / sw, centre c = (i + 0.5) ratio + origin, taps [floor(c - radius + 0.5), (int)(c + radius + 0.5)) clamped to the RASTER,
 * weight L((j + 0.5 - c) sw) / sum; rows first, then columns, f32 accumulation, NaN propagates). Equal sizes copy the window under both.
 * Limits: win / out <= 64 on either axis (385 taps), else APDS_ERR_BAD_ARG; a window outside the raster is APDS_ERR_OUT_OF_RANGE; an empty
 * window or output APDS_ERR_ASSERT; an unknown `resample` APDS_ERR_BAD_ARG. */
#define APDS_RESAMPLE_NEAREST 0
#define APDS_RESAMPLE_LANCZOS 1
/* Copies three rows x cols f32 bands (row_stride elements between rows; on_device 1: device pointers) into one device allocation
 * [3][rows][cols] on the calling thread's device. The handle is immutable afterwards and may be shared between threads. */
int apds_mosaic_create(void** mosaic, const void* red, const void* green, const void* blue, int rows, int cols, size_t row_stride, int on_device);
int apds_mosaic_destroy(void* mosaic);
int apds_mosaic_info(const void* mosaic, int* rows, int* cols);
/* mod.rs:200-229 datasets_min_max: {red_min, red_max, green_min, ...}, NaN ignored (a band of NaN only gives NaN): a device reduction,
 * computed by the first call and cached in the handle. */
int apds_mosaic_min_max(void* mosaic, double* minmax6);
/* The tables of one axis, host arithmetic only (no device needed): a window of `span` source pixels at `offset` of a raster of n_src, resampled
 * to n_out. Output i reads source pixels [start[i], start[i] + count[i]) with weights[i * max_taps ..] (computed in double, rounded once
 * to f32, zero past count). NEAREST: count 1, weight 1. max_taps below the widest footprint: APDS_ERR_BAD_ARG. */
int apds_resample_weights(int n_src, double offset, double span, int n_out, int resample, int max_taps, int32_t* start, int32_t* count, float* weights);
/* The resampled window itself: out3 = host [3][out_h][out_w] f32 (what to_rgb hands band_merger). */
int apds_mosaic_window(void* mosaic, int x0, int y0, int win_w, int win_h, int out_w, int out_h, int resample, float* out3);
/* apds_tile_extract / apds_tile_extract_batch on windows of the mosaic: window -> band_merger (BGRA) -> AKAZE entirely on the device.
 * minmax6 NULL = the mosaic's own (apds_mosaic_min_max). The batch form takes n_tiles (1 .. 4096) origins xy0 = {x0, y0, x1, y1, ...} of
 * ONE window and output shape: one resampling launch per pass covers all tiles and bands. Results are exactly those of apds_tile_extract
 * on the window apds_mosaic_window returns. Outputs as apds_akaze_extract / apds_akaze_extract_batch. */
int apds_mosaic_tile_extract(void* mosaic, int x0, int y0, int win_w, int win_h, int out_w, int out_h, int resample, const double* minmax6, int max_points,
                             apds_keypoint** kps, uint8_t** desc, int* n, int* desc_bytes);
int apds_mosaic_tile_extract_batch(void* mosaic, const int32_t* xy0, int n_tiles, int win_w, int win_h, int out_w, int out_h, int resample, const double* minmax6,
                                   int max_points, apds_keypoint** kps, uint8_t** desc, int* counts, int* desc_bytes);
/* with mask_mode (APDS_TILE_MASK_*, see apds_tile_extract_ex) */
int apds_mosaic_tile_extract_ex(void* mosaic, int x0, int y0, int win_w, int win_h, int out_w, int out_h, int resample, const double* minmax6, int max_points,
                                int mask_mode, apds_keypoint** kps, uint8_t** desc, int* n, int* desc_bytes);
int apds_mosaic_tile_extract_batch_ex(void* mosaic, const int32_t* xy0, int n_tiles, int win_w, int win_h, int out_w, int out_h, int resample,
                                      const double* minmax6, int max_points, int mask_mode, apds_keypoint** kps, uint8_t** desc, int* counts, int* desc_bytes);

/* The overview pyramid of the mosaic. The preprocessor opens its dataset as a COG (preprocessor/src/main.rs:142-161,
 * geotiff_extractor/src/image_extractor/mod.rs:141-164), and a COG carries overviews: GDAL serves read_as(window, tile * 2^lod, tile, ..)
 * from the overview of factor 2^lod, which the COG driver has built by CUBIC resampling, each level from the one below. These calls put
 * that pyramid beside the raster (a third of its bytes) and route the window reads through it (restated from GDAL's
 * behaviour, not pinned against it).
 * Level k (k >= 1) has ceil(rows / 2^k) x ceil(cols / 2^k) pixels; levels are added while the level below exceeds min_size on either axis
 * (min_size <= 0: 512, the COG block size). Level k is level k - 1 filtered by the convolution rule of apds_resample_weights with Keys'
 * cubic (a = -0.5: W(x) = 1.5|x|^3 - 2.5|x|^2 + 1 for |x| <= 1, -0.5|x|^3 + 2.5|x|^2 - 4|x| + 2 for 1 < |x| < 2, else 0) over the whole
 * axis: ratio = n(k-1) / n(k) in double (not 2 for an odd size), sw = 1 / ratio, radius = 2 / sw, taps clamped to the raster, weights
 * divided by their sum and rounded once to f32; rows first, then columns, f32 fused multiply-adds in tap order; NaN propagates (no mask band).
 *
 * apds_overview_weights: the table of one axis of one such step, host arithmetic only. Outputs as apds_resample_weights. RETURNS the
 * widest footprint (>= 1; at most 9 for n_out = ceil(n_src / 2)) or a negative status; max_taps = 0 with three null outputs computes only
 * that. n_out > n_src or max_taps below the footprint: APDS_ERR_BAD_ARG. */
int apds_overview_weights(int n_src, int n_out, int max_taps, int32_t* start, int32_t* count, float* weights);
/* Builds the levels on the calling thread's device (the mosaic's, else APDS_ERR_BAD_ARG): one fused kernel launch per level. To be
 * called once, before the handle is shared between threads; afterwards the handle is immutable again. A second call with the same
 * min_size changes nothing and gives the same *n_levels (may be NULL); another min_size is APDS_ERR_BAD_ARG. apds_mosaic_destroy frees
 * the levels; apds_mosaic_min_max stays a reduction over level 0. */
int apds_mosaic_build_overviews(void* mosaic, int min_size, int* n_levels);
/* Size of level 0 .. n_levels (0: the raster itself); any other level: APDS_ERR_OUT_OF_RANGE. */
int apds_mosaic_level_info(const void* mosaic, int level, int* rows, int* cols);
/* The level a read of win -> out is served from: the largest k with min(cols / cols_k, rows / rows_k) <= min(win_w / out_w, win_h / out_h),
 * all in double; 0 without overviews or when the right-hand side is below 2. */
int apds_mosaic_best_level(const void* mosaic, int win_w, int win_h, int out_w, int out_h, int* level);
/* apds_mosaic_window on the raster of `level`, in that level's own pixel coordinates (level 0: apds_mosaic_window on a handle without
 * overviews, exactly). A level the handle does not have, or a window outside the level: APDS_ERR_OUT_OF_RANGE.
 *
 * On a handle WITH overviews apds_mosaic_window, apds_mosaic_tile_extract and apds_mosaic_tile_extract_batch check the window against
 * the base raster as before, pick k = apds_mosaic_best_level and, for k > 0, read the window's image on level k with the caller's mode:
 * per axis fx = cols / cols_k, origin min(cols_k - 1, (int)(x0 / fx + 0.5)), extent max(1, (int)(win_w / fx + 0.5)) shortened to the
 * level's edge. For a window of 2^k times the output size at an origin divisible by 2^k that is a copy of the overview. On a handle
 * without overviews nothing changes. */
int apds_mosaic_window_level(void* mosaic, int level, int x0, int y0, int win_w, int win_h, int out_w, int out_h, int resample, float* out3);

/* homographier/src/homographier/mod.rs:271-300 warp_image_perspective: warpPerspective(src, M, size, INTER_LINEAR, BORDER_CONSTANT,
 * Scalar(1,1,1,1)). M (9 doubles) maps source to destination coordinates. The reference function is generic over the element type
 * (warp_image_perspective<T: DataType>): u8 elements with 1, 3 or 4 interleaved channels here (u8, Vec3b, Vec4b - the type the reference's
 * own caller warps), f32 elements (f32, Vec3f, Vec4f) through the _f32 entry. */
int apds_warp_perspective(const uint8_t* src, int rows, int cols, int channels, const double* M, int dst_rows, int dst_cols, uint8_t* dst);
int apds_warp_perspective_f32(const float* src, int rows, int cols, int channels, const double* M, int dst_rows, int dst_cols, float* dst);

/* homographier/src/homographier/mod.rs:320-369 pnp_solver_ransac(point_correspondences, camera_intrinsic, iter_count, reproj_thres,
 * confidence, dist_coeffs, method) -> Result<Option<PNPRANSACSolution>, MatError>: cv::solvePnPRansac with useExtrinsicGuess = false and
 * distCoeffs = zeros(4,1) (mod.rs:344 shadows the dist_coeffs argument with zeros, so it never reaches OpenCV and is not part of this ABI).
 * obj_xyz: n Point3d (ImgObjCorrespondence::obj_point, mod.rs:53-65), img_xy: n Point2d, camera_intrinsic: 3x3 f64 row major.
 * method: cv::SolvePnPMethod; the shim passes method.unwrap_or(SOLVEPNP_EPNP) (mod.rs:360). Built: APDS_SOLVEPNP_EPNP (RANSAC kernel
 * EPnP on 5 points), APDS_SOLVEPNP_P3P (Gao's P3P on 4 points; also the kernel OpenCV switches to when n == 4), APDS_SOLVEPNP_AP3P (Ke and
 * Roumeliotis' algebraic P3P on 4 points) - the final pose over the inliers is EPnP in these cases, as in OpenCV - and APDS_SOLVEPNP_ITERATIVE (EPnP kernel; final pose = solvePnP(ITERATIVE) over
 * the inliers WITHOUT an extrinsic guess, as the reference's use_extrinsic_guess = false makes it: a homography (planar object points) or
 * DLT (>= 6 points) start, then <= 20 Levenberg-Marquardt iterations on the reprojection error; with five non-planar inliers the RANSAC
 * model stays, as in solvePnPRansac), APDS_SOLVEPNP_SQPNP (EPnP kernel; final pose = Terzakis and Lourakis' SQPnP over the inliers, calib3d/sqpnp.cpp;
 * no pose in front of the camera -> *found = 0 with the RANSAC model in rvec / tvec, as solvePnPRansac leaves it), APDS_SOLVEPNP_DLS and
 * APDS_SOLVEPNP_UPNP (OpenCV 4 runs EPnP for both: identical to APDS_SOLVEPNP_EPNP), APDS_SOLVEPNP_IPPE_SQUARE (what solvePnPRansac makes of it:
 * four correspondences are solved by P3P directly like under every other flag; with more, the final solvePnP over the >= 5 inliers of the
 * EPnP RANSAC asserts npoints == 4 -> APDS_ERR_ASSERT, the reference's Err(MatError::Opencv); no consensus -> *found = 0), APDS_SOLVEPNP_IPPE
 * (EPnP kernel; final pose = Collins and Bartoli's plane-based solver, calib3d/ippe.cpp, over the inliers: object points moved to the plane
 * z = 0 about their centroid, Harker-O'Leary homography, the better of the two poses; inliers that are not coplanar within 1e-3 of their own
 * unit have no IPPE pose -> *found = 0 with the RANSAC model in rvec / tvec, as solvePnPRansac leaves it). Values past cv::SolvePnPMethod's
 * last member return APDS_ERR_NOT_IMPLEMENTED.
 * n < 4 -> APDS_ERR_ASSERT (mod.rs:627-638).
 * *found = 1: rvec[3], tvec[3], inliers[0..*n_inliers) filled (inliers: caller allocated, n ints); *found = 0: Ok(None). */
#define APDS_SOLVEPNP_ITERATIVE 0
#define APDS_SOLVEPNP_EPNP 1
#define APDS_SOLVEPNP_P3P 2
#define APDS_SOLVEPNP_DLS 3
#define APDS_SOLVEPNP_UPNP 4
#define APDS_SOLVEPNP_AP3P 5
#define APDS_SOLVEPNP_IPPE 6
#define APDS_SOLVEPNP_IPPE_SQUARE 7
#define APDS_SOLVEPNP_SQPNP 8
int apds_pnp_solver_ransac(const double* obj_xyz, const double* img_xy, int n, const double* camera_intrinsic, int iter_count, float reproj_thres,
                           double confidence, int method, double* rvec, double* tvec, int32_t* inliers, int* n_inliers, int* found);
/* pnp_solver_ransac with the argument the reference documents ("distortion coefficients from camera calibration", mod.rs:310,326) and
 * then shadows: dist = n_dist coefficients of the lens model below (see apds_undistort_points). The image points are undistorted in f64
 * (apds_undistort_points' arithmetic with iters = 5 and K = camera_intrinsic) before solvePnPRansac's f32 conversion; everything after
 * that is apds_pnp_solver_ransac. With no distortion (n_dist 0, dist NULL, or every coefficient exactly 0) it IS apds_pnp_solver_ransac,
 * bit for bit. reproj_thres is therefore measured in UNDISTORTED pixels. OpenCV measures it in the distorted image (it projects with the
 * coefficients inside the RANSAC loop): a deliberate difference, not pinned against OpenCV. The lens arguments are checked first
 * (status codes: apds_undistort_points), then the plain call's own (n < 4 -> APDS_ERR_ASSERT), all before any device work. */
int apds_pnp_solver_ransac_dist(const double* obj_xyz, const double* img_xy, int n, const double* camera_intrinsic, int iter_count, float reproj_thres,
                                double confidence, int method, const double* dist, int n_dist, double* rvec, double* tvec, int32_t* inliers,
                                int* n_inliers, int* found);

/* ---- lens distortion ------------------------------------------------------------------------------------------------------------------
 * OpenCV's radial-tangential model with the rational denominator; the reference's calibrator computes these coefficients
 * (calibrator/src/main.rs:59-73, calibrate_camera_def). All arithmetic in f64, every operation in the order csrc/lens_core.h writes down.
 * K: 3x3 row major, fx = K[0], cx = K[2], fy = K[4], cy = K[5]; the skew K[1] is ignored, as OpenCV ignores it. Normalised coordinates
 * x = (u - cx) / fx, y = (v - cy) / fy, r2 = x x + y y. dist in OpenCV's order (k1, k2, p1, p2[, k3[, k4, k5, k6]]):
 *   forward (ideal -> distorted): rc = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3),
 *       x' = x rc + 2 p1 x y + p2 (r2 + 2 x x), y' = y rc + p1 (r2 + 2 y y) + 2 p2 x y, u' = fx x' + cx, v' = fy y' + cy;
 *   inverse (distorted -> ideal): cv::undistortPoints' fixed-point iteration from x = x': x <- (x' - dx(x, y)) / rc(x, y), likewise y (dx, dy
 *       the tangential part), EXACTLY iters steps, no early exit (the result is a pure function of the inputs); iters <= 0: 5, what
 *       cv::undistortPoints runs; output fx x + cx (P = cameraMatrix).
 * n_dist: 0 (or dist NULL) = no distortion; 4, 5, 8 served; 12 and 14 (thin prism, tilt) APDS_ERR_NOT_IMPLEMENTED; anything else
 * APDS_ERR_BAD_ARG; a coefficient that is not finite, or a focal length that is not finite and positive: APDS_ERR_BAD_ARG - all before any
 * device work. No distortion - n_dist 0 or every coefficient exactly 0 - launches nothing: points and images come back bit for bit. */
/* xy, out: n x 2 doubles on the host (out may be xy); computed on the device. n == 0: APDS_OK without touching the device. */
int apds_distort_points(const double* xy, int n, const double* K, const double* dist, int n_dist, double* out);
int apds_undistort_points(const double* xy, int n, const double* K, const double* dist, int n_dist, int iters, double* out);
/* The inverse in place on device points: n pairs of f32 (x, y), one pair at the head of every stride_bytes bytes - 8: a point array
 * (apds_dev_points_from_matches, apds_dev_pnp_correspondences' img_xy); 28: apds_keypoint rows, of which only x and y are rewritten; any
 * other stride >= 8 that is a multiple of 4 (else APDS_ERR_BAD_ARG). Each pair is widened to f64, undistorted, and rounded once on the
 * store. One kernel, one thread per point, asynchronous on `stream` (NULL: the thread's own); it takes nothing from the workspace. */
int apds_dev_undistort_points(void* xy_dev, int n, int stride_bytes, const double* K, const double* dist, int n_dist, int iters, void* stream);
/* cv::undistort's shape: dst (rows x cols x channels u8, packed, channels 1, 3 or 4; the size of src) = the image an ideal camera new_K
 * (NULL: K) would have taken. Per destination pixel (u, v), no iteration: x = (u - cx') / fx', y = (v - cy') / fy' with new_K's entries,
 * the forward model with K gives (us, vs), X = sat_int_rn(32 us), Y = sat_int_rn(32 vs), then the fixed-point bilinear sample of
 * apds_warp_perspective (1/32-pixel fractions, 15-bit weights, (sum + 2^14) >> 15) with border value 0 in every channel, as in
 * cv::undistort (the warp keeps the reference's 1). cv::initUndistortRectifyMap accumulates its map along the row, so bit parity with
 * OpenCV is not claimed. No distortion and new_K NULL: dst = src, no launch. rows <= 65535. The device form is asynchronous on `stream`,
 * takes its weight table from the calling thread's workspace, and needs dst_dev apart from src_dev (APDS_ERR_BAD_ARG otherwise). */
int apds_undistort_image(const uint8_t* src, int rows, int cols, int channels, const double* K, const double* dist, int n_dist, const double* new_K,
                         uint8_t* dst);
int apds_dev_undistort_image(const void* src_dev, int rows, int cols, int channels, const double* K, const double* dist, int n_dist, const double* new_K,
                             void* dst_dev, void* stream);

/* apds_pnp_solver_ransac (mod.rs:320-369) on correspondences that are already on the device as the float values solvePnPRansac converts
 * its points to: obj_xyz_dev n x 3 floats, img_xy_dev n x 2 floats, ordered on `stream` (NULL: the thread's own). rvec, tvec, *n_inliers
 * and *found go to the host; inliers: a host buffer of n ints, or NULL. For the same float values the result is apds_pnp_solver_ransac's
 * in every respect (one RANSAC loop serves both): every method, the direct solves of n == 4 / n == 5, n < 4 -> APDS_ERR_ASSERT,
 * IPPE_SQUARE's assertion, SQPnP / IPPE's *found = 0 with the RANSAC model in rvec / tvec. */
int apds_dev_pnp_solver_ransac(const void* obj_xyz_dev, const void* img_xy_dev, int n, const double* camera_intrinsic, int iter_count, float reproj_thres,
                               double confidence, int method, double* rvec, double* tvec, int32_t* inliers, int* n_inliers, int* found, void* stream);
/* The 2D-3D pairs of a frame's matches for apds_dev_pnp_solver_ransac, on the device, one thread per match: img_xy[m] = kps[queryIdx].xy
 * (n_matches x 2 floats), obj_xyz[m] = (float)(db_xyz[trainIdx] - origin) (n_matches x 3 floats; subtracted in double, rounded once).
 * kps: the frame's n_kps keypoints (28 bytes each); db_xyz: n_db x 3 doubles, the world point of every GLOBAL train row (e.g. ECEF metres
 * from apds_get_world_coordinates, elevationdb.rs:64-104); matches: apds_dev_ratio_filter's output; origin: 3 doubles (host). The origin
 * exists because solvePnPRansac works in f32, which resolves ECEF magnitudes to 0.5 m only: the pose is then relative to it.
 * An index outside either side -> APDS_ERR_OUT_OF_RANGE (as apds_dev_points_from_matches). Returns when the gather is done. */
int apds_dev_pnp_correspondences(const void* kps, int n_kps, const void* db_xyz, int64_t n_db, const double* origin, const void* matches, int n_matches,
                                 void* img_xy, void* obj_xyz, void* stream);

/* feature_database/src/elevationdb.rs:64-104 get_world_coordinates, batched (the object points pnp_solver_ransac consumes): pixel
 * (x, y) of the reference mosaic -> dataset geotransform -> elevation through the inverse elevation geotransform (row id of
 * elevationdb.rs:240) -> EPSG:4326 -> EPSG:4978 (ECEF metres). xy: n x 2, xyz: n x 3 doubles; geotransforms: GDAL's 6 doubles;
 * elevation_gt NULL = no elevation data -> height 0 (elevationdb.rs:74-77); elevation: eh x ew doubles, row major.
 * APDS_ERR_OUT_OF_RANGE if a lookup misses the elevation table (the reference returns Err; those points are NaN here),
 * APDS_ERR_BAD_ARG if elevation_gt is singular (the reference panics). */
int apds_get_world_coordinates(const double* xy, int n, const double* dataset_gt, const double* elevation_gt, const double* elevation, int ew, int eh,
                               double* xyz);

/* BASELINE config 3 (no reference call site: the reference matches Hamming only, lib.rs:101,121): brute-force L2 k-NN of float
 * descriptors (dim <= 128) as an MFMA distance GEMM with a fused top-k; semantics of BFMatcher(NORM_L2).knnMatch
 * (dist = sqrt(sum (q-t)^2), ties to the lower train index). k in {1,2}. idx/dist: n_query*k. */
int apds_l2_knn_match(const float* query, int n_query, const float* train, int n_train, int dim, int k, int32_t* idx, float* dist);
/* device form: out_keys = n_query*k uint64 (f32 bits of the SQUARED distance << 32 | train_index + index_base), ascending */
int apds_dev_l2_topk(const void* query, int n_query, const void* train, int64_t n_train, int dim, uint32_t index_base, int k, void* out_keys,
                     void* stream);
/* The same with a choice of arithmetic. APDS_L2_EXACT: every distance in f32 MFMA (what apds_dev_l2_topk does). APDS_L2_SCREEN: a bf16
 * MFMA screen (16x the f32 matrix rate) selects, with a proved error bound, every row that can be among the two nearest; those are
 * re-ranked with exactly the f32 arithmetic of the exact mode, so the returned keys are the exact mode's, bit for bit. The screen is built
 * for dim == 128, k == 2, 16-byte aligned rows; otherwise (or if the candidate buffer overflows) the exact kernel runs: *mode_used says
 * which one did; *candidates_per_query = re-ranked rows per query (both may be NULL). */
enum { APDS_L2_EXACT = 0, APDS_L2_SCREEN = 1 };
int apds_dev_l2_topk_ex(const void* query, int n_query, const void* train, int64_t n_train, int dim, uint32_t index_base, int k, int mode, void* out_keys,
                        void* stream, int* mode_used, double* candidates_per_query);
/* A resident L2 train set: n_train rows of dim floats (dim 1..128) whose global indices start at index_base, BORROWED until
 * apds_l2_train_destroy and unchanged meanwhile. What the screen derives from the rows is made once, here, and owned by the handle: |t|^2
 * per row (the exact kernel's value), the bf16 copy pre-scaled by -2 and the largest norm. *screen_ready (apds_l2_train_info; every
 * output may be NULL) = 1 iff dim is 64 or 128, the rows are 16-byte aligned and n_train >= 2: the bf16 screen exists for that handle.
 * apds_dev_l2_train_top2: out_keys = the keys of apds_dev_l2_topk(query, n_query, rows, n_train, dim, index_base, k = 2), bit for bit, in
 * either mode (APDS_L2_EXACT / APDS_L2_SCREEN); per call only the query side is prepared, and the scratch is the calling thread's workspace
 * (nothing grows with the number of calls). A handle that is not screen_ready, a query pointer that is not 16-byte aligned and a candidate
 * overflow run the exact kernel for that call: *mode_used says which ran, *candidates_per_query = re-ranked rows per query (both may be
 * NULL). The handle lives on the calling thread's device; concurrent calls on one handle are allowed (it is read-only after create). */
int apds_l2_train_create(void** set, const void* train_f32_dev, int64_t n_train, int dim, uint32_t index_base);
int apds_l2_train_destroy(void* set);
int apds_l2_train_info(const void* set, int64_t* n_train, int* dim, int* screen_ready);
int apds_dev_l2_train_top2(void* set, const void* query_f32_dev, int n_query, int mode, void* out_keys, void* stream, int* mode_used,
                           double* candidates_per_query);

/* GPU-resident keypoint table: the reference's `keypoint` table and its access paths without Postgres.
 * insert: preprocessor/src/main.rs:296-324 (x,y lifted to level-of-detail-0 pixels: v * 2^lod + index * tile * 2^lod).
 * select: feature_database/src/keypointdb.rs:38-90, mode 0 by image id, 1 by level of detail, 2 by level of detail and bounding box
 * (floor(start) <= v <= ceil(end)); always ORDER BY response DESC LIMIT 262143 (keypointdb.rs:12). The selection stays on the
 * device as the table's "view": 64-byte descriptor rows ready to be a train set for apds_dev_hamming_topk. */
int apds_db_create(void** db, int64_t capacity);
int apds_db_destroy(void* db);
int64_t apds_db_rows(const void* db);
/* A table has a KIND, fixed at create: apds_db_create makes a byte table (descriptor column of 64-byte M-LDB rows), apds_db_create_float a
 * float table (descriptor column of 64 x f32 = 256 bytes, the M-SURF rows of apds_akaze_extract_float). apds_db_info reports
 * APDS_AKAZE_DESCRIPTOR_MLDB / 64 or APDS_AKAZE_DESCRIPTOR_KAZE / 256 (either output may be NULL). Every other column, the ids, the
 * selections, the deletes and the world points are the same for both kinds, from the same kernels.
 * ROWS OF THE TABLE'S KIND: every call that takes or returns descriptor rows through a void* device pointer (apds_db_insert_dev,
 * apds_db_insert_batch_dev, apds_db_view, apds_db_view_pointers, apds_db_table) means rows of the table's kind: 64-byte rows on a byte
 * table, rows of 64 floats on a float table (what apds_dev_akaze_extract_float(_batch) writes; stored whole, nothing zeroed). Calls with a
 * TYPED host pointer come in twins (apds_db_insert_image / _float, apds_db_view_download / _float, apds_db_read_keypoint_from_id /
 * _float, apds_db_knn_match / apds_db_l2_knn_match): the byte-typed call on a float table and the float-typed call on a byte table
 * return APDS_ERR_BAD_ARG and leave the table unchanged. apds_db_shard on a float table is APDS_ERR_BAD_ARG (the sharded matcher is
 * Hamming). apds_mosaic_tiles_to_db extracts rows of the table's kind; the keypoint columns of a float table are those a byte table gets
 * from the same tiles, bit for bit. */
int apds_db_create_float(void** db, int64_t capacity);
int apds_db_info(const void* db, int* descriptor, int* row_bytes);
/* apds_db_insert_image on a float table: desc64f = n rows of 64 floats. */
int apds_db_insert_image_float(void* db, const apds_keypoint* kps, const float* desc64f, int n, int image_id, int level_of_detail, uint64_t column,
                               uint64_t row, uint64_t tile_w, uint64_t tile_h);
int apds_db_insert_image(void* db, const apds_keypoint* kps, const uint8_t* desc61, int n, int image_id, int level_of_detail, uint64_t column,
                         uint64_t row, uint64_t tile_w, uint64_t tile_h);
int apds_db_select(void* db, int mode, int value, float x_start, float y_start, float x_end, float y_end, int* n_out);
int apds_db_view(void* db, void** rows64_dev, void** kps_dev, void** row_ids_dev, void** image_ids_dev, int* n);
int apds_db_view_download(void* db, apds_keypoint* kps, uint8_t* desc61, int32_t* ids, int32_t* image_ids);
/* knnMatch (any k >= 1 that apds_dev_hamming_topk serves) of host query descriptors against the current view; idx = position in the view (= trainIdx of the Vec the reference would hold) */
int apds_db_knn_match(void* db, const uint8_t* query_desc, int n_query, int desc_bytes, int k, int32_t* idx, int32_t* dist);
/* The float table's twins. apds_db_view_download_float: desc64f receives 64 floats per row of the current view. apds_db_l2_knn_match:
 * apds_l2_knn_match (k 1 or 2, the exact f32 kernel, dist = the distance, idx -1 / dist +inf where the view has fewer than k rows) of
 * n_query host rows of 64 floats against the current view, idx = position in the view. */
int apds_db_view_download_float(void* db, apds_keypoint* kps, float* desc64f, int32_t* ids, int32_t* image_ids);
int apds_db_l2_knn_match(void* db, const float* query, int n_query, int k, int32_t* idx, float* dist);
/* apds_db_insert_image for rows that are already on the device: kps_dev (28-byte keypoints) and desc64_dev (64-byte descriptor rows) are
 * exactly what apds_dev_akaze_extract writes, n of them; no upload, no repack. The stored rows are apds_db_insert_image's bit for bit:
 * x = k.x * 2^lod + (float)(column * tile_w * 2^lod) (the u64 product first), the same for y, the other fields copied, bytes 61-63 of
 * every stored descriptor row zero whatever the source row holds there. `stream` (NULL: the thread's own) must be the stream the
 * extraction was issued on, or be ordered after it: the extraction returns with its descriptor kernels still queued. Returns when the rows
 * are in the table (one synchronise). A full table is APDS_ERR_NOMEM with the table unchanged. Inserting - through any of the insert
 * calls - is single-threaded per table: no two threads may insert into, or insert into and read, one table at the same time. */
int apds_db_insert_dev(void* db, const void* kps_dev, const void* desc64_dev, int n, int image_id, int level_of_detail, uint64_t column, uint64_t row,
                       uint64_t tile_w, uint64_t tile_h, void* stream);
/* The batch form, on what apds_dev_akaze_extract_batch writes: tile i (0 <= i < n_tiles <= 4096) has counts[i] rows at i * capacity rows,
 * gets image_id = first_image_id + i and the tile position columns_rows = {column0, row0, column1, row1, ...}; its rows follow those of
 * the tiles before it, so the table is the one n_tiles consecutive apds_db_insert_image calls make. counts and columns_rows are host
 * arrays. One kernel launch for the whole batch. Everything is checked before anything is written: rows that do not all fit are
 * APDS_ERR_NOMEM, a negative count or one above capacity APDS_ERR_BAD_ARG, and the table is unchanged in both cases. */
int apds_db_insert_batch_dev(void* db, const void* kps_dev, const void* desc64_dev, int n_tiles, int capacity, const int32_t* counts, int first_image_id,
                             int level_of_detail, const uint32_t* columns_rows, uint64_t tile_w, uint64_t tile_h, void* stream);
/* The DB build of a group of tiles in ONE call (preprocessor/src/main.rs:197-327): apds_mosaic_tile_extract_batch_ex up to the
 * extraction (same arguments, checks and status codes), then apds_db_insert_batch_dev on the same stream with tile_w = out_w and
 * tile_h = out_h. No keypoint and no descriptor crosses PCIe: only counts[n_tiles] reaches the host. The mosaic and the table must live on
 * the same device (else APDS_ERR_BAD_ARG). The table is bit-equal to the batch extraction followed by n_tiles apds_db_insert_image calls. */
int apds_mosaic_tiles_to_db(void* mosaic, void* db, const int32_t* xy0, int n_tiles, int win_w, int win_h, int out_w, int out_h, int resample,
                            const double* minmax6, int max_points, int mask_mode, int first_image_id, int level_of_detail, const uint32_t* columns_rows,
                            int* counts);
/* apds_get_world_coordinates for every row currently in the table, where the rows live: the point ((double)x, (double)y) of row i goes
 * through the same arithmetic into row i of a table-owned column xyz (capacity x 3 doubles, allocated on first use). elevation: eh x ew
 * doubles, on the host or (elevation_on_device != 0) on the device; elevation_gt NULL = height 0; a singular elevation_gt is
 * APDS_ERR_BAD_ARG. A row whose lookup misses the raster gets three NaNs and the call still returns APDS_OK: *n_missing (may be NULL) is
 * the exact number of such rows. */
int apds_db_world_coordinates(void* db, const double* dataset_gt, const double* elevation_gt, const void* elevation, int ew, int eh,
                              int elevation_on_device, int64_t* n_missing);
/* The WHOLE table in the layout the pipeline takes (no selection, no 262143-row limit, insertion order): *rows64_dev = the table's own
 * descriptor column (not a copy), *kps_dev = a table-owned buffer of 28-byte keypoints with the lifted coordinates, indexed by row
 * (gathered by one kernel, and only for rows added since the last call), *xyz_dev = the column of apds_db_world_coordinates, or NULL if
 * it was never computed or rows were added since it was; *n = rows. Any output may be NULL. The pointers hold until the next insert, delete
 * or apds_db_destroy. They are the arguments of apds_pipeline_create(.., rows64, n, 0, NULL, kps, n, ..) and apds_pipeline_pose_params'
 * db_xyz_dev; a match's trainIdx is then the table row: the id - 1 that apds_db_view_download reports while the table has seen no
 * delete, and the index into apds_db_ids always. */
int apds_db_table(void* db, void** rows64_dev, void** kps_dev, void** xyz_dev, int64_t* n);
/* View objects: the read of keypointdb.rs:50-90 (read_keypoints_from_lod / read_keypoints_from_coordinates: the rows of one level of
 * detail, optionally inside a bounding box, ORDER BY response DESC LIMIT 262143) as something a caller repeats for every frame. A view
 * owns its result buffers and every byte of scratch a selection takes, allocated at create from the table's capacity and the view's,
 * so any number of views of one table select at the same time from different threads on different streams, and nothing grows with
 * the number of calls. A view never touches the table's own "current view" (apds_db_select, apds_db_view, apds_db_knn_match).
 * capacity <= 0: min(262143, table capacity) rows; else min(capacity, 262143). The view borrows the table: destroy it first. The
 * table must not receive inserts while a select of any of its views is in flight. */
int apds_db_view_create(void* db, int capacity, void** view);
int apds_db_view_destroy(void* view);
/* apds_db_select's selection (same modes, same floor / ceil of the box, same order: response descending with -0.0 tied to +0.0, then
 * table row ascending - SQL leaves ties in response unspecified, here they fall to row order), cut at the view's capacity, into the
 * view. With equal limits the rows, keypoints, row ids and image ids are apds_db_select's bit for bit. with_xyz != 0 also gathers
 * the table's world points (apds_db_world_coordinates; three doubles per row); APDS_ERR_BAD_ARG if that column was never computed or
 * rows were added since. Everything runs on `stream` (NULL: the calling thread's own). The call synchronises the stream ONCE, for the
 * number of qualifying rows, queues the cut, the sort and the gather behind it and returns: *n_out is final, the view's buffers are
 * complete when the stream has run, so work queued later on the same stream (or ordered behind it by an event) reads them safely.
 * One select at a time per view. */
int apds_db_view_select(void* view, int mode, int value, float x_start, float y_start, float x_end, float y_end, int with_xyz, void* stream,
                        int* n_out);
/* Device pointers of the view's last selection: n x 64-byte descriptor rows (a ready train set; trainIdx = position in the view),
 * n x 28-byte keypoints, table row ids, image ids, and n x 3 doubles (*xyz_dev NULL unless that selection ran with_xyz). Any output may
 * be NULL. The pointers hold until apds_db_view_destroy; their contents until the next select. */
int apds_db_view_pointers(const void* view, void** rows64_dev, void** kps_dev, void** row_ids_dev, void** image_ids_dev, void** xyz_dev,
                          int* n);
/* A view of a FLOAT table also owns the train side of its current selection for the L2 matcher: per row |t|^2, the bf16 copy scaled by
 * -2 and the largest norm (what apds_l2_train_create derives from resident rows), allocated at create for the view's capacity and written
 * by the select's own gather launch from the rows it moves - no further pass over the selection, no further synchronisation. *set = a
 * BORROWED train set over the view's rows with index base 0 (a key's row is the position in the view): pass it to
 * apds_dev_l2_train_top2 / apds_l2_train_info; apds_l2_train_destroy refuses it (APDS_ERR_BAD_ARG, nothing released). The handle is valid until apds_db_view_destroy; its
 * contents are those of the view's last select, complete when that select's stream has run, so a top-2 queued on the same stream (or
 * ordered behind it) reads them safely. The keys are those of apds_dev_l2_topk over the view's rows bit for bit, in either mode; a
 * selection of 0 or 1 rows is served by the exact kernel (screen_ready = 0), from 2 rows on the screen is ready. One thread at a time
 * per view, as for selects. APDS_ERR_BAD_ARG on a view of a byte table. */
int apds_db_view_l2_train(void* view, void** set);
/* Ids and deletes: the two access paths of the reference's KeypointDatabase trait that take an id, read_keypoint_from_id
 * (keypointdb.rs:28-36) and delete_keypoint (keypointdb.rs:92-97), and the deletes by image, level of detail and region that replacing
 * imagery needs. Every row has an id that behaves like the reference's SERIAL column: the first row ever inserted gets 1, every insert
 * continues from the highest id ever given plus one, an id is never reused and never changes when other rows are deleted. Ids therefore
 * ascend with the row; on a table that never saw a delete, id = row + 1. apds_db_view_download reports these ids.
 * A delete closes the table up on the device: the surviving rows keep their order and every bit of every column, their world points
 * (apds_db_world_coordinates) move with them and stay current, and apds_db_rows shrinks. A delete is a writer like an insert: single-
 * threaded per table, never while a select of any view of the table is in flight, never while a pipeline holds the table
 * (apds_pipeline_create_table). A delete that removes at least one row invalidates the pointers of apds_db_table and apds_db_ids (ask
 * again), the table's current view (apds_db_select: it is emptied) and the row ids of every earlier selection. View objects stay usable:
 * their next select sees the new table. Handles made by apds_db_shard earlier are copies and do not change. A delete that removes
 * nothing changes nothing, and pointers handed out earlier stay valid. The calls run on the calling thread's own stream and return when
 * the table is final. */
/* *ids_dev = the id column by row (int32, apds_db_rows of them; the table's own column, not a copy). Holds until the next insert or
 * delete. Indexing it with the row ids of apds_db_view / apds_db_view_pointers, or with a match's trainIdx over apds_db_table, gives ids. */
int apds_db_ids(void* db, void** ids_dev);
/* keypointdb.rs:28-36: the row that has `id` (a binary search of the id column on the device): its keypoint (lifted coordinates), the
 * first 61 bytes of its descriptor, its image id and its current row. Any output may be NULL. An id no row has - deleted, never given,
 * below 1 - is APDS_ERR_OUT_OF_RANGE (the reference returns Err(NotFound)). */
int apds_db_read_keypoint_from_id(void* db, int id, apds_keypoint* kp, uint8_t* desc61, int* image_id, int64_t* row);
/* The same on a float table: desc64f receives the row's 64 floats. */
int apds_db_read_keypoint_from_id_float(void* db, int id, apds_keypoint* kp, float* desc64f, int* image_id, int64_t* row);
/* Deletes every row apds_db_select qualifies for the same mode, value and box (mode 0: an image's keypoints; 1: a level of detail; 2: a
 * region at a level of detail, floor(start) <= v <= ceil(end)) - all of them: no 262143-row limit, no ordering. *n_deleted (may be
 * NULL) = the exact number of rows removed. */
int apds_db_delete_where(void* db, int mode, int value, float x_start, float y_start, float x_end, float y_end, int64_t* n_deleted);
/* Deletes the rows whose id is in the host array ids[0 .. n). An id no row has deletes nothing and is no error (keypointdb.rs:92-97: diesel's
 * execute returns Ok(0)); an id listed twice counts once; the list need not be sorted. n == 1 is the reference's delete_keypoint. */
int apds_db_delete_ids(void* db, const int32_t* ids, int n, int64_t* n_deleted);

/* ---- multi-GPU: the descriptor DB row-sharded over the GPUs of one node (BASELINE config 5) -------------------------------
 * No counterpart upstream: the reference matches on one CPU (feature_extraction/src/lib.rs:94-126) against whatever train set
 * feature_database/src/keypointdb.rs:50-90 returned, and its only parallelism is the preprocessor's rayon pool
 * (preprocessor/src/main.rs:86-89,227-245). Here one rank (a process, or a thread) drives each GPU; rank r keeps rows
 * [index_base, index_base + n_rows) of the train set resident, every rank brings its own frame's queries, and apds_shard_knn returns to
 * every rank the top-k of ITS queries over the WHOLE train set: all-gather of the query rows -> local scan -> all-to-all of the
 * per-shard keys -> u64-min merge. The result equals apds_dev_hamming_topk over the unsharded rows bit for bit (ties to the lower
 * global row). All ranks must issue the collective calls (create, counts, knn, gather, exchange_merge, destroy) in the same order.
 *
 * Transports: APDS_TRANSPORT_RCCL (one rank per GPU; the id comes from apds_comm_id_create on rank 0 and reaches the other ranks by any
 * host-side means - a file, MPI, the parent process), APDS_TRANSPORT_LOOPBACK (the ranks are threads of one process, any number per
 * GPU: the identical choreography on a one-GPU box), APDS_TRANSPORT_HOST (the host program's communicator as two callbacks on HOST
 * buffers, e.g. gloo or MPI; device data is staged around them, so it synchronises with the host). */
#define APDS_COMM_ID_BYTES 128
typedef struct apds_comm_id {
    char bytes[APDS_COMM_ID_BYTES];
} apds_comm_id;
enum { APDS_TRANSPORT_RCCL = 0, APDS_TRANSPORT_LOOPBACK = 1, APDS_TRANSPORT_HOST = 2, APDS_TRANSPORT_DEVICE = 3 };
typedef struct apds_host_transport {
    void* user;
    /* recv = every rank's bytes_per_rank bytes, rank-major; return 0 on success */
    int (*all_gather)(void* user, const void* send, void* recv, size_t bytes_per_rank);
    /* to rank p: send[send_off[p] .. + send_bytes[p]); from rank p: recv_bytes[p] bytes to recv + recv_off[p] */
    int (*all_to_all)(void* user, const void* send, const size_t* send_off, const size_t* send_bytes, void* recv, const size_t* recv_off,
                      const size_t* recv_bytes);
} apds_host_transport;
/* APDS_TRANSPORT_DEVICE: the host program's communicator as two callbacks on DEVICE buffers, ordered on the hipStream_t they are given (e.g.
 * torch.distributed's device collectives over its own RCCL communicator: the second way onto xGMI if the library's own communicator cannot be
 * set up beside the host's). Passed to apds_shard_create through the `host` argument (same layout, one more argument per callback). */
typedef struct apds_device_transport {
    void* user;
    int (*all_gather)(void* user, const void* send_dev, void* recv_dev, size_t bytes_per_rank, void* stream);
    int (*all_to_all)(void* user, const void* send_dev, const size_t* send_off, const size_t* send_bytes, void* recv_dev, const size_t* recv_off,
                      const size_t* recv_bytes, void* stream);
} apds_device_transport;
/* A fresh communicator id for `transport` (RCCL: ncclGetUniqueId; loopback: a process-unique name; host: zeros). Called by ONE rank. */
int apds_comm_id_create(int transport, apds_comm_id* id);
/* Collective. The shard lives on the calling thread's device (apds_set_device first). rows64_dev: n_rows x 64-byte rows, borrowed for
 * the life of the handle. index_base = global index of the shard's first row. id: RCCL / loopback; host: the host transport's callbacks
 * (APDS_TRANSPORT_DEVICE: a pointer to an apds_device_transport, cast). */
int apds_shard_create(void** shard, int rank, int world, int transport, const apds_comm_id* id, const apds_host_transport* host,
                      const void* rows64_dev, int64_t n_rows, uint32_t index_base);
int apds_shard_destroy(void* shard);
/* any output may be NULL; *rccl_version = ncclGetVersion() of the RCCL this library runs on */
int apds_shard_info(const void* shard, int* rank, int* world, int64_t* n_rows, uint32_t* index_base, const char** transport_name, int* rccl_version);
/* Collective: every rank's query count of one frame, as host ints (counts[world]). Synchronises `stream` on the RCCL transport. */
int apds_shard_counts(void* shard, int n_query, int* counts, void* stream);
/* Collective: out_keys_dev = n_query x k uint64 ((distance << 32) | global row; 0xFFFF... when absent) for THIS rank's queries over the
 * whole train set. counts: every rank's n_query (apds_shard_counts), or NULL to exchange them inside the call. Any k >= 1 the
 * single-device scan serves (k <= 2 tuned, above 16 in pages of 16); the exchange buffers bound it at 4096. */
int apds_shard_knn(void* shard, const void* q_rows64_dev, int n_query, const int* counts, int k, void* out_keys_dev, void* stream);
/* Strong-scaling (latency) form, SURVEY 8e's literal shape. Collective: ONE frame whose n_query queries are the same on every rank -
 * root < 0: every rank passes them (each extracted the frame itself: ~1.5 ms, no communication); root >= 0: rank `root`'s rows are broadcast
 * first, the other ranks' q_rows64_dev is ignored (n_query must still be the same number everywhere). Every rank scans its shard (1 / world of
 * the rows), the [n_query, k] key lists are ALL-GATHERED and merged by u64 min: out_keys_dev = n_query x k keys of the whole frame over the
 * whole train set on EVERY rank, equal to apds_dev_hamming_topk over the unsharded rows bit for bit. */
int apds_shard_knn_replicated(void* shard, const void* q_rows64_dev, int n_query, int root, int k, void* out_keys_dev, void* stream);
/* The same in three steps on per-frame exchange slots, for pipelines that keep two frames in flight: frame i+1's gather (collective) may be
 * issued - on another stream - before frame i's exchange_merge (collective), so it travels under frame i's scan (no collective). */
int apds_shard_slot_create(void* shard, int max_queries_per_rank, int kmax, void** slot);
int apds_shard_slot_destroy(void* shard, void* slot);
int apds_shard_gather(void* shard, void* slot, const void* q_rows64_dev, int n_query, const int* counts, void* stream);
int apds_shard_scan(void* shard, void* slot, int k, void* stream);
int apds_shard_exchange_merge(void* shard, void* slot, int k, void* out_keys_dev, void* stream);
/* SURVEY §8(b) "apds_db_create / append / shard / destroy": this rank's block of the resident keypoint table's current view (every rank
 * holds the same table and selection; rank r keeps rows [r n / world, (r + 1) n / world) of the view) as a shard; train indices stay the
 * positions in the view, i.e. what apds_db_knn_match returns. */
int apds_db_shard(void* db, int rank, int world, int transport, const apds_comm_id* id, const apds_host_transport* host, void** shard);

/* ---- the streamed frame pipeline ------------------------------------------------------------------------------------------------------
 * frame -> apds_dev_akaze_extract -> Hamming top-2 against the resident train rows -> ratio test (lib.rs:107-111) -> matched points
 * (lib.rs:161-180, the intended gather) -> find_homography_mat (mod.rs:231-259), software-pipelined over a stream of frames by host
 * threads INSIDE the library: two extraction workers on alternate frames | the match (matrix-core matcher, the default: one stream, against
 * a copy of the train rows expanded to FP4 operands once at create - 256 bytes per row on top of the caller's 64; vector-ALU matcher:
 * threshold pre-pass, main scan and record merge of consecutive frames on three streams; with a shard handle: the query gather of frame
 * i+1 issued before the key exchange of frame i) |
 * ratio filter + points + homography, each with its own HIP stream and device workspace. This is the composed path the north-star metric
 * (frames/s) is measured on; a host needs four calls. The reference chains the steps only inside unit tests (lib.rs:197-249); its
 * production caller runs extraction from a rayon pool without a lock (preprocessor/src/main.rs:227-245), which is what the workers mirror.
 * Results leave in frame order and equal, frame by frame, what the one-call entry points give (tests/cpp/pipeline_test.cpp). */
typedef struct apds_pipeline_params {
    int rows, cols, channels;   /* frame geometry: every frame of one pipeline has it (channels 1, 3 or 4) */
    int max_points;             /* <= 0: APDS_MAX_POINTS (lib.rs:12-13) */
    int n_slots;                /* frames in flight; 0 = 6 (never fewer than two per extraction worker) */
    int extract_workers;        /* host threads extracting alternate frames; 0 = 2 */
    float filter_strength;      /* Lowe ratio of get_knn_matches (lib.rs:107-111; the reference's test uses 0.3, lib.rs:222) */
    int homography_method;      /* APDS_HOMOGRAPHY_* (mod.rs:25-31) */
    double reproj_threshold;    /* <= 0: 3.0 (mod.rs:248) */
    int max_iters;              /* <= 0: 2000 (OpenCV's default) */
    double confidence;          /* outside (0, 1): 0.995 (OpenCV's default) */
    int timing;                 /* 1: HIP-event timing of the stage kernels on their launch streams (apds_pipeline_stats) */
    int match_lds_cap;          /* > 0: occupancy cap of this pipeline's scans from the first frame on (see apds_dev_match_lds_cap); 0: the starvation watch decides */
    void* match_stream;         /* optional stream for the main scan (e.g. apds_stream_create with a CU mask); NULL = the pipeline's own */
    double debug_extract_delay_ms; /* test hook: every extraction is handed on this much late (exercises the starvation watch) */
} apds_pipeline_params;
typedef struct apds_frame_result {
    int64_t frame;              /* the number apds_pipeline_submit gave the frame */
    int status;                 /* APDS_OK, or the status of the stage that failed for THIS frame (the pipeline goes on; text: apds_last_error after the poll) */
    int n_keypoints, n_matches, n_inliers;
    int homography_found;       /* 0: fewer than four matches, or no model (MatError::Empty, mod.rs:258) */
    double H[9];                /* row major, H[8] == 1 */
} apds_frame_result;
typedef struct apds_pipeline_counters {
    int64_t frames_submitted, frames_done;
    /* summed HIP-event times and launch counts since the last reset (params.timing = 1): the main scan, the threshold pre-pass, whole
     * extractions (wall span on their stream), RANSAC scoring */
    double hamming_topk_ms, hamming_topk_sample_ms, akaze_extract_ms, ransac_score_ms;
    int hamming_topk_launches, hamming_topk_sample_launches, akaze_extract_calls, ransac_score_launches;
    /* idle time of the match stream in front of each frame's main scan (the starvation watch's measurement) */
    double match_gap_mean_ms;
    int match_gaps;
    float match_gaps_first_ms[16];
    int match_lds_cap_bytes, match_lds_cap_set_at_frame;   /* 0 / -1: the watch never capped */
    float match_lds_cap_gaps_ms[6];                        /* the six gaps that made it cap */
    int extract_workers, slots, split_scan, world;
} apds_pipeline_counters;
#define APDS_PIPELINE_NOT_READY 1   /* apds_pipeline_poll: the next frame (in submission order) is not finished, or nothing is in flight */
/* The train set: db_rows64_dev = n_rows x 64-byte rows whose global indices start at index_base (one GPU), or `shard` = an apds_shard_*
 * handle (the rows arguments are then ignored; every rank must submit the same number of frames, and all collective calls of that handle
 * come from the pipeline from then on). db_kps_dev: the keypoints of ALL train rows (n_db_total x 28 bytes, indexed by global row: the
 * matched points' coordinates). Everything is borrowed until apds_pipeline_destroy and must not change meanwhile (the train rows are resident:
 * the pipeline, like a shard handle, keeps derived copies of them). The pipeline lives on the calling thread's device. */
int apds_pipeline_create(void** pipe, const void* db_rows64_dev, int64_t n_rows, uint32_t index_base, void* shard, const void* db_kps_dev, int64_t n_db_total,
                         const apds_pipeline_params* params);
/* Hands one frame over (on_device 0: host memory, uploaded by an extraction worker on its own stream - pinned memory makes the copy
 * overlap; 1: device memory) and returns at once unless every slot is in flight (then it blocks until one is free). The frame must stay
 * valid until its result has been polled. *frame_id (may be NULL) = its number, counted from 0. One submitting thread at a time. */
int apds_pipeline_submit(void* pipe, const void* frame, size_t stride_bytes, int on_device, int64_t* frame_id);
/* The next result in submission order. wait 0: APDS_PIPELINE_NOT_READY if that frame is not finished; wait 1: blocks until it is (returns
 * APDS_PIPELINE_NOT_READY only when no frame is in flight). A negative status = the pipeline itself has failed (every later call repeats it). */
int apds_pipeline_poll(void* pipe, apds_frame_result* result, int wait);
/* Counters and (params.timing) kernel times. Waits for the frames in flight to finish first. reset 1: the sums start again from zero. */
int apds_pipeline_stats(void* pipe, apds_pipeline_counters* out, int reset);
/* Drains the frames in flight, joins the workers, releases streams and buffers. */
int apds_pipeline_destroy(void* pipe);
/* The pose stage (opt-in): after the homography, each frame's ratio-filtered matches -> 2D-3D pairs (apds_dev_pnp_correspondences) ->
 * apds_dev_pnp_solver_ransac, on a stage thread and a high-priority stream of its own, so frame i's pose overlaps frame i+1's homography.
 * This is the satellite side of the mission - DB keypoint -> world point (elevationdb.rs:64-104) -> attitude by pnp_solver_ransac
 * (mod.rs:320-369) - which the reference never committed. A pipeline that does not enable it behaves as before. */
typedef struct apds_pipeline_pose_params {
    const void* db_xyz_dev;     /* n_db_total x 3 doubles (world points of every global DB row), borrowed until destroy */
    double origin[3];           /* subtracted (in double) before the f32 conversion; poses are relative to it */
    double camera_intrinsic[9]; /* row major 3x3 (homographier Cmat) */
    int method;                 /* APDS_SOLVEPNP_*; the python/Rust fronts default to EPNP as mod.rs:359 does */
    int iter_count;             /* <= 0: 100 (solvePnPRansac's default) */
    float reproj_thres;         /* <= 0: 8.0 */
    double confidence;          /* outside (0, 1): 0.99 */
} apds_pipeline_pose_params;
typedef struct apds_frame_pose {
    int64_t frame;
    int status;                 /* APDS_OK, or what apds_pnp_solver_ransac returned for this frame's correspondences
                                   (APDS_ERR_ASSERT for < 4 matches); the frame's own status if extraction/match failed */
    int found, n_correspondences, n_inliers;
    double rvec[3], tvec[3];
} apds_frame_pose;
/* Before the first submit (else APDS_ERR_BAD_ARG). Checked before any device work: a null db_xyz_dev (APDS_ERR_BAD_ARG), focal lengths that
 * are not finite and positive (APDS_ERR_BAD_ARG), a method past cv::SolvePnPMethod (APDS_ERR_NOT_IMPLEMENTED). */
int apds_pipeline_enable_pose(void* pipe, const apds_pipeline_pose_params* pose);
/* apds_pipeline_poll with the frame's pose: *pose (may be NULL) is filled when pose is enabled, zeroed (status APDS_OK, found 0) otherwise.
 * apds_pipeline_poll is this call with pose = NULL. */
int apds_pipeline_poll_pose(void* pipe, apds_frame_result* result, apds_frame_pose* pose, int wait);
/* A pipeline whose train set is selected per frame, the reference's own access path (keypointdb.rs:50-90: a frame is matched against
 * the rows its read returns, never against the whole table). One GPU. Every slot owns a view of `db` (apds_db_view_create with
 * view_capacity; six slots of full-size views are about 200 MB); the match worker runs the frame's selection on the match stream in
 * front of the scan, matches the frame against the view's rows, and the ratio filter, matched points, homography and (if enabled) pose
 * read the view's keypoints and world points by view position. Train indices never leave the library. The table is borrowed until
 * apds_pipeline_destroy and must not receive inserts meanwhile. apds_pipeline_enable_pose on such a pipeline takes db_xyz_dev == NULL
 * (anything else is APDS_ERR_BAD_ARG) and requires the table's world points to be current (APDS_ERR_BAD_ARG otherwise).
 * A frame whose view has fewer than two rows gets the status the one-call matcher gives for such a train set (APDS_ERR_ASSERT), no
 * matches and no homography; the pipeline goes on. apds_pipeline_submit on a table pipeline and apds_pipeline_submit_select on any
 * other are APDS_ERR_BAD_ARG; so are a NULL sel and a mode outside 0..2, before any device work.
 * On a FLOAT table (apds_db_create_float) this makes a float pipeline, as apds_pipeline_create_float does for a fixed train set: the
 * workers extract M-SURF rows, the matcher is APDS_PIPELINE_MATCH_L2_RATIO for life (apds_pipeline_set_matcher with anything else is
 * APDS_ERR_BAD_ARG), and each frame's train set is its slot's view through apds_db_view_l2_train: the screen's train side comes out
 * of the select's own gather. Everything else - the selections, the status of a view of fewer than two rows, pose from the view's world
 * points - is the byte table's. For both kinds, keeping inserts and deletes away from the table while a pipeline holds it is the CALLER'S
 * obligation: the library does not check it. */
typedef struct apds_db_selection {
    int mode, value;                         /* apds_db_select's: 0 image id, 1 level of detail, 2 level of detail and bounding box */
    float x_start, y_start, x_end, y_end;    /* mode 2: floor(start) <= v <= ceil(end) */
} apds_db_selection;
int apds_pipeline_create_table(void** pipe, void* db, int view_capacity, const apds_pipeline_params* params);
int apds_pipeline_submit_select(void* pipe, const void* frame, size_t stride_bytes, int on_device, const apds_db_selection* sel, int64_t* frame_id);
/* The pipeline's matcher (opt-in; a pipeline that never calls this runs the ratio matcher as before). APDS_PIPELINE_MATCH_CROSSCHECK: the
 * reference's second matcher, get_bruteforce_matches (lib.rs:116-126) - per frame ONE roles-swapped top-1 scan (the train rows search the
 * frame's descriptors; the forward k = 2 scan is not launched), and the homography stage builds its matches with the cross-check instead
 * of the ratio test: the matches of apds_dev_crosscheck_match on (frame descriptors, train set), so n_matches, the homography and the pose
 * stage work on them. filter_strength is ignored. With the matrix-core matcher the resident expanded copy of the train rows serves the
 * swapped scan as it is (only the frame's rows are expanded per frame). Every slot gets a buffer of one u64 per train row (per view row
 * on a table pipeline) here; nothing grows with the number of frames.
 * Before the first submit (else APDS_ERR_BAD_ARG); any other value APDS_ERR_BAD_ARG; APDS_PIPELINE_MATCH_CROSSCHECK on a pipeline over a
 * shard handle APDS_ERR_NOT_IMPLEMENTED - all three before any device work. One GPU and table pipelines. */
#define APDS_PIPELINE_MATCH_RATIO 0
#define APDS_PIPELINE_MATCH_CROSSCHECK 1
int apds_pipeline_set_matcher(void* pipe, int matcher);
/* The float pipeline: the same stages over M-SURF descriptors (64 x f32, apds_dev_akaze_extract_float) and the L2 matcher. db_rows_f32_dev
 * = n_rows x 64 floats (256-byte rows, 16-byte aligned, n_rows >= 2) whose global indices start at index_base; db_kps_dev / n_db_total
 * as apds_pipeline_create takes them. The extraction workers fill slot buffers of 256 bytes per row, the match worker calls
 * apds_dev_l2_train_top2 on a train set made here and released by apds_pipeline_destroy, the homography stage builds its matches with
 * apds_dev_l2_ratio_filter (filter_strength on the distances, not their squares); matched points, homography, pose and lens are unchanged.
 * Its matcher is APDS_PIPELINE_MATCH_L2_RATIO from birth: apds_pipeline_set_matcher with any other value on a float pipeline, and with
 * this value on a byte-row pipeline, is APDS_ERR_BAD_ARG before any device work. One GPU, a fixed train set: there is no float constructor
 * over a shard handle or a table. The starvation watch and the LDS cap belong to the Hamming scan and stay off. The match runs the
 * bf16 screen (measured 5x faster than the exact kernel on M-SURF rows; the keys are the same). */
#define APDS_PIPELINE_MATCH_L2_RATIO 2
int apds_pipeline_create_float(void** pipe, const void* db_rows_f32_dev, int64_t n_rows, uint32_t index_base, const void* db_kps_dev, int64_t n_db_total,
                               const apds_pipeline_params* params);
/* The pipeline's lens (opt-in; a pipeline that never calls this, or calls it with no distortion, issues the launches it issued before).
 * The image-side matched points of every frame are undistorted on the device (apds_dev_undistort_points, stride 8, `iters` steps, <= 0: 5)
 * on the stage's own stream, with nothing more synchronised with the host: in the homography stage right after the matched-points gather
 * and in front of the estimator (reproj_threshold is then in undistorted pixels); in the pose stage on img_xy right after
 * apds_dev_pnp_correspondences. Only the matches are touched: the frame's keypoints, the match lists and every counter stay as they are.
 * The pose stage keeps solving with apds_pipeline_pose_params.camera_intrinsic: the two K are expected to be the same matrix.
 * Before the first submit (else APDS_ERR_BAD_ARG); the lens arguments are checked as apds_undistort_points checks them, before any device
 * work. Plain, table and shard pipelines. */
int apds_pipeline_set_lens(void* pipe, const double* K, const double* dist, int n_dist, int iters);

/* ---- device-resident API ------------------------------------------------------------------- */
/* All pointers below are HIP device pointers. stream: hipStream_t or NULL (the thread's own stream).
 * Calls are asynchronous on that stream unless they return a count to the host; apds_dev_akaze_extract(_batch) returns as soon as the
 * count is known, with the orientation / descriptor kernels still queued on the stream: consumers order themselves on that stream (or an
 * event recorded on it), as with any asynchronous call.
 * Scratch: the matchers, the filters, the estimators and the extraction keep their scratch in the CALLING THREAD's workspace, which every
 * such call re-uses from its start. One host thread may nevertheless issue them on different streams without synchronising in between:
 * a call that returns with work queued leaves an event behind it, and the thread's next call makes its own stream wait for that event on
 * the device when it is another stream (no host block; nothing at all while the thread stays on one stream). The outputs are not covered:
 * they are the caller's buffers, ordered by the caller. A stream must outlive the work queued on it. */

/* Pack n rows of desc_bytes (<= 64) bytes into 64-byte rows (zero padded). */
int apds_dev_pack_descriptors(const void* src_rows, int64_t n, int desc_bytes, int64_t src_stride, void* dst_rows64, void* stream);

/* Hamming top-k (k >= 1) of n_query rows against n_train rows, both 64-byte pitch. k in {1, 2} - all that lib.rs:94-126 consumes - runs on
 * the FP4 matrix pipe (bits as e2m1 operands, exact integer distances; the train rows are expanded to 256-byte operand rows in the calling
 * thread's workspace per call - apds_dev_match_backend), and so does 3 <= k <= APDS_MATCH_MFMA_KMAX (2, 4 or 8, default 8: the same kernel
 * around a sorted list of 4 or 8 entries per query, same expansion and workspace footprint); every other k on the vector ALU, above 16 one
 * pass per 16 neighbours.
 * out_keys: n_query*k uint64 = (distance << 32) | (train_index + index_base), ascending; 0xFFFF... when absent.
 * Ordering equals BFMatcher's: by distance, ties to the lower train index. */
int apds_dev_hamming_topk(const void* query_rows64, int n_query, const void* train_rows64, int64_t n_train,
                          uint32_t index_base, int k, void* out_keys, void* stream);
/* apds_dev_hamming_topk in three separately launched steps (k = 1 or 2), for pipelines that keep several frames in flight: the threshold
 * pre-pass over the first train rows, the main scan, and the merge of its per-chunk records. The intermediate buffers live in a state
 * object (one per frame in flight; grow-only device memory) instead of the calling thread's workspace, so frame i + 1's pre-pass may run
 * on another stream while frame i's scan is on the GPU. Order per frame: prepass -> scan -> merge, each after the previous one on the GPU
 * (same stream, or events); q / t / n as given to the pre-pass must stay valid until the merge has run. Result == apds_dev_hamming_topk. */
int apds_dev_topk_state_create(void** state);
int apds_dev_topk_state_destroy(void* state);
int apds_dev_topk_prepass(void* state, const void* query_rows64, int n_query, const void* train_rows64, int64_t n_train, uint32_t index_base, int k,
                          void* stream);
int apds_dev_topk_scan(void* state, const void* query_rows64, const void* train_rows64, void* stream);
int apds_dev_topk_merge(void* state, uint32_t index_base, void* out_keys, void* stream);
/* Merge `parts` candidate lists (each n_query*k keys, e.g. gathered from DB shards) into the global top-k. */
int apds_dev_merge_topk(const void* keys_parts, int parts, int n_query, int k, void* out_keys, void* stream);
/* Occupancy cap of the main Hamming scan, process-wide: the kernel requests `bytes` of (unused) dynamic LDS per workgroup, which bounds
 * the workgroups resident per CU (160 KB / bytes; 55000 -> two). A pipeline that overlaps the scan with short kernels of other stages
 * sets it when those kernels cannot get onto the GPU (the scan alone is ~1.5 % slower with the cap). 0 = none (default, or
 * APDS_MATCH_LDS_CAP). The value is process-wide: a caller that sets it for its own launches restores *previous afterwards. *previous (may be NULL) receives the old value. */
int apds_dev_match_lds_cap(int bytes, int* previous);
/* Test hook: the dynamic-LDS request of the most recent scan launch of the process (-1 before the first); equals the cap in force for
 * every kernel variant (all tile widths, all k, persistent grid). */
int apds_dev_match_last_launch_lds(int* bytes);
/* apds_dev_hamming_topk on a named backend, whatever APDS_MATCH_MFMA says: 0 = the configured one, 1 = vector ALU (xor + popcount,
 * any k), 2 = matrix cores (k <= 2; APDS_ERR_ASSERT above), 3 = matrix cores (k <= 8: k <= 2 as backend 2, 3 <= k <= 8 on
 * hamming_mfma_topk_kernel; APDS_ERR_ASSERT above 8). The keys are the same bit for bit; bench.py times backends 1 and 2 in one run, the
 * tests compare 1 with 2 and 1 with 3 in one process, tools/topk_mfma_probe.py times 1 against 3. */
int apds_dev_hamming_topk_backend(const void* query_rows64, int n_query, const void* train_rows64, int64_t n_train, uint32_t index_base, int k,
                                  void* out_keys, int backend, void* stream);
/* Which kernel serves k <= 2 (everything lib.rs:94-126 consumes): *matrix_cores = 1: hamming_mfma_kernel - bits as FP4 (e2m1) operands of
 * v_mfma_scale_f32_16x16x128_f8f6f4, exact integer distances (default); 0: hamming_topk_kernel, xor + popcount on the vector ALU
 * (APDS_MATCH_MFMA=0; also what serves every k > APDS_MATCH_MFMA_KMAX). With the matrix cores on, 3 <= k <= APDS_MATCH_MFMA_KMAX run on
 * hamming_mfma_topk_kernel (timed as "hamming_topk" and "hamming_topk_mfma_k": apds_dev_last_kernel_ms). The keys are the same bit for bit. */
int apds_dev_match_backend(int* matrix_cores);
/* Lowe ratio filter on merged keys (k >= 2): writes compacted matches in query order, count to *n_matches (host). */
int apds_dev_ratio_filter(const void* keys, int n_query, int k, float filter_strength, void* out_matches, int* n_matches, void* stream);
/* The same on the keys of the L2 matchers (apds_dev_l2_topk, apds_dev_l2_train_top2: f32 bits of d^2 << 32 | row): the distances are
 * sqrtf(d^2), the values apds_l2_knn_match returns; a query is kept iff both keys are present and d0 < d1 * filter_strength in f32;
 * distance = d0, train_idx = the key's row. The matches of get_knn_matches_l2, record for record, in query order. */
int apds_dev_l2_ratio_filter(const void* keys, int n_query, int k, float filter_strength, void* out_matches, int* n_matches, void* stream);
/* Cross-check: given for every train row its best query key (from apds_dev_hamming_topk with roles swapped, k=1),
 * produce matches in query order. */
int apds_dev_cross_check(const void* train_best_keys, int64_t n_train, int n_query, void* out_matches, int* n_matches, void* stream);
/* apds_get_bruteforce_matches on device rows (BFMatcher(NORM_HAMMING, crossCheck = true), lib.rs:116-126) in one call: every train row
 * finds its nearest query (ties to the lower query index), every query keeps the closest train row that chose it (ties to the lower
 * train index), queries nobody chose are dropped. out_matches: room for n_query 16-byte matches, written in query order with
 * train_idx = row + index_base; *n_matches (host) = their count. An empty side gives zero matches and APDS_OK; n_train above INT_MAX is
 * APDS_ERR_ASSERT (the train rows are the searching side of the scan). Synchronises the stream once, for the count. */
int apds_dev_crosscheck_match(const void* query_rows64, int n_query, const void* train_rows64, int64_t n_train, uint32_t index_base, void* out_matches,
                              int* n_matches, void* stream);

/* AKAZE on a device image. Results stay on the device: kps (capacity x 28 B), desc64 (capacity x 64 B).
 * Returns the keypoint count in *n (host). capacity >= min(max_points, APDS_MAX_POINTS). */
int apds_dev_akaze_extract(const void* img, int rows, int cols, int channels, size_t stride_bytes, int max_points,
                           void* kps, void* desc64, int capacity, int* n, void* stream);
/* Batched form on device images: image i's keypoints land at kps + i * capacity rows, its descriptors at desc64 + i * capacity * 64 bytes,
 * its count in counts[i] (host). capacity (rows per image) >= the largest count. */
int apds_dev_akaze_extract_batch(const void* imgs, int n_images, size_t image_stride_bytes, int rows, int cols, int channels, size_t stride_bytes,
                                 int max_points, void* kps, void* desc64, int capacity, int* counts, void* stream);
/* The two calls above with a detection mask on the device (the rule of apds_akaze_extract_masked): mask_dev = rows x cols u8,
 * mask_stride_bytes between rows (< cols: APDS_ERR_ASSERT); NULL = unmasked. Batch: image i's mask starts i * mask_image_stride_bytes after
 * mask_dev, 0 = one mask shared by every image. counts and capacity are about the survivors: capacity >= the largest masked count. */
int apds_dev_akaze_extract_masked(const void* img, int rows, int cols, int channels, size_t stride_bytes, const void* mask_dev, size_t mask_stride_bytes,
                                  int max_points, void* kps, void* desc64, int capacity, int* n, void* stream);
int apds_dev_akaze_extract_batch_masked(const void* imgs, int n_images, size_t image_stride_bytes, int rows, int cols, int channels, size_t stride_bytes,
                                        const void* mask_dev, size_t mask_stride_bytes, size_t mask_image_stride_bytes, int max_points, void* kps, void* desc64,
                                        int capacity, int* counts, void* stream);
/* ... and with a mask support (the rule of apds_akaze_extract_masked_support; 0 = the two calls above, negative: APDS_ERR_BAD_ARG) */
int apds_dev_akaze_extract_masked_support(const void* img, int rows, int cols, int channels, size_t stride_bytes, const void* mask_dev, size_t mask_stride_bytes,
                                          int mask_support, int max_points, void* kps, void* desc64, int capacity, int* n, void* stream);
int apds_dev_akaze_extract_batch_masked_support(const void* imgs, int n_images, size_t image_stride_bytes, int rows, int cols, int channels, size_t stride_bytes,
                                                const void* mask_dev, size_t mask_stride_bytes, size_t mask_image_stride_bytes, int mask_support, int max_points,
                                                void* kps, void* desc64, int capacity, int* counts, void* stream);
/* The two calls above with float descriptors (APDS_AKAZE_DESCRIPTOR_KAZE: see apds_akaze_extract_float): desc_f32 = capacity rows of 64
 * packed floats (256 bytes) per image, which is what apds_dev_l2_topk takes with dim = 64. kps, counts, capacity, mask and stream as above. */
int apds_dev_akaze_extract_float(const void* img, int rows, int cols, int channels, size_t stride_bytes, const void* mask_dev, size_t mask_stride_bytes,
                                 int mask_support, int max_points, void* kps, void* desc_f32, int capacity, int* n, void* stream);
int apds_dev_akaze_extract_float_batch(const void* imgs, int n_images, size_t image_stride_bytes, int rows, int cols, int channels, size_t stride_bytes,
                                       const void* mask_dev, size_t mask_stride_bytes, size_t mask_image_stride_bytes, int mask_support, int max_points,
                                       void* kps, void* desc_f32, int capacity, int* counts, void* stream);
/* The float describe stage alone, on a caller-supplied plane (what the tests of the kernel stand on): lxy_dev = h x w interleaved (Lx, Ly)
 * f32, one level; kps_dev: n apds_keypoint whose class_id is ignored (the plane IS the level), octave / size / angle / x / y used as
 * described at apds_akaze_extract_float; desc_f32_dev: n x 64 floats. n == 0 is a no-op; asynchronous on `stream`. */
int apds_dev_akaze_describe_float(const void* lxy_dev, int w, int h, const void* kps_dev, int n, void* desc_f32_dev, void* stream);
/* The table behind the mask support, on its own: out_u32_dev[y][x], (rows + 1) x (cols + 1) u32, = the number of zero mask bytes in rows < y
 * and columns < x (exact). mask_dev: rows x cols bytes, row_stride_bytes between rows and pix_stride_bytes between the pixels of a row (1: a
 * plane; 4 with mask_dev = image + 3: the alpha of a BGRA image, read as the aligned 4-byte words that hold the bytes). Sides 1 .. 65535. */
int apds_dev_mask_zero_sat(const void* mask_dev, int rows, int cols, size_t row_stride_bytes, size_t pix_stride_bytes, void* out_u32_dev, void* stream);

/* gather matched coordinates on the device: pts1/pts2 n_matches x 2 float */
int apds_dev_points_from_matches(const void* kp1, int n1, const void* kp2, int n2, const void* matches, int n_matches,
                                 int bug_compatible, void* pts1, void* pts2, void* stream);

/* RANSAC / LMEDS / least-squares homography on device point lists. H (9 doubles) and found flag go to the host. */
int apds_dev_find_homography(const void* input_xy, const void* reference_xy, int n, int method, double reproj_threshold,
                             int max_iters, double confidence, double* H, void* mask_dev, void* stream);

/* Streams for callers that overlap stages. cu_mask (optional): bit i set = compute unit i may run the stream's kernels
 * (hipExtStreamCreateWithCUMask); priority 0 normal, -1 high (ignored when a mask is given). */
int apds_stream_create(int priority, const uint32_t* cu_mask, int cu_mask_words, void** stream);
int apds_stream_destroy(void* stream);

/* Device memory and copies on the calling thread's device, so that a host which keeps buffers resident (apds_dev_*, apds_shard_*) needs
 * no HIP binding of its own. upload is asynchronous on `stream` (the host buffer must stay valid until the stream has passed it; pinned
 * memory makes it a true async copy); download returns when the bytes are in dst_host. stream NULL = the thread's own stream. */
int apds_dev_alloc(size_t bytes, void** ptr);
int apds_dev_release(void* ptr);
int apds_dev_upload(void* dst_dev, const void* src_host, size_t bytes, void* stream);
int apds_dev_download(void* dst_host, const void* src_dev, size_t bytes, void* stream);
int apds_stream_synchronize(void* stream);

/* Releases the calling thread's HIP stream and device workspace (they are created lazily by the first call on a thread and
 * otherwise live as long as the thread; nothing is freed from thread-exit destructors, which may run after the HIP runtime has
 * shut down). Call it before a worker thread that used the library exits; the thread may use the library again afterwards. */
int apds_thread_release(void);
/* Host threads that currently hold a library context (stream + workspace): a lone caller lets the extraction use side streams
 * (apds_dev_akaze_extract forks its Hessian kernels only then). Diagnostic. */
int apds_live_contexts(void);
/* apds_thread_release keeps the thread's device workspace in a process-wide cache (a later thread reuses it instead of allocating);
 * this frees everything in that cache. */
int apds_release_cached_memory(void);
/* The device workspaces of the process: *slab_bytes = bytes held right now by every thread's workspace and by the cache above,
 * *slab_allocations = device allocations made for them since the library was loaded (either may be NULL). A steady state allocates
 * nothing: both figures stand still over any number of calls of the same shapes. Diagnostic; no device work. */
int apds_workspace_info(int64_t* slab_bytes, int64_t* slab_allocations);

/* Test hook: run apds_akaze_extract and copy one intermediate plane of evolution level `level` to out_plane
 * (which: 0 Lt, 2 Lx, 3 Ly, 4 Ldet as f32 w*h; 7 keypoint mask after cross-level suppression as u8 w*h; 8 contrast factor, 1 float). */
int apds_akaze_debug_plane(const uint8_t* img, int rows, int cols, int channels, size_t stride_bytes, int level, int which, void* out_plane);

/* Test hook: the pose (rvec, tvec: 6 doubles per sample) of n_samples explicit samples as the RANSAC kernels compute them:
 * model_points 5 = EPnP on 5 correspondences, 4 = P3P on 4 (three solve, the fourth ranks; NaNs when there is no pose), 40 = AP3P on 4. */
int apds_pnp_hypotheses(const double* obj_xyz, const double* img_xy, int n, const double* camera_intrinsic, const int32_t* samples, int n_samples,
                        int model_points, double* models);

/* Test hook: cv::solvePnP(..., SOLVEPNP_SQPNP) alone on n >= 3 correspondences - the final pose apds_pnp_solver_ransac computes over
 * its inliers when the caller names APDS_SOLVEPNP_SQPNP (mod.rs:327,359). Host arithmetic only: one 9 x 9 problem per call whatever n.
 * *found = 0: no pose (degenerate points, or none in front of the camera). */
int apds_pnp_sqpnp(const double* obj_xyz, const double* img_xy, int n, const double* camera_intrinsic, double* rvec, double* tvec, int* found);
/* Test hook: cv::solvePnP(..., SOLVEPNP_IPPE) alone on n >= 4 correspondences (host arithmetic); *found = 0: the object points are not coplanar. */
int apds_pnp_ippe(const double* obj_xyz, const double* img_xy, int n, const double* camera_intrinsic, double* rvec, double* tvec, int* found);

/* Measurement helpers used by bench.py (not part of the reference surface). */
/* Register-only xor+popcount loop: returns measured lane-ops/s (32-bit xor + bcnt counted as 2 ops). */
int apds_dev_valu_popcount_peak(double* lane_ops_per_s);
/* Calibration of that denominator: the same register-only loop with ONE instruction kind (`mode`, 0 <= mode < apds_dev_valu_peak_modes():
 * integer xor / bcnt / add / and / xor3 and FP32 fma / add / mul / pk_fma / pk_add; *name = the mnemonic) at `waves_per_simd` (1..8) resident
 * waves per SIMD. Returns wall-clock lane-ops/s (a packed instruction counts two) and s_memtime cycles per wave-instruction per SIMD. */
int apds_dev_valu_peak(int mode, int waves_per_simd, double* lane_ops_per_s, double* cycles_per_inst, const char** name);
int apds_dev_valu_peak_modes(void);
/* Time of the last hamming_topk main kernel launched by this thread, measured with hipEvents on its stream (ms). */
int apds_dev_last_kernel_ms(const char* which, float* ms, int* launches);
int apds_dev_timing_enable(int on);

#ifdef __cplusplus
}
#endif
#endif /* APDS_H */
