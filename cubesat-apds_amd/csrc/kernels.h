// csrc/kernels.h — host-callable launchers implemented in the .hip files.
#pragma once
#include <atomic>
#include "common.h"
#include "lens_core.h"

namespace apds {

// match_hamming.hip: Hamming top-k keys (topk_keys.h) on the vector ALU, and the front of both Hamming backends
// backend: 0 = the configured one (APDS_MATCH_MFMA, APDS_MATCH_MFMA_KMAX), 1 = vector ALU (hamming_topk_kernel), 2 = matrix cores (hamming_mfma_kernel, k <= 2),
// 3 = matrix cores (k <= 2 as backend 2; 3 <= k <= 8: hamming_mfma_topk_kernel)
void hamming_topk_device(const void* q, int nq, const void* t, long long nt, uint32_t index_base, int k, uint64_t* out, hipStream_t s, int backend = 0);
// the scan of hamming_topk_device in three separately launched steps on a per-frame state object (k = 1, 2)
void* topk_split_create();
void topk_split_destroy(void* state);
void topk_split_prepass(void* state, const void* q, int nq, const void* t, long long nt, uint32_t index_base, int k, hipStream_t s);
void topk_split_scan(void* state, const void* q, const void* t, hipStream_t s);
void topk_split_merge(void* state, uint32_t index_base, uint64_t* out, hipStream_t s);
void topk_split_use_train(void* state, const void* hm_train);   // a pre-expanded train set for the state's matrix-core scans (or null)
void pack_rows_device(const void* src, long long n, int desc_bytes, long long src_stride, void* dst, hipStream_t s);
std::atomic<int>& match_lds_cap();   // occupancy cap of the main Hamming scan
std::atomic<int>& last_scan_launch_lds();
void set_thread_scan_cap(int bytes);   // occupancy cap of the scans THIS thread launches (-1: the process-wide one)

// topk_merge.hip: [parts][nq][k] sorted key lists -> the k smallest per query; the first kout of kin columns
void merge_topk_device(const uint64_t* parts, int nparts, int nq, int k, uint64_t* out, hipStream_t s);
void take_first_columns_device(const uint64_t* in, int nq, int kin, int kout, uint64_t* out, hipStream_t s);

// hamming_mfma.hip: the same keys for 1 <= k <= 8 from the FP4 matrix pipe (bit -> e2m1 operand, exact). The kernels keep a sorted list of
// K = 2, 4 or 8 entries per query (the smallest that holds k); hm_plan / hm_scan_device take that K (default: the top-2 kernel)
void hamming_mfma_topk_device(const void* q, int nq, const void* t, long long nt, uint32_t index_base, int k, uint64_t* out, hipStream_t s);
struct HmPlan {
    int q_tiles, splits, tiles_per_split;
};
struct HmTrain {   // a train set expanded once (256 bytes of fp4 operands per row + popcounts), in device memory of its own
    int device = 0;
    const void* src = nullptr;
    long long n = 0;
    void* rows = nullptr;
    float* pc = nullptr;
};
HmPlan hm_plan(int nq, long long nt, int K = 2);
long long hm_padded_rows(long long n);   // expanded train rows and their popcounts are padded to whole tiles: allocate this many rows / floats
void hm_expand_device(const void* rows64, long long n, bool query, void* out_fp4, float* pc, hipStream_t s);
void hm_scan_device(const void* q_fp4, const float* qpc, int nq, const void* t_fp4, const float* tpc, long long nt, const HmPlan& p, uint32_t index_base,
                    uint64_t* parts, hipStream_t s, const uint32_t* thr = nullptr, bool timed = true, int K = 2);
long long hm_sample_rows(long long nt);
void* hm_train_create(const void* rows64, long long n, hipStream_t s);
void hm_train_destroy(void* train);
void hamming_mfma_topk_train_device(const void* q, int nq, const void* train, uint32_t index_base, int k, uint64_t* out, hipStream_t s);
// the cross-check's roles-swapped top-1 with an expanded train set as the searching side: train_best[row] = (distance << 32 | nearest of the
// n rows); train_plain_pc: hm_train_plain_popcounts_device's output (the train rows' popcounts without the bias, made once per train set)
void hm_train_plain_popcounts_device(const void* train, float* out, hipStream_t s);
void hamming_mfma_swapped_top1_device(const void* rows64, int n, const void* train, const float* train_plain_pc, uint64_t* train_best, hipStream_t s);

// match_filter.hip: ratio test, cross-check, ordered compaction
int* scan_flags_device(const uint8_t* flags, int n, int** total_dev, hipStream_t s);
int ratio_filter_device(const uint64_t* keys, int nq, int k, float fs, apds_dmatch* out, hipStream_t s);
int cross_check_device(const uint64_t* train_best, long long n_train, int nq, apds_dmatch* out, hipStream_t s);
int cross_check_base_device(const uint64_t* train_best, long long n_train, int nq, uint32_t index_base, apds_dmatch* out, hipStream_t s);   // train_idx = row + index_base

// valu_peak.hip
double valu_popcount_peak_device();
int valu_peak_modes();
const char* valu_peak_mode_name(int mode);
void valu_peak_device(int mode, int waves_per_simd, double* lane_ops_per_s, double* cycles_per_inst);

// akaze_extract.hip (the launchers of its stages: akaze.h). pmask: the detection mask (common.h; a null base = none)
// mask_support (>= 0): the mask is consulted on the square of mask_support descriptor units around the keypoint (0: its own pixel)
// descriptor: APDS_AKAZE_DESCRIPTOR_MLDB (rows of 64 bytes at `desc`) or APDS_AKAZE_DESCRIPTOR_KAZE (rows of 64 floats = 256 bytes)
int akaze_extract_device(const void* img, int rows, int cols, int channels, size_t stride, const PixelMask& pmask, int mask_support, int max_points,
                         apds_keypoint* kps, uint8_t* desc, int capacity, hipStream_t s, int descriptor = APDS_AKAZE_DESCRIPTOR_MLDB);
int akaze_extract_batch_device(const void* img, int n_img, size_t img_bstride, int rows, int cols, int channels, size_t stride, const PixelMask& pmask,
                               int mask_support, int max_points, apds_keypoint* kps, uint8_t* desc, int capacity, int* counts, hipStream_t s,
                               int descriptor = APDS_AKAZE_DESCRIPTOR_MLDB);

// misc.hip
void points_from_matches_device(const apds_keypoint* kp1, int n1, const apds_keypoint* kp2, int n2, const apds_dmatch* m, int nm,
                                int bug_compatible, float* pts1, float* pts2, int* err_flag, hipStream_t s);
void rgba_to_bgra_device(const uint8_t* rgba, size_t n_pixels, uint8_t* bgra, hipStream_t s);
int count_nonzero_device(const uint8_t* bytes, int n, int* count_dev, hipStream_t s);   // synchronises s

// ingest.hip
void band_merger_device(const float* r, const float* g, const float* b, size_t n, const double* mm, int bgra, uint8_t* out, hipStream_t s);
void warp_perspective_device(const uint8_t* src, int rows, int cols, const double* M, int dst_rows, int dst_cols, uint8_t* dst, hipStream_t s);
void warp_perspective_any_device(const void* src, int rows, int cols, int channels, int elem_bytes, const double* M, int dst_rows, int dst_cols, void* dst,
                                 hipStream_t s);
int world_coordinates_device(const double* xy, int n, const double* dgt_host, const double* egt_host, const double* elev, int ew, int eh, double* xyz,
                             hipStream_t s);
int64_t world_coordinates_columns_device(const float* x, const float* y, int n, const double* dgt_host, const double* egt_host, const double* elev, int ew,
                                         int eh, double* xyz, hipStream_t s);   // x, y: device f32 columns; returns the number of missed lookups

// lens.hip (the model: lens_core.h). lens_from_args: every argument check of a (K, dist, n_dist) triple, before any device work; returns
// whether the lens distorts at all. points_f64: iters 0 = forward model, >= 1 = that many inverse steps. points_host: host arrays through
// the calling thread's workspace (not reset), synchronises s. undistort_points_f32: in place on f32 pairs every stride_bytes, no workspace.
bool lens_from_args(const double* K, const double* dist, int n_dist, lens::Lens* out);
void lens_points_f64_device(const double* xy_dev, int n, const lens::Lens& L, int iters, double* out_dev, hipStream_t s);
void lens_points_host(const double* xy, int n, const lens::Lens& L, int iters, double* out, hipStream_t s);
void lens_undistort_points_f32_device(void* xy_dev, int n, size_t stride_bytes, const lens::Lens& L, int iters, hipStream_t s);
void undistort_image_device(const uint8_t* src, int rows, int cols, int channels, const lens::Lens& L, const double* new_K, uint8_t* dst, hipStream_t s);

// keypoint_table.hip: the device a table lives on; n_tiles tiles of an extraction's device output (tile i at i * capacity rows) appended in
// tile order by one launch on s (checks first, then writes; takes its small tile table from the calling thread's workspace WITHOUT
// resetting it; synchronises s)
int table_device(const void* db);
int table_descriptor(const void* db);   // APDS_AKAZE_DESCRIPTOR_MLDB (64-byte rows) or APDS_AKAZE_DESCRIPTOR_KAZE (rows of 64 floats): the rows the inserts take
void table_insert_batch_device(void* db, const void* kps_dev, const void* desc64_dev, int n_tiles, int capacity, const int32_t* counts, int first_image_id,
                               int lod, const uint32_t* columns_rows, uint64_t tile_w, uint64_t tile_h, hipStream_t s);

// mosaic.hip: the mosaic resident in HBM (apds_mosaic_*). check_window throws what the entry points report for windows of the raster of
// `level` (0: the base raster); read_device writes out[band][tile][out_h][out_w] f32 (the layout band_merger_device reads a batch in) and
// returns when the kernels are done: the base-raster windows themselves, or, on a handle with overviews, their image on the level GDAL
// would serve the read from.
struct Mosaic;
int mosaic_device(const Mosaic* m);   // the device the handle's raster lives on
void mosaic_check_window(const Mosaic* m, int level, const int32_t* xy0, int n_tiles, int win_w, int win_h, int out_w, int out_h, int resample);
void mosaic_read_device(const Mosaic* m, const int32_t* xy0, int n_tiles, int win_w, int win_h, int out_w, int out_h, int resample, float* out, hipStream_t s);
void mosaic_min_max(Mosaic* m, double* minmax6);   // cached in the handle; resets the calling thread's workspace when it computes

// homography.hip (the refit it drives: homography.h, homography_refit.hip)
int find_homography_device(const float* src, const float* dst, int n, int method, double thr, int max_iters, double confidence,
                           double* H_host, uint8_t* mask_dev, hipStream_t s);

// l2_match.hip / l2_screen.hip
void l2_row_norms_device(const float* x, long long n, int dim, float* out, hipStream_t s);
void l2_topk_device(const float* q, int nq, const float* t, long long nt, int dim, uint32_t index_base, int k, uint64_t* out, hipStream_t s);
bool l2_topk_screen_device(const float* q, int nq, const float* t, long long nt, int dim, uint32_t index_base, int k, uint64_t* out, hipStream_t s,
                           double* candidates_per_query);
// a resident L2 train set (apds_l2_train_*): the rows are borrowed; the norms, the bf16 copy scaled by -2 and the largest norm are made
// once at create and owned by the handle (the bf16 copy and the largest norm only where the screen applies: screen_ready)
struct L2Train {
    int device = 0;
    const float* rows = nullptr;
    long long n = 0;
    int dim = 0;
    uint32_t index_base = 0;
    bool screen_ready = false;
    float* norms = nullptr;          // n floats: row_norms_kernel's values
    uint16_t* rows_bf = nullptr;     // n x dim bf16 of -2 * row (screen_ready)
    unsigned int* tmax_bits = nullptr;   // bits of the largest |t|^2 (screen_ready)
    bool borrowed = false;               // a member of a table view (apds_db_view_l2_train): its buffers are the view's, apds_l2_train_destroy refuses it
};
L2Train* l2_train_create(const float* t, long long nt, int dim, uint32_t index_base, hipStream_t s);   // synchronises s
void l2_train_destroy(L2Train* set);
// both: top-2 keys of q against the set; the exact one is l2_topk_device's launch on the handle's norms. The screen returns false where
// it could not be used (handle not screen_ready, misaligned q, candidate overflow): the caller resets the workspace and runs the exact one
void l2_train_top2_exact_device(const L2Train* set, const float* q, int nq, uint64_t* out, hipStream_t s);
bool l2_train_top2_screen_device(const L2Train* set, const float* q, int nq, uint64_t* out, hipStream_t s, double* candidates_per_query);
// match_filter.hip: the ratio test on L2 keys (distances sqrtf(d^2), compared in f32), compacted in query order
int l2_ratio_filter_device(const uint64_t* keys, int nq, int k, float fs, apds_dmatch* out, hipStream_t s);

// homography_rho.hip
int find_homography_rho_device(const float* src, const float* dst, int n, double thr, int max_iters, double confidence, double* H_host, uint8_t* mask_dev,
                               hipStream_t s);

// pnp.hip
int pnp_ransac_device(const double* obj_xyz, const double* img_xy, int n, const double* K, int iterations, float reproj_thr, double confidence, int method,
                      double* rvec, double* tvec, int32_t* inliers, int* n_inliers, hipStream_t s);
// the RANSAC loop on float correspondences already on the device (pnp_ransac_device is its host-array front); inliers may be null
int pnp_ransac_core(const float* obj_dev, const float* img_dev, int n, const double* K, int iterations, float reproj_thr, double confidence, int method,
                    double* rvec, double* tvec, int32_t* inliers, int* n_inliers, hipStream_t s);
int pnp_checked_method(int n, int method);   // APDS_ERR_ASSERT for n < 4, APDS_ERR_NOT_IMPLEMENTED past cv::SolvePnPMethod; DLS / UPNP -> EPNP
void pnp_correspondences_device(const apds_keypoint* kps, int n_kps, const double* db_xyz, long long n_db, const double* origin, const apds_dmatch* m, int nm,
                                float* img_xy, float* obj_xyz, int* err_flag, hipStream_t s);
void pnp_hypotheses_device(const double* obj_xyz, const double* img_xy, int n, const double* K, const int32_t* idx5, int B, int model_points,
                           double* models_host, hipStream_t s);
int pnp_ippe_host(const double* obj_xyz, const double* img_xy, int n, const double* K, double* rvec, double* tvec);
int pnp_sqpnp_host(const double* obj_xyz, const double* img_xy, int n, const double* K, double* rvec, double* tvec);

}  // namespace apds
