"""ctypes binding of libapds_hip.so (C ABI: include/apds.h). Fails loudly when the library is missing."""
import ctypes as C
import os
import sys
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("APDS_LIB_PATH") or os.path.join(_HERE, "libapds_hip.so")   # (override: A/B runs of differently built libraries)
_LIB = None

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])
DMATCH_DTYPE = np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("img_idx", "<i4"), ("distance", "<f4")])
assert KEYPOINT_DTYPE.itemsize == 28 and DMATCH_DTYPE.itemsize == 16

ERR_INTERNAL, ERR_NOMEM, ERR_BAD_ARG, ERR_NO_DEVICE, ERR_OUT_OF_RANGE, ERR_ASSERT, ERR_EMPTY = -2, -4, -5, -216, -211, -215, -1000
ERR_NOT_IMPLEMENTED = -213
PIPELINE_MATCH_RATIO, PIPELINE_MATCH_CROSSCHECK = 0, 1   # apds_pipeline_set_matcher
PIPELINE_MATCH_L2_RATIO = 2                              # a float pipeline's matcher (apds_pipeline_create_float), from birth
PIPELINE_MATCHERS = {"ratio": PIPELINE_MATCH_RATIO, "crosscheck": PIPELINE_MATCH_CROSSCHECK, "l2": PIPELINE_MATCH_L2_RATIO}
L2_EXACT, L2_SCREEN = 0, 1                               # APDS_L2_*: the arithmetic of the float top-2
L2_MODES = {"exact": L2_EXACT, "screen": L2_SCREEN}
ERR_NOT_IMPLEMENTED = -213

# every symbol include/apds.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "apds_last_error", "apds_free", "apds_device_count", "apds_set_device", "apds_build_info", "apds_thread_release", "apds_live_contexts", "apds_release_cached_memory",
    "apds_akaze_extract", "apds_akaze_extract_batch", "apds_dev_akaze_extract_batch", "apds_tile_extract", "apds_tile_extract_batch", "apds_get_knn_matches", "apds_get_bruteforce_matches", "apds_knn_match",
    "apds_get_points_from_matches", "apds_find_homography", "apds_find_homography_ex", "apds_raster_to_mat",
    "apds_dev_pack_descriptors", "apds_dev_hamming_topk", "apds_dev_merge_topk", "apds_dev_match_lds_cap", "apds_dev_match_last_launch_lds", "apds_dev_match_backend", "apds_dev_hamming_topk_backend", "apds_dev_ratio_filter",
    "apds_dev_cross_check", "apds_dev_akaze_extract", "apds_dev_points_from_matches", "apds_dev_find_homography",
    "apds_dev_valu_popcount_peak", "apds_dev_valu_peak", "apds_dev_valu_peak_modes", "apds_dev_last_kernel_ms", "apds_dev_timing_enable", "apds_akaze_debug_plane", "apds_stream_create", "apds_stream_destroy",
    "apds_band_merger", "apds_dev_band_merger", "apds_warp_perspective", "apds_warp_perspective_f32", "apds_pnp_solver_ransac", "apds_dev_pnp_solver_ransac", "apds_dev_pnp_correspondences", "apds_pnp_hypotheses", "apds_pnp_sqpnp", "apds_pnp_ippe", "apds_get_world_coordinates", "apds_l2_knn_match", "apds_dev_l2_topk", "apds_dev_l2_topk_ex",
    "apds_db_create", "apds_db_destroy", "apds_db_rows", "apds_db_insert_image", "apds_db_select", "apds_db_view", "apds_db_view_download", "apds_db_knn_match",
    "apds_comm_id_create", "apds_shard_create", "apds_shard_destroy", "apds_shard_info", "apds_shard_counts", "apds_shard_knn", "apds_shard_knn_replicated", "apds_shard_slot_create",
    "apds_shard_slot_destroy", "apds_shard_gather", "apds_shard_scan", "apds_shard_exchange_merge", "apds_db_shard",
    "apds_dev_alloc", "apds_dev_release", "apds_dev_upload", "apds_dev_download", "apds_stream_synchronize",
    "apds_pipeline_create", "apds_pipeline_submit", "apds_pipeline_poll", "apds_pipeline_stats", "apds_pipeline_destroy", "apds_pipeline_enable_pose",
    "apds_pipeline_poll_pose",
    "apds_dev_topk_state_create", "apds_dev_topk_state_destroy", "apds_dev_topk_prepass", "apds_dev_topk_scan", "apds_dev_topk_merge",
    "apds_mosaic_create", "apds_mosaic_destroy", "apds_mosaic_info", "apds_mosaic_min_max", "apds_resample_weights", "apds_mosaic_window",
    "apds_mosaic_tile_extract", "apds_mosaic_tile_extract_batch",
    "apds_overview_weights", "apds_mosaic_build_overviews", "apds_mosaic_level_info", "apds_mosaic_best_level", "apds_mosaic_window_level",
    "apds_akaze_extract_masked", "apds_akaze_extract_batch_masked", "apds_dev_akaze_extract_masked", "apds_dev_akaze_extract_batch_masked",
    "apds_tile_extract_ex", "apds_tile_extract_batch_ex", "apds_mosaic_tile_extract_ex", "apds_mosaic_tile_extract_batch_ex",
    "apds_akaze_extract_masked_support", "apds_akaze_extract_batch_masked_support", "apds_dev_akaze_extract_masked_support",
    "apds_dev_akaze_extract_batch_masked_support", "apds_dev_mask_zero_sat",
    "apds_db_insert_dev", "apds_db_insert_batch_dev", "apds_mosaic_tiles_to_db", "apds_db_world_coordinates", "apds_db_table",
    "apds_db_view_create", "apds_db_view_destroy", "apds_db_view_select", "apds_db_view_pointers", "apds_pipeline_create_table", "apds_pipeline_submit_select",
    "apds_dev_crosscheck_match", "apds_pipeline_set_matcher",
    "apds_db_ids", "apds_db_read_keypoint_from_id", "apds_db_delete_where", "apds_db_delete_ids",
    "apds_distort_points", "apds_undistort_points", "apds_dev_undistort_points", "apds_undistort_image", "apds_dev_undistort_image",
    "apds_pnp_solver_ransac_dist", "apds_pipeline_set_lens",
    "apds_akaze_extract_float", "apds_akaze_extract_float_batch", "apds_dev_akaze_extract_float", "apds_dev_akaze_extract_float_batch",
    "apds_dev_akaze_describe_float",
    "apds_l2_train_create", "apds_l2_train_destroy", "apds_l2_train_info", "apds_dev_l2_train_top2", "apds_dev_l2_ratio_filter", "apds_pipeline_create_float",
    "apds_workspace_info",
    "apds_db_create_float", "apds_db_info", "apds_db_insert_image_float", "apds_db_view_download_float", "apds_db_read_keypoint_from_id_float",
    "apds_db_view_l2_train", "apds_db_l2_knn_match",
]

RESAMPLE_NEAREST, RESAMPLE_LANCZOS = 0, 1
RESAMPLE_MODES = {"nearest": RESAMPLE_NEAREST, "lanczos": RESAMPLE_LANCZOS}
TILE_MASK_NONE, TILE_MASK_ALPHA = 0, 1     # APDS_TILE_MASK_*: the mask_mode of the apds_*tile_extract*_ex calls
TILE_MASK_ALPHA_SUPPORT = 3                # the alpha mask with MASK_SUPPORT_DESCRIPTOR
MASK_SUPPORT_DESCRIPTOR = 15               # APDS_MASK_SUPPORT_DESCRIPTOR: the mask support that covers the descriptor lattice at any orientation
AKAZE_DESCRIPTOR_KAZE, AKAZE_DESCRIPTOR_MLDB = 3, 5   # APDS_AKAZE_DESCRIPTOR_*: OpenCV's enum values
AKAZE_DESCRIPTORS = {"kaze": AKAZE_DESCRIPTOR_KAZE, "mldb": AKAZE_DESCRIPTOR_MLDB}
DESC_FLOAT_DIM = 64                        # APDS_DESC_FLOAT_DIM: floats per row of the "kaze" descriptor


def resample_mode(name):
    """"nearest" | "lanczos" -> APDS_RESAMPLE_*"""
    try:
        return RESAMPLE_MODES[name]
    except (KeyError, TypeError):
        raise ApdsError(ERR_BAD_ARG, f"unknown resampling mode {name!r}: 'nearest' or 'lanczos'") from None

# multi-GPU sharded matcher (include/apds.h: apds_comm_id, apds_host_transport)
TRANSPORT_RCCL, TRANSPORT_LOOPBACK, TRANSPORT_HOST, TRANSPORT_DEVICE = 0, 1, 2, 3
COMM_ID_BYTES = 128


class CommId(C.Structure):
    _fields_ = [("bytes", C.c_char * COMM_ID_BYTES)]


HOST_ALL_GATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
HOST_ALL_TO_ALL = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t),
                              C.POINTER(C.c_size_t))


class HostTransport(C.Structure):
    _fields_ = [("user", C.c_void_p), ("all_gather", HOST_ALL_GATHER), ("all_to_all", HOST_ALL_TO_ALL)]


# apds_device_transport: the same two callbacks on DEVICE buffers, with the stream they are ordered on
DEV_ALL_GATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
DEV_ALL_TO_ALL = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t),
                             C.POINTER(C.c_size_t), C.c_void_p)


class DeviceTransport(C.Structure):
    _fields_ = [("user", C.c_void_p), ("all_gather", DEV_ALL_GATHER), ("all_to_all", DEV_ALL_TO_ALL)]


class PipelineParams(C.Structure):
    """apds_pipeline_params (include/apds.h)"""
    _fields_ = [("rows", C.c_int), ("cols", C.c_int), ("channels", C.c_int), ("max_points", C.c_int), ("n_slots", C.c_int), ("extract_workers", C.c_int),
                ("filter_strength", C.c_float), ("homography_method", C.c_int), ("reproj_threshold", C.c_double), ("max_iters", C.c_int),
                ("confidence", C.c_double), ("timing", C.c_int), ("match_lds_cap", C.c_int), ("match_stream", C.c_void_p), ("debug_extract_delay_ms", C.c_double)]


class FrameResult(C.Structure):
    """apds_frame_result"""
    _fields_ = [("frame", C.c_int64), ("status", C.c_int), ("n_keypoints", C.c_int), ("n_matches", C.c_int), ("n_inliers", C.c_int), ("homography_found", C.c_int),
                ("H", C.c_double * 9)]


class PipelineCounters(C.Structure):
    """apds_pipeline_counters"""
    _fields_ = [("frames_submitted", C.c_int64), ("frames_done", C.c_int64),
                ("hamming_topk_ms", C.c_double), ("hamming_topk_sample_ms", C.c_double), ("akaze_extract_ms", C.c_double), ("ransac_score_ms", C.c_double),
                ("hamming_topk_launches", C.c_int), ("hamming_topk_sample_launches", C.c_int), ("akaze_extract_calls", C.c_int), ("ransac_score_launches", C.c_int),
                ("match_gap_mean_ms", C.c_double), ("match_gaps", C.c_int), ("match_gaps_first_ms", C.c_float * 16),
                ("match_lds_cap_bytes", C.c_int), ("match_lds_cap_set_at_frame", C.c_int), ("match_lds_cap_gaps_ms", C.c_float * 6),
                ("extract_workers", C.c_int), ("slots", C.c_int), ("split_scan", C.c_int), ("world", C.c_int)]


class PipelinePoseParams(C.Structure):
    """apds_pipeline_pose_params"""
    _fields_ = [("db_xyz_dev", C.c_void_p), ("origin", C.c_double * 3), ("camera_intrinsic", C.c_double * 9), ("method", C.c_int), ("iter_count", C.c_int),
                ("reproj_thres", C.c_float), ("confidence", C.c_double)]


class FramePose(C.Structure):
    """apds_frame_pose"""
    _fields_ = [("frame", C.c_int64), ("status", C.c_int), ("found", C.c_int), ("n_correspondences", C.c_int), ("n_inliers", C.c_int),
                ("rvec", C.c_double * 3), ("tvec", C.c_double * 3)]


class DbSelection(C.Structure):
    """apds_db_selection: one frame's train-set selection on a table pipeline (apds_db_select's mode, value and bounding box)"""
    _fields_ = [("mode", C.c_int), ("value", C.c_int), ("x_start", C.c_float), ("y_start", C.c_float), ("x_end", C.c_float), ("y_end", C.c_float)]


PIPELINE_NOT_READY = 1


class ApdsError(RuntimeError):
    """Mirror of opencv::Error{code, message} as surfaced by the reference crates."""

    def __init__(self, code, message):
        super().__init__(f"apds error {code}: {message}")
        self.code = code
        self.message = message


def build_library(force=False):
    """hipcc --offload-arch=gfx950 build of csrc/ into libapds_hip.so (cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", csrc, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", csrc, "-j8"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ApdsError(ERR_NO_DEVICE, f"{LIB_PATH} is missing: build it with __graft_entry__.build(); there is no CPU fallback")
        # torch ships a HIP runtime of its own: a process that loads this library first and torch afterwards ends up with two runtimes, and
        # the second one to initialise finds no device (-216 from the first call). Loading torch first makes both use the same one.
        if "torch" not in sys.modules:
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(LIB_PATH)
        vp, i, f, d, sz, i64, u32 = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t, C.c_int64, C.c_uint32
        pp, ip = C.POINTER(C.c_void_p), C.POINTER(C.c_int)
        sig = {
            "apds_last_error": (C.c_char_p, []),
            "apds_free": (None, [vp]),
            "apds_device_count": (i, []),
            "apds_set_device": (i, [i]),
            "apds_thread_release": (i, []),
            "apds_live_contexts": (i, []),
            "apds_release_cached_memory": (i, []),
            "apds_build_info": (C.c_char_p, []),
            "apds_akaze_extract": (i, [vp, i, i, i, sz, i, pp, pp, ip, ip]),
            "apds_akaze_extract_batch": (i, [vp, i, sz, i, i, i, sz, i, pp, pp, ip, ip]),
            "apds_dev_akaze_extract_batch": (i, [vp, i, sz, i, i, i, sz, i, vp, vp, i, ip, vp]),
            "apds_tile_extract_batch": (i, [vp, vp, vp, i, i, i, sz, vp, i, pp, pp, ip, ip]),
            "apds_tile_extract": (i, [vp, vp, vp, i, i, sz, vp, i, pp, pp, ip, ip]),
            "apds_get_knn_matches": (i, [vp, i, vp, i, i, i, f, pp, ip]),
            "apds_get_bruteforce_matches": (i, [vp, i, vp, i, i, pp, ip]),
            "apds_knn_match": (i, [vp, i, vp, i, i, i, vp, vp]),
            "apds_get_points_from_matches": (i, [vp, i, vp, i, vp, i, i, vp, vp]),
            "apds_find_homography": (i, [vp, vp, i, i, d, vp, vp]),
            "apds_find_homography_ex": (i, [vp, vp, i, i, d, i, d, vp, vp]),
            "apds_raster_to_mat": (i, [vp, sz, i, i, vp]),
            "apds_dev_pack_descriptors": (i, [vp, i64, i, i64, vp, vp]),
            "apds_dev_hamming_topk": (i, [vp, i, vp, i64, u32, i, vp, vp]),
            "apds_dev_merge_topk": (i, [vp, i, i, i, vp, vp]),
            "apds_dev_match_lds_cap": (i, [i, ip]),
            "apds_dev_match_last_launch_lds": (i, [ip]),
            "apds_dev_match_backend": (i, [ip]),
            "apds_dev_hamming_topk_backend": (i, [vp, i, vp, i64, u32, i, vp, i, vp]),
            "apds_dev_ratio_filter": (i, [vp, i, i, f, vp, ip, vp]),
            "apds_dev_cross_check": (i, [vp, i64, i, vp, ip, vp]),
            "apds_dev_akaze_extract": (i, [vp, i, i, i, sz, i, vp, vp, i, ip, vp]),
            "apds_dev_points_from_matches": (i, [vp, i, vp, i, vp, i, i, vp, vp, vp]),
            "apds_dev_find_homography": (i, [vp, vp, i, i, d, i, d, vp, vp, vp]),
            "apds_dev_valu_popcount_peak": (i, [C.POINTER(d)]),
            "apds_dev_valu_peak": (i, [i, i, C.POINTER(d), C.POINTER(d), C.POINTER(C.c_char_p)]),
            "apds_dev_valu_peak_modes": (i, []),
            "apds_dev_last_kernel_ms": (i, [C.c_char_p, C.POINTER(f), ip]),
            "apds_dev_timing_enable": (i, [i]),
            "apds_akaze_debug_plane": (i, [vp, i, i, i, sz, i, i, vp]),
            "apds_stream_create": (i, [i, vp, i, pp]),
            "apds_stream_destroy": (i, [vp]),
            "apds_band_merger": (i, [vp, vp, vp, sz, vp, i, vp]),
            "apds_dev_band_merger": (i, [vp, vp, vp, sz, vp, i, vp, vp]),
            "apds_warp_perspective": (i, [vp, i, i, i, vp, i, i, vp]),
            "apds_warp_perspective_f32": (i, [vp, i, i, i, vp, i, i, vp]),
            "apds_pnp_solver_ransac": (i, [vp, vp, i, vp, i, f, d, i, vp, vp, vp, ip, ip]),
            "apds_dev_pnp_solver_ransac": (i, [vp, vp, i, vp, i, f, d, i, vp, vp, vp, ip, ip, vp]),
            "apds_dev_pnp_correspondences": (i, [vp, i, vp, i64, vp, vp, i, vp, vp, vp]),
            "apds_pnp_hypotheses": (i, [vp, vp, i, vp, vp, i, i, vp]),
            "apds_pnp_sqpnp": (i, [vp, vp, i, vp, vp, vp, vp]),
            "apds_pnp_ippe": (i, [vp, vp, i, vp, vp, vp, vp]),
            "apds_get_world_coordinates": (i, [vp, i, vp, vp, vp, i, i, vp]),
            "apds_l2_knn_match": (i, [vp, i, vp, i, i, i, vp, vp]),
            "apds_dev_l2_topk": (i, [vp, i, vp, i64, i, u32, i, vp, vp]),
            "apds_dev_l2_topk_ex": (i, [vp, i, vp, i64, i, u32, i, i, vp, vp, ip, C.POINTER(d)]),
            "apds_workspace_info": (i, [C.POINTER(i64), C.POINTER(i64)]),
            "apds_l2_train_create": (i, [pp, vp, i64, i, u32]),
            "apds_l2_train_destroy": (i, [vp]),
            "apds_l2_train_info": (i, [vp, C.POINTER(i64), ip, ip]),
            "apds_dev_l2_train_top2": (i, [vp, vp, i, i, vp, vp, ip, C.POINTER(d)]),
            "apds_dev_l2_ratio_filter": (i, [vp, i, i, f, vp, ip, vp]),
            "apds_pipeline_create_float": (i, [pp, vp, i64, u32, vp, i64, C.POINTER(PipelineParams)]),
            "apds_db_create": (i, [pp, i64]),
            "apds_db_destroy": (i, [vp]),
            "apds_db_rows": (i64, [vp]),
            "apds_db_insert_image": (i, [vp, vp, vp, i, i, i, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]),
            "apds_db_select": (i, [vp, i, i, f, f, f, f, ip]),
            "apds_db_view": (i, [vp, pp, pp, pp, pp, ip]),
            "apds_db_view_download": (i, [vp, vp, vp, vp, vp]),
            "apds_db_knn_match": (i, [vp, vp, i, i, i, vp, vp]),
            "apds_comm_id_create": (i, [i, C.POINTER(CommId)]),
            "apds_shard_create": (i, [pp, i, i, i, C.POINTER(CommId), vp, vp, i64, u32]),
            "apds_shard_destroy": (i, [vp]),
            "apds_shard_info": (i, [vp, ip, ip, C.POINTER(i64), C.POINTER(u32), C.POINTER(C.c_char_p), ip]),
            "apds_shard_counts": (i, [vp, i, ip, vp]),
            "apds_shard_knn": (i, [vp, vp, i, ip, i, vp, vp]),
            "apds_shard_knn_replicated": (i, [vp, vp, i, i, i, vp, vp]),
            "apds_shard_slot_create": (i, [vp, i, i, pp]),
            "apds_shard_slot_destroy": (i, [vp, vp]),
            "apds_shard_gather": (i, [vp, vp, vp, i, ip, vp]),
            "apds_shard_scan": (i, [vp, vp, i, vp]),
            "apds_shard_exchange_merge": (i, [vp, vp, i, vp, vp]),
            "apds_db_shard": (i, [vp, i, i, i, C.POINTER(CommId), C.POINTER(HostTransport), pp]),
            "apds_dev_alloc": (i, [sz, pp]),
            "apds_dev_release": (i, [vp]),
            "apds_dev_upload": (i, [vp, vp, sz, vp]),
            "apds_dev_download": (i, [vp, vp, sz, vp]),
            "apds_stream_synchronize": (i, [vp]),
            "apds_pipeline_create": (i, [pp, vp, i64, u32, vp, vp, i64, C.POINTER(PipelineParams)]),
            "apds_pipeline_submit": (i, [vp, vp, sz, i, C.POINTER(i64)]),
            "apds_pipeline_poll": (i, [vp, C.POINTER(FrameResult), i]),
            "apds_pipeline_stats": (i, [vp, C.POINTER(PipelineCounters), i]),
            "apds_pipeline_destroy": (i, [vp]),
            "apds_pipeline_enable_pose": (i, [vp, C.POINTER(PipelinePoseParams)]),
            "apds_pipeline_poll_pose": (i, [vp, C.POINTER(FrameResult), C.POINTER(FramePose), i]),
            "apds_dev_topk_state_create": (i, [pp]),
            "apds_dev_topk_state_destroy": (i, [vp]),
            "apds_dev_topk_prepass": (i, [vp, vp, i, vp, i64, u32, i, vp]),
            "apds_dev_topk_scan": (i, [vp, vp, vp, vp]),
            "apds_dev_topk_merge": (i, [vp, u32, vp, vp]),
            "apds_mosaic_create": (i, [pp, vp, vp, vp, i, i, sz, i]),
            "apds_mosaic_destroy": (i, [vp]),
            "apds_mosaic_info": (i, [vp, ip, ip]),
            "apds_mosaic_min_max": (i, [vp, vp]),
            "apds_resample_weights": (i, [i, d, d, i, i, i, vp, vp, vp]),
            "apds_mosaic_window": (i, [vp, i, i, i, i, i, i, i, vp]),
            "apds_mosaic_tile_extract": (i, [vp, i, i, i, i, i, i, i, vp, i, pp, pp, ip, ip]),
            "apds_mosaic_tile_extract_batch": (i, [vp, vp, i, i, i, i, i, i, vp, i, pp, pp, ip, ip]),
            "apds_overview_weights": (i, [i, i, i, vp, vp, vp]),
            "apds_mosaic_build_overviews": (i, [vp, i, ip]),
            "apds_mosaic_level_info": (i, [vp, i, ip, ip]),
            "apds_mosaic_best_level": (i, [vp, i, i, i, i, ip]),
            "apds_mosaic_window_level": (i, [vp, i, i, i, i, i, i, i, i, vp]),
            "apds_akaze_extract_masked": (i, [vp, i, i, i, sz, vp, sz, i, pp, pp, ip, ip]),
            "apds_akaze_extract_batch_masked": (i, [vp, i, sz, i, i, i, sz, vp, sz, i, pp, pp, ip, ip]),
            "apds_dev_akaze_extract_masked": (i, [vp, i, i, i, sz, vp, sz, i, vp, vp, i, ip, vp]),
            "apds_dev_akaze_extract_batch_masked": (i, [vp, i, sz, i, i, i, sz, vp, sz, sz, i, vp, vp, i, ip, vp]),
            "apds_tile_extract_ex": (i, [vp, vp, vp, i, i, sz, vp, i, i, pp, pp, ip, ip]),
            "apds_tile_extract_batch_ex": (i, [vp, vp, vp, i, i, i, sz, vp, i, i, pp, pp, ip, ip]),
            "apds_mosaic_tile_extract_ex": (i, [vp, i, i, i, i, i, i, i, vp, i, i, pp, pp, ip, ip]),
            "apds_mosaic_tile_extract_batch_ex": (i, [vp, vp, i, i, i, i, i, i, vp, i, i, pp, pp, ip, ip]),
            "apds_akaze_extract_masked_support": (i, [vp, i, i, i, sz, vp, sz, i, i, pp, pp, ip, ip]),
            "apds_akaze_extract_batch_masked_support": (i, [vp, i, sz, i, i, i, sz, vp, sz, i, i, pp, pp, ip, ip]),
            "apds_dev_akaze_extract_masked_support": (i, [vp, i, i, i, sz, vp, sz, i, i, vp, vp, i, ip, vp]),
            "apds_dev_akaze_extract_batch_masked_support": (i, [vp, i, sz, i, i, i, sz, vp, sz, sz, i, i, vp, vp, i, ip, vp]),
            "apds_dev_mask_zero_sat": (i, [vp, i, i, sz, sz, vp, vp]),
            "apds_db_insert_dev": (i, [vp, vp, vp, i, i, i, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, vp]),
            "apds_db_insert_batch_dev": (i, [vp, vp, vp, i, i, vp, i, i, vp, C.c_uint64, C.c_uint64, vp]),
            "apds_mosaic_tiles_to_db": (i, [vp, vp, vp, i, i, i, i, i, i, vp, i, i, i, i, vp, ip]),
            "apds_db_world_coordinates": (i, [vp, vp, vp, vp, i, i, i, C.POINTER(i64)]),
            "apds_db_table": (i, [vp, pp, pp, pp, C.POINTER(i64)]),
            "apds_db_view_create": (i, [vp, i, pp]),
            "apds_db_view_destroy": (i, [vp]),
            "apds_db_view_select": (i, [vp, i, i, f, f, f, f, i, vp, ip]),
            "apds_db_view_pointers": (i, [vp, pp, pp, pp, pp, pp, ip]),
            "apds_pipeline_create_table": (i, [pp, vp, i, C.POINTER(PipelineParams)]),
            "apds_pipeline_submit_select": (i, [vp, vp, sz, i, C.POINTER(DbSelection), C.POINTER(i64)]),
            "apds_dev_crosscheck_match": (i, [vp, i, vp, i64, u32, vp, ip, vp]),
            "apds_pipeline_set_matcher": (i, [vp, i]),
            "apds_db_ids": (i, [vp, pp]),
            "apds_db_read_keypoint_from_id": (i, [vp, i, vp, vp, ip, C.POINTER(i64)]),
            "apds_db_delete_where": (i, [vp, i, i, f, f, f, f, C.POINTER(i64)]),
            "apds_db_delete_ids": (i, [vp, vp, i, C.POINTER(i64)]),
            "apds_distort_points": (i, [vp, i, vp, vp, i, vp]),
            "apds_undistort_points": (i, [vp, i, vp, vp, i, i, vp]),
            "apds_dev_undistort_points": (i, [vp, i, i, vp, vp, i, i, vp]),
            "apds_undistort_image": (i, [vp, i, i, i, vp, vp, i, vp, vp]),
            "apds_dev_undistort_image": (i, [vp, i, i, i, vp, vp, i, vp, vp, vp]),
            "apds_pnp_solver_ransac_dist": (i, [vp, vp, i, vp, i, f, d, i, vp, i, vp, vp, vp, ip, ip]),
            "apds_pipeline_set_lens": (i, [vp, vp, vp, i, i]),
            "apds_akaze_extract_float": (i, [vp, i, i, i, sz, vp, sz, i, i, pp, pp, ip, ip]),
            "apds_akaze_extract_float_batch": (i, [vp, i, sz, i, i, i, sz, vp, sz, i, i, pp, pp, ip, ip]),
            "apds_dev_akaze_extract_float": (i, [vp, i, i, i, sz, vp, sz, i, i, vp, vp, i, ip, vp]),
            "apds_dev_akaze_extract_float_batch": (i, [vp, i, sz, i, i, i, sz, vp, sz, sz, i, i, vp, vp, i, ip, vp]),
            "apds_dev_akaze_describe_float": (i, [vp, i, i, vp, i, vp, vp]),
            "apds_db_create_float": (i, [pp, i64]),
            "apds_db_info": (i, [vp, ip, ip]),
            "apds_db_insert_image_float": (i, [vp, vp, vp, i, i, i, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]),
            "apds_db_view_download_float": (i, [vp, vp, vp, vp, vp]),
            "apds_db_read_keypoint_from_id_float": (i, [vp, i, vp, vp, ip, C.POINTER(i64)]),
            "apds_db_view_l2_train": (i, [vp, pp]),
            "apds_db_l2_knn_match": (i, [vp, vp, i, i, vp, vp]),
        }
        for name, (rt, at) in sig.items():
            fn = getattr(L, name)
            fn.restype = rt
            fn.argtypes = at
        _LIB = L
    return _LIB


def lens_args(K, dist):
    """(K [3, 3] f64, dist f64 or None, pointer to K, pointer to dist or None, n_dist) of a camera matrix and OpenCV-ordered distortion
    coefficients (None or empty: no distortion) as the apds_*distort* calls take them. Keep the arrays alive across the call."""
    K = np.ascontiguousarray(K, np.float64).reshape(3, 3)
    d = None if dist is None else np.ascontiguousarray(dist, np.float64).ravel()
    if d is not None and d.size == 0:
        d = None
    return K, d, ptr(K), (ptr(d) if d is not None else None), (int(d.size) if d is not None else 0)


def check(rc):
    if rc != 0:
        raise ApdsError(rc, lib().apds_last_error().decode("utf-8", "replace"))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def take(pointer, count, dtype, shape=None):
    """Copy `count` items from a library-allocated host buffer into numpy and apds_free() it."""
    out = np.zeros(count if shape is None else shape, dtype)
    if pointer.value:
        if out.nbytes:
            C.memmove(ptr(out), pointer, out.nbytes)
        lib().apds_free(pointer)
    return out


def workspace_info():
    """(bytes held by every thread's device workspace and the slab cache, device allocations made for them so far): apds_workspace_info"""
    b, n = C.c_int64(0), C.c_int64(0)
    check(lib().apds_workspace_info(C.byref(b), C.byref(n)))
    return b.value, n.value


def kernel_ms(name):
    ms, n = C.c_float(0), C.c_int(0)
    check(lib().apds_dev_last_kernel_ms(name.encode(), C.byref(ms), C.byref(n)))
    return ms.value, n.value
