//! The streamed frame pipeline of libapds_hip (`apds_pipeline_*`, include/apds.h) for a Rust host: frame -> AKAZE -> Hamming top-2 against
//! a train set resident on the GPU -> ratio test -> matched points -> homography, software-pipelined over a stream of frames by host
//! threads that live inside the library (two extraction workers | the match on three streams | ratio filter + RANSAC). The reference
//! chains `akaze_keypoint_descriptor_extraction_def` -> `get_knn_matches` -> `get_points_from_matches` only inside unit tests
//! (feature_extraction/src/lib.rs:197-249) and calls extraction from a rayon pool without a lock (preprocessor/src/main.rs:227-245); this
//! is that chain for a stream of frames, one `submit` and one `poll` per frame. NOT compiled in the build container (no Rust toolchain).
use apds_sys::{apds_db_selection, apds_frame_pose, apds_frame_result, apds_pipeline_counters, apds_pipeline_params, apds_pipeline_pose_params, APDS_PIPELINE_NOT_READY,
               APDS_SOLVEPNP_EPNP};
use std::ffi::CStr;
use std::os::raw::c_void;
use std::ptr;

fn err(rc: i32) -> String {
    format!("apds error {}: {}", rc, unsafe { CStr::from_ptr(apds_sys::apds_last_error()) }.to_string_lossy())
}

pub struct FrameResult {
    pub frame: i64,
    pub keypoints: i32,
    pub matches: i32,
    pub inliers: i32,
    /// row major, `h[8] == 1`; `None`: fewer than four matches survived the ratio test, or no model (`MatError::Empty`, mod.rs:258)
    pub homography: Option<[f64; 9]>,
}

/// The pose stage's answer for one frame (`apds_frame_pose`): cv::solvePnPRansac over the frame's ratio-filtered matches paired with the
/// world points of their DB rows, re-centred on the origin given to `enable_pose` (the pose is relative to it).
pub struct FramePose {
    pub frame: i64,
    /// 0, or what `pnp_solver_ransac` returned for these pairs (`APDS_ERR_ASSERT` for fewer than four), or the frame's own failure
    pub status: i32,
    pub found: bool,
    pub correspondences: i32,
    pub inliers: i32,
    pub rvec: [f64; 3],
    pub tvec: [f64; 3],
}

/// `apds_pipeline_set_matcher`'s values (`APDS_PIPELINE_MATCH_RATIO`, `APDS_PIPELINE_MATCH_CROSSCHECK`)
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
#[repr(i32)]
pub enum Matcher {
    Ratio = 0,
    CrossCheck = 1,
}

pub struct FramePipeline {
    pipe: *mut c_void,
    stride: usize,
}

// the handle may move between threads; one thread submits at a time (the library serialises submitters anyway)
unsafe impl Send for FramePipeline {}

impl FramePipeline {
    /// `train_rows_dev`: n x 64-byte descriptor rows on the device (apds_dev_pack_descriptors), `train_kps_dev`: their n `KeyPoint`s (28 bytes
    /// each); both stay borrowed until the pipeline is dropped. `filter_strength`: Lowe ratio of get_knn_matches (lib.rs:107-111).
    pub fn new(gpu: i32, rows: i32, cols: i32, channels: i32, train_rows_dev: *const c_void, train_kps_dev: *const c_void, n: i64, filter_strength: f32,
               method: i32, reproj_threshold: f64) -> Result<Self, String> {
        let params = apds_pipeline_params {
            rows, cols, channels, max_points: 0, n_slots: 0, extract_workers: 0, filter_strength, homography_method: method, reproj_threshold,
            max_iters: 0, confidence: 0.0, timing: 0, match_lds_cap: 0, match_stream: ptr::null_mut(), debug_extract_delay_ms: 0.0,
        };
        let mut pipe = ptr::null_mut();
        unsafe {
            let rc = apds_sys::apds_set_device(gpu);
            if rc != 0 {
                return Err(err(rc));
            }
            let rc = apds_sys::apds_pipeline_create(&mut pipe, train_rows_dev, n, 0, ptr::null_mut(), train_kps_dev, n, &params);
            if rc != 0 {
                return Err(err(rc));
            }
        }
        Ok(FramePipeline { pipe, stride: (cols * channels) as usize })
    }

    /// The float pipeline (`apds_pipeline_create_float`): M-SURF descriptors (64 x f32), the L2 matcher on a resident train set and the L2
    /// ratio filter; everything behind the matches as in `new`. `train_rows_f32_dev`: n x 64 floats on the device (16-byte aligned, n >= 2),
    /// `train_kps_dev`: their n `KeyPoint`s; both stay borrowed until the pipeline is dropped. `filter_strength`: the ratio on the distances.
    /// Its matcher is `APDS_PIPELINE_MATCH_L2_RATIO` for life: `set_matcher` on it is an error.
    pub fn new_float(gpu: i32, rows: i32, cols: i32, channels: i32, train_rows_f32_dev: *const c_void, train_kps_dev: *const c_void, n: i64,
                     filter_strength: f32, method: i32, reproj_threshold: f64) -> Result<Self, String> {
        let params = apds_pipeline_params {
            rows, cols, channels, max_points: 0, n_slots: 0, extract_workers: 0, filter_strength, homography_method: method, reproj_threshold,
            max_iters: 0, confidence: 0.0, timing: 0, match_lds_cap: 0, match_stream: ptr::null_mut(), debug_extract_delay_ms: 0.0,
        };
        let mut pipe = ptr::null_mut();
        unsafe {
            let rc = apds_sys::apds_set_device(gpu);
            if rc != 0 {
                return Err(err(rc));
            }
            let rc = apds_sys::apds_pipeline_create_float(&mut pipe, train_rows_f32_dev, n, 0, train_kps_dev, n, &params);
            if rc != 0 {
                return Err(err(rc));
            }
        }
        Ok(FramePipeline { pipe, stride: (cols * channels) as usize })
    }

    /// Hands a frame in host memory over (the `Mat::data()` of a CV_8UC4 frame); returns its number. Blocks only while every slot is in
    /// flight. The pixels must stay valid until the frame's result has been polled.
    pub fn submit(&self, pixels: &[u8]) -> Result<i64, String> {
        let mut id = -1i64;
        let rc = unsafe { apds_sys::apds_pipeline_submit(self.pipe, pixels.as_ptr() as *const c_void, self.stride, 0, &mut id) };
        if rc != 0 {
            return Err(err(rc));
        }
        Ok(id)
    }

    /// A pipeline whose train set is selected per frame from a keypoint table (`db`: an `apds_db_create` handle, borrowed until the
    /// pipeline is dropped and frozen meanwhile): the reference's access path, keypointdb.rs:50-90. Frames go in through `submit_select`.
    /// `view_capacity` <= 0: 262143 rows (keypointdb.rs:12).
    pub fn new_table(gpu: i32, rows: i32, cols: i32, channels: i32, db: *mut c_void, view_capacity: i32, filter_strength: f32, method: i32,
                     reproj_threshold: f64) -> Result<Self, String> {
        let params = apds_pipeline_params {
            rows, cols, channels, max_points: 0, n_slots: 0, extract_workers: 0, filter_strength, homography_method: method, reproj_threshold,
            max_iters: 0, confidence: 0.0, timing: 0, match_lds_cap: 0, match_stream: ptr::null_mut(), debug_extract_delay_ms: 0.0,
        };
        let mut pipe = ptr::null_mut();
        unsafe {
            let rc = apds_sys::apds_set_device(gpu);
            if rc != 0 {
                return Err(err(rc));
            }
            let rc = apds_sys::apds_pipeline_create_table(&mut pipe, db, view_capacity, &params);
            if rc != 0 {
                return Err(err(rc));
            }
        }
        Ok(FramePipeline { pipe, stride: (cols * channels) as usize })
    }

    /// `submit` on a `new_table` pipeline: the frame is matched against the rows `read_keypoints_from_coordinates(x_start, y_start, x_end,
    /// y_end, level_of_detail)` returns (keypointdb.rs:67-90: floor(start) <= v <= ceil(end), ORDER BY response DESC LIMIT 262143).
    pub fn submit_select(&self, pixels: &[u8], x_start: f32, y_start: f32, x_end: f32, y_end: f32, level_of_detail: i32) -> Result<i64, String> {
        let sel = apds_db_selection { mode: 2, value: level_of_detail, x_start, y_start, x_end, y_end };
        let mut id = -1i64;
        let rc = unsafe { apds_sys::apds_pipeline_submit_select(self.pipe, pixels.as_ptr() as *const c_void, self.stride, 0, &sel, &mut id) };
        if rc != 0 {
            return Err(err(rc));
        }
        Ok(id)
    }

    /// The next result in submission order; `Ok(None)` when it is not finished yet (`wait == false`) or nothing is in flight.
    pub fn poll(&self, wait: bool) -> Result<Option<FrameResult>, String> {
        let mut r = apds_frame_result { frame: 0, status: 0, n_keypoints: 0, n_matches: 0, n_inliers: 0, homography_found: 0, H: [0.0; 9] };
        let rc = unsafe { apds_sys::apds_pipeline_poll(self.pipe, &mut r, wait as i32) };
        if rc == APDS_PIPELINE_NOT_READY {
            return Ok(None);
        }
        if rc != 0 {
            return Err(err(rc));
        }
        if r.status != 0 {
            return Err(err(r.status));
        }
        Ok(Some(FrameResult {
            frame: r.frame,
            keypoints: r.n_keypoints,
            matches: r.n_matches,
            inliers: r.n_inliers,
            homography: if r.homography_found != 0 { Some(r.H) } else { None },
        }))
    }

    /// Turns the pose stage on; before the first `submit`. `db_xyz_dev`: n x 3 f64 world points of the train rows on the device (e.g.
    /// `get_world_coordinates`, elevationdb.rs:64-104), borrowed until the pipeline is dropped; `origin` is subtracted in f64 before
    /// solvePnPRansac's f32 conversion; `camera_intrinsic` row major 3x3; `method` defaults to SOLVEPNP_EPNP as mod.rs:359 does;
    /// `iter_count` <= 0, `reproj_thres` <= 0 and `confidence` outside (0, 1) take solvePnPRansac's defaults (100, 8.0, 0.99).
    pub fn enable_pose(&self, db_xyz_dev: *const c_void, origin: [f64; 3], camera_intrinsic: [f64; 9], method: Option<i32>, iter_count: i32,
                       reproj_thres: f32, confidence: f64) -> Result<(), String> {
        let params = apds_pipeline_pose_params {
            db_xyz_dev, origin, camera_intrinsic, method: method.unwrap_or(APDS_SOLVEPNP_EPNP), iter_count, reproj_thres, confidence,
        };
        let rc = unsafe { apds_sys::apds_pipeline_enable_pose(self.pipe, &params) };
        if rc != 0 {
            return Err(err(rc));
        }
        Ok(())
    }

    /// Chooses the pipeline's matcher; before the first `submit`. `Matcher::Ratio` (the default of a pipeline that never calls this) is
    /// `get_knn_matches` with k = 2 and the Lowe ratio (lib.rs:94-114); `Matcher::CrossCheck` is `get_bruteforce_matches` (lib.rs:116-126,
    /// `BFMatcher(NORM_HAMMING, crossCheck = true)`): `filter_strength` is then ignored, and the homography and the pose stage work on the
    /// cross-checked matches. Not built over a shard handle (`APDS_ERR_NOT_IMPLEMENTED`).
    pub fn set_matcher(&self, matcher: Matcher) -> Result<(), String> {
        let rc = unsafe { apds_sys::apds_pipeline_set_matcher(self.pipe, matcher as i32) };
        if rc != 0 {
            return Err(err(rc));
        }
        Ok(())
    }

    /// Gives the pipeline the camera's lens; before the first `submit`. `camera_intrinsic` row major 3x3, `dist_coeffs` as the
    /// calibrator computes them (calibrator/src/main.rs:59-73; OpenCV's order, 4, 5 or 8 values; empty: no distortion), `iters` steps of
    /// cv::undistortPoints' iteration (<= 0: 5). The image side of every frame's matches is undistorted on the device in front of the
    /// homography and the pose; `reproj_threshold` / `reproj_thres` are then in undistorted pixels. `camera_intrinsic` is expected to be
    /// the matrix `enable_pose` was given.
    pub fn set_lens(&self, camera_intrinsic: [f64; 9], dist_coeffs: &[f64], iters: i32) -> Result<(), String> {
        let dist = if dist_coeffs.is_empty() { ptr::null() } else { dist_coeffs.as_ptr() };
        let rc = unsafe { apds_sys::apds_pipeline_set_lens(self.pipe, camera_intrinsic.as_ptr(), dist, dist_coeffs.len() as i32, iters) };
        if rc != 0 {
            return Err(err(rc));
        }
        Ok(())
    }

    /// `poll` with the frame's pose (all zero, `found == false`, when the pose stage is off). A failed pose does not fail the frame: it is
    /// in `FramePose::status`.
    pub fn poll_pose(&self, wait: bool) -> Result<Option<(FrameResult, FramePose)>, String> {
        let mut r = apds_frame_result { frame: 0, status: 0, n_keypoints: 0, n_matches: 0, n_inliers: 0, homography_found: 0, H: [0.0; 9] };
        let mut p = apds_frame_pose { frame: 0, status: 0, found: 0, n_correspondences: 0, n_inliers: 0, rvec: [0.0; 3], tvec: [0.0; 3] };
        let rc = unsafe { apds_sys::apds_pipeline_poll_pose(self.pipe, &mut r, &mut p, wait as i32) };
        if rc == APDS_PIPELINE_NOT_READY {
            return Ok(None);
        }
        if rc != 0 {
            return Err(err(rc));
        }
        if r.status != 0 {
            return Err(err(r.status));
        }
        Ok(Some((
            FrameResult {
                frame: r.frame,
                keypoints: r.n_keypoints,
                matches: r.n_matches,
                inliers: r.n_inliers,
                homography: if r.homography_found != 0 { Some(r.H) } else { None },
            },
            FramePose { frame: p.frame, status: p.status, found: p.found != 0, correspondences: p.n_correspondences, inliers: p.n_inliers, rvec: p.rvec, tvec: p.tvec },
        )))
    }

    pub fn frames_done(&self) -> Result<i64, String> {
        let mut c: apds_pipeline_counters = unsafe { std::mem::zeroed() };
        let rc = unsafe { apds_sys::apds_pipeline_stats(self.pipe, &mut c, 0) };
        if rc != 0 {
            return Err(err(rc));
        }
        Ok(c.frames_done)
    }
}

impl Drop for FramePipeline {
    fn drop(&mut self) {
        unsafe { apds_sys::apds_pipeline_destroy(self.pipe) };
    }
}
