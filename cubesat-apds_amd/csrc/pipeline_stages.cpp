// csrc/pipeline_stages.cpp — the streamed pipeline's stages around the match: extraction in front of it, homography and (opt-in) pose
// behind it. Each is one worker thread's loop over the slots it is handed; the train side of a frame is its slot's (pipeline.h).
#include <chrono>
#include <cstring>

#include "pipeline.h"

namespace apds {

// ---- stage 1: extraction ----------------------------------------------------------------------------------------------------------
void Pipeline::extract_worker(int e) {
    const std::initializer_list<const char*> timed = {"akaze_extract"};
    hipStream_t st = st_extract[e];
    Slot* s = nullptr;
    while (q_jobs[(size_t)e]->pop(s)) {
        if (!s) {   // apds_pipeline_stats on the idle pipeline: this thread's event timers -> the totals
            harvest(timed);
            continue;
        }
        const void* img = s->src;
        s->status = APDS_OK;
        s->K = 0;
        if (!s->on_device) {
            // a host frame: uploaded on THIS worker's stream in front of the extraction, into the slot's own buffer; the other
            // extraction worker and the match run meanwhile, so the PCIe copy is hidden (pinned memory makes it a true async copy)
            const size_t bytes = s->stride * (size_t)p.rows;
            if (s->frame_dev_bytes < bytes) {
                if (s->frame_dev) HIP_CHECK(hipFree(s->frame_dev));
                s->frame_dev = nullptr;
                HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&s->frame_dev), bytes));
                s->frame_dev_bytes = bytes;
            }
            HIP_CHECK(hipMemcpyAsync(s->frame_dev, s->src, bytes, hipMemcpyHostToDevice, st));
            img = s->frame_dev;
        }
        int n = 0;
        const int rc = float_rows ? apds_dev_akaze_extract_float(img, p.rows, p.cols, p.channels, s->stride, nullptr, 0, 0, cap, s->kps, s->desc, cap, &n, st)
                                  : apds_dev_akaze_extract(img, p.rows, p.cols, p.channels, s->stride, cap, s->kps, s->desc, cap, &n, st);
        if (rc != APDS_OK) {   // this frame fails, the pipeline goes on (a sharded run contributes zero queries for it)
            s->status = rc;
            s->error = apds_last_error();
            n = 0;
        }
        s->K = n;
        HIP_CHECK(hipEventRecord(s->ev_extract, st));
        if (extract_delay_s > 0) std::this_thread::sleep_for(std::chrono::duration<double>(extract_delay_s));   // test hook: a box on which extraction cannot keep up
        q_ext[(size_t)e]->push(s);
        if (world == 1) q_any.push(e);
    }
    collect(timed);
}

// ---- stage 3: ratio filter, matched points, homography ---------------------------------------------------------------------------
void Pipeline::homography_worker() {
    const std::initializer_list<const char*> timed = {"ransac_score"};
    hipStream_t st = st_homography;
    Slot* s = nullptr;
    int* count_dev = nullptr;
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&count_dev), 256));
    while (q_homography.pop(s)) {
        if (!s) {
            harvest(timed);
            continue;
        }
        apds_frame_result r{};
        r.frame = s->index;
        r.status = s->status;
        r.n_keypoints = s->K;
        std::string why = s->status != APDS_OK ? s->error : std::string();
        const TrainSide& T = s->train;
        try {
            HIP_CHECK(hipStreamWaitEvent(st, s->ev_match, 0));
            int M = 0;
            // a frame with keypoints whose status is not OK: its selection had fewer than two rows, nothing was scanned (a frame whose
            // extraction failed has K = 0)
            const bool matched = s->K > 0 && s->status == APDS_OK;
            if (matched && matcher == APDS_PIPELINE_MATCH_CROSSCHECK) {
                // per query the closest train row that chose it, in query order; train_idx = row + index_base (a view: its position)
                PIPE_OK(guarded([&] {
                    ctx().ws_reset(st);
                    M = cross_check_base_device(s->train_best, (long long)T.n_rows, s->K, T.index_base, s->matches, st);
                }));
            } else if (matched && float_rows) {
                PIPE_OK(apds_dev_l2_ratio_filter(s->keys, s->K, 2, p.filter_strength, s->matches, &M, st));
            } else if (matched) {
                PIPE_OK(apds_dev_ratio_filter(s->keys, s->K, 2, p.filter_strength, s->matches, &M, st));
            }
            r.n_matches = M;
            if (M >= 4) {
                // query_idx -> this frame's keypoints, train_idx -> the DB rows' keypoints (the intended gather: lib.rs:161-180 has two bugs)
                PIPE_OK(apds_dev_points_from_matches(s->kps, s->K, T.kps, (int)T.n_kps, s->matches, M, 0, s->p1, s->p2, st));
                // the frame side of the matches to ideal pixels (the train side is map geometry): one launch on this stream, no workspace
                if (lens_on) PIPE_OK(guarded([&] { lens_undistort_points_f32_device(s->p1, M, 2 * sizeof(float), lens, lens_iters, st); }));
                const int rc = apds_dev_find_homography(s->p1, s->p2, M, p.homography_method, p.reproj_threshold, p.max_iters, p.confidence, r.H, s->mask, st);
                if (rc == APDS_OK) {
                    r.homography_found = 1;
                    r.n_inliers = count_nonzero_device(s->mask, M, count_dev, st);
                } else if (rc != APDS_ERR_EMPTY) {
                    stage_fail(rc);
                }
            }
        } catch (const StageError& e) {   // this frame's failure: reported with the frame, the pipeline goes on
            r.status = e.code;
            why = e.msg;
        }
        if (pose_on) {   // the pose worker finishes the frame: its ratio-filtered matches are ordered on this stream
            s->res = r;
            s->res_why = why;
            HIP_CHECK(hipEventRecord(s->ev_homography, st));
            q_pose.push(s);
        } else {
            finish(s, r, why);
        }
    }
    (void)hipFree(count_dev);
    collect(timed);
    q_pose.close();
}

// ---- stage 4 (opt-in): world-point gather, PnP RANSAC ------------------------------------------------------------------------------
// Frame i's pose runs here while frame i + 1's homography runs on the stage before. Both calls start from an empty workspace of this
// thread (they reset it themselves), so nothing grows with the frame count. A frame whose pose fails reports it in its pose status.
void Pipeline::pose_worker() {
    hipStream_t st = st_pose;
    Slot* s = nullptr;
    while (q_pose.pop(s)) {
        const apds_frame_result& r = s->res;
        apds_frame_pose fp{};
        fp.frame = s->index;
        fp.status = r.status;
        if (r.status == APDS_OK) {
            const int M = r.n_matches;
            fp.n_correspondences = M;
            try {
                HIP_CHECK(hipStreamWaitEvent(st, s->ev_homography, 0));
                PIPE_OK(apds_dev_pnp_correspondences(s->kps, s->K, s->train.xyz, s->train.n_kps, pose.origin, s->matches, M, s->pose_img, s->pose_obj, st));
                if (lens_on) PIPE_OK(guarded([&] { lens_undistort_points_f32_device(s->pose_img, M, 2 * sizeof(float), lens, lens_iters, st); }));
                // fewer than four pairs: the one-call entry's APDS_ERR_ASSERT, without device work
                fp.status = apds_dev_pnp_solver_ransac(s->pose_obj, s->pose_img, M, pose.camera_intrinsic, pose.iter_count, pose.reproj_thres, pose.confidence,
                                                      pose.method, fp.rvec, fp.tvec, nullptr, &fp.n_inliers, &fp.found, st);
            } catch (const StageError& e) {
                fp.status = e.code;
            }
            if (fp.status != APDS_OK) {   // (as the serial front reports a failed solve: nothing but the status and the pair count)
                fp.found = fp.n_inliers = 0;
                std::memset(fp.rvec, 0, sizeof(fp.rvec));
                std::memset(fp.tvec, 0, sizeof(fp.tvec));
            }
        }
        finish(s, r, s->res_why, &fp);
    }
}

}  // namespace apds
