// csrc/pipeline.cpp — the streamed frame pipeline behind the C ABI (apds_pipeline_*, include/apds.h).
//
// frame -> AKAZE -> Hamming top-2 against the resident descriptor DB -> ratio test -> matched points -> homography, software-pipelined
// over a stream of frames by host threads that live INSIDE the library, so that a host which is not Python (the reference's host is
// Rust: preprocessor/src/main.rs:227-245 calls the path from a rayon pool, no lock) reaches the same frames/s bench.py reports:
//
//   extraction workers (2)   frame i+1, i+2: upload (host frames), AKAZE; HBM-bound stencils at raised wave priority
//   match worker (1)         frame i: threshold pre-pass | main scan | record merge on three streams, so the main scans of consecutive
//                            frames follow each other without the pre-pass, the merge and the dependent-launch gaps between them;
//                            with a row-sharded DB (apds_shard_*): query gather of frame i+1 before the key exchange of frame i
//   homography worker (1)    frame i-1: ratio filter, point gather, RANSAC (its host round trips hide behind the other two stages)
//   pose worker (opt-in, 1)  frame i-2: world-point gather, PnP RANSAC (apds_pipeline_enable_pose; overlaps the next frame's homography)
//
// A table pipeline (apds_pipeline_create_table) selects each frame's train set from a keypoint table first (keypointdb.rs:50-90): the match
// worker runs the slot's view select on the match stream in front of the scan, and the later stages read the view by position.
//
// The matcher is selectable before the first submit (apds_pipeline_set_matcher): the cross-check (get_bruteforce_matches, lib.rs:116-126)
// replaces the forward top-2 scan by ONE roles-swapped top-1 scan per frame - every train row's nearest query, into the slot's train_best;
// with the matrix-core matcher the resident expanded copy of the DB is its searching side as it is - and the ratio filter by the
// cross-check's scatter / flags / ordered compaction; everything behind the matches is unchanged.
//
// A float pipeline (apds_pipeline_create_float) runs the same stages over M-SURF rows (64 x f32): the extraction workers call the float
// extraction into slot buffers of 256 bytes per row, the match worker calls the resident L2 train set's top-2 (l2_screen.hip: bf16 screen +
// exact re-rank, or the exact kernel) on the single-stream branch, and the homography stage builds its matches with the L2 ratio filter;
// everything behind the matches is unchanged. The split scan, the expanded copy, the starvation watch and the LDS cap are the Hamming scan's.
//
// Every worker owns a HIP stream and a device workspace (the per-thread context every entry point uses), stages hand frames over
// through HIP events, results leave in frame order. The reference only chains these steps inside unit tests
// (feature_extraction/src/lib.rs:197-249) and never calls find_homography_mat on the result; this is the composed path the
// north-star metric (frames/s) is measured on. The Python class cubesat-apds_amd/pipeline.py:StreamedFramePipeline is a front of this.
#include <climits>
#include <cmath>
#include <cstring>

#include "pipeline.h"

using namespace apds;

void Pipeline::fail(int code, const std::string& msg) {
    {
        std::lock_guard<std::mutex> g(m);
        if (!failed) {
            failed = true;
            fail_code = code;
            fail_msg = msg;
        }
    }
    close_all();
    cv.notify_all();
}
void Pipeline::close_all() {
    for (auto& q : q_free) q->close();
    for (auto& q : q_jobs) q->close();
    for (auto& q : q_ext) q->close();
    q_any.close();
    q_homography.close();
    q_pose.close();
}
void Pipeline::collect(std::initializer_list<const char*> names) {
    if (!p.timing) return;
    for (const char* n : names) {
        float ms = 0;
        int k = 0;
        if (apds_dev_last_kernel_ms(n, &ms, &k) != APDS_OK || k <= 0) continue;
        std::lock_guard<std::mutex> g(m);
        auto& t = timers[n];
        t.first += ms;
        t.second += k;
    }
}
void Pipeline::harvest(std::initializer_list<const char*> names) {
    collect(names);
    {
        std::lock_guard<std::mutex> g(m);
        harvest_acks++;
    }
    cv.notify_all();
}
void Pipeline::finish(Slot* s, const apds_frame_result& r, const std::string& why, const apds_frame_pose* fp) {
    {
        std::lock_guard<std::mutex> g(m);
        results[s->index] = r;
        if (fp) poses[s->index] = *fp;
        if (r.status != APDS_OK) result_errors[s->index] = why;
        done++;
    }
    cv.notify_all();
    q_free[(size_t)s->owner]->push(s);
}

namespace {

void destroy_pipeline(Pipeline* P) {
    {
        std::lock_guard<std::mutex> g(P->m);
        P->closing = true;
    }
    // the stages drain in order: no more jobs -> extraction ends -> match ends (closes the homography queue) -> homography ends (closes the
    // pose queue) -> pose ends
    for (auto& q : P->q_jobs) q->close();
    for (auto& q : P->q_free) q->close();
    for (size_t e = 0; e < P->threads.size() && e < (size_t)P->E; e++)
        if (P->threads[e].joinable()) P->threads[e].join();
    for (auto& q : P->q_ext) q->close();
    P->q_any.close();
    for (auto& t : P->threads)
        if (t.joinable()) t.join();
    DeviceGuard on(P->device);
    (void)hipDeviceSynchronize();
    for (auto& up : P->slots) {
        Slot* s = up.get();
        for (void* ptr : {(void*)s->kps, (void*)s->desc, (void*)s->keys, (void*)s->matches, (void*)s->p1, (void*)s->p2, (void*)s->mask, (void*)s->frame_dev,
                          (void*)s->pose_img, (void*)s->pose_obj, (void*)s->train_best})
            if (ptr) (void)hipFree(ptr);
        for (hipEvent_t ev : {s->ev_extract, s->ev_pre, s->ev_scan, s->ev_match, s->ev_mstart, s->ev_mend, s->ev_homography})
            if (ev) (void)hipEventDestroy(ev);
        if (s->topk_state) topk_split_destroy(s->topk_state);
        if (s->shard_slot && P->shard) (void)apds_shard_slot_destroy(P->shard, s->shard_slot);
        if (s->view) (void)apds_db_view_destroy(s->view);
    }
    if (P->db_expanded) hm_train_destroy(P->db_expanded);
    P->db_expanded = nullptr;
    l2_train_destroy(P->train.l2);
    P->train.l2 = nullptr;
    if (P->db_plain_pc) (void)hipFree(P->db_plain_pc);
    P->db_plain_pc = nullptr;
    if (!P->own_match_stream) P->st_match = nullptr;
    for (hipStream_t st : {P->st_match, P->st_pre, P->st_merge, P->st_homography, P->st_gather, P->st_counts, P->st_pose})
        if (st) (void)hipStreamDestroy(st);
    for (hipStream_t st : P->st_extract)
        if (st) (void)hipStreamDestroy(st);
    delete P;
}

Pipeline* pipe_handle(void* h) {
    APDS_REQUIRE(h, APDS_ERR_BAD_ARG, "null pipeline handle");
    return static_cast<Pipeline*>(h);
}

// The frame of a setter, configure before the first submit: the submitter's lock (the caller holds it for the rest of its body), a failed
// pipeline's error again, and no frame submitted yet (too_late: the setter's own text for that).
std::unique_lock<std::mutex> configure_lock(Pipeline* P, const char* too_late) {
    std::unique_lock<std::mutex> one(P->submit_m);
    std::lock_guard<std::mutex> g(P->m);
    if (P->failed) fail(P->fail_code, P->fail_msg);
    APDS_REQUIRE(P->next_submit == 0, APDS_ERR_BAD_ARG, too_late);
    return one;
}

// table != null: the train set is a per-frame view of that keypoint table (view_capacity rows at most); the rows arguments are unused
// float_rows: db_rows64_dev are rows of 64 floats (apds_pipeline_create_float; no shard, no table)
int create_pipeline(void** pipe, const void* db_rows64_dev, int64_t n_rows, uint32_t index_base, void* shard, const void* db_kps_dev, int64_t n_db_total,
                    void* table, int view_capacity, const apds_pipeline_params* params, bool float_rows = false) {
    return guarded([&] {
        APDS_REQUIRE(pipe && params, APDS_ERR_BAD_ARG, "null argument");
        *pipe = nullptr;
        const apds_pipeline_params& in = *params;
        APDS_REQUIRE(in.rows > 0 && in.cols > 0 && (in.channels == 1 || in.channels == 3 || in.channels == 4), APDS_ERR_ASSERT, "bad frame geometry");
        if (!table) {
            APDS_REQUIRE(shard || (db_rows64_dev && n_rows >= 2), APDS_ERR_ASSERT, "a train set of at least two rows (or a shard handle) is required");
            APDS_REQUIRE(db_kps_dev && n_db_total > 0 && n_db_total < (1ll << 31), APDS_ERR_ASSERT, "the train rows' keypoints are required (n_db_total x 28 bytes)");
        }
        APDS_REQUIRE(!float_rows || (n_rows < (1ll << 31) && (reinterpret_cast<uintptr_t>(db_rows64_dev) & 15) == 0), APDS_ERR_ASSERT,
                     "float train rows: 16-byte aligned, fewer than 2^31 of them");
        ThreadCtx& c = ctx();
        APDS_REQUIRE(!table || table_device(table) == c.device, APDS_ERR_BAD_ARG, "the table lives on another device than the calling thread's");
        std::unique_ptr<Pipeline, void (*)(Pipeline*)> P(new Pipeline(), destroy_pipeline);
        P->p = in;
        P->device = c.device;
        P->table = table;
        P->view_capacity = view_capacity;
        P->train.rows = db_rows64_dev;
        P->train.n_rows = n_rows;
        P->train.index_base = index_base;
        P->train.kps = static_cast<const apds_keypoint*>(db_kps_dev);
        P->train.n_kps = n_db_total;
        P->shard = shard;
        P->float_rows = float_rows;
        if (float_rows) P->matcher = APDS_PIPELINE_MATCH_L2_RATIO;
        const Config& cfg = config();
        if (shard) {
            int w = 1;
            int64_t nr = 0;
            uint32_t base = 0;
            const int rc = apds_shard_info(shard, nullptr, &w, &nr, &base, nullptr, nullptr);
            if (rc != APDS_OK) fail(rc, apds_last_error());
            P->world = w;
            P->train.n_rows = nr;
            P->train.index_base = base;
        }
        P->cap = in.max_points > 0 ? std::min(in.max_points, APDS_MAX_POINTS) : APDS_MAX_POINTS;
        P->E = std::max(1, std::min(8, in.extract_workers > 0 ? in.extract_workers : cfg.pipe_extract_workers));
        const int n_slots = std::max(in.n_slots > 0 ? in.n_slots : 6, 2 * P->E);
        // three streams for the pre-pass, main scan and merge of consecutive frames: the vector-ALU matcher's pipeline (its pre-pass and record
        // merge are 0.8 ms of small kernels per frame). The matrix-core matcher has one main launch and two tiny ones: on one stream 131.6
        // frames/s, split over three 126.8 (profiles/r04/ab_bench_env.txt); APDS_MATCH_SPLIT=2 forces the split for it as well.
        // (a table pipeline matches each frame against another view: one stream, the one-call matcher, no expanded copy of a resident train set)
        P->split = P->world == 1 && !shard && !table && !float_rows && (cfg.match_mfma ? cfg.pipe_match_split == 2 : cfg.pipe_match_split != 0);
        // (the starvation watch caps hamming_topk_kernel's occupancy: the matrix-core matcher has no such knob and is not watched)
        P->adaptive_cap = cfg.pipe_adaptive_cap != 0 && P->split && in.match_lds_cap == 0 && !cfg.match_mfma;
        P->extract_delay_s = in.debug_extract_delay_ms > 0 ? in.debug_extract_delay_ms * 1e-3 : 0.0;
        if (P->p.reproj_threshold <= 0) P->p.reproj_threshold = 3.0;
        if (P->p.max_iters <= 0) P->p.max_iters = 2000;
        if (!(P->p.confidence > 0 && P->p.confidence < 1)) P->p.confidence = 0.995;
        // the short kernels of extraction / homography / query gather get high-priority queues: their blocks are dispatched as soon as match
        // workgroups retire (the match kernel alone fills every CU for ~22 ms)
        const int hp = cfg.pipe_prio;
        for (int e = 0; e < P->E; e++) HIP_CHECK(hipStreamCreateWithPriority(&P->st_extract[e], hipStreamNonBlocking, hp));
        if (in.match_stream) P->st_match = static_cast<hipStream_t>(in.match_stream), P->own_match_stream = false;
        else HIP_CHECK(hipStreamCreateWithPriority(&P->st_match, hipStreamNonBlocking, 0));
        HIP_CHECK(hipStreamCreateWithPriority(&P->st_homography, hipStreamNonBlocking, hp));
        if (P->split) {
            HIP_CHECK(hipStreamCreateWithPriority(&P->st_pre, hipStreamNonBlocking, 0));
            HIP_CHECK(hipStreamCreateWithPriority(&P->st_merge, hipStreamNonBlocking, hp));
        }
        if (shard) {
            HIP_CHECK(hipStreamCreateWithPriority(&P->st_gather, hipStreamNonBlocking, hp));
            HIP_CHECK(hipStreamCreateWithPriority(&P->st_counts, hipStreamNonBlocking, hp));
        }
        if (float_rows && !table) P->train.l2 = l2_train_create(static_cast<const float*>(db_rows64_dev), n_rows, 64, index_base, P->st_match);
        if (P->world == 1 && !shard && !table && !float_rows && cfg.match_mfma) P->db_expanded = hm_train_create(P->train.rows, P->train.n_rows, P->st_match);
        const size_t cap = (size_t)P->cap;
        for (int i = 0; i < n_slots; i++) {
            auto s = std::make_unique<Slot>();
            s->owner = i % P->E;
            s->train = P->train;
            HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&s->kps), cap * sizeof(apds_keypoint)));
            HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&s->desc), cap * (float_rows ? 256 : 64)));
            HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&s->keys), cap * 2 * 8));
            HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&s->matches), cap * sizeof(apds_dmatch)));
            HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&s->p1), cap * 8));
            HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&s->p2), cap * 8));
            HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&s->mask), cap));
            for (hipEvent_t* ev : {&s->ev_extract, &s->ev_pre, &s->ev_scan, &s->ev_match}) HIP_CHECK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
            HIP_CHECK(hipEventCreate(&s->ev_mstart));
            HIP_CHECK(hipEventCreate(&s->ev_mend));
            if (P->split) {
                s->topk_state = topk_split_create();
                if (P->db_expanded) topk_split_use_train(s->topk_state, P->db_expanded);
            }
            if (shard) {
                const int rc = apds_shard_slot_create(shard, P->cap, 2, &s->shard_slot);
                if (rc != APDS_OK) fail(rc, apds_last_error());
            }
            if (table) {
                int rc = apds_db_view_create(table, view_capacity, &s->view);
                void *rows64 = nullptr, *kps = nullptr, *l2 = nullptr;
                if (rc == APDS_OK) rc = apds_db_view_pointers(s->view, &rows64, &kps, nullptr, nullptr, nullptr, nullptr);
                if (rc == APDS_OK && float_rows) rc = apds_db_view_l2_train(s->view, &l2);   // (borrowed: the view owns it)
                if (rc != APDS_OK) {
                    const std::string why = apds_last_error();
                    P->slots.push_back(std::move(s));   // (destroy releases what this slot already holds)
                    fail(rc, why);
                }
                // the slot's train side is its view: the counts and xyz come with each frame's select (index_base 0: a match's train index is the view position)
                s->train.rows = rows64;
                s->train.kps = static_cast<const apds_keypoint*>(kps);
                s->train.l2 = static_cast<L2Train*>(l2);
            }
            P->slots.push_back(std::move(s));
        }
        for (int e = 0; e < P->E; e++) {
            P->q_free.push_back(std::make_unique<Chan<Slot*>>());
            P->q_jobs.push_back(std::make_unique<Chan<Slot*>>());
            P->q_ext.push_back(std::make_unique<Chan<Slot*>>());
        }
        for (auto& s : P->slots) P->q_free[(size_t)s->owner]->push(s.get());
        HIP_CHECK(hipDeviceSynchronize());
        Pipeline* raw = P.get();
        for (int e = 0; e < P->E; e++)   // (the first E threads are the extraction workers: destroy joins them first)
            P->threads.emplace_back([raw, e] { raw->worker("extraction", [&] { raw->extract_worker(e); }); });
        if (P->world > 1 || shard) P->threads.emplace_back([raw] { raw->worker("sharded match", [&] { raw->sharded_match_worker(); }); });
        else P->threads.emplace_back([raw] { raw->worker("match", [&] { raw->match_worker(); }); });
        P->threads.emplace_back([raw] { raw->worker("homography", [&] { raw->homography_worker(); }); });
        *pipe = P.release();
    });
}

int submit_frame(void* pipe, const void* frame, size_t stride_bytes, int on_device, const apds_db_selection* sel, bool with_selection, int64_t* frame_id) {
    return guarded([&] {
        Pipeline* P = pipe_handle(pipe);
        APDS_REQUIRE(with_selection == (P->table != nullptr), APDS_ERR_BAD_ARG,
                     with_selection ? "this pipeline has a fixed train set: use apds_pipeline_submit"
                                    : "this pipeline selects its train set per frame: use apds_pipeline_submit_select");
        APDS_REQUIRE(!with_selection || (sel && sel->mode >= 0 && sel->mode <= 2), APDS_ERR_BAD_ARG, "a selection with mode 0, 1 or 2 is required");
        APDS_REQUIRE(frame, APDS_ERR_BAD_ARG, "null frame");
        APDS_REQUIRE(stride_bytes >= (size_t)P->p.cols * (size_t)P->p.channels, APDS_ERR_ASSERT, "row stride shorter than a row");
        std::lock_guard<std::mutex> one(P->submit_m);
        int64_t index;
        {
            std::lock_guard<std::mutex> g(P->m);
            if (P->failed) fail(P->fail_code, P->fail_msg);
            index = P->next_submit;
        }
        Slot* s = nullptr;
        const size_t e = (size_t)(index % P->E);
        if (!P->q_free[e]->pop(s)) {   // blocks while every slot of this worker is in flight
            std::lock_guard<std::mutex> g(P->m);
            fail(P->failed ? P->fail_code : APDS_ERR_INTERNAL, P->failed ? P->fail_msg : "the pipeline is shutting down");
        }
        s->src = frame;
        s->stride = stride_bytes;
        s->on_device = on_device != 0;
        s->index = index;
        if (sel) s->sel = *sel;
        {
            std::lock_guard<std::mutex> g(P->m);
            P->next_submit = index + 1;
        }
        if (frame_id) *frame_id = index;
        P->q_jobs[e]->push(s);
    });
}

}  // namespace

extern "C" {

int apds_pipeline_create(void** pipe, const void* db_rows64_dev, int64_t n_rows, uint32_t index_base, void* shard, const void* db_kps_dev, int64_t n_db_total,
                         const apds_pipeline_params* params) {
    return create_pipeline(pipe, db_rows64_dev, n_rows, index_base, shard, db_kps_dev, n_db_total, nullptr, 0, params);
}

int apds_pipeline_create_float(void** pipe, const void* db_rows_f32_dev, int64_t n_rows, uint32_t index_base, const void* db_kps_dev, int64_t n_db_total,
                               const apds_pipeline_params* params) {
    return create_pipeline(pipe, db_rows_f32_dev, n_rows, index_base, nullptr, db_kps_dev, n_db_total, nullptr, 0, params, true);
}

int apds_pipeline_create_table(void** pipe, void* db, int view_capacity, const apds_pipeline_params* params) {
    if (!db) return guarded([] { fail(APDS_ERR_BAD_ARG, "null table"); });
    // a float table makes a float pipeline: M-SURF extraction, the L2 matcher for life, each frame's train side from its slot's view
    int descriptor = APDS_AKAZE_DESCRIPTOR_MLDB;
    const int rc = apds_db_info(db, &descriptor, nullptr);
    if (rc != APDS_OK) return rc;
    return create_pipeline(pipe, nullptr, 0, 0, nullptr, nullptr, 0, db, view_capacity, params, descriptor == APDS_AKAZE_DESCRIPTOR_KAZE);
}

int apds_pipeline_submit(void* pipe, const void* frame, size_t stride_bytes, int on_device, int64_t* frame_id) {
    return submit_frame(pipe, frame, stride_bytes, on_device, nullptr, false, frame_id);
}

int apds_pipeline_submit_select(void* pipe, const void* frame, size_t stride_bytes, int on_device, const apds_db_selection* sel, int64_t* frame_id) {
    return submit_frame(pipe, frame, stride_bytes, on_device, sel, true, frame_id);
}

int apds_pipeline_poll(void* pipe, apds_frame_result* result, int wait) { return apds_pipeline_poll_pose(pipe, result, nullptr, wait); }

int apds_pipeline_poll_pose(void* pipe, apds_frame_result* result, apds_frame_pose* pose, int wait) {
    int ready = 0;
    const int rc = guarded([&] {
        Pipeline* P = pipe_handle(pipe);
        APDS_REQUIRE(result, APDS_ERR_BAD_ARG, "null output");
        std::unique_lock<std::mutex> g(P->m);
        auto have = [&] { return P->results.count(P->next_result) > 0; };
        if (wait) P->cv.wait(g, [&] { return have() || P->failed || P->next_result >= P->next_submit; });
        if (have()) {
            *result = P->results[P->next_result];
            P->results.erase(P->next_result);
            auto fp = P->poses.find(P->next_result);
            if (pose) {
                std::memset(pose, 0, sizeof(*pose));
                pose->frame = P->next_result;
                if (fp != P->poses.end()) *pose = fp->second;
            }
            if (fp != P->poses.end()) P->poses.erase(fp);
            auto why = P->result_errors.find(P->next_result);
            if (why != P->result_errors.end()) {   // (the frame's own status is in result->status; the text goes where every entry point leaves it)
                set_last_error(why->second);
                P->result_errors.erase(why);
            }
            P->next_result++;
            ready = 1;
            return;
        }
        if (P->failed) fail(P->fail_code, P->fail_msg);
    });
    return rc != APDS_OK ? rc : (ready ? APDS_OK : APDS_PIPELINE_NOT_READY);
}

int apds_pipeline_enable_pose(void* pipe, const apds_pipeline_pose_params* pose) {
    return guarded([&] {
        // the parameters first: every argument error is found before the handle is touched
        APDS_REQUIRE(pose, APDS_ERR_BAD_ARG, "null pose parameters");
        Pipeline* Q = pipe ? static_cast<Pipeline*>(pipe) : nullptr;
        const bool per_frame = Q && Q->table;
        APDS_REQUIRE(per_frame || pose->db_xyz_dev, APDS_ERR_BAD_ARG, "the DB rows' world points are required (n_db_total x 3 doubles)");
        APDS_REQUIRE(!per_frame || !pose->db_xyz_dev, APDS_ERR_BAD_ARG, "a table pipeline takes the world points from the table: db_xyz_dev must be NULL");
        const double* K = pose->camera_intrinsic;
        APDS_REQUIRE(std::isfinite(K[0]) && std::isfinite(K[4]) && K[0] > 0 && K[4] > 0, APDS_ERR_BAD_ARG, "the focal lengths must be finite and positive");
        APDS_REQUIRE(pose->method >= APDS_SOLVEPNP_ITERATIVE && pose->method <= APDS_SOLVEPNP_SQPNP, APDS_ERR_NOT_IMPLEMENTED,
                     "unknown cv::SolvePnPMethod (MAX_COUNT and beyond)");
        Pipeline* P = pipe_handle(pipe);
        const auto one = configure_lock(P, "the pose stage is enabled before the first submit");
        APDS_REQUIRE(!P->pose_on, APDS_ERR_BAD_ARG, "the pose stage is already enabled");
        if (P->table) {   // the views gather the table's xyz column: it has to cover every row now (the table is frozen from here on)
            void* xyz = nullptr;
            const int rc = apds_db_table(P->table, nullptr, nullptr, &xyz, nullptr);
            if (rc != APDS_OK) fail(rc, apds_last_error());
            APDS_REQUIRE(xyz, APDS_ERR_BAD_ARG, "the table's world points are absent or older than its rows (apds_db_world_coordinates)");
        }
        P->pose = *pose;
        if (P->pose.iter_count <= 0) P->pose.iter_count = 100;
        if (P->pose.reproj_thres <= 0) P->pose.reproj_thres = 8.0f;
        if (!(P->pose.confidence > 0 && P->pose.confidence < 1)) P->pose.confidence = 0.99;
        DeviceGuard on(P->device);
        if (!P->st_pose) HIP_CHECK(hipStreamCreateWithPriority(&P->st_pose, hipStreamNonBlocking, config().pipe_prio));
        const size_t cap = (size_t)P->cap;
        for (auto& s : P->slots) {
            if (!s->pose_img) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&s->pose_img), cap * 2 * sizeof(float)));
            if (!s->pose_obj) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&s->pose_obj), cap * 3 * sizeof(float)));
            if (!s->ev_homography) HIP_CHECK(hipEventCreateWithFlags(&s->ev_homography, hipEventDisableTiming));
            if (!P->table) s->train.xyz = pose->db_xyz_dev;   // (a table pipeline: each frame's select gives its view's)
        }
        P->pose_on = true;
        Pipeline* raw = P;
        P->threads.emplace_back([raw] { raw->worker("pose", [&] { raw->pose_worker(); }); });
    });
}

int apds_pipeline_set_matcher(void* pipe, int matcher) {
    return guarded([&] {
        // the three contract checks first, before any device work
        APDS_REQUIRE(matcher == APDS_PIPELINE_MATCH_RATIO || matcher == APDS_PIPELINE_MATCH_CROSSCHECK || matcher == APDS_PIPELINE_MATCH_L2_RATIO, APDS_ERR_BAD_ARG,
                     "matcher: APDS_PIPELINE_MATCH_RATIO (0), APDS_PIPELINE_MATCH_CROSSCHECK (1) or, on a float pipeline, APDS_PIPELINE_MATCH_L2_RATIO (2)");
        Pipeline* P = pipe_handle(pipe);
        APDS_REQUIRE(P->float_rows == (matcher == APDS_PIPELINE_MATCH_L2_RATIO), APDS_ERR_BAD_ARG,
                     P->float_rows ? "a float pipeline's matcher is APDS_PIPELINE_MATCH_L2_RATIO for life" : "APDS_PIPELINE_MATCH_L2_RATIO needs a float pipeline (apds_pipeline_create_float, or apds_pipeline_create_table on a float table)");
        APDS_REQUIRE(matcher == APDS_PIPELINE_MATCH_RATIO || !(P->shard || P->world > 1), APDS_ERR_NOT_IMPLEMENTED,
                     "the cross-check over a row-sharded train set (the per-query minimum across shards) is not built");
        const auto one = configure_lock(P, "the matcher is chosen before the first submit");
        if (matcher == APDS_PIPELINE_MATCH_CROSSCHECK) {
            // every slot's train_best: one key per train row (a table pipeline: per row a view can hold); the swapped scan's searching side
            // counts its rows in an int
            APDS_REQUIRE(P->table || P->train.n_rows <= (int64_t)INT_MAX, APDS_ERR_ASSERT, "the train rows are the searching side of the swapped scan: at most INT_MAX of them");
            const size_t rows = P->table ? (size_t)(P->view_capacity > 0 ? std::min(P->view_capacity, APDS_MAX_POINTS) : APDS_MAX_POINTS) : (size_t)P->train.n_rows;
            DeviceGuard on(P->device);
            for (auto& s : P->slots)
                if (!s->train_best) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&s->train_best), rows * sizeof(uint64_t)));
            if (P->db_expanded && !P->db_plain_pc) {
                HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&P->db_plain_pc), (size_t)P->train.n_rows * sizeof(float)));
                hm_train_plain_popcounts_device(P->db_expanded, P->db_plain_pc, P->st_match);
                HIP_CHECK(hipStreamSynchronize(P->st_match));
            }
        }
        P->matcher = matcher;
    });
}

int apds_pipeline_set_lens(void* pipe, const double* K, const double* dist, int n_dist, int iters) {
    return guarded([&] {
        lens::Lens L;
        const bool distorts = lens_from_args(K, dist, n_dist, &L);   // the argument checks first, before the handle is touched
        Pipeline* P = pipe_handle(pipe);
        const auto one = configure_lock(P, "the lens is set before the first submit");
        P->lens = L;
        P->lens_iters = iters > 0 ? iters : lens::DEFAULT_ITERS;
        P->lens_on = distorts;   // no distortion: the stages launch what they launched without a lens
    });
}

int apds_pipeline_stats(void* pipe, apds_pipeline_counters* out, int reset) {
    return guarded([&] {
        Pipeline* P = pipe_handle(pipe);
        APDS_REQUIRE(out, APDS_ERR_BAD_ARG, "null output");
        std::memset(out, 0, sizeof(*out));
        if (P->p.timing) {
            // the kernel timers are HIP events held by the worker threads: once the pipeline is idle every worker is asked (a null job through
            // its own queue) to add its finished timers to the totals
            std::unique_lock<std::mutex> g(P->m);
            P->cv.wait(g, [&] { return P->done >= P->next_submit || P->failed; });
            if (!P->failed && !P->closing) {
                P->harvest_acks = 0;
                const int64_t consumed = P->next_submit;
                g.unlock();
                for (auto& q : P->q_jobs) q->push(nullptr);
                if (P->world > 1 || P->shard) P->q_ext[(size_t)(consumed % P->E)]->push(nullptr);
                else P->q_any.push(-1);
                P->q_homography.push(nullptr);
                g.lock();
                P->cv.wait(g, [&] { return P->harvest_acks >= P->E + 2 || P->failed; });
            }
        }
        std::lock_guard<std::mutex> g(P->m);
        out->frames_submitted = P->next_submit;
        out->frames_done = P->done;
        auto get = [&](const char* n, double& ms, int& k) {
            auto it = P->timers.find(n);
            if (it != P->timers.end()) ms = it->second.first, k = it->second.second;
        };
        get("hamming_topk", out->hamming_topk_ms, out->hamming_topk_launches);
        get("hamming_topk_sample", out->hamming_topk_sample_ms, out->hamming_topk_sample_launches);
        get("akaze_extract", out->akaze_extract_ms, out->akaze_extract_calls);
        get("ransac_score", out->ransac_score_ms, out->ransac_score_launches);
        out->match_gaps = (int)P->gaps.size();
        double sum = 0;
        for (size_t i = 0; i < P->gaps.size(); i++) {
            sum += P->gaps[i];
            if (i < 16) out->match_gaps_first_ms[i] = P->gaps[i];
        }
        out->match_gap_mean_ms = P->gaps.empty() ? 0.0 : sum / (double)P->gaps.size();
        for (size_t i = 0; i < P->cap_gaps.size() && i < 6; i++) out->match_lds_cap_gaps_ms[i] = P->cap_gaps[i];
        out->match_lds_cap_bytes = P->p.match_lds_cap > 0 ? P->p.match_lds_cap : P->cap_bytes;
        out->match_lds_cap_set_at_frame = P->cap_frame;
        out->extract_workers = P->E;
        out->slots = (int)P->slots.size();
        out->split_scan = P->split ? 1 : 0;
        out->world = P->world;
        if (reset) {
            P->timers.clear();
            P->gaps.clear();
        }
    });
}

int apds_pipeline_destroy(void* pipe) {
    return guarded([&] {
        if (!pipe) return;
        destroy_pipeline(static_cast<Pipeline*>(pipe));
    });
}

}  // extern "C"
