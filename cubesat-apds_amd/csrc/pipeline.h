// csrc/pipeline.h — what the streamed frame pipeline's files share (internal): the queue between stages, a frame's slot with its train
// side, and the pipeline with its workers declared. The layout of the stages is described at the head of pipeline.cpp; the workers
// are defined in pipeline_stages.cpp (extraction, homography, pose) and pipeline_match.cpp (match, sharded match).
#pragma once
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

#include "config.h"
#include "kernels.h"

namespace apds {

// a blocking queue; close() wakes every waiter (pop then returns false once the queue is empty)
template <class T>
class Chan {
    std::mutex m;
    std::condition_variable cv;
    std::deque<T> q;
    bool closed = false;

public:
    void push(T v) {
        {
            std::lock_guard<std::mutex> g(m);
            q.push_back(std::move(v));
        }
        cv.notify_one();
    }
    bool pop(T& out) {
        std::unique_lock<std::mutex> g(m);
        cv.wait(g, [&] { return !q.empty() || closed; });
        if (q.empty()) return false;
        out = std::move(q.front());
        q.pop_front();
        return true;
    }
    void close() {
        {
            std::lock_guard<std::mutex> g(m);
            closed = true;
        }
        cv.notify_all();
    }
};

struct StageError {
    int code;
    std::string msg;
};
[[noreturn]] inline void stage_fail(int rc) { throw StageError{rc, apds_last_error()}; }
#define PIPE_OK(call)                       \
    do {                                    \
        const int rc_ = (call);             \
        if (rc_ != APDS_OK) stage_fail(rc_); \
    } while (0)

// The train set one frame is matched against, as every stage reads it. A fixed train set: the pipeline's own (Pipeline::train), copied
// into every slot at create. A table pipeline: the slot's view - the pointers never change, each frame's select sets the counts and xyz,
// and the contents hold until the slot's next frame.
struct TrainSide {
    const void* rows = nullptr;            // descriptor rows: 64 bytes each, or 64 floats (then l2 is set)
    int64_t n_rows = 0;                    // rows this GPU scans (a sharded DB: the local ones) ...
    uint32_t index_base = 0;               // ... and the first one's global index
    const apds_keypoint* kps = nullptr;    // the keypoints of ALL train rows, by global index ...
    int64_t n_kps = 0;                     // ... (a sharded DB: n_db_total, not n_rows)
    const void* xyz = nullptr;             // their world points (the pose stage)
    L2Train* l2 = nullptr;                 // float rows: the resident train set over them (the pipeline's, or borrowed from the view)
};

struct Slot {
    // device buffers of one frame in flight
    apds_keypoint* kps = nullptr;
    uint8_t* desc = nullptr;
    uint64_t* keys = nullptr;
    apds_dmatch* matches = nullptr;
    float *p1 = nullptr, *p2 = nullptr;
    uint8_t* mask = nullptr;
    uint8_t* frame_dev = nullptr;   // staging buffer of a host frame
    size_t frame_dev_bytes = 0;
    hipEvent_t ev_extract = nullptr, ev_pre = nullptr, ev_scan = nullptr, ev_match = nullptr;
    hipEvent_t ev_mstart = nullptr, ev_mend = nullptr;   // (timing enabled) the match stream's idle gaps: starvation watch
    void* topk_state = nullptr;   // split scan (one GPU)
    uint64_t* train_best = nullptr;   // cross-check mode (apds_pipeline_set_matcher): every train row's nearest query of this slot's frame
    void* shard_slot = nullptr;   // exchange slot (sharded DB)
    TrainSide train;
    // a table pipeline (apds_pipeline_create_table): this slot's view of the table and the frame's selection
    void* view = nullptr;
    apds_db_selection sel{};
    int owner = 0;
    // the job
    const void* src = nullptr;
    size_t stride = 0;
    bool on_device = false;
    int64_t index = 0;
    int K = 0, status = APDS_OK;
    std::string error;
    std::vector<int> counts;
    // the pose stage (apds_pipeline_enable_pose): the frame's 2D-3D pairs, and the homography stage's result handed on with the slot
    float *pose_img = nullptr, *pose_obj = nullptr;
    hipEvent_t ev_homography = nullptr;
    apds_frame_result res{};
    std::string res_why;
};

struct Pipeline {
    apds_pipeline_params p{};
    int device = 0;
    TrainSide train;               // the fixed train set (unused by a table pipeline); train.l2 is made at create and released at destroy
    void* db_expanded = nullptr;   // the train rows as matrix-core operands (hm_train_create), made once: the DB is resident for the pipeline's life
    void* shard = nullptr;
    int world = 1;
    void* table = nullptr;   // the train set is selected per frame from this keypoint table (borrowed)
    int cap = 0, E = 2;
    bool split = true, adaptive_cap = true, own_match_stream = true;
    double extract_delay_s = 0;

    std::vector<std::unique_ptr<Slot>> slots;
    std::vector<std::unique_ptr<Chan<Slot*>>> q_free, q_jobs, q_ext;
    Chan<int> q_any;          // which worker finished a frame (arrival order; one GPU)
    Chan<Slot*> q_homography, q_pose;
    std::vector<std::thread> threads;
    hipStream_t st_extract[8] = {}, st_match = nullptr, st_pre = nullptr, st_merge = nullptr, st_homography = nullptr, st_gather = nullptr, st_counts = nullptr;
    hipStream_t st_pose = nullptr;
    std::atomic<bool> pose_on{false};   // set once, before the first submit
    std::atomic<int> matcher{APDS_PIPELINE_MATCH_RATIO};   // set before the first submit (apds_pipeline_set_matcher)
    bool float_rows = false;        // M-SURF rows (256 bytes), the L2 matcher (matcher == APDS_PIPELINE_MATCH_L2_RATIO for life)
    float* db_plain_pc = nullptr;   // cross-check mode on the expanded copy: the train rows' popcounts as the swapped scan's column side takes them
    int view_capacity = 0;
    apds_pipeline_pose_params pose{};
    std::atomic<bool> lens_on{false};   // set before the first submit (apds_pipeline_set_lens), and only for a lens that distorts
    lens::Lens lens{};
    int lens_iters = lens::DEFAULT_ITERS;

    std::mutex m;   // results, counters, errors
    std::condition_variable cv;
    std::map<int64_t, apds_frame_result> results;
    std::map<int64_t, std::string> result_errors;
    std::map<int64_t, apds_frame_pose> poses;
    int64_t next_submit = 0, next_result = 0, done = 0;
    bool failed = false, closing = false;
    int fail_code = 0;
    std::string fail_msg;
    // statistics (timing enabled)
    std::map<std::string, std::pair<double, int>> timers;
    std::vector<float> gaps;
    int cap_bytes = 0, cap_frame = -1;
    std::vector<float> cap_gaps;   // the six gaps that triggered the cap
    int harvest_acks = 0;
    std::mutex submit_m;   // one submitter at a time keeps frame numbers and slot hand-out in step

    // pipeline.cpp
    void fail(int code, const std::string& msg);
    void close_all();
    // this worker thread's event timers of the named kernels -> the pipeline's totals (the events were recorded on the launch streams)
    void collect(std::initializer_list<const char*> names);
    void harvest(std::initializer_list<const char*> names);   // collect, for apds_pipeline_stats on the idle pipeline: acknowledged
    void finish(Slot* s, const apds_frame_result& r, const std::string& why, const apds_frame_pose* fp = nullptr);
    // pipeline_stages.cpp
    void extract_worker(int e);
    void homography_worker();
    void pose_worker();
    // pipeline_match.cpp
    void match_worker();
    void sharded_match_worker();

    template <class F>
    void worker(const char* what, F body) {
        try {
            PIPE_OK(apds_set_device(device));
            PIPE_OK(apds_dev_timing_enable(p.timing ? 1 : 0));
            body();
        } catch (const StageError& e) {
            fail(e.code, std::string(what) + ": " + e.msg);
        } catch (const Error& e) {
            fail(e.code, std::string(what) + ": " + e.msg);
        } catch (const std::exception& e) {
            fail(APDS_ERR_INTERNAL, std::string(what) + ": " + e.what());
        }
        (void)apds_dev_timing_enable(0);
        (void)apds_thread_release();   // this worker's stream + workspace go back to the process-wide cache
    }
};

}  // namespace apds
