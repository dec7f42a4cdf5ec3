// csrc/pipeline_match.cpp — the streamed pipeline's match stage: one worker that scans each frame against its slot's train side
// (pipeline.h) on one GPU, with the starvation watch, or the worker that issues a row-sharded DB's collectives in frame order.
#include "pipeline.h"

namespace apds {

namespace {

// Starvation watch: the match stream should never wait for a frame. On some boxes the short extraction kernels are dispatched so late
// under the match kernel, which owns every wave slot, that extraction paces the pipeline. The gap on the match stream between one
// frame's last match kernel and the next frame's first is measured with events; if three of six consecutive gaps exceed 4 ms (healthy:
// 0.01 / 1.2 ms alternating) the main scan's occupancy is capped at two workgroups per CU (apds_dev_match_lds_cap), which leaves
// wave slots for the other stages at ~1.5 % of match throughput. The cap is scoped to THIS thread's scan launches (set_thread_scan_cap):
// other matchers of the process are not touched and nothing has to be restored.
struct GapWatch {
    std::deque<std::pair<Slot*, Slot*>> pending;   // (previous frame, this frame): gap = prev.ev_mend -> this.ev_mstart
    std::vector<float> recent;

    // frame s has been issued behind prev; true: the cap has just been set, and the watch is over
    bool issued(Pipeline& P, Slot* prev, Slot* s, int64_t seen) {
        if (prev && seen >= 4) pending.emplace_back(prev, s);   // the first frames are the pipeline filling up
        while (!pending.empty() && hipEventQuery(pending.front().second->ev_mstart) == hipSuccess) {
            float g = -1;
            // (a slot that was re-used in the meantime re-recorded its events: the sample is skipped)
            if (hipEventElapsedTime(&g, pending.front().first->ev_mend, pending.front().second->ev_mstart) != hipSuccess) (void)hipGetLastError(), g = -1;
            pending.pop_front();
            if (g >= 0 && g < 1000) {
                recent.push_back(g);
                std::lock_guard<std::mutex> lk(P.m);
                P.gaps.push_back(g);
            }
        }
        (void)hipGetLastError();   // hipEventQuery's hipErrorNotReady is not an error
        int late = 0;
        for (size_t i = recent.size() >= 6 ? recent.size() - 6 : 0; i < recent.size(); i++) late += recent[i] > 4.0f;
        if (recent.size() < 6 || late < 3 || P.cap_bytes != 0) return false;
        set_thread_scan_cap(55000);
        std::lock_guard<std::mutex> lk(P.m);
        P.cap_bytes = 55000;
        P.cap_frame = (int)s->index;
        for (size_t i = recent.size() - 6; i < recent.size(); i++) P.cap_gaps.push_back(recent[i]);
        return true;
    }
};

}  // namespace

// ---- stage 2: match (one GPU) ------------------------------------------------------------------------------------------------------
void Pipeline::match_worker() {
    const std::initializer_list<const char*> timed = {"hamming_topk", "hamming_topk_sample"};
    bool watch = adaptive_cap;
    if (p.match_lds_cap > 0 && !float_rows) set_thread_scan_cap(p.match_lds_cap), watch = false;   // the caller asked for a cap from the first frame on
    GapWatch gap_watch;
    Slot* prev = nullptr;
    int e = 0;
    int64_t seen = 0;
    while (q_any.pop(e)) {
        // cross-check mode: one roles-swapped top-1 per frame (every train row's nearest query) on the single-stream branch; the split
        // scan, the threshold pre-pass and the starvation watch belong to the ratio matcher
        const bool crosscheck = matcher == APDS_PIPELINE_MATCH_CROSSCHECK;
        if (e < 0) {
            harvest(timed);
            continue;
        }
        // One GPU: nothing requires frame order on the match stream (results are stored by frame index), so frames are matched first come,
        // first served: one of the two extraction workers tends to finish just after a match ends, and in frame order the match stream
        // then waited ~1.2 ms for every second frame
        Slot* s = nullptr;
        if (!q_ext[(size_t)e]->pop(s)) break;
        const int K = s->K;
        TrainSide& T = s->train;
        if (table) {
            // the frame's train set first: the select needs nothing from the extraction. Its one synchronisation waits for the previous
            // frame's scan on this stream; the cut, sort and gather it queues run in front of this frame's scan.
            int n_view = 0;
            PIPE_OK(apds_db_view_select(s->view, s->sel.mode, s->sel.value, s->sel.x_start, s->sel.y_start, s->sel.x_end, s->sel.y_end, pose_on ? 1 : 0,
                                        st_match, &n_view));
            T.n_rows = T.n_kps = n_view;
            void* xyz = nullptr;
            PIPE_OK(apds_db_view_pointers(s->view, nullptr, nullptr, nullptr, nullptr, &xyz, nullptr));
            T.xyz = xyz;
        }
        if (K > 0 && split && !crosscheck) {
            HIP_CHECK(hipStreamWaitEvent(st_pre, s->ev_extract, 0));   // threshold pre-pass: beside the previous frame's main scan
            PIPE_OK(apds_dev_topk_prepass(s->topk_state, s->desc, K, T.rows, T.n_rows, T.index_base, 2, st_pre));
            HIP_CHECK(hipEventRecord(s->ev_pre, st_pre));
            HIP_CHECK(hipStreamWaitEvent(st_match, s->ev_pre, 0));
            HIP_CHECK(hipEventRecord(s->ev_mstart, st_match));
            PIPE_OK(apds_dev_topk_scan(s->topk_state, s->desc, T.rows, st_match));
            HIP_CHECK(hipEventRecord(s->ev_scan, st_match));
            HIP_CHECK(hipEventRecord(s->ev_mend, st_match));
            HIP_CHECK(hipStreamWaitEvent(st_merge, s->ev_scan, 0));    // record merge: beside the next frame's main scan
            PIPE_OK(apds_dev_topk_merge(s->topk_state, T.index_base, s->keys, st_merge));
            HIP_CHECK(hipEventRecord(s->ev_match, st_merge));
        } else {
            HIP_CHECK(hipStreamWaitEvent(st_match, s->ev_extract, 0));
            HIP_CHECK(hipEventRecord(s->ev_mstart, st_match));
            if (T.n_rows < 2) {   // a selection of that size (a fixed train set has two rows since create): what such a train set is to apds_pipeline_create
                if (s->status == APDS_OK) {
                    s->status = APDS_ERR_ASSERT;
                    s->error = "the frame's selection has fewer than two rows: a train set of at least two rows is required";
                }
            } else if (K > 0 && float_rows) {   // the resident L2 train set (a view's: what the select's gather has just queued on this stream), screen mode: 3.1 ms against 16.0 ms exact on M-SURF rows (the screen reads its candidate counts back: this thread waits for the frame's passes)
                PIPE_OK(apds_dev_l2_train_top2(T.l2, s->desc, K, APDS_L2_SCREEN, s->keys, st_match, nullptr, nullptr));
            } else if (K > 0 && crosscheck && db_expanded) {   // the resident expanded copy as the searching side: only the frame's rows are expanded
                PIPE_OK(guarded([&] {
                    QueuedWorkspaceCall call(st_match);
                    hamming_mfma_swapped_top1_device(s->desc, K, db_expanded, db_plain_pc, s->train_best, st_match);
                }));
            } else if (K > 0 && crosscheck) {   // (vector-ALU matcher, or a view: the swapped scan directly)
                PIPE_OK(apds_dev_hamming_topk(T.rows, (int)T.n_rows, s->desc, K, 0, 1, s->train_best, st_match));
            } else if (K > 0 && db_expanded) {   // the matrix-core matcher on the DB's expanded copy
                PIPE_OK(guarded([&] {
                    QueuedWorkspaceCall call(st_match);   // (as apds_dev_hamming_topk does: the scan's scratch is this thread's workspace, and it is queued on return)
                    hamming_mfma_topk_train_device(s->desc, K, db_expanded, T.index_base, 2, static_cast<uint64_t*>(s->keys), st_match);
                }));
            } else if (K > 0) {
                PIPE_OK(apds_dev_hamming_topk(s->desc, K, T.rows, T.n_rows, T.index_base, 2, s->keys, st_match));
            }
            HIP_CHECK(hipEventRecord(s->ev_match, st_match));
            HIP_CHECK(hipEventRecord(s->ev_mend, st_match));
        }
        if (watch && !crosscheck && gap_watch.issued(*this, prev, s, seen)) watch = false;
        prev = s;
        seen++;
        q_homography.push(s);
    }
    collect(timed);
    q_homography.close();
}

// ---- stage 2: match (row-sharded DB) -----------------------------------------------------------------------------------------------
// This thread issues ALL collectives of the pipeline, in frame order, the same order on every rank: counts(i) [a tiny all-gather on its
// own stream; the only host synchronisation, and frame i-1's scan is already queued behind it], gather(i) [its own stream, after that
// frame's extraction] BEFORE exchange(i-1) [match stream, after scan(i-1)]: the query all-gather of a frame travels under the previous
// frame's scan. Deferring exchange(i-1) until frame i has arrived is only safe when frame i is certain to arrive on EVERY rank, and the
// choice must be the same everywhere (the collectives' order is at stake): each rank adds to its count a flag "frame i+1 is already
// submitted here", and frame i's exchange is deferred iff every rank set it. A host that streams (submits ahead of the results) gets
// the overlap on all frames but its last; a host that submits one frame and waits gets that frame's result without a successor.
void Pipeline::sharded_match_worker() {
    const std::initializer_list<const char*> timed = {"hamming_topk", "hamming_topk_sample"};
    constexpr int NEXT_FLAG = 1 << 30;
    Slot* prev = nullptr;
    for (int64_t i = 0;; i++) {
        Slot* s = nullptr;
        if (!q_ext[(size_t)(i % E)]->pop(s)) break;
        if (!s) {   // apds_pipeline_stats on the idle pipeline (no frame is between gather and exchange)
            harvest(timed);
            i--;
            continue;
        }
        bool next_here;
        {
            std::lock_guard<std::mutex> g(m);
            next_here = next_submit > i + 1;
        }
        s->counts.assign((size_t)world, 0);
        PIPE_OK(apds_shard_counts(shard, s->K | (next_here ? NEXT_FLAG : 0), s->counts.data(), st_counts));
        bool next_everywhere = true;
        for (int& c : s->counts) {
            next_everywhere = next_everywhere && (c & NEXT_FLAG);
            c &= NEXT_FLAG - 1;
        }
        HIP_CHECK(hipStreamWaitEvent(st_gather, s->ev_extract, 0));
        PIPE_OK(apds_shard_gather(shard, s->shard_slot, s->K ? s->desc : nullptr, s->K, s->counts.data(), st_gather));
        auto finish_exchange = [&](Slot* f) {
            PIPE_OK(apds_shard_exchange_merge(shard, f->shard_slot, 2, f->keys, st_match));
            HIP_CHECK(hipEventRecord(f->ev_match, st_match));
            q_homography.push(f);
        };
        if (prev) finish_exchange(prev);
        prev = nullptr;
        PIPE_OK(apds_shard_scan(shard, s->shard_slot, 2, st_match));
        if (next_everywhere) prev = s;   // frame i+1 is on its way on every rank: its gather goes out first
        else finish_exchange(s);
    }
    collect(timed);
    q_homography.close();
}

}  // namespace apds
