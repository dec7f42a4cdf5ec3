// csrc/akaze_extract.hip — the AKAZE extraction driver: one call = one batch of equal-sized device images through the plan of
// akaze_plan.h, the filter launchers (the stage files akaze_base / _smooth_flow / _fed / _level_* / _resize / _doh_* .hip) and the keypoint launchers (akaze_suppress.hip,
// akaze_compact.hip, akaze_describe.hip).
//
// Replaces cv::AKAZE::detectAndCompute (AKAZEFeatures::Create_Nonlinear_Scale_Space, Feature_Detection, Compute_Descriptors) behind
// feature_extraction/src/lib.rs:61-92.
#include <chrono>

#include "akaze.h"
#include "config.h"

namespace apds {

AkazeDebugRequest& akaze_debug_request() {
    static thread_local AkazeDebugRequest r;
    return r;
}

// Zero the first `bytes` (a multiple of 16) of every image's slab: one launch for the batch. (hipMemset2DAsync / hipMemcpy2DAsync take a
// slow, serialising path in the runtime: with them N host threads extracting concurrently stopped scaling, 2200 -> 880 tiles/s.)
struct ZeroRanges {
    size_t from[3], bytes[3];   // 16-byte aligned offsets into the slab; blockIdx.y picks the range
};
__global__ void zero_slab_heads_kernel(char* __restrict__ base, ZeroRanges r, size_t bstride) {
    APDS_RAISE_WAVE_PRIORITY();
    uint4* p = reinterpret_cast<uint4*>(base + (size_t)blockIdx.z * bstride + r.from[blockIdx.y]);
    const size_t n = r.bytes[blockIdx.y] / 16;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = make_uint4(0, 0, 0, 0);
}

// out[b * n + i] = src_b[i] for the first n ints at `src` of every image's slab
__global__ void gather_slab_ints_kernel(const int* __restrict__ src, int n, size_t bstride, int batch, int* __restrict__ out) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * batch) return;
    const int b = i / n, k = i - b * n;
    out[i] = reinterpret_cast<const int*>(reinterpret_cast<const char*>(src) + (size_t)b * bstride)[k];
}
namespace {

template <class T>
T* upload(const std::vector<T>& v, hipStream_t s) {
    T* d = ctx().alloc_n<T>(v.size());
    HIP_CHECK(hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return d;
}

// What the steps of one call share: the caller's stream, the batch, the plan and the slab.
struct Frame {
    ThreadCtx& c;
    hipStream_t s;
    Batch bt;
    std::vector<LevelDesc> ev;
    SlabLayout sl;
    ExtractionPlan plan;      // which kernels serve every level (akaze_plan.h)
    bool dense_det = false;   // the determinant plane of a level is stored whole only when somebody asked to see it (apds_akaze_debug_plane)
    int levels() const { return (int)ev.size(); }
};

// Zero the counters at the head of every slab and the masks / statuses of the levels that need it. The streaming Hessian kernel
// (akaze_doh_strips.hip) writes the keypoint-mask byte and the suppression-status byte of EVERY pixel of its level, so those levels - the
// large ones, a prefix of the level list - need no clearing. (Round 2 cleared all of it: 181 MB per 4096^2 frame.)
void zero_slab_heads(const Frame& f) {
    const SlabLayout& sl = f.sl;
    const int B = f.bt.n;
    const int n_strip = f.plan.n_strip_levels;
    const size_t first = n_strip < f.levels() ? (size_t)f.ev[n_strip].pix_offset : (size_t)sl.total_pix;
    ZeroRanges zr{};
    zr.from[0] = 0;
    zr.bytes[0] = sl.mask_off;                                                   // counters (all planes start on 256-byte boundaries)
    zr.from[1] = sl.mask_off + (first & ~(size_t)15);
    zr.bytes[1] = (sl.status_off - zr.from[1]) & ~(size_t)15;                    // masks of the remaining levels + the padding line behind the last one
    zr.from[2] = sl.status_off + (first & ~(size_t)15);
    zr.bytes[2] = (sl.zero_bytes - zr.from[2]) & ~(size_t)15;
    const size_t most = std::max(zr.bytes[0], std::max(zr.bytes[1], zr.bytes[2]));
    // (the runtime's fill kernel reaches 1.7 TB/s; 16-byte stores from a wide grid are quicker)
    hipLaunchKernelGGL(zero_slab_heads_kernel, dim3((unsigned)std::min<size_t>(B > 1 ? 1024 : 4096, (most / 16 + 255) / 256), 3, B), dim3(256), 0, f.s,
                       reinterpret_cast<char*>(sl.list_count), zr, f.bt.stride);   // (list_count is the first thing in a slab)
}

// The fork of the Hessian / extrema kernels to a second stream, and the join. The Hessian kernel of a level hangs off the main chain (it
// only needs the level's Lsmooth and nothing waits for it before the suppression): on a second stream the latency-bound launches of the
// small octaves overlap the smoothing and diffusion launches of the levels that follow. Lsmooth then needs a plane per level.
//
// It shortens a LONE caller's extraction (4096^2: 2.19 -> 2.08 ms, 512^2: 0.48 -> 0.45), but when several host threads extract at once (the
// reference's rayon pool, main.rs:233-243) extra streams make the threads' streams share the few hardware queues and the threads serialise
// each other — even an idle side stream shifts the mapping: 4 threads reach 2400 tiles/s of 1024^2 when no thread ever forked, 1240 - 1320
// when some did. So a thread forks only while it is the ONLY host thread holding a library context (apds_thread_release drops one);
// APDS_AKAZE_FORK = 0 never, 2 always.
// (A call costs the host ~3.5 us per launch, event record or stream wait, ~90 of them: a 512^2 tile's 0.32 ms is mostly that. Not forking
// below 0.5 Mpx saves 30 of those calls and was measured both ways: 0.355 against 0.367 ms in tools/ab_probe.py, 0.36 against 0.32 in
// tools/extract_probe.py — no threshold.)
// (Round 3, measured and removed: holding the first octave's four big Hessian kernels back until the level chain has left that octave, on
// a stream of their own, so that they run under the latency-bound chains of the later octaves instead of beside the first octave's
// bandwidth-bound ones: 1.828 against 1.807 ms at 4096^2 - they are off the critical path either way, which is the level chain
// followed by the keypoint tail, and beside the small octaves' kernels they delay those. Lowest priority for the side streams: no
// difference. profiles/r03/doh_ab.txt)
// (a stream of their own for the small levels' Hessian kernels, which queue up behind the large levels' on this one: measured, no gain)
//
// The fork is an event: hipEventRecord on the main stream where a level's Lsmooth exists, hipStreamWaitEvent on the Hessian stream. In a
// chain of short kernels an event recorded on the main stream costs 3.4 us each time (the marker packet sits between two dependent
// kernels: tools/probes/fork_probe.hip, profiles/r04/fork_probe.txt - 16 forks: 236 us against 174 for the same kernels without any
// dependency), and under rocprofv3 the timeline shows 5 us gaps behind every fork.
// (Round 4, measured and removed: the value fork - the next kernel of the chain stores a sequence number as its first act and the Hessian
// stream waits for that value in signal memory, so that nothing sits between the chain's kernels: 189 us in the probe, but 1.635 against
// 1.641 ms on the real frame over nine same-box rounds, profiles/r04/ab_env_flag_fork.txt - the chain's kernels are long and the marker is
// processed under the tail of the one before it; the 42 us the profiled timeline promises, profiles/r04/timeline_flag_fork.txt, are the
// profiler's. 6 us do not pay for a polling kernel per fork. DESIGN_HISTORY.md)
// (Round 4, measured and removed: the early fork - level 0's Hessian kernel needs Lt[0] only and started after the fused base pass, beside
// the contrast-factor pass: 1.649 / 1.656 / 1.642 against 1.649 / 1.636 / 1.636 ms, profiles/r04/ab_env_half_fuse.txt - the histogram
// kernel the level chain waits for shares the machine with a kernel nothing waits for, and what the Hessian stream gains at the front it has
// no use for at the back: its kernels follow the level chain from the second octave on.)
class HessianFork {
  public:
    const bool on;   // the Hessian kernels go to a side stream

    HessianFork(ThreadCtx& c, hipStream_t s) : on(decide()), c(c), s(s), s_doh(s) {
        if (c.fork_open) {   // an earlier call failed between fork and join (whether or not THIS call forks): its side-stream kernels may still use the workspace
            if (c.side) HIP_CHECK(hipStreamSynchronize(c.side));
            for (hipStream_t st : c.side_pool)
                if (st) HIP_CHECK(hipStreamSynchronize(st));
            c.fork_open = false;
        }
    }
    // after the base stage: pick the side stream
    void open(const Frame& frame) {
        f = &frame;
        if (on) s_doh = side_stream_beside(s);
    }
    // Lsmooth of level i exists from here on (level 0: Lt[0], ready after the base stage)
    void smooth_ready(int i) {
        if (!on) return;
        if (i == 0) c.fork_open = true;
        HIP_CHECK(hipEventRecord(c.fork_event(i), s));
        HIP_CHECK(hipStreamWaitEvent(s_doh, c.fork_event(i), 0));
    }
    // a1.5 + a1.6 of level i: first / second derivatives, determinant, and the level's 3x3 extrema (mask + candidate list)
    void hessian(int i, const float* smooth) {
        const LevelDesc& le = f->ev[i];
        const SlabLayout& sl = f->sl;
        float kside, kmid;
        deriv_weights(le.sigma_size, kside, kmid);
        uint8_t* mask = sl.mask_all + le.pix_offset;
        if (f->plan.level[i].doh_strips)
            launch_doh_strips(smooth, sl.Lxy[i], sl.Ldet[i], le.w, le.h, le.sigma_size, kside, kmid, le.border, AKAZE_DTHRESHOLD, mask, sl.status_all + le.pix_offset,
                              sl.list[i], sl.list_count + i, s_doh, f->bt, f->dense_det);
        else
            launch_doh_fused(smooth, sl.Lxy[i], sl.Ldet[i], le.w, le.h, le.sigma_size, kside, kmid, le.border, AKAZE_DTHRESHOLD, mask, sl.list[i], sl.list_count + i,
                             s_doh, f->bt);
    }
    // everything after this point reads what the Hessian kernels wrote
    void join() {
        if (!on) return;
        if (!c.join_event) HIP_CHECK(hipEventCreateWithFlags(&c.join_event, stream_event_flags()));
        HIP_CHECK(hipEventRecord(c.join_event, s_doh));
        HIP_CHECK(hipStreamWaitEvent(s, c.join_event, 0));
        c.fork_open = false;
    }

  private:
    static bool decide() {
        const int fork_env = config().akaze_fork;
        return fork_env == 2 || (fork_env == 1 && live_contexts().load() <= 1);
    }

    ThreadCtx& c;
    const hipStream_t s;
    hipStream_t s_doh;
    const Frame* f = nullptr;
};

// ---- a1.1 / a1.2 / a1.3: gray, Lt[0] (= Lsmooth[0]) and the contrast factor of every octave
void base_stage(const Frame& f, BaseStage kind, const void* img, int channels, size_t stride) {
    const SlabLayout& sl = f.sl;
    const int W = f.ev[0].w, H = f.ev[0].h, L = f.levels(), n_oct = f.ev.back().octave + 1;
    const GaussTaps g16 = gauss_taps(9, (double)AKAZE_SOFFSET), g10 = gauss_taps(5, 1.0);
    switch (kind) {
        case BaseStage::Strips:   // large images: one fused pass
            launch_base_strips(img, H, W, channels, stride, g16, g10, sl.Lt[0], sl.tmpF, sl.hmax_bits, L > 1, f.s, f.bt);
            if (L > 1) launch_kcontrast(nullptr, sl.tmpF, W, H, sl.hmax_bits, sl.hist, sl.k_oct, n_oct, f.s, f.bt, /*gradient_done=*/true);
            break;
        case BaseStage::Separate:
            launch_gray(img, H, W, channels, stride, sl.gray, f.s, f.bt);
            launch_gauss(sl.gray, sl.Lt[0], W, H, g16, 4, f.s, f.bt);
            if (L > 1) {
                launch_gauss(sl.gray, sl.tmpS, W, H, g10, 2, f.s, f.bt);
                launch_kcontrast(sl.tmpS, sl.tmpF, W, H, sl.hmax_bits, sl.hist, sl.k_oct, n_oct, f.s, f.bt);
            }
            break;
    }
}

// ---- a1.4 / a1.5 per level, as the plan says: start image, a separate smoothing pass or a head that smooths (either makes the level's
// Lsmooth, which its Hessian kernel waits for), FED passes ping-ponging into Lt[i], the Hessian kernel.
// Round 4: the launch that finishes the last level of an octave also writes the next octave's start image (the 2 x 2 area means of its
// Lt, into tmpH) when its kernel family can (level_stream, nld_strip, level_fused): half_sample_kernel - 40 + 14 + 5 us of passes over
// finished planes on the critical path of a 4096^2 frame - then does not run. APDS_HALF_FUSE=0: always the separate kernel.
struct LevelChain {
    const Frame& f;
    HessianFork& fork;
    const GaussTaps g10 = gauss_taps(5, 1.0);

    // the level's starting image: the previous level's Lt, or at the start of an octave its half-size image
    const float* start_image(int i, const LevelPlan& p) {
        const LevelDesc &e = f.ev[i], &prev = f.ev[i - 1];
        const SlabLayout& sl = f.sl;
        float* dst = p.start_in_lt() ? sl.Lt[i] : sl.tmpP;
        switch (p.start) {
            case Start::PrevLt: return sl.Lt[i - 1];
            case Start::Written: return sl.tmpH;
            case Start::HalfSample: launch_half_sample(sl.Lt[i - 1], prev.w, dst, e.w, e.h, f.s, f.bt); break;
            case Start::AreaResize: {
                std::vector<int> xo, yo, xc, yc;
                std::vector<float> xw, yw;
                area_tables(prev.w, e.w, xo, xw, xc);
                area_tables(prev.h, e.h, yo, yw, yc);
                HIP_CHECK(hipStreamSynchronize(f.s));   // host tables must outlive the async copies
                launch_area_resize(sl.Lt[i - 1], prev.w, dst, e.w, e.h, upload(xo, f.s), upload(xw, f.s), upload(xc, f.s), upload(yo, f.s), upload(yw, f.s), upload(yc, f.s), f.s, f.bt);
                HIP_CHECK(hipStreamSynchronize(f.s));
                break;
            }
        }
        return dst;
    }

    void step(int i) {
        const LevelDesc& e = f.ev[i];
        const SlabLayout& sl = f.sl;
        const hipStream_t s = f.s;
        const Batch& bt = f.bt;
        if (i == 0) {
            fork.smooth_ready(0);
            fork.hessian(0, sl.Lt[0]);
            return;
        }
        const LevelPlan& p = f.plan.level[i];
        const float* P = start_image(i, p);
        const float* kptr = sl.k_oct + e.octave;
        float* const smooth = sl.lsm[i];
        float st[32];
        // pass `q`: its step sizes into st, where it lands, whether it also leaves the next octave's start image
        struct Pass {
            int n;
            float* out;
            float* half_out;
        };
        const auto prepare = [&](int q) {
            for (int j = 0; j < p.steps[q]; j++) st[j] = e.tau[p.first[q] + j] * 0.5f;
            return Pass{p.steps[q], p.lands_in_lt(q) ? sl.Lt[i] : sl.tmpP, q == p.half_pass ? sl.tmpH : nullptr};
        };
        const bool smooth_first = p.smooth != Smooth::None;
        if (smooth_first) {
            launch_smooth_flow(P, smooth, sl.tmpF, e.w, e.h, g10, kptr, s, bt, p.smooth == Smooth::Strips);   // Lsmooth and the conductivity in one pass
            fork.smooth_ready(i);
        }
        const float* in = P;
        if (p.head != Head::None) {
            const Pass a = prepare(0);
            float* flow = !smooth_first && p.launches > 1 ? sl.tmpF : nullptr;   // the conductivity, for the passes that follow
            switch (p.head) {
                case Head::Stream: launch_level_stream(P, smooth, flow, a.out, e.w, e.h, g10, kptr, st, a.n, s, bt, a.half_out); break;
                case Head::Strips: launch_level_strips(P, smooth, flow, a.out, e.w, e.h, g10, kptr, st, a.n, s, bt); break;
                default: launch_level_fused(P, smooth, flow, smooth_first ? sl.tmpF : nullptr, a.out, e.w, e.h, g10, kptr, st, a.n, s, bt, a.half_out); break;
            }
            if (!smooth_first) fork.smooth_ready(i);
            in = a.out;
        }
        for (int q = p.first_fed_pass(); q < p.launches; q++) {
            const Pass a = prepare(q);
            if (p.strip_pass[q]) launch_nld_strips(in, sl.tmpF, a.out, e.w, e.h, st, a.n, s, bt, a.half_out);
            else launch_nld_tiles(in, sl.tmpF, a.out, e.w, e.h, st, a.n, s, bt);
            in = a.out;
        }
        if (e.nsteps == 0 && P != sl.Lt[i])   // (never with AKAZE's parameters: every level but the first has FED steps)
            for (int bi = 0; bi < bt.n; bi++)
                HIP_CHECK(hipMemcpyAsync(reinterpret_cast<char*>(sl.Lt[i]) + (size_t)bi * bt.stride, reinterpret_cast<const char*>(P) + (size_t)bi * bt.stride,
                                         (size_t)e.w * e.h * 4, hipMemcpyDeviceToDevice, s));
        fork.hessian(i, smooth);
    }
};

// level table for the keypoint kernels (pointers of image 0; kernels add blockIdx.z * slab)
LevelTable level_table(const Frame& f) {
    LevelTable T{};
    const SlabLayout& sl = f.sl;
    T.n = f.levels();
    T.bstride = f.bt.stride;
    for (int i = 0; i < T.n; i++) {
        const LevelDesc& e = f.ev[i];
        T.w[i] = e.w;
        T.h[i] = e.h;
        T.octave[i] = e.octave;
        T.sigma_size[i] = e.sigma_size;
        T.border[i] = e.border;
        T.esigma[i] = e.esigma;
        T.ratio[i] = e.ratio;
        T.pix_offset[i] = e.pix_offset;
        T.Lt[i] = sl.Lt[i];
        T.Lxy[i] = sl.Lxy[i];
        T.Ldet[i] = sl.Ldet[i];
        T.mask[i] = sl.mask_all + e.pix_offset;
        T.list[i] = sl.list[i];
        T.ref[i] = reinterpret_cast<float*>(sl.pend[i]);   // the pending lists are idle once the suppression passes are done
    }
    T.pix_offset[T.n] = sl.total_pix;
    return T;
}

// Every image's keypoint count (kp_base[1] of its slab) on its way to pinned host memory; the caller waits for stream or event.
int* copy_counts(const Frame& f, int* counts_dev) {
    const int B = f.bt.n;
    int* K = f.c.pinned_ints(B);
    if (B == 1) {
        HIP_CHECK(hipMemcpyAsync(K, f.sl.kp_base + 1, sizeof(int), hipMemcpyDeviceToHost, f.s));
    } else {
        hipLaunchKernelGGL(gather_slab_ints_kernel, dim3(ceil_div(B, 256)), dim3(256), 0, f.s, (const int*)(f.sl.kp_base + 1), 1, f.bt.stride, B, counts_dev);
        HIP_CHECK(hipMemcpyAsync(K, counts_dev, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, f.s));
    }
    return K;
}

// the plane a test asked for (akaze_debug_request), of image 0 of the batch
void copy_debug_plane(const Frame& f, AkazeDebugRequest& dbg) {
    if (!dbg.armed || dbg.level < 0 || dbg.level >= f.levels()) return;
    const LevelDesc& e = f.ev[dbg.level];
    const SlabLayout& sl = f.sl;
    const size_t n = (size_t)e.w * e.h;
    const void* src = nullptr;
    size_t bytes = n * 4;
    if (dbg.which == 2 || dbg.which == 3)   // de-interleave one component of (Lx, Ly)
        HIP_CHECK(hipMemcpy2DAsync(dbg.host_out, 4, reinterpret_cast<const char*>(sl.Lxy[dbg.level]) + (dbg.which == 3 ? 4 : 0), 8, 4, n, hipMemcpyDeviceToHost, f.s));
    switch (dbg.which) {
        case 0: src = sl.Lt[dbg.level]; break;
        case 4: src = sl.Ldet[dbg.level]; break;
        case 7: src = sl.mask_all + e.pix_offset; bytes = n; break;   // NB: after the sub-pixel filter as well
        case 8: src = sl.k_oct; bytes = 4; break;
    }
    if (src) HIP_CHECK(hipMemcpyAsync(dbg.host_out, src, bytes, hipMemcpyDeviceToHost, f.s));
    HIP_CHECK(hipStreamSynchronize(f.s));
    dbg.armed = false;
}

// APDS_DEBUG_HOST_TIME=n: the host's share of a call (everything up to here is enqueue work; the GPU may still be running), every n calls
void report_host_time(int every, std::chrono::steady_clock::time_point t0, const Frame& f) {
    static thread_local double acc = 0;
    static thread_local int calls = 0;
    acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (++calls % every == 0) {
        fprintf(stderr, "[apds] akaze_extract %dx%d x%d: %.1f us of host enqueue time per call\n", f.ev[0].w, f.ev[0].h, f.bt.n, acc / every * 1e6);
        acc = 0;
    }
}

// Some image has more keypoints than max_points (rare): those images again, through the rank selection (response descending, ties by
// detection order) over ALL their K[bi] keypoints; the tables of image bi are image 0's shifted by bi slabs.
void select_strongest(const Frame& f, const LevelTable& T, const int* K, const int* counts, int max_points, apds_keypoint* kps_out, uint8_t* desc_out, int capacity,
                      int descriptor, size_t row_bytes) {
    const size_t slab = f.bt.stride;
    for (int bi = 0; bi < f.bt.n; bi++) {
        if (K[bi] <= max_points) continue;
        LevelTable Tb = T;
        Tb.bstride = 0;
        for (int i = 0; i < T.n; i++) {
            Tb.Lt[i] = reinterpret_cast<const float*>(reinterpret_cast<const char*>(T.Lt[i]) + (size_t)bi * slab);
            Tb.Lxy[i] = reinterpret_cast<const float2*>(reinterpret_cast<const char*>(T.Lxy[i]) + (size_t)bi * slab);
            Tb.Ldet[i] = reinterpret_cast<const float*>(reinterpret_cast<const char*>(T.Ldet[i]) + (size_t)bi * slab);
            Tb.mask[i] = T.mask[i] + (size_t)bi * slab;
        }
        const int keep = counts[bi];
        apds_keypoint* kp_b = kps_out + (size_t)bi * capacity;
        compact_strongest(Tb, f.sl, slab, bi, K[bi], keep, kp_b, f.s);
        describe_keypoints(Tb, kp_b, nullptr, keep, 0, desc_out + (size_t)bi * capacity * row_bytes, 0, ceil_div(keep, 4), 1, 0, f.s, descriptor);
    }
    HIP_CHECK(hipGetLastError());
    // these kernels read the calling thread's workspace (kps_all, masks, planes): the same thread's NEXT call, possibly on another
    // stream (apds_dev_* take one), starts by re-using that memory, so the rare over-capacity path ends synchronously like the main one
    HIP_CHECK(hipStreamSynchronize(f.s));
}

}  // namespace

// feature_extraction/src/lib.rs:61-92 on `n_img` device images of one size (a batch goes through every kernel's grid together:
// gridDim.z = n_img; a single image is a batch of one). Image i starts `img_bstride` bytes after image i-1; its keypoints go to
// kps_out + i * capacity, its descriptors to desc_out + i * capacity rows (64 bytes each, or 64 floats for APDS_AKAZE_DESCRIPTOR_KAZE), its
// count to counts[i] (host). Returns the largest count.
// pmask: the detection mask (a null base = none): keypoints whose refined position rounds onto a zero byte are dropped before the count,
// so max_points and `capacity` are about the survivors. mask_support > 0: any zero byte within mask_support units of the keypoint's level
// (akaze_plan.h: mask_support_unit) of that position drops it; the mask's summed-area table is built in the workspace for that.
int akaze_extract_batch_device(const void* img, int n_img, size_t img_bstride, int rows, int cols, int channels, size_t stride, const PixelMask& pmask,
                               int mask_support, int max_points, apds_keypoint* kps_out, uint8_t* desc_out, int capacity, int* counts, hipStream_t s,
                               int descriptor) {
    APDS_REQUIRE(img != nullptr, APDS_ERR_BAD_ARG, "null image");
    APDS_REQUIRE(descriptor == APDS_AKAZE_DESCRIPTOR_MLDB || descriptor == APDS_AKAZE_DESCRIPTOR_KAZE, APDS_ERR_BAD_ARG, "unknown descriptor kind");
    const size_t row_bytes = descriptor == APDS_AKAZE_DESCRIPTOR_KAZE ? APDS_DESC_FLOAT_DIM * sizeof(float) : 64;
    APDS_REQUIRE(n_img >= 1 && n_img <= 4096, APDS_ERR_BAD_ARG, "batch must hold 1 .. 4096 images");
    APDS_REQUIRE(channels == 1 || channels == 3 || channels == 4, APDS_ERR_ASSERT, "image must have 1, 3 or 4 channels");
    APDS_REQUIRE(rows > 2 && cols > 2, APDS_ERR_ASSERT, "image must be larger than 2x2");   // AKAZE CV_Assert(img_height > 2 && img_width > 2)
    APDS_REQUIRE(rows < 65536 && cols < 65536, APDS_ERR_ASSERT, "image side must be < 65536");
    APDS_REQUIRE(stride >= (size_t)cols * channels, APDS_ERR_ASSERT, "row stride smaller than a row");
    APDS_REQUIRE(n_img == 1 || img_bstride >= (size_t)rows * stride, APDS_ERR_ASSERT, "image stride smaller than an image");
    if (pmask.base) {   // detectAndCompute: CV_Assert(mask.empty() || mask.size() == image.size())
        APDS_REQUIRE(pmask.rows == rows && pmask.cols == cols, APDS_ERR_ASSERT, "mask must have the image's size");
        APDS_REQUIRE(pmask.pix_stride >= 1 && pmask.row_stride >= (size_t)cols * pmask.pix_stride, APDS_ERR_ASSERT, "mask row stride smaller than a row");
        APDS_REQUIRE(n_img == 1 || pmask.img_stride == 0 || pmask.img_stride >= (size_t)rows * pmask.row_stride, APDS_ERR_ASSERT,
                     "mask image stride smaller than a mask");
    }
    APDS_REQUIRE(mask_support >= 0, APDS_ERR_BAD_ARG, "mask_support must be >= 0");
    if (max_points <= 0) max_points = APDS_MAX_POINTS;
    ThreadCtx& c = ctx();
    KernelTimer whole("akaze_extract", s);   // whole extraction (all kernels + the count read-backs), for bench.py
    const int host_time_env = config().debug_host_time;
    const auto host_t0 = std::chrono::steady_clock::now();
    AkazeDebugRequest& dbg = akaze_debug_request();
    const int B = n_img;

    // ---- plan: the evolution list (Allocate_Memory_Evolution), whether the Hessian kernels fork, and which kernels serve every stage
    Frame f{c, s, Batch{}, akaze_levels(cols, rows), SlabLayout{}};
    const int L = f.levels();
    HessianFork fork(c, s);
    f.dense_det = dbg.armed;
    const Config& cf = config();
    const PlanSwitches sw{cf.nld_strip, cf.sf_strip, cf.base_strip, cf.level_strip, cf.level_fuse, cf.level_stream, cf.doh_strip, cf.half_fuse, fork.on};
    f.plan = plan_extraction(f.ev, B, sw);
    const BaseStage base = plan_base(rows, cols, channels, stride, reinterpret_cast<uintptr_t>(img), img_bstride, B, sw);

    // ---- slab: one per image, the same layout `bytes` apart
    f.sl.lay_out(nullptr, f.ev, fork.on);
    f.bt.n = B;
    f.bt.stride = f.sl.bytes;
    f.bt.img_stride = img_bstride;
    f.sl.lay_out(static_cast<char*>(c.alloc(f.sl.bytes * (size_t)B)), f.ev, fork.on);
    zero_slab_heads(f);
    int* counts_dev = B > 1 ? c.alloc_n<int>(B) : nullptr;
    // the mask support: every level's radius from the plan, and the table of the mask(s), which depends on nothing but the mask - its two
    // launches go out first and are long done when the sub-pixel stage reads it
    MaskSupport support;
    if (pmask.base && mask_support > 0) {
        for (int i = 0; i < L; i++) support.radius[i] = mask_support_radius(mask_support, f.plan.level[i].support_unit);
        const int n_tables = B > 1 && pmask.img_stride != 0 ? B : 1;
        support.img_stride = n_tables > 1 ? (mask_zero_sat_elems(rows, cols) + 63) & ~(size_t)63 : 0;
        uint32_t* sat = c.alloc_n<uint32_t>(n_tables > 1 ? support.img_stride * n_tables : mask_zero_sat_elems(rows, cols));
        mask_zero_sat_device(pmask, n_tables, sat, support.img_stride, s);
        support.sat = sat;
    }

    // ---- scale space: base stage, then the level chain with every level's Hessian kernel forked off it, joined at the end
    base_stage(f, base, img, channels, stride);
    fork.open(f);
    LevelChain chain{f, fork};
    for (int i = 0; i < L; i++) chain.step(i);
    fork.join();
    HIP_CHECK(hipGetLastError());

    // ---- the keypoint stage: once every level has its Hessian, all levels are made final and emitted
    const LevelTable T = level_table(f);
    suppress_all_levels(f.ev, f.sl, s, f.bt);
    compact_all_levels(T, f.sl, pmask, support, kps_out, capacity, s, f.bt);
    // The image's keypoint count (kp_base[1]) is final here, before orientation and descriptors: its copy to the host goes out now, so that
    // the call can return ~0.3 ms before the stream is idle (APDS_EARLY_COUNT).
    int* K = nullptr;
    if (config().early_count != 0 && !dbg.armed) {
        K = copy_counts(f, counts_dev);
        if (!c.count_event) HIP_CHECK(hipEventCreateWithFlags(&c.count_event, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(c.count_event, s));
    }
    // ---- a1.8 / a1.9 over the image's keypoints [kp_base[0], kp_base[1]), capped at the output capacity. The per-keypoint kernels stride over
    // them: the grid only has to be of the right order (this thread's last image)
    const int kp_blocks = (std::min(16384, std::max(256, ceil_div((long long)(c.akaze_kp_estimate > 0 ? c.akaze_kp_estimate : 32768) * 5 / 4, 4))) + 7) & ~7;
    describe_keypoints(T, kps_out, f.sl.kp_base, std::min(capacity, max_points), (size_t)capacity * sizeof(apds_keypoint), desc_out, (size_t)capacity * row_bytes,
                       kp_blocks, B, config().kp_xcd ? 1 : 0, s, descriptor);
    HIP_CHECK(hipGetLastError());

    copy_debug_plane(f, dbg);
    if (host_time_env) report_host_time(host_time_env, host_t0, f);

    // ---- the only read-back of the call: every image's keypoint count
    if (K) {
        // the count went out in front of the orientation / descriptor kernels: wait for IT, not for the stream. What is still running reads
        // this thread's workspace: the thread's next call waits for it unless it goes to the same stream (ThreadCtx::mark_tail / ws_reset).
        c.mark_tail(s);
        HIP_CHECK(hipEventSynchronize(c.count_event));
    } else {
        K = copy_counts(f, counts_dev);
        HIP_CHECK(hipStreamSynchronize(s));
    }
    int kmax = 0;
    bool over = false;
    for (int bi = 0; bi < B; bi++) {
        counts[bi] = std::min(K[bi], max_points);
        kmax = std::max(kmax, counts[bi]);
        over |= K[bi] > max_points;
        APDS_REQUIRE(counts[bi] <= capacity, APDS_ERR_ASSERT, "output capacity smaller than the keypoint count");
    }
    c.akaze_kp_estimate = kmax;
    if (over) select_strongest(f, T, K, counts, max_points, kps_out, desc_out, capacity, descriptor, row_bytes);
    return kmax;
}

int akaze_extract_device(const void* img, int rows, int cols, int channels, size_t stride, const PixelMask& pmask, int mask_support, int max_points,
                         apds_keypoint* kps_out, uint8_t* desc_out, int capacity, hipStream_t s, int descriptor) {
    int count = 0;
    akaze_extract_batch_device(img, 1, 0, rows, cols, channels, stride, pmask, mask_support, max_points, kps_out, desc_out, capacity, &count, s, descriptor);
    return count;
}

}  // namespace apds
