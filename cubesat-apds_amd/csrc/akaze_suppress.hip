// csrc/akaze_suppress.hip — AKAZE cross-level suppression on gfx950: a keypoint deletes the weaker keypoints of the neighbouring levels
// that lie inside its search window.
//
// Replaces the two neighbour loops of OpenCV AKAZEFeatures::Find_Scale_Space_Extrema (the comparison with the level below, then with the
// level above) behind feature_extraction/src/lib.rs:79.
//
// The cross-level suppression is sequential in OpenCV (each keypoint may delete a keypoint of the neighbouring level, which changes what
// later keypoints find); it is reproduced exactly by dependency rounds: a keypoint is processed in the first round in which no EARLIER
// (row-major) keypoint of its own level with an overlapping search window is still pending. All levels run in the same rounds because the
// passes of one phase only read snapshots of the level they iterate over.
#include "akaze.h"
#include "config.h"

namespace apds {

// ---- cross-level suppression -------------------------------------------------------------------------------
static constexpr uint8_t ST_PENDING = 255, ST_DONE_OLD = 254;

struct SuppressArgs {
    size_t bstride;   // batch: slab stride in bytes (all pointers below are image 0's)
    int n_levels;
    int phase;   // 0: compare with the previous level (ascending passes), 1: with the next level
    int w[AKAZE_MAX_LEVELS], h[AKAZE_MAX_LEVELS], sigma_size[AKAZE_MAX_LEVELS], iratio[AKAZE_MAX_LEVELS];
    const float* Ldet[AKAZE_MAX_LEVELS];
    uint8_t* mask[AKAZE_MAX_LEVELS];     // live keypoint masks (searched and cleared)
    uint8_t* status[AKAZE_MAX_LEVELS];   // snapshot of the iterated level: 0 none, 255 pending, else done stamp
    const uint32_t* list[AKAZE_MAX_LEVELS];
    const int* list_count;               // [n_levels]
    // candidates still pending after a round, three rotating buffers per level (read / append / being zeroed)
    uint32_t* pend[AKAZE_MAX_LEVELS];    // 3 * pend_cap[lvl] entries
    int pend_cap[AKAZE_MAX_LEVELS];
    int* pend_count;                     // [3][AKAZE_MAX_LEVELS] counters, one 128-byte line each (PEND_PITCH ints apart)
};

// Snapshot of levels [snap_lo, snap_lo + snap_n) (status = pending where the mask is set) and zeroing of the three rotating
// pending counters of levels [zero_lo, zero_lo + zero_n) (the levels whose passes are about to run). grid.y = max(snap_n, zero_n).
__global__ void suppress_init_status_kernel(SuppressArgs A, int snap_lo, int snap_n, int zero_lo, int zero_n) {
    APDS_RAISE_WAVE_PRIORITY();
    if ((int)blockIdx.y < zero_n && blockIdx.x == 0 && threadIdx.x < 3)
        bofs(A.pend_count, A.bstride)[(threadIdx.x * AKAZE_MAX_LEVELS + zero_lo + blockIdx.y) * PEND_PITCH] = 0;
    if ((int)blockIdx.y >= snap_n) return;
    const int lvl = snap_lo + blockIdx.y;
    const int cnt = bofs(A.list_count, A.bstride)[lvl];
    const uint32_t* __restrict__ list = bofs(A.list[lvl], A.bstride);
    uint8_t* __restrict__ status = bofs(A.status[lvl], A.bstride);
    const uint8_t* __restrict__ mask = bofs(A.mask[lvl], A.bstride);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x) {
        const uint32_t e = list[i];
        const size_t p = (size_t)(e >> 16) * A.w[lvl] + (e & 0xFFFF);
        status[p] = mask[p] ? ST_PENDING : 0;
    }
}

// stamps 1..253 of finished candidates -> ST_DONE_OLD, so that the stamp values can be reused (every 253 rounds)
__device__ __forceinline__ void suppress_canon_level(const SuppressArgs& A, int lvl, int first, int stride) {
    const int cnt = bofs(A.list_count, A.bstride)[lvl];
    const uint32_t* __restrict__ list = bofs(A.list[lvl], A.bstride);
    uint8_t* __restrict__ status = bofs(A.status[lvl], A.bstride);
    for (int i = first; i < cnt; i += stride) {
        const uint32_t e = list[i];
        const size_t p = (size_t)(e >> 16) * A.w[lvl] + (e & 0xFFFF);
        const uint8_t s = status[p];
        if (s >= 1 && s <= 253) status[p] = ST_DONE_OLD;
    }
}

static constexpr int SUPPRESS_STAGE = 192;   // still-blocked candidates staged per block before one global append

// One round of one level's pass, executed by the `nwaves` waves of the calling block set that share (s_stage, s_n, s_base):
// wave `wave0` takes candidates wave0, wave0 + nwaves, ... of `in[0, cnt)`.
// One WAVE per candidate keypoint: the readiness window (up to 37 x 19 status bytes) and the neighbour search window
// (up to 16 x 16 mask bytes) are scanned 64 elements at a time; "first hit in row-major order" is the lowest set bit
// of the ballot of the first 64-element slab that has one. (A single thread walking these windows byte by byte took
// ~48 us per round; a frame needs ~20 rounds.) Candidates that are still blocked are appended to `out`.
__device__ __forceinline__ void suppress_round_body(const SuppressArgs& A, int lvl, int other, uint8_t stamp, const uint32_t* in, int cnt, uint32_t* out,
                                                    int* out_count, int wave0, int nwaves, uint32_t* s_stage, int* s_n, int* s_base) {
    constexpr int STAGE = SUPPRESS_STAGE;
    const size_t bstride = A.bstride;
    if (threadIdx.x == 0) *s_n = 0;
    __syncthreads();
    const int w = A.w[lvl];
    const int lane = threadIdx.x & 63;
    uint8_t* status = bofs(A.status[lvl], bstride);
    const float* ldet_own = bofs(A.Ldet[lvl], bstride);
    const float* ldet_other = bofs(A.Ldet[other], bstride);
    uint8_t* omask_w = bofs(A.mask[other], bstride);
    // interaction distance in this level's pixels (conservative superset of "search windows overlap")
    int D, diff, radius;
    if (A.phase == 0) {
        diff = A.iratio[lvl] / A.iratio[other];
        radius = A.sigma_size[lvl] * diff;
        D = 2 * A.sigma_size[lvl];
    } else {
        diff = A.iratio[other] / A.iratio[lvl];
        radius = A.sigma_size[other];
        D = (2 * radius + 1) * diff;
    }
    const int W = 2 * D + 1, total = W * (D + 1);
    const int side = 2 * radius, total2 = side * side;
    const int ow = A.w[other], oh = A.h[other];
    const uint8_t* omask = omask_w;
    for (int i = wave0; i < cnt; i += nwaves) {
        const uint32_t e = in[i];
        const int x = e & 0xFFFF, y = e >> 16;
        const size_t p = (size_t)y * w + x;
        if (status[p] != ST_PENDING) continue;   // wave-uniform
        // The first trip of BOTH windows (four 64-element slabs each) and the candidate's own response are loaded before anything is
        // evaluated: the neighbour search of the other level does not depend on the readiness test, so its memory round trip overlaps
        // the readiness one instead of following it (a round is bound by one candidate's chain of dependent loads). A blocked
        // candidate discards the search; a ready candidate's search window cannot be touched by another candidate of the same round
        // (that is what "ready" means), so reading it early sees the same bytes. (The other order — the search first, the readiness
        // window only for the candidates that have a victim, i.e. half the loads for most candidates — was measured: 65 + 44 us for the
        // two first rounds against 57 + 41: the round is bound by the dependent round trips, not by the number of loads. Round 4 measured
        // the opposite remedy as well — two candidates per trip, their entries, status bytes and windows fetched together: 59 + 40 us,
        // no change (profiles/r04/timeline_suppress_two_per_trip.txt): 85 000 candidates x ~25 scattered 64-byte lines in 56 us is
        // 2.4 TB/s of line fetches for a few useful bytes each; the windows' footprint, not their latency, is the round.)
        const int px = A.phase == 0 ? x * diff : x / diff, py = A.phase == 0 ? y * diff : y / diff;
        uint8_t sv[4], mv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int idx = u * 64 + lane;
            sv[u] = 0;
            if (idx < total) {
                const int ry = idx / W, rx = idx - ry * W;
                const int yy = y - D + ry, xx = x - D + rx;
                if (yy >= 0 && xx >= 0 && xx < w && (yy < y || xx < x)) sv[u] = status[(size_t)yy * w + xx];
            }
            mv[u] = 0;
            if (idx < total2) {
                const int iy = idx / side, ix = idx - iy * side;
                const int ii = py - radius + iy, jj = px - radius + ix;
                if (ii >= 0 && ii < oh && jj >= 0 && jj < ow) mv[u] = omask[(size_t)ii * ow + jj];
            }
        }
        const float own_response = ldet_own[p];
        // ready iff no EARLIER (row-major) keypoint of this level within D is pending or finished only in this round
        bool hit0 = false;
#pragma unroll
        for (int u = 0; u < 4; u++) hit0 |= sv[u] == ST_PENDING || sv[u] == stamp;
        bool blocked = __any(hit0);
        for (int base = 256; base < total && !blocked; base += 256) {
            bool hit = false;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int idx = base + u * 64 + lane;
                if (idx < total) {
                    const int ry = idx / W, rx = idx - ry * W;
                    const int yy = y - D + ry, xx = x - D + rx;
                    if (yy >= 0 && xx >= 0 && xx < w && (yy < y || xx < x)) {
                        const uint8_t st = status[(size_t)yy * w + xx];
                        hit |= st == ST_PENDING || st == stamp;
                    }
                }
            }
            blocked = __any(hit);
        }
        // the candidate's victim: the first live keypoint of the other level inside its search window, row-major
        int found = -1;
        {
#pragma unroll
            for (int u = 0; u < 4; u++) {   // first hit in row-major order: lowest slab, lowest lane
                const int idx = u * 64 + lane;
                bool ok = false;
                if (mv[u]) {
                    const int iy = idx / side, ix = idx - iy * side;
                    const int dx = ix - radius, dy = iy - radius;
                    ok = dx * dx + dy * dy <= radius * radius;
                }
                const unsigned long long bb = __ballot(ok);
                if (found < 0 && bb) {
                    const int first = u * 64 + __ffsll((long long)bb) - 1;
                    const int iy = first / side, ix = first - iy * side;
                    found = (py - radius + iy) * ow + (px - radius + ix);
                }
            }
            for (int base = 256; base < total2 && found < 0; base += 256) {   // (windows wider than 16 x 16: none with AKAZE's parameters)
                unsigned long long b[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int idx = base + u * 64 + lane;
                    bool ok = false;
                    if (idx < total2) {
                        const int iy = idx / side, ix = idx - iy * side;
                        const int ii = py - radius + iy, jj = px - radius + ix;
                        if (ii >= 0 && ii < oh && jj >= 0 && jj < ow && omask[(size_t)ii * ow + jj]) {
                            const int dx = jj - px, dy = ii - py;
                            ok = dx * dx + dy * dy <= radius * radius;
                        }
                    }
                    b[u] = __ballot(ok);
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (found < 0 && b[u]) {
                        const int first = base + u * 64 + __ffsll((long long)b[u]) - 1;
                        const int iy = first / side, ix = first - iy * side;
                        found = (py - radius + iy) * ow + (px - radius + ix);
                    }
            }
        }
        if (found < 0) {
            // No live keypoint of the other level in the window, and keypoints are only ever deleted: whatever the earlier candidates
            // do, this one deletes nothing. It is finished now and, having no effect, never makes a later candidate wait.
            if (lane == 0) status[p] = ST_DONE_OLD;
            continue;
        }
        if (blocked) {
            // An earlier candidate in reach is still pending. It matters only if it can take this candidate's victim v away: victims
            // ahead of v in the window are dead for good, and a deletion behind v does not change "the first live one". So: blocked
            // iff an earlier pending (or finished-this-round) candidate e' of this level has v inside ITS search window. The scan
            // covers every position of this level whose window can contain v, and tests membership exactly as find_neighbor_point
            // does (half-open square [-r, r) and the disc).
            const int vy = found / ow, vx = found - vy * ow;
            int cx0, cx1, cy0, cy1;
            if (A.phase == 0) {   // e' = (x', y') searches around (x' * diff, y' * diff)
                cx0 = (vx - radius) / diff - 1, cx1 = (vx + radius) / diff + 1;
                cy0 = (vy - radius) / diff - 1, cy1 = (vy + radius) / diff + 1;
            } else {              // around (x' / diff, y' / diff)
                cx0 = (vx - radius) * diff, cx1 = (vx + radius + 1) * diff;
                cy0 = (vy - radius) * diff, cy1 = (vy + radius + 1) * diff;
            }
            cx0 = max(cx0, 0), cy0 = max(cy0, 0), cx1 = min(cx1, w - 1), cy1 = min(cy1, y);   // rows after y are later candidates
            const int cw = cx1 - cx0 + 1, cn = cw * (cy1 - cy0 + 1);
            bool still = false;
            for (int base = 0; base < cn && !still; base += 256) {
                bool hit = false;
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int idx = base + u * 64 + lane;
                    if (idx < cn) {
                        const int ry = idx / cw, rx = idx - ry * cw;
                        const int yy = cy0 + ry, xx = cx0 + rx;
                        if (yy < y || xx < x) {
                            const uint8_t st = status[(size_t)yy * w + xx];
                            if (st == ST_PENDING || st == stamp) {
                                const int qx = A.phase == 0 ? xx * diff : xx / diff, qy = A.phase == 0 ? yy * diff : yy / diff;
                                const int dx = vx - qx, dy = vy - qy;
                                hit |= dx >= -radius && dx < radius && dy >= -radius && dy < radius && dx * dx + dy * dy <= radius * radius;
                            }
                        }
                    }
                }
                still = __any(hit);
            }
            blocked = still;
        }
        if (blocked) {
            if (lane == 0) {
                const int slot = atomicAdd(s_n, 1);
                if (slot < STAGE) s_stage[slot] = e;
                else out[atomicAdd(out_count, 1)] = e;   // staging full (dense clusters): append directly
            }
            continue;
        }
        if (lane == 0) {
            if (found >= 0 && own_response > ldet_other[found]) omask_w[found] = 0;
            status[p] = stamp;
        }
    }
    __syncthreads();
    const int staged = min(*s_n, STAGE);
    if (threadIdx.x == 0 && staged) *s_base = atomicAdd(out_count, staged);
    __syncthreads();
    for (int i = threadIdx.x; i < staged; i += blockDim.x) out[*s_base + i] = s_stage[i];
}

// Wide form of a round: the passes of levels [lvl0, lvl0 + gridDim.y) with gridDim.x blocks of four waves each. Round r reads the
// candidates that were still pending after round r-1 (in_sel: -1 = the level's full candidate list) and appends the ones that are
// still blocked to buffer out_sel; the counter of buffer zero_sel is cleared for the round after.
__global__ __launch_bounds__(256) void suppress_round_kernel(SuppressArgs A, int lvl0, uint8_t stamp, int in_sel, int out_sel, int zero_sel) {
    APDS_RAISE_WAVE_PRIORITY();
    const int lvl = lvl0 + blockIdx.y;
    const int other = A.phase == 0 ? lvl - 1 : lvl + 1;
    if (other < 0 || other >= A.n_levels) return;
    const size_t bstride = A.bstride;
    int* __restrict__ pend_count = bofs(A.pend_count, bstride);
    uint32_t* __restrict__ pend = bofs(A.pend[lvl], bstride);
    const uint32_t* __restrict__ in = in_sel < 0 ? bofs(A.list[lvl], bstride) : pend + (size_t)in_sel * A.pend_cap[lvl];
    const int cnt = in_sel < 0 ? bofs(A.list_count, bstride)[lvl] : pend_count[(in_sel * AKAZE_MAX_LEVELS + lvl) * PEND_PITCH];
    if (blockIdx.x == 0 && threadIdx.x == 0) pend_count[(zero_sel * AKAZE_MAX_LEVELS + lvl) * PEND_PITCH] = 0;
    if (cnt == 0) return;   // nothing pending for this level: the block has no work
    __shared__ uint32_t s_stage[SUPPRESS_STAGE];
    __shared__ int s_n, s_base;
    suppress_round_body(A, lvl, other, stamp, in, cnt, pend + (size_t)out_sel * A.pend_cap[lvl], &pend_count[(out_sel * AKAZE_MAX_LEVELS + lvl) * PEND_PITCH],
                        blockIdx.x * 4 + (threadIdx.x >> 6), gridDim.x * 4, s_stage, &s_n, &s_base);
}

// Tail of the passes of levels [lvl0, lvl0 + gridDim.y): ONE block per level runs the remaining rounds (from round `round0`) back to
// back until the level has no pending candidate left. After the first wide rounds only the ends of the dependency chains are left
// (tens of candidates, up to ~15 more rounds): as separate launches each of those rounds cost a launch latency plus a host check for
// convergence every few rounds; inside one block a round costs one candidate's chain of dependent loads and a barrier, and the loop
// ends exactly when the work does: no host synchronisation at all. The passes of different levels are independent within a phase
// (see the file header), so the blocks never wait for each other. Every thread leaves the loop on the same block-uniform count.
__global__ __launch_bounds__(1024) void suppress_tail_kernel(SuppressArgs A, int lvl0, int round0) {
    APDS_RAISE_WAVE_PRIORITY();
    const int lvl = lvl0 + blockIdx.y;
    const int other = A.phase == 0 ? lvl - 1 : lvl + 1;
    if (other < 0 || other >= A.n_levels) return;
    const size_t bstride = A.bstride;
    int* pend_count = bofs(A.pend_count, bstride);
    uint32_t* pend = bofs(A.pend[lvl], bstride);
    __shared__ uint32_t s_stage[SUPPRESS_STAGE];
    __shared__ int s_n, s_base, s_cnt;
    for (int round = round0;; round++) {
        const int in_sel = (round - 1) % 3, out_sel = round % 3;
        if (threadIdx.x == 0) {
            // the counters are updated by L2 atomics: read and reset them there as well, not through this CU's L1
            s_cnt = round == 0 ? bofs(A.list_count, bstride)[lvl]
                               : __hip_atomic_load(&pend_count[(in_sel * AKAZE_MAX_LEVELS + lvl) * PEND_PITCH], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicExch(&pend_count[(out_sel * AKAZE_MAX_LEVELS + lvl) * PEND_PITCH], 0);
        }
        __syncthreads();
        const int cnt = s_cnt;
        if (cnt == 0) break;   // block-uniform
        if (round > 0 && round % 253 == 0) {   // the stamp values come round again: retire the old ones first
            suppress_canon_level(A, lvl, threadIdx.x, blockDim.x);
            __syncthreads();
        }
        const uint32_t* in = round == 0 ? bofs(A.list[lvl], bstride) : pend + (size_t)in_sel * A.pend_cap[lvl];
        suppress_round_body(A, lvl, other, (uint8_t)(round % 253 + 1), in, cnt, pend + (size_t)out_sel * A.pend_cap[lvl],
                            &pend_count[(out_sel * AKAZE_MAX_LEVELS + lvl) * PEND_PITCH], threadIdx.x >> 6, blockDim.x >> 6, s_stage, &s_n, &s_base);
        __syncthreads();       // this round's status / mask / list writes are visible to the whole block before the next round reads them
    }
}
// ---- host side ---------------------------------------------------------------------------------------------------
// Each pass: a snapshot / counter-reset launch, WIDE_ROUNDS wide rounds (most candidates are ready at once), then suppress_tail_kernel
// finishes the chains without any host check.
// (fewer wide rounds for small tiles — whose calls are bound by the host's enqueue time — were measured: the tail kernel's one block
// per level then walks every candidate, 512^2 0.32 -> 0.37 ms)
static constexpr int WIDE_ROUNDS = 3;

// the passes of levels [lo, lo + np) in A.phase, after a snapshot of levels [snap_lo, snap_lo + ns)
static void run_passes(const SuppressArgs& A, int lo, int np, int snap_lo, int ns, hipStream_t s, int B) {
    const dim3 lblock(256);
    hipLaunchKernelGGL(suppress_init_status_kernel, dim3(B > 1 ? 64 : 256, std::max(np, ns), B), lblock, 0, s, A, snap_lo, ns, lo, np);
    for (int round = 0; round < WIDE_ROUNDS; round++)
        // (a wider grid for the first round, which visits every candidate, is slower: 512 blocks 59 us, 1024 blocks 69 us against 51 us
        // with 256: more waves in flight do not help, and neither do fewer loads per candidate — see suppress_round_body)
        hipLaunchKernelGGL(suppress_round_kernel, dim3(B > 1 ? 64 : 256, np, B), lblock, 0, s, A, lo, (uint8_t)(round % 253 + 1),
                           round == 0 ? -1 : (round - 1) % 3, round % 3, (round + 1) % 3);
    hipLaunchKernelGGL(suppress_tail_kernel, dim3(1, np, B), dim3(1024), 0, s, A, lo, WIDE_ROUNDS);
}

// Level j is final after phase-0 pass j + 1 (the candidates of level j + 1 delete weaker neighbours in level j) and phase-1 pass j - 1
// (... of level j - 1, in the level above them). Phase 0: passes 1 .. L-1, each snapshotting its own level. Phase 1: passes 0 .. L-2; the
// snapshot of levels 0 .. L-1 is taken when their phase-0 state is final and BEFORE a phase-1 pass deletes in them.
// (Round 2 ran this for the large octaves' levels early, on a third stream under the small octaves' chain - "staged" mode: 2.14 against
// 2.18 ms stand-alone then, 1.91 against 1.83 in round 3, and slower inside the streamed pipeline: the per-keypoint kernels fill every CU
// and the chain's blocks wait for room whatever the priorities or occupancy caps; removed. Only the suppression passes of those levels
// early was built and measured as well: bit-identical, 1.844 against 1.825 ms — the passes' scattered loads slow the chain by more than
// they hide.)
void suppress_all_levels(const std::vector<LevelDesc>& ev, const SlabLayout& sl, hipStream_t s, const Batch& b) {
    const int L = (int)ev.size();
    if (L <= 1) return;
    SuppressArgs A{};
    A.bstride = b.stride;
    A.n_levels = L;
    for (int i = 0; i < L; i++) {
        A.w[i] = ev[i].w;
        A.h[i] = ev[i].h;
        A.sigma_size[i] = ev[i].sigma_size;
        A.iratio[i] = (int)ev[i].ratio;
        A.Ldet[i] = sl.Ldet[i];
        A.mask[i] = sl.mask_all + ev[i].pix_offset;
        A.status[i] = sl.status_all + ev[i].pix_offset;
        A.list[i] = sl.list[i];
        A.pend[i] = sl.pend[i];
        A.pend_cap[i] = sl.pend_cap[i];
    }
    A.list_count = sl.list_count;
    A.pend_count = sl.pend_count;
    A.phase = 0;
    run_passes(A, 1, L - 1, 1, L - 1, s, b.n);
    A.phase = 1;
    run_passes(A, 0, L - 1, 0, L, s, b.n);
}
}  // namespace apds
