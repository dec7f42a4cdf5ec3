// csrc/match_hamming.hip — Hamming brute-force top-k on gfx950 (integer VALU + scalar broadcast).
//
// Replaces BFMatcher(NORM_HAMMING).knnMatch / match(crossCheck) behind
// /root/reference/feature_extraction/src/lib.rs:94-126.
//
// Mapping (CDNA4): one LANE owns T query descriptors (16 dwords each, in VGPRs for the whole kernel);
// one WAVE walks a contiguous chunk of train rows. A train row is wave-uniform, so it is fetched with
// scalar loads (s_load_dwordx16: one 64-byte line per row) and fed to the VALU as an SGPR operand:
//     v_xor_b32  t, s_row[j], v_q[j]      v_bcnt_u32_b32  acc, t, acc
// = 30 VALU lane-ops per (query,row) pair on the fast path (15 dwords; the 16th holds 6 descriptor bits and is only
// needed to finish a candidate hit; the algorithmic figure used for the roofline stays 32), no LDS and no cross-lane traffic on the hot path. The running
// top-k lives per lane; the popcount chain starts at -threshold so "distance < current k-th best" is the
// sign bit, a whole group of pairs is screened with one v_min3/v_cmp, and the insertion code runs only for
// the rare groups that contain a hit. Train rows are split into chunks over blockIdx.y so the grid fills
// 256 CUs; per-chunk candidates are merged by a second tiny kernel. Keys are (distance << 32 | index):
// unsigned 64-bit min reproduces BFMatcher's order (distance, then lower train index).
//
// In this file: the scan kernels, their record format and its merge (merge_records_kernel), pack_rows, the occupancy-cap hooks, and the
// host side - ONE threshold pre-pass -> main scan -> merge sequence (ScanLayout, scan_prepass / scan_main / scan_merge) under the one-call
// scan, the paged scan and the per-frame split state. Merges of plain key lists: topk_merge.hip; ratio test and cross-check:
// match_filter.hip; the VALU microbenchmark: valu_peak.hip.
#include <atomic>

#include "config.h"
#include "kernels.h"
#include "popcount_row.h"
#include "topk_keys.h"

namespace apds {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

static constexpr int INF_THR = 1 << 20;          // > any Hamming distance of a 512-bit row
static constexpr uint32_t NO_INDEX = 0xFFFFFFFFu;
// Per-chunk candidate lists. A work item (one wave: 64*T queries x one row chunk) leaves one RECORD: T*K 64-bit presence masks
// (bit = lane; slot s = t*K + k) followed by the present keys only, slot-major, lanes ascending. After the threshold pre-pass
// ~5 of 6 slots are empty (the chunk held nothing better than the query's starting threshold), so records are mostly header:
// the lists cost ~0.8 bytes per slot instead of 4 (and instead of 8 as 64-bit keys). Keys are 32 bits: distance (<= 512,
// 10 bits) << 22 | row offset inside the chunk (chunks hold at most 2^22 rows); same order as the 64-bit
// (distance << 32 | global row) keys they expand to in the merge. Records sit at a fixed pitch (capacity for all slots
// present); untouched bytes cost no traffic.
static constexpr int PART_ROW_BITS = 22;
template <int T, int K>
struct PartRecord {
    static constexpr int SLOTS = T * K;
    static constexpr int HEADER = 2 * SLOTS;             // u32 words of masks
    static constexpr int PITCH = HEADER + 64 * SLOTS;    // u32 words per record
};

// Lower bound of the distances of one train row to the lane's T queries: popcount over the first 15 dwords (480 bits)
// on top of start[t] = -threshold. M-LDB uses 486 bits, so dword 15 holds at most 6 set bits of the XOR: if the bound
// is already >= threshold the pair cannot be a hit, and dword 15 is only looked at in the rare hit path.
// 30 VALU ops per pair instead of 32.
//
// Issue order (measured, profiles/r02/valu_calib.log): on a gfx950 SIMD a VOP2 v_xor_b32 takes 2 issue cycles and the VOP3
// v_bcnt_u32_b32 takes 4, but one wave issues at most one VALU op per 4-cycle window, so an xor only costs 2 when the xor of
// ANOTHER wave shares its window. With the waves of a SIMD running the plain stream xor, bcnt, xor, bcnt, ... in step that
// pairing rarely happens (3.83 cycles per op, 38.5 T lane-ops/s chip-wide); an `s_nop 0` between each xor and the bcnt that
// consumes it takes the wave out of step with its neighbours and the pairs settle at 2 + 4 cycles (2.9 per op, 50.7 T lane-ops/s,
// 99 % of the 6-cycle pair). A nop after every op, or the xor issued one or two steps ahead, does not: only this placement.
#ifndef APDS_PAIR_NOP
#define APDS_PAIR_NOP 1
#endif
template <int T>
__device__ __forceinline__ void row_distances(const u32x16 row, const uint32_t (&q)[T][16], const int (&start)[T], int (&acc)[T]) {
#pragma unroll
    for (int t = 0; t < T; t++) {
        int a = start[t];
#pragma unroll
        for (int j = 0; j < 15; j++) {
#if APDS_PAIR_NOP
            const uint32_t x = q[t][j] ^ row[j];
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_nop 0");
            __builtin_amdgcn_sched_barrier(0);
            a = bcnt_acc(x, a);
            __builtin_amdgcn_sched_barrier(0);
#else
            a = bcnt_acc(q[t][j] ^ row[j], a);
#endif
        }
        acc[t] = a;
    }
}

// Paged scans (k > 16, see hamming_topk_device) look for the best K keys ABOVE a per-query floor key (the last key of the page before):
// FLOOR adds that one comparison to the rare hit path - the rows at or below the floor are the query's best, so they all reach it, but
// there are only 16 per page of them.
struct KeyFloor {
    uint32_t dist, index;   // the floor key (distance << 32 | global row index), split
    uint32_t base;          // global index of row 0 of the scanned array
};

template <int T, int K, bool FLOOR = false>
__device__ __forceinline__ void insert_hits(const int (&acc)[T], const int (&nthr_old)[T], const uint32_t (&q)[T][16], uint32_t row15, uint32_t r,
                                            int (&bd)[T][K], uint32_t (&bi)[T][K], const KeyFloor (&fl)[T]) {
#pragma unroll
    for (int t = 0; t < T; t++) {
        if (acc[t] < 0) {   // the 480-bit bound is below the threshold this pair was screened with: finish the distance
            const int d = acc[t] - nthr_old[t] + __popc(q[t][15] ^ row15);
            if (FLOOR && !((uint32_t)d > fl[t].dist || ((uint32_t)d == fl[t].dist && r + fl[t].base > fl[t].index))) continue;
            if (d < bd[t][K - 1]) {
                // insertion with strict '<': a later row never moves ahead of an equal earlier one
                bool placed = false;
#pragma unroll
                for (int j = K - 1; j > 0; j--) {
                    if (!placed) {
                        if (bd[t][j - 1] > d) {
                            bd[t][j] = bd[t][j - 1];
                            bi[t][j] = bi[t][j - 1];
                        } else {
                            bd[t][j] = d;
                            bi[t][j] = r;
                            placed = true;
                        }
                    }
                }
                if (!placed) {
                    bd[t][0] = d;
                    bi[t][0] = r;
                }
            }
        }
    }
}

// One work item = (64*T queries per wave, 4 waves) x (one chunk of train rows).
template <int T, int K, bool FLOOR = false>
__device__ __forceinline__ void hamming_topk_item(const u32x16* __restrict__ train, int n_train, const u32x4* __restrict__ queries, int nq,
                                                  int rows_per_chunk, const int* __restrict__ init_thr, uint32_t* __restrict__ out, int chunk,
                                                  int qblock, const uint64_t* __restrict__ floor_keys = nullptr, uint32_t floor_base = 0) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int qbase = (qblock * 4 + wave) * (64 * T);
    if (qbase >= nq) return;   // wave-uniform
    const int row0 = chunk * rows_per_chunk;
    const int row1 = min(n_train, row0 + rows_per_chunk);
    uint32_t q[T][16];
    int bd[T][K];
    uint32_t bi[T][K];
    int nthr[T];
    KeyFloor fl[T];
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int qi = min(qbase + t * 64 + lane, nq - 1);
        if (FLOOR) {   // the last key of the query's previous page (all ones when that page was not full: nothing is above it)
            const uint64_t f = floor_keys[(size_t)qi * K + (K - 1)];
            fl[t].dist = (uint32_t)(f >> 32);
            fl[t].index = (uint32_t)f;
            fl[t].base = floor_base;
        }
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const u32x4 x = queries[(size_t)qi * 4 + v];
            q[t][4 * v + 0] = x.x;
            q[t][4 * v + 1] = x.y;
            q[t][4 * v + 2] = x.z;
            q[t][4 * v + 3] = x.w;
        }
        const int thr0 = init_thr ? init_thr[qi] : INF_THR;
#pragma unroll
        for (int k = 0; k < K; k++) {
            bd[t][k] = thr0;
            bi[t][k] = NO_INDEX;
        }
        nthr[t] = -thr0;
    }

    // Screen two rows against the lane's T queries; run the insertion code only if some lane has a hit.
    auto pair_step = [&](const u32x16& a0, const u32x16& a1, int r) {
        int acc0[T], acc1[T];
        row_distances<T>(a0, q, nthr, acc0);
        row_distances<T>(a1, q, nthr, acc1);
        int m = acc0[0];
#pragma unroll
        for (int t = 1; t < T; t++) m = min(m, acc0[t]);
#pragma unroll
        for (int t = 0; t < T; t++) m = min(m, acc1[t]);
        if (__any(m < 0)) {
            int nthr_old[T];
#pragma unroll
            for (int t = 0; t < T; t++) nthr_old[t] = nthr[t];
            insert_hits<T, K, FLOOR>(acc0, nthr_old, q, a0[15], (uint32_t)r, bd, bi, fl);
            insert_hits<T, K, FLOOR>(acc1, nthr_old, q, a1[15], (uint32_t)(r + 1), bd, bi, fl);
#pragma unroll
            for (int t = 0; t < T; t++) nthr[t] = -bd[t][K - 1];
        }
    };

    int r = row0;
    // Main loop: four rows per trip as two ping-pong pairs (A, B). The scalar loads of one pair are issued
    // before the 2*T*32 VALU ops of the other pair, so their latency sits under compute; SMEM returns out
    // of order, hence the only wait is lgkmcnt(0) and it always lands after a full compute phase.
    if (r + 3 < row1) {
        u32x16 a0 = train[r], a1 = train[r + 1];
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
        for (; r + 3 < row1; r += 4) {
            const u32x16 b0 = train[r + 2], b1 = train[r + 3];
            __builtin_amdgcn_sched_barrier(0);
            pair_step(a0, a1, r);
            __builtin_amdgcn_s_waitcnt(0xC07F);   // pair B has landed (issued one compute phase ago)
            const int rn = min(r + 4, row1 - 1), rm = min(r + 5, row1 - 1);
            a0 = train[rn];
            a1 = train[rm];
            __builtin_amdgcn_sched_barrier(0);
            pair_step(b0, b1, r + 2);
            __builtin_amdgcn_s_waitcnt(0xC07F);   // pair A has landed
        }
    }
    for (; r < row1; r++) {   // tail: at most three rows
        const u32x16 a0 = train[r];
        int acc0[T];
        row_distances<T>(a0, q, nthr, acc0);
        insert_hits<T, K, FLOOR>(acc0, nthr, q, a0[15], (uint32_t)r, bd, bi, fl);
#pragma unroll
        for (int t = 0; t < T; t++) nthr[t] = -bd[t][K - 1];
    }

    // one record per (chunk, wave tile): presence masks + the present keys, compacted with ballot / popcount prefix sums
    using Rec = PartRecord<T, K>;
    const int n_wtiles = (nq + 64 * T - 1) / (64 * T);
    uint32_t* rec = out + ((size_t)chunk * n_wtiles + (qblock * 4 + wave)) * Rec::PITCH;
    const uint64_t lt = (1ull << lane) - 1;
    int base = 0;
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int qi = qbase + t * 64 + lane;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const bool present = qi < nq && bi[t][k] != NO_INDEX;
            const uint64_t m = __ballot(present);
            if (present) rec[Rec::HEADER + base + __popcll(m & lt)] = ((uint32_t)bd[t][k] << PART_ROW_BITS) | (bi[t][k] - (uint32_t)row0);
            if (lane == 0) {
                rec[2 * (t * K + k)] = (uint32_t)m;
                rec[2 * (t * K + k) + 1] = (uint32_t)(m >> 32);
            }
            base += __popcll(m);
        }
    }
}

// grid: 1-D, 8 * ceil(chunks/8) * ceil(nq / (256*T)) blocks. block = 256 threads = 4 waves, each wave its own 64*T queries.
template <int T, int K>
__global__ __launch_bounds__(256) void hamming_topk_kernel(const u32x16* __restrict__ train, int n_train,
                                                           const u32x4* __restrict__ queries, int nq, int rows_per_chunk,
                                                           const int* __restrict__ init_thr, uint32_t* __restrict__ out, int qtile_blocks,
                                                           int n_chunks, int xcd_aware) {
    // 1-D grid, XCD-aware by default: workgroups are dealt round-robin over the 8 XCDs, so all query tiles of one row
    // chunk are given the same (id % 8): the chunk is then streamed into ONE XCD's L2 instead of all eight (13x less
    // L2->fabric traffic at equal speed, once the chunk count is a multiple of 8 so that no XCD gets extra chunks).
    // APDS_MATCH_XCD=0 restores the plain (chunk-major) order. Placement only affects speed, never results.
    const int nqb = qtile_blocks;
    int chunk, qblock;
    if (xcd_aware) {
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        chunk = (slot / nqb) * 8 + xcd;
        qblock = slot - (slot / nqb) * nqb;
    } else {
        chunk = blockIdx.x / nqb;
        qblock = blockIdx.x - chunk * nqb;
    }
    if (chunk >= n_chunks) return;   // block-uniform
    hamming_topk_item<T, K>(train, n_train, queries, nq, rows_per_chunk, init_thr, out, chunk, qblock);
}

// One page of a paged scan: the K best keys above floor_keys[query][K - 1] (one query per lane, plain chunk-major grid).
template <int K>
__global__ __launch_bounds__(256) void hamming_topk_page_kernel(const u32x16* __restrict__ train, int n_train, const u32x4* __restrict__ queries, int nq,
                                                                int rows_per_chunk, const int* __restrict__ init_thr, uint32_t* __restrict__ out,
                                                                int qtile_blocks, int n_chunks, const uint64_t* __restrict__ floor_keys,
                                                                uint32_t floor_base) {
    const int chunk = blockIdx.x / qtile_blocks, qblock = blockIdx.x - chunk * qtile_blocks;
    if (chunk >= n_chunks) return;   // block-uniform
    hamming_topk_item<1, K, true>(train, n_train, queries, nq, rows_per_chunk, init_thr, out, chunk, qblock, floor_keys, floor_base);
}

// (A persistent work-queue form of this kernel - resident workgroups pulling items from an atomic counter - was kept through round 2 behind
// APDS_MATCH_PERSIST; the plain grid was as fast in every sweep (profiles/r01/match_persistent_sweep.log): deleted in round 3.)

// Merge of the per-chunk records of hamming_topk_kernel. One BLOCK per query tile (lane = the T queries it owned in the match
// kernel): its four waves take every fourth chunk each, four chunks per trip with all of a trip's loads issued before the first
// insertion (a wave walking all chunks one by one was a chain of 360 dependent memory round trips: 0.23 ms for 138 waves on an
// otherwise idle GPU), then wave 0 folds the other waves' lists into its own through LDS. A present key expands to
// (distance << 32 | row offset + p * rows_per_chunk + row_base); keys are unique, so the K smallest do not depend on the order of
// insertion. `extra` (nq x K 64-bit keys, may be null) is one more already-expanded sorted list (the sample pass).
template <int T, int K>
__global__ __launch_bounds__(256) void merge_records_kernel(const uint32_t* __restrict__ recs, int parts, int rows_per_chunk, uint32_t row_base,
                                                            const uint64_t* __restrict__ extra, int nq, uint64_t* __restrict__ out) {
    APDS_RAISE_WAVE_PRIORITY();
    using Rec = PartRecord<T, K>;
    constexpr int G = T * K <= 8 ? 4 : 1;       // chunks per trip (the wide records of large k: one)
    __shared__ uint64_t s_best[3][T * K][64];   // lists of waves 1..3
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_wtiles = (nq + 64 * T - 1) / (64 * T);
    const int wtile = blockIdx.x;
    uint64_t best[T][K];
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int qi = wtile * 64 * T + t * 64 + lane;
#pragma unroll
        for (int k = 0; k < K; k++) best[t][k] = (wave == 0 && extra && qi < nq) ? extra[(size_t)qi * K + k] : EMPTY_KEY;   // a sorted list: a valid start
    }
    const uint64_t lt = (1ull << lane) - 1;
    for (int p0 = wave; p0 < parts; p0 += 4 * G) {
        uint32_t keys[G][Rec::SLOTS];
#pragma unroll
        for (int g = 0; g < G; g++) {           // all loads of the trip first
            const int p = p0 + 4 * g;
            const bool live = p < parts;        // wave-uniform
            const uint32_t* rec = recs + ((size_t)(live ? p : p0) * n_wtiles + wtile) * Rec::PITCH;
            int base = 0;
#pragma unroll
            for (int s = 0; s < Rec::SLOTS; s++) {
                const uint64_t m = live ? ((uint64_t)rec[2 * s] | ((uint64_t)rec[2 * s + 1] << 32)) : 0ull;   // wave-uniform
                const bool present = (m >> lane) & 1;
                keys[g][s] = present ? rec[Rec::HEADER + base + __popcll(m & lt)] : 0xFFFFFFFFu;
                base += __popcll(m);
            }
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
            const uint32_t chunk_base = (uint32_t)(p0 + 4 * g) * (uint32_t)rows_per_chunk + row_base;
#pragma unroll
            for (int t = 0; t < T; t++)
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const uint32_t part = keys[g][t * K + k];
                    if (part == 0xFFFFFFFFu) continue;   // distance 1023 cannot occur: "absent"
                    topk_insert<K>(best[t], ((uint64_t)(part >> PART_ROW_BITS) << 32) |
                                                (uint64_t)(uint32_t)((part & ((1u << PART_ROW_BITS) - 1)) + chunk_base));
                }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int k = 0; k < K; k++) s_best[wave - 1][t * K + k][lane] = best[t][k];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w = 0; w < 3; w++)
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int k = 0; k < K; k++) {
                const uint64_t key = s_best[w][t * K + k][lane];
                if (key != EMPTY_KEY) topk_insert<K>(best[t], key);
            }
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int qi = wtile * 64 * T + t * 64 + lane;
        if (qi < nq)
#pragma unroll
            for (int k = 0; k < K; k++) out[(size_t)qi * K + k] = best[t][k];
    }
}

// second-best distance of a sample of train rows -> initial thresholds for the full scan
__global__ void thr_from_keys_kernel(const uint64_t* __restrict__ keys, int nq, int K, int* __restrict__ thr) {
    APDS_RAISE_WAVE_PRIORITY();
    const int qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    const uint64_t key = keys[(size_t)qi * K + (K - 1)];
    thr[qi] = key == EMPTY_KEY ? INF_THR : (int)key_rank(key);
}

__global__ void pack_rows_kernel(const uint8_t* __restrict__ src, long long n, int desc_bytes, long long src_stride,
                                 uint32_t* __restrict__ dst) {
    APDS_RAISE_WAVE_PRIORITY();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // one dword of one row
    if (i >= n * 16) return;
    const long long row = i >> 4;
    const int w = (int)(i & 15);
    const uint8_t* p = src + row * src_stride + w * 4;
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++)
        if (w * 4 + b < desc_bytes) v |= (uint32_t)p[b] << (8 * b);
    dst[i] = v;
}

// ---- host launchers -------------------------------------------------------------------------------------
struct ChunkPlan {
    int T, chunks, rows_per_chunk, qtiles_blocks;
};

// dynamic-LDS bytes the most recent scan launch of the process was made with (test hook: the cap reaches every kernel variant)
std::atomic<int>& last_scan_launch_lds() {
    static std::atomic<int> v{-1};
    return v;
}
// Occupancy cap of the main scan (bytes of unused dynamic LDS per workgroup; 0 = none), process-wide: APDS_MATCH_LDS_CAP at first
// use, then apds_dev_match_lds_cap(). See launch_topk.
std::atomic<int>& match_lds_cap() {
    static std::atomic<int> cap{config().match_lds_cap};
    return cap;
}
// The same cap for the scans launched by ONE host thread (the streamed pipeline's match worker, when its starvation watch decides to
// cap): -1 = the process-wide value applies.
static thread_local int tl_scan_cap = -1;
void set_thread_scan_cap(int bytes) { tl_scan_cap = bytes; }

// Work items are (64*T queries) x (rows_per_chunk train rows) per wave. Items are kept small enough that the
// grid is many dispatch rounds deep (the block scheduler then balances the tail), but not so small that the
// per-chunk candidate lists dominate the merge.
static ChunkPlan plan_chunks(int nq, long long n_train, bool sample_pass = false, bool one_query_per_lane = false) {
    ChunkPlan p;
    // (the sweeps behind these constants: profiles/r01/match_work_item_sweep.log, match_probe.log; they were environment knobs until round 3)
    constexpr int target_waves = 256 * 4 * 4 * 24;   // waves per launch: many dispatch rounds deep, so the block scheduler balances the tail
    const int min_rows = sample_pass ? 256 : 1024;   // shortest row chunk of a work item
    p.T = nq >= 64 * 4 * 64 ? 4 : (nq >= 64 * 2 * 64 ? 2 : 1);
    // the threshold pre-pass covers few rows: smaller items (T = 1, short chunks) keep all CUs busy
    // (round 3, with the pre-pass running beside the previous frame's main scan: T = 2 / 4 for it measured again, no difference)
    if (sample_pass) p.T = 1;
    if (one_query_per_lane) p.T = 1;
    const int waves_q = ceil_div(nq, 64 * p.T);
    p.qtiles_blocks = ceil_div(waves_q, 4);
    long long chunks = ceil_div(target_waves, waves_q);
    const long long max_chunks = std::max<long long>(1, n_train / min_rows);
    chunks = std::min<long long>(std::max<long long>(chunks, 1), std::min<long long>(max_chunks, 65535));
    // chunk c runs on XCD (c % 8) when the XCD-aware placement is on: keep the chunk count a multiple of 8 so that every
    // XCD gets the same number of rows (3 extra chunks on 3 XCDs was a 2 % tail)
    chunks = std::max<long long>(chunks, ceil_div(n_train, 1ll << PART_ROW_BITS));   // 22-bit row offsets in the per-chunk keys
    if (chunks >= 8) chunks = (chunks + 7) & ~7ll;
    long long rpc = (n_train + chunks - 1) / chunks;
    rpc = (rpc + 3) & ~3ll;
    p.rows_per_chunk = (int)rpc;
    p.chunks = (int)((n_train + rpc - 1) / rpc);
    return p;
}

template <int K>
static void launch_topk(const void* q, int nq, const void* t, long long nt, const int* init_thr, uint32_t* parts, const ChunkPlan& p, hipStream_t s,
                        const char* timer_name = "hamming_topk", const uint64_t* floor_keys = nullptr, uint32_t floor_base = 0) {
    constexpr int xcd = 1;   // XCD-aware chunk placement (profiles/r01/match_xcd_placement_ab.log)
    const u32x16* tr = static_cast<const u32x16*>(t);
    const u32x4* qq = static_cast<const u32x4*>(q);
    // Occupancy cap: the kernels use no LDS, so an (unused) dynamic LDS request of `cap` bytes per workgroup bounds the
    // workgroups resident per CU (160 KB / cap). Two waves per SIMD already issue at full VALU rate; capping there leaves
    // registers, wave slots and the rest of the LDS free, so the short kernels of the other pipeline stages are dispatched
    // at once instead of waiting for a match wave to retire. Applies to every variant of the scan (all T, all K).
    const size_t cap = (size_t)std::max(0, tl_scan_cap >= 0 ? tl_scan_cap : match_lds_cap().load(std::memory_order_relaxed));
    last_scan_launch_lds().store((int)cap, std::memory_order_relaxed);
    if constexpr (K == 16) {
        if (floor_keys) {   // one page of a paged scan
            dim3 grid((unsigned)(p.chunks * p.qtiles_blocks)), block(256);
            KernelTimer timer(timer_name, s);
            hipLaunchKernelGGL((hamming_topk_page_kernel<K>), grid, block, cap, s, tr, (int)nt, qq, nq, p.rows_per_chunk, init_thr, parts,
                               p.qtiles_blocks, p.chunks, floor_keys, floor_base);
            HIP_CHECK(hipGetLastError());
            return;
        }
    }
    if (K > 2) {   // larger k keeps K (distance, index) pairs per query in registers: one query per lane
        dim3 grid((unsigned)(ceil_div(p.chunks, 8) * 8 * p.qtiles_blocks)), block(256);
        KernelTimer timer(timer_name, s);
        hipLaunchKernelGGL((hamming_topk_kernel<1, K>), grid, block, cap, s, tr, (int)nt, qq, nq, p.rows_per_chunk, init_thr, parts, p.qtiles_blocks,
                           p.chunks, 0);
        HIP_CHECK(hipGetLastError());
        return;
    }
    dim3 grid((unsigned)(ceil_div(p.chunks, 8) * 8 * p.qtiles_blocks)), block(256);
    KernelTimer timer(timer_name, s);
    switch (p.T) {
        case 4: hipLaunchKernelGGL((hamming_topk_kernel<4, K>), grid, block, cap, s, tr, (int)nt, qq, nq, p.rows_per_chunk, init_thr, parts, p.qtiles_blocks, p.chunks, xcd); break;
        case 2: hipLaunchKernelGGL((hamming_topk_kernel<2, K>), grid, block, cap, s, tr, (int)nt, qq, nq, p.rows_per_chunk, init_thr, parts, p.qtiles_blocks, p.chunks, xcd); break;
        default: hipLaunchKernelGGL((hamming_topk_kernel<1, K>), grid, block, cap, s, tr, (int)nt, qq, nq, p.rows_per_chunk, init_thr, parts, p.qtiles_blocks, p.chunks, xcd); break;
    }
    HIP_CHECK(hipGetLastError());
}

template <int K>
static size_t record_words(int nq, const ChunkPlan& p) {   // u32 words of the record buffer of one launch
    const size_t wtiles = (size_t)ceil_div(nq, 64 * p.T);
    const size_t pitch = p.T == 4 ? PartRecord<4, K>::PITCH : (p.T == 2 ? PartRecord<2, K>::PITCH : PartRecord<1, K>::PITCH);
    return (size_t)p.chunks * wtiles * pitch;
}

template <int K>
static void merge_records_launch(const uint32_t* recs, const ChunkPlan& p, uint32_t row_base, const uint64_t* extra, int nq, uint64_t* out, hipStream_t s) {
    const dim3 grid(ceil_div(nq, 64 * p.T)), block(256);   // one block per query tile
    switch (p.T) {
        case 4: hipLaunchKernelGGL((merge_records_kernel<4, K>), grid, block, 0, s, recs, p.chunks, p.rows_per_chunk, row_base, extra, nq, out); break;
        case 2: hipLaunchKernelGGL((merge_records_kernel<2, K>), grid, block, 0, s, recs, p.chunks, p.rows_per_chunk, row_base, extra, nq, out); break;
        default: hipLaunchKernelGGL((merge_records_kernel<1, K>), grid, block, 0, s, recs, p.chunks, p.rows_per_chunk, row_base, extra, nq, out); break;
    }
}


// One frame's scan, laid out in one buffer: an optional threshold pre-pass over the first `sample` rows, the main scan over the rest, the
// merge of the main scan's records with the pre-pass's keys. The one-call scan, the paged scan and the split scan below all run these
// three steps; they differ in whose memory the buffer is and in what runs between the steps.
struct ScanLayout {
    int nq = 0, k = 0;
    long long nt = 0, sample = 0;
    ChunkPlan sp{}, p{};   // pre-pass, main scan
    size_t off_sparts = 0, off_sample_keys = 0, off_thr = 0, off_parts = 0;   // byte offsets: pre-pass records, its merged keys, thresholds, main records
    size_t bytes = 0;
};

// `paged`: a page of a k > 16 scan. Those, and every K > 2, keep one query per lane.
template <int K>
static ScanLayout scan_layout(int nq, long long nt, bool paged) {
    ScanLayout L;
    L.nq = nq, L.k = K, L.nt = nt;
    // The pre-pass (only for large scans): exact top-k over the first `sample` rows gives per-query thresholds that
    // every chunk starts from, so the rare-hit fast path is reached immediately. The sample rows have the
    // lowest indices, hence a later row at equal distance never outranks them: strict '<' stays exact.
    // (1/16 of the rows, at most APDS_MATCH_SAMPLE = 16384, from 32768 rows up: a 125k-row shard of an 8-GPU run still gets one)
    const int sample_rows = config().match_sample;
    if (sample_rows > 0 && nt >= 32768) L.sample = std::min<long long>(sample_rows, (nt / 16) & ~1023ll);
    auto take = [&](size_t bytes) {
        const size_t o = L.bytes;
        L.bytes += (bytes + 255) & ~(size_t)255;
        return o;
    };
    if (L.sample) {
        L.sp = plan_chunks(nq, L.sample, true, K > 2 || paged);
        L.off_sparts = take(record_words<K>(nq, L.sp) * 4);
        L.off_sample_keys = take((size_t)nq * K * 8);
        L.off_thr = take((size_t)nq * 4);
    }
    L.p = plan_chunks(nq, nt - L.sample, false, K > 2 || paged);
    L.off_parts = take(record_words<K>(nq, L.p) * 4);   // [chunks][wave tiles] records
    return L;
}

// The steps. t: all nt rows; floor_keys / floor_base: the page floor of a paged scan (the kernels compare global row indices with it, so
// floor_base is the global index of the first row the step scans).
template <int K>
static void scan_prepass(const ScanLayout& L, char* buf, const void* q, const void* t, uint32_t index_base, hipStream_t s,
                         const uint64_t* floor_keys = nullptr, uint32_t floor_base = 0) {
    if (!L.sample) return;
    uint32_t* sparts = reinterpret_cast<uint32_t*>(buf + L.off_sparts);
    uint64_t* sample_keys = reinterpret_cast<uint64_t*>(buf + L.off_sample_keys);
    launch_topk<K>(q, L.nq, t, L.sample, nullptr, sparts, L.sp, s, "hamming_topk_sample", floor_keys, floor_base);
    merge_records_launch<K>(sparts, L.sp, index_base, nullptr, L.nq, sample_keys, s);
    hipLaunchKernelGGL(thr_from_keys_kernel, dim3(ceil_div(L.nq, 256)), dim3(256), 0, s, (const uint64_t*)sample_keys, L.nq, K,
                       reinterpret_cast<int*>(buf + L.off_thr));
    HIP_CHECK(hipGetLastError());
}

template <int K>
static void scan_main(const ScanLayout& L, char* buf, const void* q, const void* t, hipStream_t s, const uint64_t* floor_keys = nullptr,
                      uint32_t floor_base = 0) {
    const char* rest = static_cast<const char*>(t) + (size_t)L.sample * 64;
    launch_topk<K>(q, L.nq, rest, L.nt - L.sample, L.sample ? reinterpret_cast<const int*>(buf + L.off_thr) : nullptr,
                   reinterpret_cast<uint32_t*>(buf + L.off_parts), L.p, s, "hamming_topk", floor_keys, floor_base);
}

// the pre-pass's result joins the merge as one more (already expanded) list
template <int K>
static void scan_merge(const ScanLayout& L, const char* buf, uint32_t index_base, uint64_t* out, hipStream_t s) {
    merge_records_launch<K>(reinterpret_cast<const uint32_t*>(buf + L.off_parts), L.p, index_base + (uint32_t)L.sample,
                            L.sample ? reinterpret_cast<const uint64_t*>(buf + L.off_sample_keys) : nullptr, L.nq, out, s);
    HIP_CHECK(hipGetLastError());
}

// The three steps back to back on one stream, on the calling thread's workspace (the sample size: scan_layout).
template <int K>
static void topk_device_k(const void* q, int nq, const void* t, long long nt, uint32_t index_base, uint64_t* out, hipStream_t s) {
    const ScanLayout L = scan_layout<K>(nq, nt, false);
    char* buf = static_cast<char*>(ctx().alloc(L.bytes));
    scan_prepass<K>(L, buf, q, t, index_base, s);
    scan_main<K>(L, buf, q, t, s);
    scan_merge<K>(L, buf, index_base, out, s);
}

// k > 16 (BFMatcher::knnMatch takes any k, lib.rs:94-103): pages of 16. Page j is the plain K = 16 scan restricted to the keys above the
// last key of page j - 1 (keys are unique, so "above the floor" removes exactly the rows already reported); every page is a full pass over
// the train rows, with its own threshold pre-pass under the same floor. The scratch buffers are shared by the pages (stream order).
__global__ void gather_pages_kernel(const uint64_t* __restrict__ pages, int nq, int n_pages, int k, uint64_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)nq * k) return;
    const int q = (int)(i / k), c = (int)(i - (long long)q * k);
    const int page = c >> 4;
    out[i] = page < n_pages ? pages[((size_t)page * nq + q) * 16 + (c & 15)] : EMPTY_KEY;
}

static void topk_paged_device(const void* q, int nq, const void* t, long long nt, uint32_t index_base, int k, uint64_t* out, hipStream_t s) {
    constexpr int K = 16;
    ThreadCtx& c = ctx();
    const int n_pages = (int)std::min<long long>(ceil_div(k, K), ceil_div(nt, K));   // pages past the last train row would be empty
    const ScanLayout L = scan_layout<K>(nq, nt, true);
    char* buf = static_cast<char*>(c.alloc(L.bytes));
    uint64_t* pages = c.alloc_n<uint64_t>((size_t)n_pages * nq * K);
    for (int j = 0; j < n_pages; j++) {
        const uint64_t* floor_keys = j ? pages + (size_t)(j - 1) * nq * K : nullptr;
        scan_prepass<K>(L, buf, q, t, index_base, s, floor_keys, index_base);
        scan_main<K>(L, buf, q, t, s, floor_keys, index_base + (uint32_t)L.sample);
        scan_merge<K>(L, buf, index_base, pages + (size_t)j * nq * K, s);
    }
    hipLaunchKernelGGL(gather_pages_kernel, dim3((unsigned)ceil_div((long long)nq * k, 256)), dim3(256), 0, s, (const uint64_t*)pages, nq, n_pages, k, out);
    HIP_CHECK(hipGetLastError());
}

// ---- the same scan in three separately launched steps, for pipelines that overlap consecutive frames ---------------------------------
// topk_device_k runs threshold pre-pass -> main scan -> merge back to back on one stream: per frame ~0.6 ms of pre-pass, ~0.2 ms of
// merge and four dependent-launch gaps sit between two main scans. With the intermediate buffers owned by a per-frame state object
// (instead of the calling thread's workspace, which the next call reuses), frame i + 1's pre-pass can run on a second stream while
// frame i's main scan is on the GPU and frame i - 1's merge on a third: the main scans then follow each other directly.
struct TopkSplitState {
    int device = 0;
    char* buf = nullptr;
    size_t cap = 0;
    // the current frame, filled by the pre-pass: nq, k and nt in both forms, the rest is the vector form's layout of buf
    ScanLayout L{};
    // the matrix-core form (hamming_mfma.hip): expanded queries, the split lists, and the expanded train rows - the caller's resident copy
    // (topk_split_use_train) when it is one of exactly these rows, this state's own otherwise (expanded by every pre-pass)
    bool mfma = false;
    HmPlan hp{};
    const HmTrain* shared_train = nullptr;
    uint32_t index_base_mfma = 0;
    size_t off_q4 = 0, off_qp = 0, off_t4 = 0, off_tp = 0, off_lists = 0, off_top2 = 0;
    const void* t4 = nullptr;
    const float* tp = nullptr;
};

static void split_reserve(TopkSplitState& st, size_t need) {
    if (need <= st.cap) return;
    // grow-only; a frame still using the old buffer is finished first (rare: the first frames of a run)
    HIP_CHECK(hipDeviceSynchronize());
    if (st.buf) (void)hipFree(st.buf);
    st.buf = nullptr;
    st.cap = 0;
    const size_t want = need + need / 4;
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&st.buf), want));
    st.cap = want;
}

static void split_prepass_mfma(TopkSplitState& st, const void* q, int nq, const void* t, long long nt, int k, hipStream_t s) {
    st.mfma = true;
    st.L = ScanLayout{};
    st.L.nq = nq, st.L.k = k, st.L.nt = nt;
    st.hp = hm_plan(nq, nt);
    const bool shared = st.shared_train && st.shared_train->src == t && st.shared_train->n == nt;
    size_t need = 0;
    auto take = [&](size_t bytes) {
        const size_t o = need;
        need += (bytes + 255) & ~(size_t)255;
        return o;
    };
    st.off_q4 = take((size_t)nq * 256);
    st.off_qp = take((size_t)nq * 4);
    st.off_lists = take((size_t)st.hp.splits * nq * 16);
    st.off_top2 = take((size_t)nq * 16);
    if (!shared) {
        st.off_t4 = take((size_t)hm_padded_rows(nt) * 256);
        st.off_tp = take((size_t)hm_padded_rows(nt) * 4);
    }
    split_reserve(st, need);
    KernelTimer timer("hamming_topk_sample", s);
    hm_expand_device(q, nq, true, st.buf + st.off_q4, reinterpret_cast<float*>(st.buf + st.off_qp), s);
    if (shared) {
        st.t4 = st.shared_train->rows;
        st.tp = st.shared_train->pc;
    } else {
        hm_expand_device(t, nt, false, st.buf + st.off_t4, reinterpret_cast<float*>(st.buf + st.off_tp), s);
        st.t4 = st.buf + st.off_t4;
        st.tp = reinterpret_cast<const float*>(st.buf + st.off_tp);
    }
    HIP_CHECK(hipGetLastError());
}
static void split_scan_mfma(TopkSplitState& st, hipStream_t s) {
    hm_scan_device(st.buf + st.off_q4, reinterpret_cast<const float*>(st.buf + st.off_qp), st.L.nq, st.t4, st.tp, st.L.nt, st.hp, st.index_base_mfma,
                   reinterpret_cast<uint64_t*>(st.buf + st.off_lists), s);
}
static void split_merge_mfma(TopkSplitState& st, uint64_t* out, hipStream_t s) {
    const int nq = st.L.nq, k = st.L.k;
    const uint64_t* parts = reinterpret_cast<const uint64_t*>(st.buf + st.off_lists);
    uint64_t* top2 = k == 2 ? out : reinterpret_cast<uint64_t*>(st.buf + st.off_top2);
    if (st.hp.splits > 1) merge_topk_device(parts, st.hp.splits, nq, 2, top2, s);
    else if (k == 2) HIP_CHECK(hipMemcpyAsync(out, parts, (size_t)nq * 16, hipMemcpyDeviceToDevice, s));
    else top2 = const_cast<uint64_t*>(parts);
    if (k == 1) take_first_columns_device(top2, nq, 2, 1, out, s);
    HIP_CHECK(hipGetLastError());
}

template <int K>
static void split_prepass_k(TopkSplitState& st, const void* q, int nq, const void* t, long long nt, uint32_t index_base, hipStream_t s) {
    st.L = scan_layout<K>(nq, nt, false);
    split_reserve(st, st.L.bytes);
    scan_prepass<K>(st.L, st.buf, q, t, index_base, s);
}

void* topk_split_create() {
    TopkSplitState* st = new TopkSplitState();
    st->device = ctx().device;
    return st;
}
void topk_split_destroy(void* h) {
    TopkSplitState* st = static_cast<TopkSplitState*>(h);
    if (!st) return;
    DeviceGuard on(st->device);
    (void)hipDeviceSynchronize();
    if (st->buf) (void)hipFree(st->buf);
    delete st;
}
void topk_split_prepass(void* h, const void* q, int nq, const void* t, long long nt, uint32_t index_base, int k, hipStream_t s) {
    APDS_REQUIRE(h, APDS_ERR_BAD_ARG, "null scan state");
    APDS_REQUIRE(k == 1 || k == 2, APDS_ERR_ASSERT, "the split scan serves k = 1 and k = 2 (what the crate surface consumes, lib.rs:107-111)");
    APDS_REQUIRE(nq > 0 && nt > 0 && nt < (1ll << 31), APDS_ERR_ASSERT, "the split scan needs queries and train rows");
    TopkSplitState& st = *static_cast<TopkSplitState*>(h);
    if (config().match_mfma) {
        st.index_base_mfma = index_base;
        split_prepass_mfma(st, q, nq, t, nt, k, s);
        return;
    }
    st.mfma = false;
    if (k == 1) split_prepass_k<1>(st, q, nq, t, nt, index_base, s);
    else split_prepass_k<2>(st, q, nq, t, nt, index_base, s);
}
void topk_split_use_train(void* h, const void* hm_train) {
    APDS_REQUIRE(h, APDS_ERR_BAD_ARG, "null scan state");
    static_cast<TopkSplitState*>(h)->shared_train = static_cast<const HmTrain*>(hm_train);
}
void topk_split_scan(void* h, const void* q, const void* t, hipStream_t s) {
    APDS_REQUIRE(h, APDS_ERR_BAD_ARG, "null scan state");
    TopkSplitState& st = *static_cast<TopkSplitState*>(h);
    APDS_REQUIRE(st.L.nq > 0, APDS_ERR_ASSERT, "scan before pre-pass");
    if (st.mfma) {
        split_scan_mfma(st, s);
        return;
    }
    if (st.L.k == 1) scan_main<1>(st.L, st.buf, q, t, s);
    else scan_main<2>(st.L, st.buf, q, t, s);
}
void topk_split_merge(void* h, uint32_t index_base, uint64_t* out, hipStream_t s) {
    APDS_REQUIRE(h && out, APDS_ERR_BAD_ARG, "null scan state / output");
    TopkSplitState& st = *static_cast<TopkSplitState*>(h);
    APDS_REQUIRE(st.L.nq > 0, APDS_ERR_ASSERT, "merge before pre-pass");
    if (st.mfma) {
        APDS_REQUIRE(index_base == st.index_base_mfma, APDS_ERR_ASSERT, "the merge's index base differs from the pre-pass's");
        split_merge_mfma(st, out, s);
        return;
    }
    if (st.L.k == 1) scan_merge<1>(st.L, st.buf, index_base, out, s);
    else scan_merge<2>(st.L, st.buf, index_base, out, s);
}

// Full top-k of nq queries over nt train rows (device, 64-byte rows). out: nq*k keys. k in {1,2} is the tuned path (the reference only
// ever consumes the two nearest, lib.rs:107-111); 3 <= k <= 16 run with one query per lane here (3 <= k <= APDS_MATCH_MFMA_KMAX on the matrix
// cores instead: hamming_mfma_topk_kernel), larger k in pages of 16 (topk_paged_device).
void hamming_topk_device(const void* q, int nq, const void* t, long long nt, uint32_t index_base, int k, uint64_t* out,
                         hipStream_t s, int backend) {
    APDS_REQUIRE(k >= 1, APDS_ERR_ASSERT, "top-k needs k >= 1");
    APDS_REQUIRE(nt < (1ll << 31), APDS_ERR_ASSERT, "train set too large for one call; shard it");
    APDS_REQUIRE(!(backend == 3 && k > 8), APDS_ERR_ASSERT, "backend 3 (matrix cores) serves k <= 8");
    if (nq <= 0) return;
    if (nt <= 0) {
        HIP_CHECK(hipMemsetAsync(out, 0xFF, (size_t)nq * k * 8, s));
        return;
    }
    if (k > 16) {
        topk_paged_device(q, nq, t, nt, index_base, k, out, s);
        return;
    }
    APDS_REQUIRE(backend >= 0 && backend <= 3 && !(backend == 2 && k > 2) && !(backend == 3 && k > 8), APDS_ERR_ASSERT,
                 "backend: 0 default, 1 vector ALU, 2 matrix cores (k <= 2), 3 matrix cores (k <= 8)");
    // the two nearest (all the crate surface consumes) come from the matrix cores, and so do 3 <= k <= APDS_MATCH_MFMA_KMAX
    if (backend == 2 || backend == 3 || (backend == 0 && config().match_mfma && k <= std::max(2, config().match_mfma_kmax))) {
        hamming_mfma_topk_device(q, nq, t, nt, index_base, k, out, s);
        return;
    }
    const int K = k <= 2 ? k : (k <= 4 ? 4 : (k <= 8 ? 8 : 16));
    uint64_t* dst = K == k ? out : ctx().alloc_n<uint64_t>((size_t)nq * K);
    switch (K) {
        case 1: topk_device_k<1>(q, nq, t, nt, index_base, dst, s); break;
        case 2: topk_device_k<2>(q, nq, t, nt, index_base, dst, s); break;
        case 4: topk_device_k<4>(q, nq, t, nt, index_base, dst, s); break;
        case 8: topk_device_k<8>(q, nq, t, nt, index_base, dst, s); break;
        default: topk_device_k<16>(q, nq, t, nt, index_base, dst, s); break;
    }
    if (K != k) {
        take_first_columns_device(dst, nq, K, k, out, s);
        HIP_CHECK(hipGetLastError());
    }
}

void pack_rows_device(const void* src, long long n, int desc_bytes, long long src_stride, void* dst, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(pack_rows_kernel, dim3(ceil_div(n * 16, 256)), dim3(256), 0, s, static_cast<const uint8_t*>(src), n, desc_bytes, src_stride,
                       static_cast<uint32_t*>(dst));
    HIP_CHECK(hipGetLastError());
}


}  // namespace apds
