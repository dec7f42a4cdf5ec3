// csrc/hamming_mfma.hip — Hamming top-k of 512-bit rows on the FP4 matrix pipe (get_knn_matches, lib.rs:94-114): k <= 2 on hamming_mfma_kernel (all
// the crate consumes; the tuned path), 3 <= k <= 8 on hamming_mfma_topk_kernel further down.
//
// Brute-force Hamming matching is all pairs x all bits: Q x N x 512 one-bit products. match_hamming.hip forms them on the vector ALU
// (xor + popcount per dword: 32 lane-operations per pair, bound by the half-rate v_bcnt at 52 T lane-op/s = 1.6e12 pairs/s). CDNA4's
// matrix cores multiply 4-bit operands at ~10 PFLOP/s dense, and a bit IS a 4-bit float: with
//     train bit  -> e2m1  1.0 (0x2)        query bit -> e2m1 -2.0 (0xC)        accumulator preset to popcount(train row)
// one v_mfma_scale_f32_16x16x128_f8f6f4 (unit scales) adds -2 * (t AND q) over 128 bit positions for 16 x 16 pairs, and after four of
// them the accumulator holds popcount(t) - 2 popcount(t AND q) = hamming(t, q) - popcount(q): the ranking value of the pair, EXACT (every
// product is 0 or -2, every partial sum an integer of magnitude <= 1024: nothing rounds in binary32). The distances, the ties (lower train
// row first) and therefore the keys are those of hamming_topk_kernel bit for bit (tests/test_match_gpu.py runs both).
// 2 * 512 flop per pair on the 10 PF pipe is a ceiling of 9.8e12 pairs/s, six times the vector formulation's.
//
// Two steps per call:
//   hm_expand_rows_kernel   64-byte rows -> 256-byte rows of fp4 nibbles (one dword -> 16 bytes; bit k of dword d is element 32 d + k;
//                           any order would do as long as both operands use the same one) + popcount per row as a float
//   hamming_mfma_kernel     the structure of l2_screen_kernel (same tile shapes: there K = 128 bf16 elements are 256 bytes, here K = 512
//                           fp4 elements are): block = 8 waves x 48 queries held as B operands in registers for the whole kernel,
//                           128-row train tiles double-buffered in LDS, filled by LDS-DMA (global_load_lds_dwordx4: no staging registers,
//                           no ds_write) into an XOR-swizzled image (conflict-free ds_read_b128), each A read feeds three MFMAs, running
//                           top-2 per query column in the lanes, insertion code only when some lane has a hit.
//   The tile loop (hm_scan_tiles, shared with the k = 3 .. 8 kernel) is software-pipelined twice: the DMA of tile n + 1 is in flight
//   while tile n is computed (issued from assembly - for a DMA it knows of, the compiler waits vmcnt(0) in front of the next ds_read,
//   because it cannot tell the two buffers of the LDS array apart; each wave waits for its own share in front of the barrier that closes
//   the tile), and the operands of row block b + 1 are read right behind the twelve MFMAs of block b, under the ranking of block b. Against
//   the loop that drained the DMA in front of every tile's first MFMA and read a block's operands in front of its own MFMAs: 141.2 ->
//   148.7 frames/s in the pipeline, median of five alternating runs (profiles/hm_pipeline/ab_bench.txt). (Ranking a block's values under
//   the NEXT block's MFMAs was written twice - values carried over, ranking forced between the MFMA halves - and both times the compiler
//   put the twelve MFMAs of a block back together and ranked behind them; those wait states are filled by the SIMD's other waves.)
#include <atomic>
#include <memory>

#include "config.h"
#include "kernels.h"
#include "topk_keys.h"

namespace apds {

typedef int hm_v8i __attribute__((ext_vector_type(8)));
typedef float hm_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t hm_u32x4 __attribute__((ext_vector_type(4)));

#ifndef APDS_HM_WAVES
#define APDS_HM_WAVES 8
#endif
static constexpr int HM_WAVES = APDS_HM_WAVES;   // waves per workgroup; a wave stages 16 rows of a tile. (16: one 1024-thread workgroup per CU, 256-row
                                                 // tiles, half the barriers: 5.58 against 5.46 ms alone, 148.7 against 147.5 frames/s in the pipeline -
                                                 // no difference worth a second shape; profiles/r04/match_mfma_probe_w16.txt)
static constexpr int HM_TM = 16 * HM_WAVES;      // train rows per tile
#ifndef APDS_HM_WPE
#define APDS_HM_WPE 4
#endif
// waves per SIMD the kernel is compiled for (4: two 8-wave workgroups per CU. The 12-wave shape - APDS_HM_WAVES=12 APDS_HM_WPE=3, one
// workgroup per CU with a quarter of the registers left to the other stages' kernels - is a build-time experiment)
// The top-2 kernel's register cap. A wave's allocation is its count rounded up to the granule of 8, and a SIMD holds 512 registers per lane:
//     4 waves x 104 = 416, and 96 are left - one wave of any kernel of 96 registers or fewer beside the four match waves, on every SIMD
//     of the chip, for as long as the match runs (at 113 -> 120 allocated, 4 x 120 = 480 left 32: no wave of any other stage fitted, and
//     the extraction ran only where a whole match workgroup had retired).
// Stated to the compiler so that an edit cannot cross the granule unseen (tests/test_hamming_mfma_budget.py reads the count, scratch and
// spills back). The attribute counts the architected half of gfx90a-and-later's unified file: the backend doubles what it is given and
// clamps that to the range of amdgpu_waves_per_eu, so the kernel asks for half the cap. (128: the same as no cap - the A/B build.)
#ifndef APDS_HM_TOP2_VGPRS
#define APDS_HM_TOP2_VGPRS (APDS_HM_WPE == 4 ? 104 : 512 / APDS_HM_WPE / 8 * 8)
#endif
static_assert(APDS_HM_TOP2_VGPRS % 8 == 0 && APDS_HM_WPE * APDS_HM_TOP2_VGPRS <= 512, "the cap is whole granules that fit the SIMD's file");
#ifndef APDS_HM_NC
#define APDS_HM_NC 3
#endif
static constexpr int HM_NC = APDS_HM_NC;      // 16-query column blocks per wave (4: 15 registers spill at four waves per SIMD; 7.0 against 5.9 ms on the
                                              // headline shape, 11.0 against 11.9 on 262143^2: profiles/r04/match_mfma_probe.txt)
static constexpr int HM_Q = HM_WAVES * 16 * HM_NC;   // queries per block
static constexpr int HM_UNIT_SCALE = 0x7F7F7F7F;   // E8M0 127 = 2^0 in every byte
// Train popcounts are stored with this bias: the ranking value popcount(t) + 1024 - 2 (t AND q) is then a POSITIVE float (>= 512), and
// positive floats order like their bit patterns - the epilogue compares them as unsigned integers (v_min3_u32 / v_min_u32 / v_cmp_lt_u32:
// no NaN canonicalisation in front of every float minimum, six v_max_f32 less per 16 x 48 block of pairs). +inf (rows past the end) is
// 0x7F800000: above every finite value, below the empty marker 0xFFFFFFFF.
static constexpr int HM_BIAS = 1024;

// 8 bits -> 8 nibbles holding `nib` where the bit is set
__device__ __forceinline__ uint32_t hm_spread8(uint32_t b, uint32_t nib) {
    uint32_t t = b & 0xFFu;
    t = (t | (t << 12)) & 0x000F000Fu;
    t = (t | (t << 6)) & 0x03030303u;
    t = (t | (t << 3)) & 0x11111111u;
    return t * nib;
}

// rows: n x 16 dwords. out: n x 16 uint4 (dword d of a row -> uint4 d). pc: popcount of each row + bias. One thread per dword.
__global__ __launch_bounds__(256) void hm_expand_rows_kernel(const uint32_t* __restrict__ rows, long long n, uint32_t nib, int bias, uint4* __restrict__ out,
                                                             float* __restrict__ pc) {
    APDS_RAISE_WAVE_PRIORITY();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const uint32_t d = i < n * 16 ? rows[i] : 0u;
    int v = __popc(d);
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off);   // the 16 lanes of a row are aligned: 256 threads = 16 rows
    if (i >= n * 16) return;
    out[i] = make_uint4(hm_spread8(d, nib), hm_spread8(d >> 8, nib), hm_spread8(d >> 16, nib), hm_spread8(d >> 24, nib));
    if ((threadIdx.x & 15) == 0) pc[i >> 4] = (float)(v + bias);
}

// the rows past the end of the last tile: zero operands, popcount +inf (they never rank). One block of 128 threads x 16.
__global__ void hm_pad_rows_kernel(uint4* __restrict__ rows, float* __restrict__ pc, long long n, long long n_pad) {
    const long long i = n + (threadIdx.x >> 4);
    if (i >= n_pad) return;
    for (long long r = i; r < n_pad; r += 8) {
        rows[r * 16 + (threadIdx.x & 15)] = make_uint4(0, 0, 0, 0);
        if ((threadIdx.x & 15) == 0) pc[r] = INFINITY;
    }
}

// thr[q]: the kernel's ranking value (hamming - popcount(query) + bias, as float bits) of the last key of a finished top-K list (K = 2, 4, 8)
__global__ void hm_thresholds_kernel(const uint64_t* __restrict__ topk, int K, const float* __restrict__ qpc, int nq, uint32_t* __restrict__ thr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const uint64_t k2 = topk[(size_t)i * K + K - 1];
    thr[i] = k2 == EMPTY_KEY ? 0x7F800000u : __float_as_uint((float)((int)key_rank(k2) - (int)qpc[i] + HM_BIAS));
}

struct HmTop2 {
    uint32_t d0, d1;   // bit patterns of the (positive) ranking values
    uint32_t i0, i1;
};
__device__ __forceinline__ void hm_insert(HmTop2& b, uint32_t d, uint32_t idx) {   // rows arrive in ascending order: strict '<' keeps the lower row of a tie
    if (d < b.d1) {
        if (d < b.d0) {
            b.d1 = b.d0;
            b.i1 = b.i0;
            b.d0 = d;
            b.i0 = idx;
        } else {
            b.d1 = d;
            b.i1 = idx;
        }
    }
}

// ---- the tile loop of both kernels ----
// One wave's share of a tile by LDS-DMA: rows [16 wave, 16 wave + 16) as four pieces of 1 KB (4 rows each). The source of piece i is the
// wave-uniform tile base + a per-lane constant ((voff0 ^ 64 i) + 1024 i: hm_scan_tiles says why; pieces 1 .. 3 make theirs here, in a
// register the statement gives back - the v_xor behind the write of m0 is also the wait state a DMA needs behind it); the destination is
// wave-uniform (m0) + 1024 i + 16 lane - the instruction offset counts on both sides. Written as assembly because the DMA has to stay in flight while the tile in the OTHER buffer is read: the
// compiler cannot tell the two halves of one LDS array apart and, for a DMA it knows of, waits vmcnt(0) in front of the next ds_read
// (the builtin form of this loop had that wait two instructions behind the DMA issue, in front of every tile's first MFMA). Nothing else
// in the loop uses the vector-memory counter; the wave that issued a DMA waits for it itself (hm_dma_wait) in front of the barrier
// behind which the tile is read - a barrier alone does not wait for a DMA. m0 is the compiler's: saved and restored.
__device__ __forceinline__ void hm_dma_rows(const unsigned char* tile_base, int voff0, uint32_t lds_dst) {
    uint32_t keep;
    int t;   // the source constant of pieces 1 .. 3 (see hm_scan_tiles): live inside this statement only
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %4\n\t"
        "v_xor_b32 %1, 64, %2\n\t"
        "global_load_lds_dwordx4 %2, %3\n\t"
        "global_load_lds_dwordx4 %1, %3 offset:1024\n\t"
        "v_xor_b32 %1, 0x80, %2\n\t"
        "global_load_lds_dwordx4 %1, %3 offset:2048\n\t"
        "v_xor_b32 %1, 0xc0, %2\n\t"
        "global_load_lds_dwordx4 %1, %3 offset:3072\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep), "=&v"(t)
        : "v"(voff0), "s"(tile_base), "s"(lds_dst)
        : "memory");
}
// 64 popcounts (one float per lane; the source offset 4 * lane is made here, in a register that is free again behind the statement)
__device__ __forceinline__ void hm_dma_popcounts(const float* src, uint32_t lds_dst) {
    uint32_t keep;
    int t;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "v_mbcnt_lo_u32_b32 %1, -1, 0\n\t"
        "v_mbcnt_hi_u32_b32 %1, -1, %1\n\t"
        "v_lshlrev_b32 %1, 2, %1\n\t"
        "global_load_lds_dword %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep), "=&v"(t)
        : "s"(src), "s"(lds_dst)
        : "memory");
}
__device__ __forceinline__ void hm_dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// A loaded value is in its register from here on: the compiler's wait for it stands in front of this, not at the value's first use (which, for
// what the kernels load in front of hm_scan_tiles, would be inside the tile loop or behind it - see there).
template <class T>
__device__ __forceinline__ void hm_settle(T& v) { asm volatile("" : "+v"(v)); }

// Train tiles [tile_begin, tile_end) against the NC x 16 query columns a wave holds as B operands; rank(acc, row0) takes the values of a
// 16-row block (acc[c][j]: row row0 + j of the block's row group against column block c).
// The schedule, per wave:
//     DMA of tile n + 1 into the other buffer      (in flight until the wait below)
//     8 x { 4 NC MFMAs of block b | ds_reads of block b + 1 | ranking of block b }
// The operands of a block (four ds_read_b128 + the popcount preset) are read right behind the MFMAs of the block before - an A register is
// free once the last MFMA that reads it has issued - so the LDS latency runs under the ranking instead of in front of the first MFMA.
// Behind the LAST block's MFMAs stand the wait for this wave's DMA and the workgroup barrier (everybody's reads of this tile have fed
// their MFMAs; everybody's share of the next tile has landed), then block 0 of the next tile is read, then the last block is ranked: the
// tile border costs the barrier and nothing else. (After the last tile of a split the read fetches whatever the other buffer holds; it
// is not used.)
template <int NC, int PRIO, class Rank>
__device__ __forceinline__ void hm_scan_tiles(const uint4* __restrict__ train_fp4, const float* __restrict__ tpc, int tile_begin, int tile_end,
                                              uint4 (&B)[NC][4], uint32_t index_base, Rank&& rank) {
    extern __shared__ __attribute__((aligned(128))) unsigned char hm_lds[];
    constexpr int TILE_BYTES = HM_TM * 256;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, kq = lane >> 4;
    const uint32_t lds0 = (uint32_t)(__SIZE_TYPE__)(__attribute__((address_space(3))) unsigned char*)hm_lds;
    // (the expanded rows are padded to whole tiles - zero rows with a popcount of +inf - so a piece's source is a uniform tile base plus a
    // per-lane constant: scalar address arithmetic only)
    // Piece i holds rows r = 16 wave + 4 i + kq, and its constant is 256 r + ((col ^ (r & 15)) << 4) - 1024 i. With r & 15 = 4 i + kq = 4 i ^ kq
    // that is 4096 wave + 256 kq + (((col ^ kq) ^ 4 i) << 4): piece 0's constant with 64 i XORed in (bits 6 and 7, which no other term
    // touches). One register holds piece 0's; hm_dma_rows derives the others where it issues them - three v_xor per tile (once in about
    // 6 000 cycles) for three registers of the whole loop.
    const int voff0 = (16 * wave + kq) * 256 + ((col ^ kq) << 4);
    auto stage = [&](int tile, int buf) {
        hm_dma_rows(reinterpret_cast<const unsigned char*>(train_fp4) + (size_t)tile * TILE_BYTES, voff0, lds0 + buf * TILE_BYTES + 16 * wave * 256);
        if (wave < HM_TM / 64) hm_dma_popcounts(tpc + (size_t)tile * HM_TM + 64 * wave, lds0 + 2 * TILE_BYTES + buf * (HM_TM * 4) + 256 * wave);
    };
    // this lane's four A reads of a 16-row block: row (16 rb + col), chunk 4 s + kq at position (4 s + kq) ^ col; behind them the popcounts
    // of rows 4 kq .. + 3 of a block. Offsets into the buffer being read: they change sides at every tile border.
    // (LDS addresses as integers: the array's base is folded in once, a read is one ds_read_b128 with an immediate offset)
    typedef const __attribute__((address_space(3))) hm_u32x4* lds_u4;
    typedef const __attribute__((address_space(3))) hm_f32x4* lds_f4;
    uint32_t ra[4], rn = lds0 + 2 * TILE_BYTES + 16 * kq;
#pragma unroll
    for (int s = 0; s < 4; s++) ra[s] = lds0 + col * 256 + (((4 * s + kq) ^ col) << 4);

    hm_u32x4 a[4];
    hm_f32x4 init;                                            // biased popcounts of this lane's four rows
    auto read_block = [&](int rb) {
#pragma unroll
        for (int s = 0; s < 4; s++) a[s] = *(lds_u4)(__SIZE_TYPE__)(ra[s] + rb * 4096);
        init = *(lds_f4)(__SIZE_TYPE__)(rn + rb * 64);
    };

    // Everything the compiler loaded for this wave so far (the B operands, the thresholds) is waited for HERE: it counts its own loads only,
    // so a wait of its making behind the first DMA would both count wrongly and, inside the loop, drain the prefetch once per tile.
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
        for (int s = 0; s < 4; s++) hm_settle(B[c][s].x), hm_settle(B[c][s].y), hm_settle(B[c][s].z), hm_settle(B[c][s].w);
    hm_dma_wait();
    stage(tile_begin, 0);
    hm_dma_wait();
    __syncthreads();
    read_block(0);
    hm_f32x4 acc[NC];
    for (int tile = tile_begin; tile < tile_end; tile++) {
        const int buf = (tile - tile_begin) & 1;
        if (tile + 1 < tile_end) stage(tile + 1, buf ^ 1);
#pragma unroll
        for (int rb = 0; rb < HM_TM / 16; rb++) {                  // 16-row blocks of the tile
            // a wave about to feed the matrix pipe goes ahead of the SIMD's waves that are ranking: 5.94 -> 5.60 ms alone, 139.4 -> 147.3
            // frames/s in the pipeline (profiles/r04/mfma_prio_ab.txt, ab_bench_env.txt); levels 1, 2, 3 alike
            if (PRIO) __builtin_amdgcn_s_setprio(PRIO);
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const hm_v8i A = {(int)a[s].x, (int)a[s].y, (int)a[s].z, (int)a[s].w, 0, 0, 0, 0};
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    const hm_v8i Bv = {(int)B[c][s].x, (int)B[c][s].y, (int)B[c][s].z, (int)B[c][s].w, 0, 0, 0, 0};
                    acc[c] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A, Bv, s == 0 ? init : acc[c], 4, 4, 0, HM_UNIT_SCALE, 0, HM_UNIT_SCALE);
                }
            }
            if (PRIO) __builtin_amdgcn_s_setprio(0);
            if (rb + 1 < HM_TM / 16) {
                read_block(rb + 1);
            } else {
                hm_dma_wait();
                __syncthreads();   // the next tile has landed; everybody's MFMAs have taken the last of this one
#pragma unroll
                for (int s = 0; s < 4; s++) ra[s] += buf ? -TILE_BYTES : TILE_BYTES;
                rn += buf ? -HM_TM * 4 : HM_TM * 4;
                read_block(0);
            }
            // The accumulators are pinned behind the reads and the reads in front of the ranking: left alone, the compiler sinks the MFMAs of
            // the later column blocks behind the first block's ranking, the A registers stay live across the reads, and the next block's
            // operands take twenty registers of their own.
#pragma unroll
            for (int c = 0; c < NC; c++) hm_settle(acc[c]);
            __builtin_amdgcn_sched_barrier(0);
            rank(acc, (uint32_t)(tile * HM_TM + rb * 16 + 4 * kq) + index_base);
        }
    }
}

// ---- what the two kernels spell alike around the tile loop ----
// A workgroup's split of the train tiles and its query tile; a wave's first query. Workgroup b runs on XCD b % 8 (round-robin dispatch) and
// every XCD has an L2 of its own. With a multiple of eight splits, split x + 8 m belongs to XCD x: the workgroups resident on an XCD at any
// time are consecutive query tiles of one split, start together and walk the same train tiles at about the same pace - one fetches a tile,
// the others find it in their L2.
struct HmItem {
    int split, q0, tile_begin, tile_end;
    int col, kq;   // accumulator column / k chunk (operands) / row group (accumulators)
};
template <int NC>
__device__ __forceinline__ HmItem hm_work_item(int n_train, int tiles_per_split, int q_tiles, int splits) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    HmItem w;
    int qtile;
    if ((splits & 7) == 0) {
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        w.split = xcd + 8 * (j / q_tiles);
        qtile = j % q_tiles;
    } else {
        w.split = blockIdx.x / q_tiles;
        qtile = blockIdx.x % q_tiles;
    }
    w.q0 = qtile * (HM_WAVES * 16 * NC) + wave * 16 * NC;   // this wave's queries
    const int n_tiles = (n_train + HM_TM - 1) / HM_TM;
    w.tile_begin = w.split * tiles_per_split, w.tile_end = min(n_tiles, w.tile_begin + tiles_per_split);
    w.col = lane & 15, w.kq = lane >> 4;
    return w;
}
// B operands: query (q0 + 16 c + col), elements 128 s + 32 kq .. + 31 (dword 4 s + kq of the row), for the four k steps s
template <int NC>
__device__ __forceinline__ void hm_load_operands(const uint4* query_fp4, int nq, int q0, int col, int kq, uint4 (&B)[NC][4]) {
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const int qi = min(q0 + 16 * c + col, nq - 1);
#pragma unroll
        for (int s = 0; s < 4; s++) B[c][s] = query_fp4[(size_t)qi * 16 + 4 * s + kq];
    }
}
// ... and qq: the queries' popcounts, for a kernel that keeps them in registers across the tile loop
template <int NC>
__device__ __forceinline__ void hm_load_queries(const uint4* query_fp4, const float* qpc, int nq, int q0, int col, int kq, uint4 (&B)[NC][4], float (&qq)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const int qi = min(q0 + 16 * c + col, nq - 1);
#pragma unroll
        for (int s = 0; s < 4; s++) B[c][s] = query_fp4[(size_t)qi * 16 + 4 * s + kq];
        qq[c] = qpc[qi];
    }
}
// What every entry of the list of query qi starts as, without a row: thr[qi] when the caller has one - the K-th smallest ranking value over a
// sample of EARLIER rows (lower indices, so a row of this launch enters the query's final list only with a strictly smaller value) - or +inf.
// Real rows push the copies out; what is left of them at the end is written as empty.
template <bool THR>
__device__ __forceinline__ uint32_t hm_start_value(const uint32_t* thr, int qi) {
    return THR ? thr[qi] : 0x7F800000u;
}
// Ranking value d (float bits) of a row against a query with popcount qq -> their Hamming distance, the rank of the final key. (The whole
// key - empty for an entry without a row - as one function changed the kernels' register allocation; this much of it does not.)
__device__ __forceinline__ uint32_t hm_distance(float qq, uint32_t d) { return (uint32_t)((int)(qq + __uint_as_float(d)) - HM_BIAS); }

// out[split][nq][2]: keys (distance << 32 | row + index_base), EMPTY where the split holds fewer than two rows.
// LDS image of a tile (no padding: the tile is filled by LDS-DMA, whose destination is wave-uniform base + 16 * lane): row r at 256 r, and
// its 16-byte chunk c at position c ^ (r & 15) - the 16 rows a ds_read_b128 group reads chunk c of then sit in 16 different bank groups.
// The DMA's per-lane SOURCE address applies the same involution, so the image is a plain lane-linear copy for the hardware.
// Rows and popcounts are padded to whole tiles (zero operands, +inf: rows past the end never rank).
// THR: the launch starts from thresholds (the main launch behind a threshold launch) - a template parameter so that profilers list the two
// launches of a match under two names
template <int PRIO, bool THR>
__global__ __launch_bounds__(64 * HM_WAVES) __attribute__((amdgpu_waves_per_eu(APDS_HM_WPE, APDS_HM_WPE), amdgpu_num_vgpr(APDS_HM_TOP2_VGPRS / 2))) void hamming_mfma_kernel(const uint4* __restrict__ train_fp4, const float* __restrict__ tpc, int n_train,
                                                           const uint4* __restrict__ query_fp4, const float* __restrict__ qpc, int nq, int tiles_per_split,
                                                           int q_tiles, int splits, uint32_t index_base, const uint32_t* __restrict__ thr,
                                                           uint64_t* __restrict__ out) {
    // (no APDS_RAISE_WAVE_PRIORITY here: this is the kernel the short kernels of the other stages raise their priority against)
    const HmItem w = hm_work_item<HM_NC>(n_train, tiles_per_split, q_tiles, splits);
    // (locals, and by value into the helpers: with the struct handed on by reference the kernels' register allocation changed)
    const int split = w.split, q0 = w.q0, tile_begin = w.tile_begin, tile_end = w.tile_end, col = w.col, kq = w.kq;
    uint4 B[HM_NC][4];
    hm_load_operands<HM_NC>(query_fp4, nq, q0, col, kq, B);   // (the queries' popcounts are read where they are used: behind the tile loop)
    HmTop2 best[HM_NC];   // both entries start as hm_start_value
#pragma unroll
    for (int c = 0; c < HM_NC; c++) {
        best[c].d0 = hm_start_value<THR>(thr, min(q0 + 16 * c + col, nq - 1));
        hm_settle(best[c].d0);
        best[c].d1 = best[c].d0;
        best[c].i0 = best[c].i1 = 0xFFFFFFFFu;
    }

    if (tile_begin < tile_end) {
        // Ranking a block: one minimum and one compare per 16 x 16 accumulator in the common case. Only the query blocks in which some lane
        // has a hit run insertion code (a wave-uniform branch each): the counters put the vector instructions beside the MFMAs at 1.9 per
        // MFMA when any hit sent all three query blocks through the twelve insertions, and an MFMA leaves the SIMD's issue port free for
        // only two of them. (One threshold per lane - the largest of the three - and one minimum over all twelve values in front of the
        // per-block tests: 7 instructions and one branch instead of 9 and three in the common case, and 8 % SLOWER on every shape
        // (profiles/r04/match_mfma_probe_single_threshold.txt): a chain of six dependent minima in front of the branch. The twelve MFMAs as
        // three chains of four with the previous chain's minimum / test placed between the next chain's MFMAs by sched_group_barrier: the
        // compiler follows the directives, keeps its wait states (it counts an MFMA as one), and nothing changes: 5.45 - 5.51 ms.)
        hm_scan_tiles<HM_NC, PRIO>(train_fp4, tpc, tile_begin, tile_end, B, index_base, [&](const hm_f32x4 (&a)[HM_NC], uint32_t row0) {
            bool hit[HM_NC];
#pragma unroll
            for (int c = 0; c < HM_NC; c++) {
                const uint32_t mn = min(min(__float_as_uint(a[c][0]), __float_as_uint(a[c][1])), min(__float_as_uint(a[c][2]), __float_as_uint(a[c][3])));
                hit[c] = mn < best[c].d1;
            }
#pragma unroll
            for (int c = 0; c < HM_NC; c++)
                if (__any(hit[c])) {
#pragma unroll
                    for (int j = 0; j < 4; j++) hm_insert(best[c], __float_as_uint(a[c][j]), row0 + j);
                }
        });
    }
    // a query column lives in four lanes (kq = 0..3, different rows): fold them with shuffles, lanes 0..15 write
#pragma unroll
    for (int c = 0; c < HM_NC; c++) {
        HmTop2 b = best[c];
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) {
            const uint32_t od0 = (uint32_t)__shfl_xor((int)b.d0, off), od1 = (uint32_t)__shfl_xor((int)b.d1, off);
            const uint32_t oi0 = (uint32_t)__shfl_xor((int)b.i0, off), oi1 = (uint32_t)__shfl_xor((int)b.i1, off);
            HmTop2 m = b;   // merge two sorted pairs; equal values: lower row first
            auto ins = [&](uint32_t d, uint32_t i) {
                if (i == 0xFFFFFFFFu) return;
                if (d < m.d0 || (d == m.d0 && i < m.i0)) {
                    m.d1 = m.d0;
                    m.i1 = m.i0;
                    m.d0 = d;
                    m.i0 = i;
                } else if ((d < m.d1 || (d == m.d1 && i < m.i1)) && i != m.i0) {
                    m.d1 = d;
                    m.i1 = i;
                }
            };
            ins(od0, oi0);
            ins(od1, oi1);
            b = m;
        }
        const int qi = q0 + 16 * c + col;
        if (kq == 0 && qi < nq) {
            uint64_t* o = out + ((size_t)split * nq + qi) * 2;
            const float qq = qpc[qi];   // the query's popcount: one load per output pair, not a register per column block across the loop
            o[0] = b.i0 == 0xFFFFFFFFu ? EMPTY_KEY : make_key(hm_distance(qq, b.d0), b.i0);
            o[1] = b.i1 == 0xFFFFFFFFu ? EMPTY_KEY : make_key(hm_distance(qq, b.d1), b.i1);
        }
    }
}

// ---- 3 <= k <= 8: the same kernel around a sorted K-entry list per query column and lane (K = 4 serves k = 3, 4; K = 8 serves k = 5 .. 8) ----
// A kernel of its own rather than a K parameter of hamming_mfma_kernel: the top-2 kernel's registers and instruction stream stay what they
// are. Everything in front of the ranking is shared with it (hm_work_item, hm_load_queries, hm_start_value, hm_scan_tiles: operands, LDS
// image, LDS-DMA staging, preset accumulator, four scaled MFMAs per 16 x 16 block), and so is hm_distance behind it; what follows the list length is here: the column blocks per wave (the list registers come out of the B operands'),
// the insertion, the cross-lane fold and the K-th threshold.
template <int K>
struct HmTopK {
    uint32_t d[K];   // ascending bit patterns of the (positive) ranking values
    uint32_t i[K];
};
// Branch-free insertion into the sorted list (static register indices only). Rows arrive in ascending order inside a lane: strict '<' puts a
// value behind its equals, so the lower row of a tie stays in front and a value equal to the K-th never enters.
template <int K>
__device__ __forceinline__ void hm_insert_k(HmTopK<K>& b, uint32_t d, uint32_t idx) {
#pragma unroll
    for (int j = K - 1; j > 0; j--) {   // (descending: slot j - 1 still holds its old entry when slot j takes it over)
        const bool shift = d < b.d[j - 1], here = d < b.d[j];
        b.i[j] = shift ? b.i[j - 1] : (here ? idx : b.i[j]);
        b.d[j] = shift ? b.d[j - 1] : (here ? d : b.d[j]);
    }
    const bool first = d < b.d[0];
    b.i[0] = first ? idx : b.i[0];
    b.d[0] = first ? d : b.d[0];
}
__device__ __forceinline__ uint64_t hm_shfl_xor_u64(uint64_t v, int off) {
    return ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, off);
}

// Column blocks per wave for a list length: at four waves per SIMD (128 registers) the top-2 kernel's three blocks leave no room for 3 x 2 x 8
// list registers; two blocks (16 B-operand registers, 4 accumulators and one list fewer) do: 120 VGPRs for K = 8, 104 for K = 4, no scratch.
// (K = 4 with three blocks: 128 VGPRs and two of them spilled - 12 bytes of scratch per lane.)
#ifndef APDS_HM_NC_K4
#define APDS_HM_NC_K4 2
#endif
#ifndef APDS_HM_NC_K8
#define APDS_HM_NC_K8 2
#endif
template <int K>
struct HmShape {
    static constexpr int NC = K <= 4 ? APDS_HM_NC_K4 : APDS_HM_NC_K8;
    static constexpr int Q = HM_WAVES * 16 * NC;   // queries per workgroup
};

// out[split][nq][K]: keys (distance << 32 | row + index_base) in ascending order, EMPTY behind the rows the split holds.
template <int K, int NC, int PRIO, bool THR>
__global__ __launch_bounds__(64 * HM_WAVES) __attribute__((amdgpu_waves_per_eu(APDS_HM_WPE, APDS_HM_WPE))) void hamming_mfma_topk_kernel(
    const uint4* __restrict__ train_fp4, const float* __restrict__ tpc, int n_train, const uint4* __restrict__ query_fp4, const float* __restrict__ qpc, int nq,
    int tiles_per_split, int q_tiles, int splits, uint32_t index_base, const uint32_t* __restrict__ thr, uint64_t* __restrict__ out) {
    const HmItem w = hm_work_item<NC>(n_train, tiles_per_split, q_tiles, splits);
    const int split = w.split, q0 = w.q0, tile_begin = w.tile_begin, tile_end = w.tile_end, col = w.col, kq = w.kq;
    uint4 B[NC][4];
    float qq[NC];
    hm_load_queries<NC>(query_fp4, qpc, nq, q0, col, kq, B, qq);
    // The list starts as K copies of hm_start_value. A padding row's value is +inf and never passes the strict test, whatever the list holds.
    HmTopK<K> best[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) {
        uint32_t start = hm_start_value<THR>(thr, min(q0 + 16 * c + col, nq - 1));
        hm_settle(start), hm_settle(qq[c]);
#pragma unroll
        for (int j = 0; j < K; j++) best[c].d[j] = start, best[c].i[j] = 0xFFFFFFFFu;
    }

    if (tile_begin < tile_end) {
        // The common case is the top-2 kernel's: one minimum and one compare per accumulator, against the K-th value. Behind the wave-uniform
        // branch every one of the four rows is tested again (against the K-th value as the rows before it left it): an insertion is about
        // 6 K instructions, and most blocks with a hit have it in one row.
        hm_scan_tiles<NC, PRIO>(train_fp4, tpc, tile_begin, tile_end, B, index_base, [&](const hm_f32x4 (&a)[NC], uint32_t row0) {
            bool hit[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const uint32_t mn = min(min(__float_as_uint(a[c][0]), __float_as_uint(a[c][1])), min(__float_as_uint(a[c][2]), __float_as_uint(a[c][3])));
                hit[c] = mn < best[c].d[K - 1];
            }
#pragma unroll
            for (int c = 0; c < NC; c++)
                if (__any(hit[c])) {
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const uint32_t v = __float_as_uint(a[c][j]);
                        if (__any(v < best[c].d[K - 1])) hm_insert_k<K>(best[c], v, row0 + j);
                    }
                }
        });
    }
    // A query column lives in four lanes (kq = 0..3) whose rows interleave: the lists are folded as (value, row) pairs - one 64-bit key each,
    // a list entry without a row (0xFFFFFFFF) behind every row of its value. Two sorted K-lists -> the K smallest, sorted: min(mine[j],
    // theirs[K - 1 - j]) holds them as a bitonic sequence, log2 K rounds of compare-exchange sort it. Both partners compute the same list.
#pragma unroll
    for (int c = 0; c < NC; c++) {
        uint64_t key[K];
#pragma unroll
        for (int j = 0; j < K; j++) key[j] = ((uint64_t)best[c].d[j] << 32) | best[c].i[j];
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) {
            uint64_t other[K];
#pragma unroll
            for (int j = 0; j < K; j++) other[j] = hm_shfl_xor_u64(key[j], off);
#pragma unroll
            for (int j = 0; j < K; j++) key[j] = min(key[j], other[K - 1 - j]);
#pragma unroll
            for (int step = K / 2; step > 0; step >>= 1)
#pragma unroll
                for (int j = 0; j < K; j++)
                    if ((j & step) == 0) {
                        const uint64_t lo = min(key[j], key[j + step]), hi = max(key[j], key[j + step]);
                        key[j] = lo;
                        key[j + step] = hi;
                    }
        }
        const int qi = q0 + 16 * c + col;
        if (kq == 0 && qi < nq) {
            uint64_t* o = out + ((size_t)split * nq + qi) * K;
#pragma unroll
            for (int j = 0; j < K; j++) {
                const uint32_t d = key_rank(key[j]), i = key_index(key[j]);
                o[j] = i == 0xFFFFFFFFu ? EMPTY_KEY : make_key(hm_distance(qq[c], d), i);
            }
        }
    }
}

static int hm_list_len(int k) { return k <= 2 ? 2 : (k <= 4 ? 4 : 8); }   // the list the kernels keep for a k
static int hm_queries_per_block(int K) { return K <= 2 ? HM_Q : (K <= 4 ? HmShape<4>::Q : HmShape<8>::Q); }

HmPlan hm_plan(int nq, long long nt, int K) {
    HmPlan p;
    p.q_tiles = ceil_div(nq, hm_queries_per_block(K));
    const int t_tiles = (int)ceil_div(nt, (long long)HM_TM);
    constexpr int SLOTS = 256 * (16 / HM_WAVES);   // two 8-wave workgroups fit a CU (LDS, registers)
    constexpr int OVERHEAD = 4;      // a workgroup's prologue and epilogue (operand loads, pipeline fill, key output) in tile times
    // Splits of the train rows: they fill the slots when the query tiles alone do not, and they set the granularity of the last round of
    // workgroups (92 query tiles x 5 splits = 460 workgroups leave a tenth of the chip idle for the whole launch; x 11 = 1012 fill two
    // rounds to 99 %). The count that minimises rounds x (tiles per split + overhead); the split lists (16 bytes per query and split) stay
    // below 256 MB. Then (APDS_MATCH_MFMA_XCD, on): a multiple of eight splits, pinned to the XCDs, when the model puts one within 5 % of
    // that count - the workgroups of an XCD then share every train tile through their L2. On the headline shape 16 splits instead of 11:
    // 1.1 GB fetched per match instead of 2.65 GB (the expanded DB is 0.25 GB). Before the threshold launch existed that cost 5 % (every
    // workgroup pays its start from +inf again: 6.5 against 6.15 ms); with it 1.7 % alone on the GPU, and in the pipeline the step is
    // 3.4 % SHORTER (138.9 against 134.3 frames/s: the extraction beside it is memory-bound) - profiles/r04/mfma_xcd_ab.txt, ab_bench_env.txt.
    const int max_splits = (int)std::max<long long>(1, std::min<long long>(std::min(t_tiles, 128), (32ll << 20) / std::max(K, 2) / std::max(nq, 1)));   // (8 K bytes per query and split)
    long long best_cost = -1;
    p.splits = 1;
    for (int sp = 1; sp <= max_splits; sp++) {
        const long long rounds = ceil_div((long long)p.q_tiles * sp, (long long)SLOTS);
        const long long cost = rounds * (ceil_div(t_tiles, sp) + OVERHEAD);
        if (best_cost < 0 || cost < best_cost) best_cost = cost, p.splits = sp;
    }
    // a multiple of eight splits (pinned to the XCDs, see the kernel) when the model puts it within 5 % of the best count
    if (config().match_mfma_xcd && t_tiles >= 64) {
        long long best8 = -1;
        int sp8 = 0;
        for (int sp = 8; sp <= std::min(max_splits, 32); sp += 8) {
            const long long rounds = ceil_div((long long)p.q_tiles * sp, (long long)SLOTS);
            const long long cost = rounds * (ceil_div(t_tiles, sp) + OVERHEAD);
            if (best8 < 0 || cost < best8) best8 = cost, sp8 = sp;
        }
        if (sp8 && best8 * 100 <= best_cost * 105) {
            p.splits = sp8;
            p.tiles_per_split = ceil_div(t_tiles, p.splits);   // (the count stays a multiple of eight: trailing splits may be empty)
            return p;
        }
    }
    if (config().match_mfma_splits > 0) p.splits = std::min(t_tiles, config().match_mfma_splits);   // (experiments)
    p.tiles_per_split = ceil_div(t_tiles, p.splits);
    p.splits = ceil_div(t_tiles, p.tiles_per_split);
    return p;
}

void hm_expand_device(const void* rows64, long long n, bool query, void* out_fp4, float* pc, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(hm_expand_rows_kernel, dim3((unsigned)ceil_div(n * 16, 256)), dim3(256), 0, s, static_cast<const uint32_t*>(rows64), n, query ? 0xCu : 0x2u,
                       query ? 0 : HM_BIAS, static_cast<uint4*>(out_fp4), pc);
    if (!query && hm_padded_rows(n) > n)
        hipLaunchKernelGGL(hm_pad_rows_kernel, dim3(1), dim3(128), 0, s, static_cast<uint4*>(out_fp4), pc, n, hm_padded_rows(n));
}
long long hm_padded_rows(long long n) { return ceil_div(n, (long long)HM_TM) * HM_TM; }
// rows of the threshold launch: whole tiles, a sixteenth of the set, at most APDS_MATCH_MFMA_SAMPLE (16 384); none below 65 536 rows
long long hm_sample_rows(long long nt) {
    const long long cap = config().match_mfma_sample;   // APDS_MATCH_MFMA_SAMPLE (0: no threshold launch)
    return (cap > 0 && nt >= 65536) ? std::min<long long>(cap, nt / 16 / HM_TM * HM_TM) / HM_TM * HM_TM : 0;   // whole tiles (HM_TM need not be a power of two)
}

// The kernels ask for more dynamic LDS than the default limit: opt a set of them in once per device (idempotent, so a race is harmless).
template <class... Kernel>
static void hm_opt_in_lds(std::atomic<bool> (&opted_dev)[64], Kernel... kernel) {
    std::atomic<bool>& opted = opted_dev[ctx().device & 63];
    if (opted.load()) return;
    (HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)), ...);
    opted.store(true);
}

// The K = 4 / K = 8 launch of hm_scan_device (go: its launch of a kernel). PRIO: the wave priority around a block's MFMAs is off or 2 here
// (levels 1, 2, 3 measured alike on the top-2 kernel: one compiled level instead of three).
template <int K, class Go>
static void hm_scan_k_launch(Go&& go, bool thr) {
    constexpr int NC = HmShape<K>::NC;
    static std::atomic<bool> opted_dev[64];
    hm_opt_in_lds(opted_dev, &hamming_mfma_topk_kernel<K, NC, 0, false>, &hamming_mfma_topk_kernel<K, NC, 2, false>,
                  &hamming_mfma_topk_kernel<K, NC, 0, true>, &hamming_mfma_topk_kernel<K, NC, 2, true>);
    const bool prio = config().match_mfma_prio > 0;
    if (thr) prio ? go(&hamming_mfma_topk_kernel<K, NC, 2, true>) : go(&hamming_mfma_topk_kernel<K, NC, 0, true>);
    else prio ? go(&hamming_mfma_topk_kernel<K, NC, 2, false>) : go(&hamming_mfma_topk_kernel<K, NC, 0, false>);
}

// parts: [p.splits][nq][K] keys; p = hm_plan(nq, nt, K). K = 2: hamming_mfma_kernel; K = 4, 8: hamming_mfma_topk_kernel.
void hm_scan_device(const void* q_fp4, const float* qpc, int nq, const void* t_fp4, const float* tpc, long long nt, const HmPlan& p, uint32_t index_base,
                    uint64_t* parts, hipStream_t s, const uint32_t* thr, bool timed, int K) {
    APDS_REQUIRE(K <= 2 || K == 4 || K == 8, APDS_ERR_ASSERT, "the matrix-core matcher keeps lists of 2, 4 or 8");
    // (APDS_MATCH_MFMA_LDS_PAD: unused dynamic LDS on top, an experiment knob - e.g. 30000 leaves one workgroup per CU)
    const size_t lds = (size_t)2 * HM_TM * 256 + 2 * HM_TM * sizeof(float) + (size_t)std::max(0, config().match_mfma_lds_pad);
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)p.q_tiles * p.splits), dim3(64 * HM_WAVES), lds, s, static_cast<const uint4*>(t_fp4), tpc, (int)nt,
                           static_cast<const uint4*>(q_fp4), qpc, nq, p.tiles_per_split, p.q_tiles, p.splits, index_base, thr, parts);
    };
    // "hamming_topk": the name the pipeline's counters and bench.py know every main match launch by; for K > 2 a second name tells which
    // kernel it was
    std::unique_ptr<KernelTimer> timer, timer_k;
    if (timed) timer.reset(new KernelTimer("hamming_topk", s));
    if (timed && K > 2) timer_k.reset(new KernelTimer("hamming_topk_mfma_k", s));
    if (K == 4) return hm_scan_k_launch<4>(go, thr != nullptr);
    if (K == 8) return hm_scan_k_launch<8>(go, thr != nullptr);
    static std::atomic<bool> opted_dev[64];
    hm_opt_in_lds(opted_dev, &hamming_mfma_kernel<0, false>, &hamming_mfma_kernel<1, false>, &hamming_mfma_kernel<2, false>, &hamming_mfma_kernel<3, false>,
                  &hamming_mfma_kernel<0, true>, &hamming_mfma_kernel<1, true>, &hamming_mfma_kernel<2, true>, &hamming_mfma_kernel<3, true>);
    const int prio = std::max(0, std::min(3, config().match_mfma_prio));
    if (thr) {
        switch (prio) {
            case 0: go(&hamming_mfma_kernel<0, true>); break;
            case 1: go(&hamming_mfma_kernel<1, true>); break;
            case 2: go(&hamming_mfma_kernel<2, true>); break;
            default: go(&hamming_mfma_kernel<3, true>); break;
        }
    } else {
        switch (prio) {
            case 0: go(&hamming_mfma_kernel<0, false>); break;
            case 1: go(&hamming_mfma_kernel<1, false>); break;
            case 2: go(&hamming_mfma_kernel<2, false>); break;
            default: go(&hamming_mfma_kernel<3, false>); break;
        }
    }
}

// A train set expanded once (resident databases: the pipeline's, a shard's): rows + popcounts in memory of their own.
void* hm_train_create(const void* rows64, long long n, hipStream_t s) {
    APDS_REQUIRE(rows64 && n > 0 && n < (1ll << 31), APDS_ERR_ASSERT, "an expanded train set needs rows");
    HmTrain* t = new HmTrain();
    t->device = ctx().device;
    t->src = rows64;
    t->n = n;
    if (hipMalloc(&t->rows, (size_t)hm_padded_rows(n) * 256) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&t->pc), (size_t)hm_padded_rows(n) * 4) != hipSuccess) {
        (void)hipGetLastError();
        if (t->rows) (void)hipFree(t->rows);
        delete t;
        fail(APDS_ERR_NOMEM, "no device memory for the expanded train rows");
    }
    hm_expand_device(rows64, n, false, t->rows, t->pc, s);
    HIP_CHECK(hipStreamSynchronize(s));
    return t;
}
void hm_train_destroy(void* h) {
    HmTrain* t = static_cast<HmTrain*>(h);
    if (!t) return;
    DeviceGuard on(t->device);
    (void)hipDeviceSynchronize();
    if (t->rows) (void)hipFree(t->rows);
    if (t->pc) (void)hipFree(t->pc);
    delete t;
}

// Top-k (1 <= k <= 8) of nq 64-byte query rows against expanded train rows (t4 / tp: hm_expand_device's output, or an HmTrain's).
static void hm_topk_expanded(const void* q, int nq, const void* t4, const float* tp, long long nt, uint32_t index_base, int k, uint64_t* out, hipStream_t s) {
    ThreadCtx& c = ctx();
    void* q4 = c.alloc((size_t)nq * 256);
    float* qp = c.alloc_n<float>(nq);
    {
        KernelTimer timer("hamming_topk_sample", s);   // (the counters' name for what runs in front of the main match kernel)
        hm_expand_device(q, nq, true, q4, qp, s);
    }
    // Long train sets: a first launch over the leading rows (a sixteenth, at most 16 384: 141.5 frames/s; 32 768: 139.2; 65 536: 138.0; none:
    // 132.6 - profiles/r04/ab_bench_env.txt) gives every query a threshold, and the launch over
    // the rest starts from it - its workgroups then spend their first tiles like their last ones (a workgroup that starts from +inf runs
    // insertion code for every block of its first ~1500 rows), which is also what makes many short workgroups affordable.
    const long long sample = hm_sample_rows(nt);
    const int K = hm_list_len(k);   // the list the kernel keeps: 2, 4 or 8; the columns past k are dropped at the end
    uint64_t* topk = k == K ? out : c.alloc_n<uint64_t>((size_t)nq * K);
    // the lists the main launch's merge takes: one per split of the rest, and the sample's top-K behind them
    const HmPlan p = hm_plan(nq, nt - sample, K);
    const int lists = p.splits + (sample ? 1 : 0);
    uint64_t* parts = lists == 1 ? topk : c.alloc_n<uint64_t>((size_t)lists * nq * K);
    uint32_t* thr = nullptr;
    if (sample) {
        const HmPlan pa = hm_plan(nq, sample, K);
        uint64_t* parts_a = c.alloc_n<uint64_t>((size_t)pa.splits * nq * K);
        uint64_t* topk_a = parts + (size_t)p.splits * nq * K;
        thr = c.alloc_n<uint32_t>(nq);
        KernelTimer timer("hamming_topk_sample", s);
        hm_scan_device(q4, qp, nq, t4, tp, sample, pa, index_base, parts_a, s, nullptr, /*timed=*/false, K);
        if (pa.splits > 1) merge_topk_device(parts_a, pa.splits, nq, K, topk_a, s);
        else HIP_CHECK(hipMemcpyAsync(topk_a, parts_a, (size_t)nq * K * 8, hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(hm_thresholds_kernel, dim3(ceil_div(nq, 256)), dim3(256), 0, s, (const uint64_t*)topk_a, K, (const float*)qp, nq, thr);
    }
    hm_scan_device(q4, qp, nq, static_cast<const char*>(t4) + (size_t)sample * 256, tp + sample, nt - sample, p, index_base + (uint32_t)sample, parts, s, thr,
                   /*timed=*/true, K);
    if (lists > 1) merge_topk_device(parts, lists, nq, K, topk, s);
    if (k != K) take_first_columns_device(topk, nq, K, k, out, s);
    HIP_CHECK(hipGetLastError());
}

// Top-k (1 <= k <= 8) of nq queries over nt train rows, both 64-byte rows on the device. out: nq * k keys (distance << 32 | row + index_base).
void hamming_mfma_topk_device(const void* q, int nq, const void* t, long long nt, uint32_t index_base, int k, uint64_t* out, hipStream_t s) {
    APDS_REQUIRE(k >= 1 && k <= 8, APDS_ERR_ASSERT, "the matrix-core matcher serves 1 <= k <= 8");
    APDS_REQUIRE(nq > 0 && nt > 0 && nt < (1ll << 31), APDS_ERR_ASSERT, "the matrix-core matcher needs queries and train rows");
    ThreadCtx& c = ctx();
    void* t4 = c.alloc((size_t)hm_padded_rows(nt) * 256);
    float* tp = c.alloc_n<float>(hm_padded_rows(nt));
    {
        KernelTimer timer("hamming_topk_sample", s);
        hm_expand_device(t, nt, false, t4, tp, s);
    }
    hm_topk_expanded(q, nq, t4, tp, nt, index_base, k, out, s);
}

// The same against a train set expanded once (hm_train_create).
void hamming_mfma_topk_train_device(const void* q, int nq, const void* train, uint32_t index_base, int k, uint64_t* out, hipStream_t s) {
    const HmTrain* t = static_cast<const HmTrain*>(train);
    APDS_REQUIRE(t && k >= 1 && k <= 8 && nq > 0, APDS_ERR_ASSERT, "the matrix-core matcher needs an expanded train set, queries and 1 <= k <= 8");
    hm_topk_expanded(q, nq, t->rows, t->pc, t->n, index_base, k, out, s);
}

// ---- the roles-swapped scan of the cross-check (get_bruteforce_matches, lib.rs:116-126) against a train set expanded once ----
// Every TRAIN row looks for its nearest query: the searching side - the register columns of hamming_mfma_kernel - is the resident train
// set, the streamed side the frame's rows. The kernel never asks which side is which: a product is (tile nibble) x (column nibble), the
// accumulator is preset from the TILE rows' biased popcounts, and hm_distance adds the COLUMN row's plain popcount. So the resident
// expansion (nibble 1.0, made for the tile side) serves as the column operand as it is, the frame's rows are expanded per frame with the
// other nibble (-2.0: every product is still 0 or -2) and THEIR popcounts carry the bias:
//     acc = popcount(f) + 1024 - 2 popcount(f AND t),   distance = popcount(t) + acc - 1024 = hamming(f, t)
// - the same integers, the same exactness argument as the forward form (file header), no row of the train set expanded again. What the
// column side needs beside the operands is the train rows' popcounts WITHOUT the bias (hm_train_plain_popcounts_device: once per train
// set). Keys: (distance << 32 | frame row); equal distances keep the lower frame row, as the forward form keeps the lower train row.
__global__ void hm_plain_popcounts_kernel(const float* __restrict__ biased, long long n, float* __restrict__ plain) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) plain[i] = biased[i] - (float)HM_BIAS;   // (integers below 2^11: exact)
}

// out: n floats (n = the train set's rows) = popcount of every row, what hm_scan_device takes as qpc when the train set is the column side
void hm_train_plain_popcounts_device(const void* train, float* out, hipStream_t s) {
    const HmTrain* t = static_cast<const HmTrain*>(train);
    APDS_REQUIRE(t && out, APDS_ERR_ASSERT, "an expanded train set and an output are required");
    hipLaunchKernelGGL(hm_plain_popcounts_kernel, dim3((unsigned)ceil_div(t->n, 256ll)), dim3(256), 0, s, (const float*)t->pc, (long long)t->n, out);
    HIP_CHECK(hipGetLastError());
}

// train_best[r] = (distance << 32 | nearest of the n rows) for every row r of the expanded train set; n >= 1 rows of 64 bytes on the device.
// Scratch (the n rows' operands, the split lists) is the calling thread's workspace.
void hamming_mfma_swapped_top1_device(const void* rows64, int n, const void* train, const float* train_plain_pc, uint64_t* train_best, hipStream_t s) {
    const HmTrain* t = static_cast<const HmTrain*>(train);
    APDS_REQUIRE(t && train_plain_pc && rows64 && train_best && n > 0, APDS_ERR_ASSERT, "the swapped scan needs an expanded train set, its plain popcounts and rows");
    ThreadCtx& c = ctx();
    const long long n_pad = hm_padded_rows(n);
    uint4* f4 = static_cast<uint4*>(c.alloc((size_t)n_pad * 256));
    float* fp = c.alloc_n<float>((size_t)n_pad);
    {
        KernelTimer timer("hamming_topk_sample", s);   // (the counters' name for what runs in front of the main match kernel)
        hipLaunchKernelGGL(hm_expand_rows_kernel, dim3((unsigned)ceil_div((long long)n * 16, 256ll)), dim3(256), 0, s, static_cast<const uint32_t*>(rows64), (long long)n, 0xCu,
                           HM_BIAS, f4, fp);
        if (n_pad > n) hipLaunchKernelGGL(hm_pad_rows_kernel, dim3(1), dim3(128), 0, s, f4, fp, (long long)n, n_pad);
    }
    const int nc = (int)t->n;   // (hm_train_create: below 2^31)
    const HmPlan p = hm_plan(nc, n, 2);
    uint64_t* top2 = c.alloc_n<uint64_t>((size_t)nc * 2);
    uint64_t* parts = p.splits == 1 ? top2 : c.alloc_n<uint64_t>((size_t)p.splits * nc * 2);
    hm_scan_device(t->rows, train_plain_pc, nc, f4, fp, n, p, 0, parts, s, nullptr, /*timed=*/true, 2);
    if (p.splits > 1) merge_topk_device(parts, p.splits, nc, 2, top2, s);
    take_first_columns_device(top2, nc, 2, 1, train_best, s);
    HIP_CHECK(hipGetLastError());
}

}  // namespace apds
