// csrc/keypoint_delete.hip — deletes from the keypoint table (keypointdb.rs:92-97, delete_keypoint): stable ordered compaction of the
// whole table under a delete predicate.
// Victim flags and per-block victim counts -> block_offsets_device -> the survivors move down in row order, chunk by chunk: a chunk's
// survivors are gathered into the table's staging buffer by one launch and copied to their destination by the next one (DESIGN §7c-4
// has the argument why no launch reads what another workgroup of the same launch writes).
#include "keypoint_table.h"

namespace apds {

// a thread per entry of the caller's list: the row of that id, if any, is flagged (a duplicate flags it again, an unknown id nothing)
__global__ void delete_mark_ids_kernel(const int* __restrict__ ids, long long n, const int* __restrict__ list, int m, uint8_t* __restrict__ flags) {
    APDS_RAISE_WAVE_PRIORITY();
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const long long r = find_id_row(ids, n, list[j]);
    if (r >= 0) flags[r] = 1;
}

static constexpr int DELETE_MODE_FLAGGED = 3;   // SelectArgs.mode of a delete whose victim flags are already written (the id list)

// victims per block of TB rows and the first victim row of the table (*first_row starts at INT_MAX); modes 0..2 evaluate the select
// path's predicate and write the flags the gather reads
__global__ __launch_bounds__(TB) void delete_count_kernel(TableColumns c, int n, SelectArgs a, uint8_t* __restrict__ flags, int* __restrict__ block_counts,
                                                          int* __restrict__ first_row) {
    APDS_RAISE_WAVE_PRIORITY();
    const long long i = (long long)blockIdx.x * TB + threadIdx.x;
    int f = 0;
    if (i < n) {
        if (a.mode == DELETE_MODE_FLAGGED) f = flags[i] != 0;
        else flags[i] = f = row_selected(c, i, a);
    }
    int total;
    const int pos = block_rank(f, &total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
    if (f && pos == 0) atomicMin(first_row, (int)i);
}

// rows one gather / scatter pair moves, a multiple of TB: 2^20 of a byte table (128-byte staging rows), 2^18 of a float table (320-byte
// staging rows), so the staging buffer of either stays near 128 MB
static constexpr int DELETE_CHUNK_ROWS = 1 << 20, DELETE_CHUNK_ROWS_FLOAT = 1 << 18;
static constexpr int MOVE_COLUMNS = 10;             // x, y, size, angle, response, octave, class_id, image_id, lod, id: one dword each
// dwords of a staging row: the columns + the descriptor row (16 or 64 dwords) + the world point
static constexpr int stage_row_dwords(int desc_dwords) { return MOVE_COLUMNS + desc_dwords + 6; }

struct MoveColumns {
    uint32_t* col[MOVE_COLUMNS];
    uint32_t* desc;   // 1 << desc_shift dwords per row
    uint32_t* xyz;    // 6 dwords per row, or null (no valid world points: nothing to move)
    int desc_shift;   // 4 or 6: log2 of the dwords of a descriptor row
};
// the staging buffer: MOVE_COLUMNS planes of `rows` dwords, then rows x desc_dwords descriptor dwords, then rows x 6 world point dwords
struct StageColumns {
    uint32_t* base;
    int rows, desc_dwords;
    __device__ __forceinline__ uint32_t* col(int k) const { return base + (size_t)k * rows; }
    __device__ __forceinline__ uint32_t* desc() const { return base + (size_t)MOVE_COLUMNS * rows; }
    __device__ __forceinline__ uint32_t* xyz() const { return base + (size_t)(MOVE_COLUMNS + desc_dwords) * rows; }
};

// Chunk = blocks [block0, block0 + gridDim.x) of TB rows. Its survivors go to consecutive staging slots in row order: slot = survivors of
// the chunk before the row. Rows below first_row (all survivors, the first slots of the first chunk) stay where they are: not read here,
// their slots not written, and skipped by the scatter. Reads the table, writes the staging buffer only.
__global__ __launch_bounds__(TB) void delete_gather_kernel(MoveColumns m, int n, const uint8_t* __restrict__ flags, const int* __restrict__ victim_offsets,
                                                           int block0, int first_row, StageColumns st) {
    APDS_RAISE_WAVE_PRIORITY();
    __shared__ unsigned short src_of[TB];   // the thread (row of the block) of the block's pos-th survivor
    const int b = block0 + blockIdx.x;
    const long long r0 = (long long)b * TB, r = r0 + threadIdx.x;
    const int f = r < n && !flags[r];
    int total;
    const int pos = block_rank(f, &total);
    const size_t before = (size_t)blockIdx.x * TB - (size_t)(victim_offsets[b] - victim_offsets[block0]);
    const int skip = (int)std::min<long long>(std::max<long long>(first_row - r0, 0), TB);
    if (f) {
        src_of[pos] = (unsigned short)threadIdx.x;
        if (pos >= skip) {
#pragma unroll
            for (int k = 0; k < MOVE_COLUMNS; k++) st.col(k)[before + pos] = m.col[k][r];
        }
    }
    __syncthreads();
    const int W = 1 << m.desc_shift;
    uint32_t* sd = st.desc() + before * W;
    for (int e = skip * W + threadIdx.x; e < total * W; e += TB) sd[e] = m.desc[(size_t)(r0 + src_of[e >> m.desc_shift]) * W + (e & (W - 1))];
    if (m.xyz) {
        uint32_t* sx = st.xyz() + before * 6;
        for (int e = skip * 6 + threadIdx.x; e < total * 6; e += TB) {
            const int j = e / 6;
            sx[e] = m.xyz[(size_t)(r0 + src_of[j]) * 6 + (e - j * 6)];
        }
    }
}

// The staged survivors of the chunk (blocks [block0, block_end), region_rows = their rows, a multiple of TB) to rows dst0, dst0 + 1, ..:
// dst0 = the chunk's first row minus the victims before it. Every copy is contiguous; a block of 256 threads serves one segment of the
// flat index space [descriptor dwords | MOVE_COLUMNS column planes | world point dwords]. Reads the staging buffer, writes the table only.
__global__ __launch_bounds__(256) void delete_scatter_kernel(StageColumns st, const int* __restrict__ victim_offsets, int block0, int block_end, int n,
                                                             int region_rows, int first_row, MoveColumns m) {
    APDS_RAISE_WAVE_PRIORITY();
    const long long start = (long long)block0 * TB, end = std::min<long long>((long long)block_end * TB, n);
    const int victims_before = victim_offsets[block0];
    const long long survivors = (end - start) - (victim_offsets[block_end] - victims_before);
    const long long dst0 = start - victims_before;
    const long long skip = std::max<long long>(first_row - dst0, 0);   // slots of rows that did not move (never staged)
    const long long R = region_rows, g0 = (long long)blockIdx.x * 256, W = 1 << m.desc_shift;
    if (g0 < R * W) {
        const long long e = g0 + threadIdx.x;
        if (e >= skip * W && e < survivors * W) m.desc[dst0 * W + e] = st.desc()[e];
    } else if (g0 < R * (W + MOVE_COLUMNS)) {
        const int k = (int)((g0 - R * W) / R);
        const long long j = g0 - R * (W + k) + threadIdx.x;
        if (j >= skip && j < survivors) m.col[k][dst0 + j] = st.col(k)[j];
    } else {
        const long long e = g0 - R * (W + MOVE_COLUMNS) + threadIdx.x;
        if (e >= skip * 6 && e < survivors * 6) m.xyz[dst0 * 6 + e] = st.xyz()[e];
    }
}

}  // namespace apds

using namespace apds;

namespace {
// The rows `a` selects (or, with DELETE_MODE_FLAGGED, the rows already flagged) leave the table; the survivors close up in row order on the
// calling thread's stream. One host synchronisation for the count and the first victim row, one at the end. Returns the rows deleted.
int64_t table_delete_rows(KeypointTable* t, ThreadCtx& c, const SelectArgs& a, uint8_t* flags) {
    hipStream_t s = c.stream;
    const int n = (int)t->n, nb = ceil_div(n, TB);
    int* counts = c.alloc_n<int>((size_t)nb + 2);   // victims per block -> their exclusive offsets; [nb] the sum, [nb + 1] the first victim row
    static const int no_row = 0x7fffffff;
    HIP_CHECK(hipMemcpyAsync(counts + nb + 1, &no_row, sizeof(int), hipMemcpyHostToDevice, s));
    const TableColumns cols = columns_of(t);
    hipLaunchKernelGGL(delete_count_kernel, dim3(nb), dim3(TB), 0, s, cols, n, a, flags, counts, counts + nb + 1);
    block_offsets_device(counts, nb, s);
    HIP_CHECK(hipGetLastError());
    int h[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(h, counts + nb, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const int m = h[0], first_row = h[1];
    if (!m) return 0;
    const bool xyz_valid = t->xyz && t->xyz_rows == t->n;
    if ((int64_t)first_row + m < n) {   // a survivor sits behind a victim: rows move (a deleted tail moves nothing)
        if (!t->stage) {
            t->stage_rows = (int)std::min<int64_t>(t->is_float() ? DELETE_CHUNK_ROWS_FLOAT : DELETE_CHUNK_ROWS, (int64_t)ceil_div(t->capacity, TB) * TB);
            dev_alloc(t->stage, (size_t)t->stage_rows * stage_row_dwords(t->row_dwords));
        }
        MoveColumns mv;
        uint32_t* const planes[MOVE_COLUMNS] = {reinterpret_cast<uint32_t*>(t->x), reinterpret_cast<uint32_t*>(t->y), reinterpret_cast<uint32_t*>(t->size),
                                               reinterpret_cast<uint32_t*>(t->angle), reinterpret_cast<uint32_t*>(t->response),
                                               reinterpret_cast<uint32_t*>(t->octave), reinterpret_cast<uint32_t*>(t->class_id),
                                               reinterpret_cast<uint32_t*>(t->image_id), reinterpret_cast<uint32_t*>(t->lod), reinterpret_cast<uint32_t*>(t->id)};
        for (int k = 0; k < MOVE_COLUMNS; k++) mv.col[k] = planes[k];
        mv.desc = reinterpret_cast<uint32_t*>(t->desc64);
        mv.xyz = xyz_valid ? reinterpret_cast<uint32_t*>(t->xyz) : nullptr;
        mv.desc_shift = cols.row_shift;
        const StageColumns st{t->stage, t->stage_rows, t->row_dwords};
        const int chunk_blocks = t->stage_rows / TB, segments = stage_row_dwords(t->row_dwords) - (xyz_valid ? 0 : 6);
        for (int b0 = first_row / TB; b0 < nb; b0 += chunk_blocks) {
            const int b1 = std::min(b0 + chunk_blocks, nb), region_rows = (b1 - b0) * TB;
            hipLaunchKernelGGL(delete_gather_kernel, dim3(b1 - b0), dim3(TB), 0, s, mv, n, (const uint8_t*)flags, (const int*)counts, b0, first_row, st);
            hipLaunchKernelGGL(delete_scatter_kernel, dim3((unsigned int)((int64_t)region_rows * segments / 256)), dim3(256), 0, s, st, (const int*)counts, b0,
                               b1, n, region_rows, first_row, mv);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
    }
    t->n -= m;
    t->view_n = 0;                                                     // the current view's row ids name rows that have moved
    t->all_kps_rows = std::min<int64_t>(t->all_kps_rows, first_row);   // apds_db_table gathers the moved rows again
    t->xyz_rows = xyz_valid ? t->n : -1;                               // the world points moved with their rows
    return m;
}
}  // namespace

extern "C" {

int apds_db_delete_where(void* db, int mode, int value, float x_start, float y_start, float x_end, float y_end, int64_t* n_deleted) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t && mode >= 0 && mode <= 2, APDS_ERR_BAD_ARG, "bad argument");
        if (n_deleted) *n_deleted = 0;
        if (!t->n) return;
        ThreadCtx& c = ctx();
        require_table_device(t);
        c.ws_reset();
        const int64_t m = table_delete_rows(t, c, select_args(mode, value, x_start, y_start, x_end, y_end), c.alloc_n<uint8_t>((size_t)t->n));
        if (n_deleted) *n_deleted = m;
    });
}

int apds_db_delete_ids(void* db, const int32_t* ids, int n, int64_t* n_deleted) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t && n >= 0 && (ids || !n), APDS_ERR_BAD_ARG, "bad argument");
        if (n_deleted) *n_deleted = 0;
        if (!t->n || !n) return;
        ThreadCtx& c = ctx();
        require_table_device(t);
        c.ws_reset();
        hipStream_t s = c.stream;
        uint8_t* flags = c.alloc_n<uint8_t>((size_t)t->n);
        int* list = c.alloc_n<int>(n);
        HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)t->n, s));
        HIP_CHECK(hipMemcpyAsync(list, ids, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(delete_mark_ids_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, (const int*)t->id, (long long)t->n, (const int*)list, n, flags);
        const int64_t m = table_delete_rows(t, c, SelectArgs{DELETE_MODE_FLAGGED, 0, 0, 0, 0, 0}, flags);
        if (n_deleted) *n_deleted = m;
    });
}

}  // extern "C"
