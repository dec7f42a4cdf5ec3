// csrc/keypoint_table.h — what the three sources of the GPU-resident keypoint table share: the table itself, its columns as a kernel
// argument, the select / delete predicate, the rank of a row inside its block, the sort key, and the few host helpers every entry uses.
//   keypoint_table.hip  : create / destroy, the inserts, world points, the whole-table arguments of the pipeline, reads by id
//   keypoint_select.hip : the selection engine and its two fronts (apds_db_select, the view objects), the reads of the current view
//   keypoint_delete.hip : deletes (ordered compaction of the whole table)
#pragma once
#include <algorithm>
#include <cmath>

#include "kernels.h"

namespace apds {

struct KeypointTable {
    int device = 0;
    int64_t capacity = 0, n = 0;
    float *x = nullptr, *y = nullptr, *size = nullptr, *angle = nullptr, *response = nullptr;
    int *octave = nullptr, *class_id = nullptr, *image_id = nullptr, *lod = nullptr;
    // the descriptor column: rows of row_dwords dwords, 16 (M-LDB, 64 bytes) or 64 (M-SURF, 64 x f32 = 256 bytes). The kind is fixed at
    // create (apds_db_create / apds_db_create_float); every kernel that touches a descriptor row receives the width with the columns.
    int row_dwords = 16;
    uint8_t* desc64 = nullptr;
    // the reference's SERIAL column: the id of every row, and the next id to give. Ids are never reused, so they ascend with the row.
    int* id = nullptr;
    int64_t next_id = 1;
    // last selection of apds_db_select (device): the table's current view, allocated with the table
    int64_t view_n = 0, view_cap = 0;
    int* view_rows = nullptr;
    apds_keypoint* view_kps = nullptr;
    int* view_image_id = nullptr;
    uint8_t* view_desc64 = nullptr;
    // the whole table in the pipeline's layout (apds_db_table): 28-byte keypoints by row, gathered up to row all_kps_rows; the world point
    // of every row (apds_db_world_coordinates), valid for the first xyz_rows rows (-1: never computed). Both allocated on first use.
    apds_keypoint* all_kps = nullptr;
    int64_t all_kps_rows = 0;
    double* xyz = nullptr;
    int64_t xyz_rows = -1;
    // staging buffer of a delete's compaction (one chunk of rows, every moved column), allocated on the first delete that moves a row
    uint32_t* stage = nullptr;
    int stage_rows = 0;

    bool is_float() const { return row_dwords == 64; }
    size_t row_bytes() const { return (size_t)row_dwords * 4; }
};

struct TableColumns {
    float *x, *y, *size, *angle, *response;
    int *octave, *class_id, *image_id, *lod;
    uint32_t* desc64;
    int* id;
    int row_shift;   // log2 of the dwords of a descriptor row: 4 (16 dwords) or 6 (64); a kernel gives a row that many lanes, one dword each
    __host__ __device__ __forceinline__ int row_dwords() const { return 1 << row_shift; }
};

inline TableColumns columns_of(KeypointTable* t) {
    return TableColumns{t->x, t->y, t->size, t->angle, t->response, t->octave, t->class_id, t->image_id, t->lod, reinterpret_cast<uint32_t*>(t->desc64), t->id,
                        t->is_float() ? 6 : 4};
}

// the typed entries: a byte-typed call serves byte tables only, a float-typed call float tables only
inline void require_table_kind(const KeypointTable* t, bool want_float) {
    APDS_REQUIRE(t->is_float() == want_float, APDS_ERR_BAD_ARG,
                 want_float ? "this call takes a float table (apds_db_create_float)" : "this call takes a byte table (apds_db_create); a float table has a _float twin");
}

template <class T>
void dev_alloc(T*& p, size_t n) {
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(T)));
}

// every entry that launches on the calling thread's device with the table's pointers
inline void require_table_device(const KeypointTable* t) {
    APDS_REQUIRE(t->device == ctx().device, APDS_ERR_BAD_ARG, "the table lives on another device than the calling thread's");
}

// keypointdb.rs:38-90. mode 0: image_id == value; 1: level_of_detail == value; 2: level_of_detail == value and
// floor(x_start) <= x <= ceil(x_end), floor(y_start) <= y <= ceil(y_end)
struct SelectArgs {
    int mode;   // 0 image id, 1 level of detail, 2 level of detail + bounding box (a delete adds one of its own)
    int value;
    float x0, y0, x1, y1;   // already floor()/ceil()ed
};

inline SelectArgs select_args(int mode, int value, float x_start, float y_start, float x_end, float y_end) {
    return SelectArgs{mode, value, floorf(x_start), floorf(y_start), ceilf(x_end), ceilf(y_end)};
}

__device__ __forceinline__ bool row_selected(const TableColumns& c, long long i, const SelectArgs& a) {
    if (a.mode == 0) return c.image_id[i] == a.value;
    if (c.lod[i] != a.value) return false;
    if (a.mode == 1) return true;
    const float x = c.x[i], y = c.y[i];
    return x >= a.x0 && x <= a.x1 && y >= a.y0 && y <= a.y1;
}

static constexpr int TB = 1024;   // rows (or keys) per workgroup of every kernel that ranks them

// Position of a flagged thread among the flagged threads of its block (TB threads), and the block's count. The __shared__ array belongs
// to the kernel this is inlined into: a kernel calls it ONCE (a second call would reuse the array with no barrier in between).
__device__ __forceinline__ int block_rank(int f, int* block_total) {
    __shared__ int wsum[TB / 64];
    const unsigned long long b = __ballot(f);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wsum[wv] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < TB / 64; k++) {
        if (k < wv) before += wsum[k];
        all += wsum[k];
    }
    *block_total = all;
    return before + __popcll(b & ((1ull << lane) - 1ull));
}

// counts[0 .. nblocks) -> exclusive offsets in place, the sum to counts[nblocks]: one workgroup on s (keypoint_select.hip)
void block_offsets_device(int* counts, int nblocks, hipStream_t s);

// the 28-byte keypoint of table row r
__device__ __forceinline__ apds_keypoint load_keypoint(const TableColumns& c, long long r) {
    apds_keypoint k;
    k.x = c.x[r]; k.y = c.y[r]; k.size = c.size[r]; k.angle = c.angle[r]; k.response = c.response[r];
    k.octave = c.octave[r]; k.class_id = c.class_id[r];
    return k;
}

// ascending u64 key order == response descending, then row ascending, for every finite response and both infinities: the usual monotone
// map of float bits (all bits flipped under a set sign, the sign bit set otherwise) ascends with the value, its complement descends.
// -0.0 is made +0.0 first, so the two tie and fall to row order. A positive response gives ~bits with bit 31 cleared: the order among
// positive responses is the one ~bits alone gave. The row is below 2^31, so the all-ones padding key stays strictly above every real key.
__device__ __forceinline__ uint64_t order_key(float response, uint32_t row) {
    uint32_t b = __float_as_uint(response);
    if (b == 0x80000000u) b = 0;
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)(~b) << 32) | row;
}

// the row that holds `id`, or -1: ids ascend strictly with the row
__device__ __forceinline__ long long find_id_row(const int* __restrict__ ids, long long n, int id) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (ids[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && ids[lo] == id) ? lo : -1;
}

}  // namespace apds
