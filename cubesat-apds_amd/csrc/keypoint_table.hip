// csrc/keypoint_table.hip — GPU-resident keypoint table: what fills the descriptor database the matcher scans
// (SURVEY §8f-1). Mirrors the reference's `keypoint` table and its access paths, without Postgres:
//   insert  : preprocessor/src/main.rs:296-324 (to_db_type + level-of-detail rescale of x,y, one INSERT per tile)
//   read    : feature_database/src/keypointdb.rs:38-90 (by image id / by level of detail / by bounding box at a level of
//             detail), each `ORDER BY response DESC LIMIT 262143` (OPENCV_KEYPOINT_LIMIT, keypointdb.rs:12)
// Columns are stored SoA (coalesced predicate scans); descriptors as 64-byte rows, i.e. already in the layout the
// Hamming kernel streams, so a selection is directly usable as a train set and `train_idx` = position in the selection
// (the index the reference would get from the returned Vec).
// Selection = predicate flags -> ordered compaction of u64 keys (~response_bits << 32 | row) -> radix select of the
// LIMIT-th key when more rows qualify -> bitonic sort of the survivors -> row gather. Ties in response are ordered by
// insertion order (row id), which SQL leaves unspecified.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "kernels.h"
#include "topk_keys.h"

namespace apds {

struct KeypointTable {
    int device = 0;
    int64_t capacity = 0, n = 0;
    float *x = nullptr, *y = nullptr, *size = nullptr, *angle = nullptr, *response = nullptr;
    int *octave = nullptr, *class_id = nullptr, *image_id = nullptr, *lod = nullptr;
    uint8_t* desc64 = nullptr;
    // the reference's SERIAL column: the id of every row, and the next id to give. Ids are never reused, so they ascend with the row.
    int* id = nullptr;
    int64_t next_id = 1;
    // last selection (device)
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
};

struct TableColumns {
    float *x, *y, *size, *angle, *response;
    int *octave, *class_id, *image_id, *lod;
    uint32_t* desc64;
    int* id;
};

// The keypoint columns of table row r from one extracted keypoint: the ONE copy of the coordinate lift, whichever side the row comes from.
// main.rs:299-300: x * 2^lod + (column * tile_w * 2^lod) as f32 (scale = 2^lod; xoff, yoff: the u64 products rounded once to f32)
__device__ __forceinline__ void store_keypoint_columns(const TableColumns& c, long long r, const apds_keypoint& k, float scale, float xoff, float yoff,
                                                       int image_id, int lod, int id) {
    c.x[r] = k.x * scale + xoff;
    c.y[r] = k.y * scale + yoff;
    c.size[r] = k.size;
    c.angle[r] = k.angle;
    c.response[r] = k.response;
    c.octave[r] = k.octave;
    c.class_id[r] = k.class_id;
    c.image_id[r] = image_id;
    c.lod[r] = lod;
    c.id[r] = id;
}

__global__ void table_insert_kernel(const apds_keypoint* __restrict__ kps, const uint8_t* __restrict__ desc61, int n, int image_id, int lod,
                                    float scale, float xoff, float yoff, long long base, int first_id, TableColumns c) {
    APDS_RAISE_WAVE_PRIORITY();
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n * 16) return;
    const int i = (int)(t >> 4), w = (int)(t & 15);
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++)
        if (w * 4 + b < 61) v |= (uint32_t)desc61[(size_t)i * 61 + w * 4 + b] << (8 * b);
    c.desc64[(base + i) * 16 + w] = v;
    if (w == 0) store_keypoint_columns(c, base + i, kps[i], scale, xoff, yoff, image_id, lod, first_id + i);
}

// The same rows from the device buffers an extraction has written (28-byte keypoints, 64-byte descriptor rows; tile i at i * capacity
// rows), every tile of a batch in one launch: 16 lanes per table row, one dword each. tile_offsets[i] = rows of the tiles < i
// (tile_offsets[n_tiles] = all rows), copied to LDS; a row group finds its tile by binary search (empty tiles repeat an offset: the last
// tile whose offset is <= the row is the one that holds it). tile_xy_off[i] = that tile's (xoff, yoff). Bytes 61-63 of a source row are
// not trusted: word 15 keeps byte 60 alone.
__global__ __launch_bounds__(256) void table_insert_dev_kernel(const apds_keypoint* __restrict__ kps, const uint32_t* __restrict__ desc64_src, int n_tiles,
                                                               int capacity, const int* __restrict__ tile_offsets, const float2* __restrict__ tile_xy_off,
                                                               int first_image_id, int lod, float scale, long long base, int first_id, TableColumns c) {
    APDS_RAISE_WAVE_PRIORITY();
    extern __shared__ int offs[];   // n_tiles + 1
    for (int i = threadIdx.x; i <= n_tiles; i += blockDim.x) offs[i] = tile_offsets[i];
    __syncthreads();
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)offs[n_tiles] * 16) return;
    const int r = (int)(t >> 4), w = (int)(t & 15);
    int lo = 0, hi = n_tiles - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offs[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    const long long src = (long long)lo * capacity + (r - offs[lo]);
    uint32_t v = desc64_src[src * 16 + w];
    if (w == 15) v &= 0xFFu;
    c.desc64[(base + r) * 16 + w] = v;
    if (w == 0) {
        const float2 o = tile_xy_off[lo];
        store_keypoint_columns(c, base + r, kps[src], scale, o.x, o.y, first_image_id + lo, lod, first_id + r);
    }
}

// rows [from, from + n) of the columns as 28-byte keypoints (what the pipeline takes for its train rows)
__global__ void table_keypoints_kernel(TableColumns c, long long from, int n, apds_keypoint* __restrict__ out) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long r = from + i;
    apds_keypoint k;
    k.x = c.x[r]; k.y = c.y[r]; k.size = c.size[r]; k.angle = c.angle[r]; k.response = c.response[r];
    k.octave = c.octave[r]; k.class_id = c.class_id[r];
    out[r] = k;
}

struct SelectArgs {
    int mode;   // 0 image id, 1 level of detail, 2 level of detail + bounding box
    int value;
    float x0, y0, x1, y1;   // already floor()/ceil()ed
};

__global__ void table_flags_kernel(const int* __restrict__ img, const int* __restrict__ lod, const float* __restrict__ x, const float* __restrict__ y,
                                   long long n, SelectArgs a, uint8_t* __restrict__ flags) {
    APDS_RAISE_WAVE_PRIORITY();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool f;
    if (a.mode == 0) f = img[i] == a.value;
    else if (a.mode == 1) f = lod[i] == a.value;
    else f = lod[i] == a.value && x[i] >= a.x0 && x[i] <= a.x1 && y[i] >= a.y0 && y[i] <= a.y1;
    flags[i] = f;
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

static constexpr int TB = 1024;

__global__ __launch_bounds__(TB) void table_emit_keys_kernel(const uint8_t* __restrict__ flags, const float* __restrict__ response, int n,
                                                             const int* __restrict__ block_offsets, uint64_t* __restrict__ keys) {
    APDS_RAISE_WAVE_PRIORITY();
    __shared__ int wsum[TB / 64];
    const int i = blockIdx.x * TB + threadIdx.x;
    const int f = i < n ? (flags[i] != 0) : 0;
    const unsigned long long b = __ballot(f);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wsum[wv] = __popcll(b);
    __syncthreads();
    if (!f) return;
    int before = 0;
    for (int k = 0; k < wv; k++) before += wsum[k];
    keys[block_offsets[blockIdx.x] + before + __popcll(b & ((1ull << lane) - 1ull))] = order_key(response[i], (uint32_t)i);
}

// one radix-select pass: histogram of byte `shift/8` over keys that match `prefix` on the bits above it
__global__ void key_hist_kernel(const uint64_t* __restrict__ keys, int m, uint64_t prefix, uint64_t mask_hi, int shift, unsigned int* __restrict__ hist) {
    APDS_RAISE_WAVE_PRIORITY();
    __shared__ unsigned int s[256];
    if (threadIdx.x < 256) s[threadIdx.x] = 0;
    __syncthreads();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        const uint64_t k = keys[i];
        if ((k & mask_hi) == prefix) atomicAdd(&s[(k >> shift) & 0xFF], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 256 && s[threadIdx.x]) atomicAdd(&hist[threadIdx.x], s[threadIdx.x]);
}

__global__ void key_leq_flags_kernel(const uint64_t* __restrict__ keys, int m, uint64_t kth, uint8_t* __restrict__ flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) flags[i] = keys[i] <= kth;
}

__global__ __launch_bounds__(TB) void key_compact_kernel(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ flags, int m,
                                                         const int* __restrict__ block_offsets, uint64_t* __restrict__ out) {
    __shared__ int wsum[TB / 64];
    const int i = blockIdx.x * TB + threadIdx.x;
    const int f = i < m ? (flags[i] != 0) : 0;
    const unsigned long long b = __ballot(f);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wsum[wv] = __popcll(b);
    __syncthreads();
    if (!f) return;
    int before = 0;
    for (int k = 0; k < wv; k++) before += wsum[k];
    out[block_offsets[blockIdx.x] + before + __popcll(b & ((1ull << lane) - 1ull))] = keys[i];
}

__global__ void bitonic_step_kernel(uint64_t* __restrict__ keys, int n_pow2, int k, int j) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pow2) return;
    const int l = i ^ j;
    if (l > i) {
        const uint64_t a = keys[i], b = keys[l];
        const bool up = (i & k) == 0;
        if ((a > b) == up) {
            keys[i] = b;
            keys[l] = a;
        }
    }
}

__global__ void table_gather_kernel(const uint64_t* __restrict__ keys, int m, const float* x, const float* y, const float* size, const float* angle,
                                    const float* response, const int* octave, const int* class_id, const int* img, const uint32_t* desc64,
                                    int* __restrict__ rows, apds_keypoint* __restrict__ kps, int* __restrict__ out_img, uint32_t* __restrict__ out_desc) {
    APDS_RAISE_WAVE_PRIORITY();
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)m * 16) return;
    const int i = (int)(t >> 4), w = (int)(t & 15);
    const uint32_t r = (uint32_t)keys[i];
    out_desc[(size_t)i * 16 + w] = desc64[(size_t)r * 16 + w];
    if (w == 0) {
        rows[i] = (int)r;
        apds_keypoint k;
        k.x = x[r]; k.y = y[r]; k.size = size[r]; k.angle = angle[r]; k.response = response[r];
        k.octave = octave[r]; k.class_id = class_id[r];
        kps[i] = k;
        out_img[i] = img[r];
    }
}

// ---- the view path (apds_db_view_select): the same selection, stream-ordered, on buffers a view object owns ---------------------------
// One host synchronisation per call (the count of qualifying rows, right after the flag scan: every later grid is sized by it); the
// radix select keeps its prefix and remaining rank in device memory; the sort does every stride below SORT_B in LDS.
static constexpr int SORT_B = 2048;             // keys one workgroup sorts / merges in LDS: 16 KB of u64, two per thread of 1024
static constexpr uint64_t PAD_KEY = ~0ull;      // strictly above every real key (order_key: the row is below 2^31)

struct ViewSelectState {
    unsigned int hist[256];
    unsigned long long prefix, mask_hi;   // the bytes of the limit-th key decided so far, and the mask that covers them
    unsigned int rank, pad;               // rank of that key among the keys that share the prefix
};

__device__ __forceinline__ bool view_row_selected(const TableColumns& c, long long i, const SelectArgs& a) {
    if (a.mode == 0) return c.image_id[i] == a.value;
    if (c.lod[i] != a.value) return false;
    if (a.mode == 1) return true;
    const float x = c.x[i], y = c.y[i];
    return x >= a.x0 && x <= a.x1 && y >= a.y0 && y <= a.y1;
}

// position of a flagged thread among the flagged threads of its block (TB threads), and the block's count
__device__ __forceinline__ int view_block_rank(int f, int* block_total) {
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

__global__ __launch_bounds__(TB) void view_count_rows_kernel(TableColumns c, int n, SelectArgs a, int* __restrict__ block_counts) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * TB + threadIdx.x;
    int total;
    (void)view_block_rank(i < n && view_row_selected(c, i, a), &total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// one block: block_counts[0 .. nblocks) -> exclusive offsets in place, the sum to block_counts[nblocks]
__global__ __launch_bounds__(1024) void view_offsets_kernel(int* __restrict__ block_counts, int nblocks) {
    APDS_RAISE_WAVE_PRIORITY();
    __shared__ int wtot[16];
    __shared__ int carry;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nblocks; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < nblocks ? block_counts[i] : 0;
        int incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        if (lane == 63) wtot[wv] = incl;
        __syncthreads();
        int before = carry;
        for (int k = 0; k < wv; k++) before += wtot[k];
        if (i < nblocks) block_counts[i] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) block_counts[nblocks] = carry;
}

__global__ __launch_bounds__(TB) void view_emit_keys_kernel(TableColumns c, int n, SelectArgs a, const int* __restrict__ block_offsets,
                                                            uint64_t* __restrict__ keys) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * TB + threadIdx.x;
    const int f = i < n && view_row_selected(c, i, a);
    int total;
    const int pos = view_block_rank(f, &total);
    if (f) keys[block_offsets[blockIdx.x] + pos] = order_key(c.response[i], (uint32_t)i);
}

__global__ __launch_bounds__(256) void view_radix_init_kernel(ViewSelectState* __restrict__ st, unsigned int rank) {
    st->hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) st->prefix = 0, st->mask_hi = 0, st->rank = rank, st->pad = 0;
}

// key_hist_kernel with the prefix read from the state the decide kernel keeps
__global__ __launch_bounds__(256) void view_radix_hist_kernel(const uint64_t* __restrict__ keys, int m, int shift, ViewSelectState* __restrict__ st) {
    APDS_RAISE_WAVE_PRIORITY();
    __shared__ unsigned int s[256];
    s[threadIdx.x] = 0;
    const uint64_t prefix = st->prefix, mask_hi = st->mask_hi;
    __syncthreads();
    for (int i = blockIdx.x * 256 + threadIdx.x; i < m; i += gridDim.x * 256) {
        const uint64_t k = keys[i];
        if ((k & mask_hi) == prefix) atomicAdd(&s[(k >> shift) & 0xFF], 1u);
    }
    __syncthreads();
    if (s[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], s[threadIdx.x]);
}

// one block of 256: the bucket of this byte that holds the wanted rank -> prefix, mask and remaining rank; the histogram is cleared for
// the next byte. More keys than the rank share the prefix (the host takes this path only when more rows qualify than the limit), so
// exactly one bucket holds it.
__global__ __launch_bounds__(256) void view_radix_decide_kernel(ViewSelectState* __restrict__ st, int shift) {
    __shared__ unsigned int s[256];
    const unsigned int t = threadIdx.x;
    const unsigned int h = st->hist[t], rank = st->rank;
    s[t] = h;
    __syncthreads();
    for (unsigned int off = 1; off < 256; off <<= 1) {
        const unsigned int add = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    const unsigned int excl = s[t] - h;
    st->hist[t] = 0;
    if (rank >= excl && rank - excl < h) {
        st->prefix |= (unsigned long long)t << shift;
        st->mask_hi |= 0xFFull << shift;
        st->rank = rank - excl;
    }
}

// after the last byte st->prefix is the limit-th key: the keys not above it, counted per block and then compacted in order
__global__ __launch_bounds__(TB) void view_cut_count_kernel(const uint64_t* __restrict__ keys, int m, const ViewSelectState* __restrict__ st,
                                                            int* __restrict__ block_counts) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * TB + threadIdx.x;
    int total;
    (void)view_block_rank(i < m && keys[i] <= st->prefix, &total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(TB) void view_cut_compact_kernel(const uint64_t* __restrict__ keys, int m, const ViewSelectState* __restrict__ st,
                                                              const int* __restrict__ block_offsets, int limit, uint64_t* __restrict__ out) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * TB + threadIdx.x;
    const uint64_t k = i < m ? keys[i] : PAD_KEY;
    const int f = i < m && k <= st->prefix;
    int total;
    const int pos = block_offsets[blockIdx.x] + view_block_rank(f, &total);
    if (f && pos < limit) out[pos] = k;   // (keys are distinct, so exactly `limit` are kept; the bound guards the buffer all the same)
}

// Steps j_from, j_from / 2, .., 1 of merge stage k on the SORT_B keys of this block in LDS; s[i] is key base + i of the whole array.
// Thread t owns the pair (i, i | j) whose lower index has bit j clear. Strides of 32 keys and more are conflict-free ds_read_b64; below
// that the two halves of a pair interleave and the reads go 2-way.
__device__ __forceinline__ void lds_bitonic_steps(uint64_t* s, unsigned int base, unsigned int k, unsigned int j_from) {
    const unsigned int t = threadIdx.x;
    for (unsigned int j = j_from; j > 0; j >>= 1) {
        const unsigned int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint64_t a = s[i], b = s[l];
        const bool up = ((base + i) & k) == 0;
        if ((a > b) == up) {
            s[i] = b;
            s[l] = a;
        }
        __syncthreads();
    }
}

// blocks of SORT_B keys sorted in one launch (ascending / descending by the block's place in the bitonic network); keys past m read as
// padding. src may be dst.
__global__ __launch_bounds__(SORT_B / 2) void view_block_sort_kernel(const uint64_t* src, int m, uint64_t* dst) {
    APDS_RAISE_WAVE_PRIORITY();
    __shared__ uint64_t s[SORT_B];
    const unsigned int base = blockIdx.x * SORT_B;
    for (unsigned int e = threadIdx.x; e < SORT_B; e += SORT_B / 2) s[e] = base + e < (unsigned int)m ? src[base + e] : PAD_KEY;
    __syncthreads();
    for (unsigned int k = 2; k <= SORT_B; k <<= 1) lds_bitonic_steps(s, base, k, k >> 1);
    for (unsigned int e = threadIdx.x; e < SORT_B; e += SORT_B / 2) dst[base + e] = s[e];
}

// every step of merge stage k (> SORT_B) whose stride is below SORT_B, in one launch
__global__ __launch_bounds__(SORT_B / 2) void view_merge_tail_kernel(uint64_t* __restrict__ keys, unsigned int k) {
    APDS_RAISE_WAVE_PRIORITY();
    __shared__ uint64_t s[SORT_B];
    const unsigned int base = blockIdx.x * SORT_B;
    for (unsigned int e = threadIdx.x; e < SORT_B; e += SORT_B / 2) s[e] = keys[base + e];
    __syncthreads();
    lds_bitonic_steps(s, base, k, SORT_B / 2);
    for (unsigned int e = threadIdx.x; e < SORT_B; e += SORT_B / 2) keys[base + e] = s[e];
}

// one step of stride j >= SORT_B: a thread per pair
__global__ __launch_bounds__(256) void view_merge_step_kernel(uint64_t* __restrict__ keys, unsigned int pairs, unsigned int k, unsigned int j) {
    APDS_RAISE_WAVE_PRIORITY();
    const unsigned int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= pairs) return;
    const unsigned int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
    const uint64_t a = keys[i], b = keys[l];
    if ((a > b) == ((i & k) == 0)) {
        keys[i] = b;
        keys[l] = a;
    }
}

// everything a view holds, in one launch: 16 lanes per row, one descriptor dword each (as table_gather_kernel); lane 0 also writes the
// keypoint, row id and image id, lanes 1..3 one coordinate of the world point each when xyz is asked for
__global__ __launch_bounds__(256) void view_gather_kernel(const uint64_t* __restrict__ keys, int m, TableColumns c, const double* __restrict__ xyz,
                                                          int* __restrict__ rows, apds_keypoint* __restrict__ kps, int* __restrict__ out_img,
                                                          uint32_t* __restrict__ out_desc, double* __restrict__ out_xyz) {
    APDS_RAISE_WAVE_PRIORITY();
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)m * 16) return;
    const int i = (int)(t >> 4), w = (int)(t & 15);
    const uint32_t r = (uint32_t)keys[i];
    out_desc[(size_t)i * 16 + w] = c.desc64[(size_t)r * 16 + w];
    if (w == 0) {
        rows[i] = (int)r;
        apds_keypoint k;
        k.x = c.x[r]; k.y = c.y[r]; k.size = c.size[r]; k.angle = c.angle[r]; k.response = c.response[r];
        k.octave = c.octave[r]; k.class_id = c.class_id[r];
        kps[i] = k;
        out_img[i] = c.image_id[r];
    } else if (w <= 3 && xyz) {
        out_xyz[(size_t)i * 3 + (w - 1)] = xyz[(size_t)r * 3 + (w - 1)];
    }
}

// ---- ids and deletes (keypointdb.rs:28-36, 92-97): stable ordered compaction of the whole table under a delete predicate ---------------
// Victim flags and per-block victim counts -> view_offsets_kernel -> the survivors move down in row order, chunk by chunk: a chunk's
// survivors are gathered into the table's staging buffer by one launch and copied to their destination by the next one (DESIGN §7c-4
// has the argument why no launch reads what another workgroup of the same launch writes).

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

__global__ void table_ids_of_rows_kernel(const int* __restrict__ ids, const int* __restrict__ rows, int m, int* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) out[i] = ids[rows[i]];
}

struct FoundRow {
    long long row;   // -1: no row has the id
    apds_keypoint kp;
    int image_id;
    uint32_t desc[16];
};

// one wave: lane 0 searches the id column, 16 lanes copy the descriptor row
__global__ __launch_bounds__(64) void table_read_id_kernel(TableColumns c, long long n, int id, FoundRow* __restrict__ out) {
    __shared__ long long found;
    if (threadIdx.x == 0) found = find_id_row(c.id, n, id);
    __syncthreads();
    const long long r = found;
    if (threadIdx.x == 0) out->row = r;
    if (r < 0) return;
    if (threadIdx.x < 16) out->desc[threadIdx.x] = c.desc64[r * 16 + threadIdx.x];
    if (threadIdx.x == 0) {
        apds_keypoint k;
        k.x = c.x[r]; k.y = c.y[r]; k.size = c.size[r]; k.angle = c.angle[r]; k.response = c.response[r];
        k.octave = c.octave[r]; k.class_id = c.class_id[r];
        out->kp = k;
        out->image_id = c.image_id[r];
    }
}

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
        else flags[i] = f = view_row_selected(c, i, a);
    }
    int total;
    const int pos = view_block_rank(f, &total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
    if (f && pos == 0) atomicMin(first_row, (int)i);
}

static constexpr int DELETE_CHUNK_ROWS = 1 << 20;   // rows one gather / scatter pair moves: a multiple of TB
static constexpr int MOVE_COLUMNS = 10;             // x, y, size, angle, response, octave, class_id, image_id, lod, id: one dword each
static constexpr int STAGE_ROW_DWORDS = MOVE_COLUMNS + 16 + 6;   // + the descriptor row + the world point: 128 bytes

struct MoveColumns {
    uint32_t* col[MOVE_COLUMNS];
    uint32_t* desc;   // 16 dwords per row
    uint32_t* xyz;    // 6 dwords per row, or null (no valid world points: nothing to move)
};
// the staging buffer: MOVE_COLUMNS planes of `rows` dwords, then rows x 16 descriptor dwords, then rows x 6 world point dwords
struct StageColumns {
    uint32_t* base;
    int rows;
    __device__ __forceinline__ uint32_t* col(int k) const { return base + (size_t)k * rows; }
    __device__ __forceinline__ uint32_t* desc() const { return base + (size_t)MOVE_COLUMNS * rows; }
    __device__ __forceinline__ uint32_t* xyz() const { return base + (size_t)(MOVE_COLUMNS + 16) * rows; }
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
    const int pos = view_block_rank(f, &total);
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
    uint32_t* sd = st.desc() + before * 16;
    for (int e = skip * 16 + threadIdx.x; e < total * 16; e += TB) sd[e] = m.desc[(size_t)(r0 + src_of[e >> 4]) * 16 + (e & 15)];
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
    const long long R = region_rows, g0 = (long long)blockIdx.x * 256;
    if (g0 < R * 16) {
        const long long e = g0 + threadIdx.x;
        if (e >= skip * 16 && e < survivors * 16) m.desc[dst0 * 16 + e] = st.desc()[e];
    } else if (g0 < R * (16 + MOVE_COLUMNS)) {
        const int k = (int)((g0 - R * 16) / R);
        const long long j = g0 - R * (16 + k) + threadIdx.x;
        if (j >= skip && j < survivors) m.col[k][dst0 + j] = st.col(k)[j];
    } else {
        const long long e = g0 - R * (16 + MOVE_COLUMNS) + threadIdx.x;
        if (e >= skip * 6 && e < survivors * 6) m.xyz[dst0 * 6 + e] = st.xyz()[e];
    }
}

// A view of one table: the outputs of a selection and all the scratch it takes, allocated once (apds_db_view_create).
struct TableView {
    KeypointTable* t = nullptr;
    int limit = 0, n = 0;
    int64_t sort_cap = 0;   // keys the sort buffer holds: the power of two that holds `limit`, at least SORT_B
    bool has_xyz = false;
    int *block_counts = nullptr, *cut_counts = nullptr;   // table capacity / TB + 1 each
    uint64_t *keys = nullptr, *sorted = nullptr;          // table capacity; sort_cap
    ViewSelectState* state = nullptr;
    int* host_count = nullptr;                            // pinned
    int *rows = nullptr, *image_id = nullptr;
    apds_keypoint* kps = nullptr;
    uint8_t* desc64 = nullptr;
    double* xyz = nullptr;
};

}  // namespace apds

using namespace apds;

namespace {
template <class T>
void dev_alloc(T*& p, size_t n) {
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(T)));
}
void table_free(KeypointTable* t) {
    for (void* p : {(void*)t->x, (void*)t->y, (void*)t->size, (void*)t->angle, (void*)t->response, (void*)t->octave, (void*)t->class_id,
                    (void*)t->image_id, (void*)t->lod, (void*)t->desc64, (void*)t->view_rows, (void*)t->view_kps, (void*)t->view_image_id,
                    (void*)t->view_desc64, (void*)t->all_kps, (void*)t->xyz, (void*)t->id, (void*)t->stage})
        if (p) (void)hipFree(p);
    delete t;
}
void view_free(TableView* v) {
    for (void* p : {(void*)v->block_counts, (void*)v->cut_counts, (void*)v->keys, (void*)v->sorted, (void*)v->state, (void*)v->rows, (void*)v->image_id,
                    (void*)v->kps, (void*)v->desc64, (void*)v->xyz})
        if (p) (void)hipFree(p);
    if (v->host_count) (void)hipHostFree(v->host_count);
    delete v;
}
TableColumns columns_of(KeypointTable* t) {
    return TableColumns{t->x, t->y, t->size, t->angle, t->response, t->octave, t->class_id, t->image_id, t->lod, reinterpret_cast<uint32_t*>(t->desc64), t->id};
}
float lift_offset(uint64_t index, uint64_t tile, int lod) { return (float)(index * tile * (1ull << lod)); }   // (u64 product) as f32

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
    hipLaunchKernelGGL(view_offsets_kernel, dim3(1), dim3(1024), 0, s, counts, nb);
    HIP_CHECK(hipGetLastError());
    int h[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(h, counts + nb, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const int m = h[0], first_row = h[1];
    if (!m) return 0;
    const bool xyz_valid = t->xyz && t->xyz_rows == t->n;
    if ((int64_t)first_row + m < n) {   // a survivor sits behind a victim: rows move (a deleted tail moves nothing)
        if (!t->stage) {
            t->stage_rows = (int)std::min<int64_t>(DELETE_CHUNK_ROWS, (int64_t)ceil_div(t->capacity, TB) * TB);
            dev_alloc(t->stage, (size_t)t->stage_rows * STAGE_ROW_DWORDS);
        }
        MoveColumns mv;
        uint32_t* const planes[MOVE_COLUMNS] = {reinterpret_cast<uint32_t*>(t->x), reinterpret_cast<uint32_t*>(t->y), reinterpret_cast<uint32_t*>(t->size),
                                               reinterpret_cast<uint32_t*>(t->angle), reinterpret_cast<uint32_t*>(t->response),
                                               reinterpret_cast<uint32_t*>(t->octave), reinterpret_cast<uint32_t*>(t->class_id),
                                               reinterpret_cast<uint32_t*>(t->image_id), reinterpret_cast<uint32_t*>(t->lod), reinterpret_cast<uint32_t*>(t->id)};
        for (int k = 0; k < MOVE_COLUMNS; k++) mv.col[k] = planes[k];
        mv.desc = reinterpret_cast<uint32_t*>(t->desc64);
        mv.xyz = xyz_valid ? reinterpret_cast<uint32_t*>(t->xyz) : nullptr;
        const StageColumns st{t->stage, t->stage_rows};
        const int chunk_blocks = t->stage_rows / TB, segments = xyz_valid ? STAGE_ROW_DWORDS : STAGE_ROW_DWORDS - 6;
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

namespace apds {

int table_device(const void* db) {
    APDS_REQUIRE(db, APDS_ERR_BAD_ARG, "null table");
    return static_cast<const KeypointTable*>(db)->device;
}

// n_tiles tiles of an extraction's device output appended in tile order by one launch on s; the small tile table comes from the calling
// thread's workspace (no ws_reset here: the extraction's buffers may live there). Everything is checked before anything is written.
// Synchronises s.
void table_insert_batch_device(void* db, const void* kps_dev, const void* desc64_dev, int n_tiles, int capacity, const int32_t* counts, int first_image_id,
                               int lod, const uint32_t* columns_rows, uint64_t tile_w, uint64_t tile_h, hipStream_t s) {
    KeypointTable* t = static_cast<KeypointTable*>(db);
    APDS_REQUIRE(t && lod >= 0 && lod < 31 && capacity >= 0, APDS_ERR_BAD_ARG, "bad argument");
    APDS_REQUIRE(n_tiles >= 1 && n_tiles <= 4096, APDS_ERR_BAD_ARG, "batch must hold 1 .. 4096 tiles");
    APDS_REQUIRE(counts && columns_rows, APDS_ERR_BAD_ARG, "null argument");
    const size_t xy_at = ((size_t)n_tiles + 2) & ~size_t(1);             // an even number of ints: the float2 rows stay 8-byte aligned
    std::vector<int> table(xy_at + 2 * (size_t)n_tiles);                 // offsets (n_tiles + 1), then (xoff, yoff) per tile as float bits
    float* xy = reinterpret_cast<float*>(table.data() + xy_at);
    int64_t total = 0;
    for (int i = 0; i < n_tiles; i++) {
        APDS_REQUIRE(counts[i] >= 0 && counts[i] <= capacity, APDS_ERR_BAD_ARG, "a tile's count is negative or exceeds the capacity");
        total += counts[i];
    }
    APDS_REQUIRE(t->n + total <= t->capacity, APDS_ERR_NOMEM, "keypoint table is full");
    APDS_REQUIRE(t->next_id + total <= (1ll << 31), APDS_ERR_NOMEM, "keypoint table has given out every 32-bit id");
    for (int i = 0, off = 0; i < n_tiles; off += counts[i], i++) {
        table[i] = off;
        xy[2 * i] = lift_offset(columns_rows[2 * i], tile_w, lod);
        xy[2 * i + 1] = lift_offset(columns_rows[2 * i + 1], tile_h, lod);
    }
    table[n_tiles] = (int)total;
    if (!total) return;
    APDS_REQUIRE(kps_dev && desc64_dev, APDS_ERR_BAD_ARG, "null argument");
    APDS_REQUIRE(reinterpret_cast<uintptr_t>(kps_dev) % 4 == 0 && reinterpret_cast<uintptr_t>(desc64_dev) % 4 == 0, APDS_ERR_BAD_ARG,
                 "device keypoints and descriptor rows must be 4-byte aligned");
    int* dtab = ctx().alloc_n<int>(table.size());
    HIP_CHECK(hipMemcpyAsync(dtab, table.data(), table.size() * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(table_insert_dev_kernel, dim3(ceil_div(total * 16, 256)), dim3(256), ((size_t)n_tiles + 1) * sizeof(int), s,
                       static_cast<const apds_keypoint*>(kps_dev), static_cast<const uint32_t*>(desc64_dev), n_tiles, capacity, (const int*)dtab,
                       reinterpret_cast<const float2*>(dtab + xy_at), first_image_id, lod, ldexpf(1.0f, lod), (long long)t->n, (int)t->next_id, columns_of(t));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
    t->n += total;
    t->next_id += total;
}

}  // namespace apds

extern "C" {

int apds_db_create(void** db, int64_t capacity) {
    return guarded([&] {
        APDS_REQUIRE(db && capacity > 0 && capacity < (1ll << 31), APDS_ERR_BAD_ARG, "bad capacity");
        ThreadCtx& c = ctx();
        KeypointTable* t = new KeypointTable();
        t->device = c.device;
        t->capacity = capacity;
        try {
            dev_alloc(t->x, capacity); dev_alloc(t->y, capacity); dev_alloc(t->size, capacity); dev_alloc(t->angle, capacity);
            dev_alloc(t->response, capacity); dev_alloc(t->octave, capacity); dev_alloc(t->class_id, capacity);
            dev_alloc(t->image_id, capacity); dev_alloc(t->lod, capacity); dev_alloc(t->desc64, (size_t)capacity * 64);
            dev_alloc(t->id, capacity);
            t->view_cap = std::min<int64_t>(capacity, APDS_MAX_POINTS);
            dev_alloc(t->view_rows, t->view_cap); dev_alloc(t->view_kps, t->view_cap); dev_alloc(t->view_image_id, t->view_cap);
            dev_alloc(t->view_desc64, (size_t)t->view_cap * 64);
        } catch (...) {
            table_free(t);
            throw;
        }
        *db = t;
    });
}

int apds_db_destroy(void* db) {
    return guarded([&] {
        if (db) table_free(static_cast<KeypointTable*>(db));
    });
}

int64_t apds_db_rows(const void* db) { return db ? static_cast<const KeypointTable*>(db)->n : -1; }

// preprocessor/src/main.rs:296-324: all keypoints of one tile image, coordinates lifted to level-of-detail-0 mosaic pixels
int apds_db_insert_image(void* db, const apds_keypoint* kps, const uint8_t* desc61, int n, int image_id, int lod, uint64_t column, uint64_t row,
                         uint64_t tile_w, uint64_t tile_h) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t && n >= 0 && lod >= 0 && lod < 31, APDS_ERR_BAD_ARG, "bad argument");
        APDS_REQUIRE(t->n + n <= t->capacity, APDS_ERR_NOMEM, "keypoint table is full");
        APDS_REQUIRE(t->next_id + n <= (1ll << 31), APDS_ERR_NOMEM, "keypoint table has given out every 32-bit id");
        if (!n) return;
        APDS_REQUIRE(kps && desc61, APDS_ERR_BAD_ARG, "null argument");
        ThreadCtx& c = ctx();
        c.ws_reset();
        hipStream_t s = c.stream;
        apds_keypoint* dk = c.alloc_n<apds_keypoint>(n);
        uint8_t* dd = c.alloc_n<uint8_t>((size_t)n * 61);
        HIP_CHECK(hipMemcpyAsync(dk, kps, (size_t)n * sizeof(apds_keypoint), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(dd, desc61, (size_t)n * 61, hipMemcpyHostToDevice, s));
        const float scale = ldexpf(1.0f, lod);                                   // 2_f32.powi(lod)
        const float xoff = lift_offset(column, tile_w, lod), yoff = lift_offset(row, tile_h, lod);
        hipLaunchKernelGGL(table_insert_kernel, dim3(ceil_div((long long)n * 16, 256)), dim3(256), 0, s, (const apds_keypoint*)dk, (const uint8_t*)dd, n,
                           image_id, lod, scale, xoff, yoff, (long long)t->n, (int)t->next_id, columns_of(t));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
        t->n += n;
        t->next_id += n;
    });
}

// the same rows from what apds_dev_akaze_extract has written on the device (no upload, no repack): one tile, then a batch of them
int apds_db_insert_batch_dev(void* db, const void* kps_dev, const void* desc64_dev, int n_tiles, int capacity, const int32_t* counts, int first_image_id,
                             int lod, const uint32_t* columns_rows, uint64_t tile_w, uint64_t tile_h, void* stream) {
    return guarded([&] {
        hipStream_t s = pick_stream(stream);
        ctx().ws_reset(s);
        table_insert_batch_device(db, kps_dev, desc64_dev, n_tiles, capacity, counts, first_image_id, lod, columns_rows, tile_w, tile_h, s);
    });
}

int apds_db_insert_dev(void* db, const void* kps_dev, const void* desc64_dev, int n, int image_id, int lod, uint64_t column, uint64_t row, uint64_t tile_w,
                       uint64_t tile_h, void* stream) {
    return guarded([&] {
        APDS_REQUIRE(column <= 0xFFFFFFFFull && row <= 0xFFFFFFFFull, APDS_ERR_BAD_ARG, "tile column / row beyond 32 bits");
        const int32_t counts[1] = {n};
        const uint32_t cr[2] = {(uint32_t)column, (uint32_t)row};
        hipStream_t s = pick_stream(stream);
        ctx().ws_reset(s);
        table_insert_batch_device(db, kps_dev, desc64_dev, 1, std::max(n, 0), counts, image_id, lod, cr, tile_w, tile_h, s);
    });
}

// The world point of every row (ingest.hip's arithmetic on ((double)x, (double)y)) into the table's xyz column; a row whose elevation
// lookup misses is three NaNs and is counted in *n_missing.
int apds_db_world_coordinates(void* db, const double* dataset_gt, const double* elevation_gt, const void* elevation, int ew, int eh, int elevation_on_device,
                              int64_t* n_missing) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t && dataset_gt, APDS_ERR_BAD_ARG, "null argument");
        APDS_REQUIRE(!elevation_gt || (elevation && ew > 0 && eh > 0), APDS_ERR_BAD_ARG, "elevation geotransform without a raster");
        if (n_missing) *n_missing = 0;
        ThreadCtx& c = ctx();
        APDS_REQUIRE(t->device == c.device, APDS_ERR_BAD_ARG, "the table lives on another device than the calling thread's");
        c.ws_reset();
        hipStream_t s = c.stream;
        if (!t->xyz) dev_alloc(t->xyz, (size_t)t->capacity * 3);
        const double* del = nullptr;
        if (elevation_gt) {
            del = static_cast<const double*>(elevation);
            if (!elevation_on_device) {
                double* up = c.alloc_n<double>((size_t)ew * eh);
                HIP_CHECK(hipMemcpyAsync(up, elevation, (size_t)ew * eh * sizeof(double), hipMemcpyHostToDevice, s));
                del = up;
            }
        }
        t->xyz_rows = -1;
        const int64_t miss = world_coordinates_columns_device(t->x, t->y, (int)t->n, dataset_gt, elevation_gt, del, ew, eh, t->xyz, s);
        t->xyz_rows = t->n;
        if (n_missing) *n_missing = miss;
    });
}

// The whole table as the arguments the pipeline takes: its own descriptor column, 28-byte keypoints by row (gathered here for the rows
// added since the last call) and the xyz column while it covers every row.
int apds_db_table(void* db, void** rows64_dev, void** kps_dev, void** xyz_dev, int64_t* n) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t, APDS_ERR_BAD_ARG, "null table");
        if (kps_dev) {
            ThreadCtx& c = ctx();
            APDS_REQUIRE(t->device == c.device, APDS_ERR_BAD_ARG, "the table lives on another device than the calling thread's");
            if (!t->all_kps) dev_alloc(t->all_kps, (size_t)t->capacity);
            const int64_t fresh = t->n - t->all_kps_rows;
            if (fresh > 0) {
                hipStream_t s = c.stream;
                hipLaunchKernelGGL(table_keypoints_kernel, dim3(ceil_div(fresh, 256)), dim3(256), 0, s, columns_of(t), (long long)t->all_kps_rows, (int)fresh,
                                   t->all_kps);
                HIP_CHECK(hipGetLastError());
                HIP_CHECK(hipStreamSynchronize(s));
                t->all_kps_rows = t->n;
            }
            *kps_dev = t->all_kps;
        }
        if (rows64_dev) *rows64_dev = t->desc64;
        if (xyz_dev) *xyz_dev = (t->xyz && t->xyz_rows == t->n) ? t->xyz : nullptr;
        if (n) *n = t->n;
    });
}

// keypointdb.rs:38-90. mode 0: image_id == value; 1: level_of_detail == value; 2: level_of_detail == value and
// floor(x_start) <= x <= ceil(x_end), floor(y_start) <= y <= ceil(y_end). Result (ordered by response desc, at most 262143
// rows) stays on the device as the table's current view; *n_out is its row count.
int apds_db_select(void* db, int mode, int value, float x_start, float y_start, float x_end, float y_end, int* n_out) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t && n_out && mode >= 0 && mode <= 2, APDS_ERR_BAD_ARG, "bad argument");
        *n_out = 0;
        t->view_n = 0;
        const int n = (int)t->n;
        if (!n) return;
        ThreadCtx& c = ctx();
        c.ws_reset();
        hipStream_t s = c.stream;
        SelectArgs a{mode, value, floorf(x_start), floorf(y_start), ceilf(x_end), ceilf(y_end)};
        uint8_t* flags = c.alloc_n<uint8_t>(n);
        hipLaunchKernelGGL(table_flags_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, (const int*)t->image_id, (const int*)t->lod, (const float*)t->x,
                           (const float*)t->y, (long long)n, a, flags);
        int* total_dev = nullptr;
        int* offs = scan_flags_device(flags, n, &total_dev, s);
        int m = 0;
        HIP_CHECK(hipMemcpyAsync(&m, total_dev, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (!m) return;
        uint64_t* keys = c.alloc_n<uint64_t>(m);
        hipLaunchKernelGGL(table_emit_keys_kernel, dim3(ceil_div(n, TB)), dim3(TB), 0, s, (const uint8_t*)flags, (const float*)t->response, n, (const int*)offs,
                           keys);
        const int limit = (int)std::min<int64_t>(APDS_MAX_POINTS, t->view_cap);
        if (m > limit) {
            // radix select of the limit-th smallest key, most significant byte first
            unsigned int* hist = c.alloc_n<unsigned int>(256);
            uint64_t prefix = 0, mask_hi = 0;
            unsigned int k = (unsigned int)(limit - 1), h[256];
            for (int shift = 56; shift >= 0; shift -= 8) {
                HIP_CHECK(hipMemsetAsync(hist, 0, 256 * sizeof(unsigned int), s));
                hipLaunchKernelGGL(key_hist_kernel, dim3(256), dim3(256), 0, s, (const uint64_t*)keys, m, prefix, mask_hi, shift, hist);
                HIP_CHECK(hipMemcpyAsync(h, hist, sizeof(h), hipMemcpyDeviceToHost, s));
                HIP_CHECK(hipStreamSynchronize(s));
                unsigned int b = 0;
                for (; b < 256; b++) {
                    if (k < h[b]) break;
                    k -= h[b];
                }
                prefix |= (uint64_t)b << shift;
                mask_hi |= 0xFFull << shift;
            }
            uint8_t* f2 = c.alloc_n<uint8_t>(m);
            hipLaunchKernelGGL(key_leq_flags_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, s, (const uint64_t*)keys, m, prefix, f2);
            int* tot2 = nullptr;
            int* offs2 = scan_flags_device(f2, m, &tot2, s);
            uint64_t* kept = c.alloc_n<uint64_t>(limit);
            hipLaunchKernelGGL(key_compact_kernel, dim3(ceil_div(m, TB)), dim3(TB), 0, s, (const uint64_t*)keys, (const uint8_t*)f2, m, (const int*)offs2, kept);
            keys = kept;
            m = limit;
        }
        // bitonic sort of the (<= 2^18) surviving keys, padded with +inf keys
        int p2 = 1;
        while (p2 < m) p2 <<= 1;
        uint64_t* sorted = c.alloc_n<uint64_t>(p2);
        HIP_CHECK(hipMemsetAsync(sorted, 0xFF, (size_t)p2 * 8, s));
        HIP_CHECK(hipMemcpyAsync(sorted, keys, (size_t)m * 8, hipMemcpyDeviceToDevice, s));
        for (int k = 2; k <= p2; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) hipLaunchKernelGGL(bitonic_step_kernel, dim3(ceil_div(p2, 256)), dim3(256), 0, s, sorted, p2, k, j);
        hipLaunchKernelGGL(table_gather_kernel, dim3(ceil_div((long long)m * 16, 256)), dim3(256), 0, s, (const uint64_t*)sorted, m, (const float*)t->x,
                           (const float*)t->y, (const float*)t->size, (const float*)t->angle, (const float*)t->response, (const int*)t->octave,
                           (const int*)t->class_id, (const int*)t->image_id, reinterpret_cast<const uint32_t*>(t->desc64), t->view_rows, t->view_kps,
                           t->view_image_id, reinterpret_cast<uint32_t*>(t->view_desc64));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
        t->view_n = m;
        *n_out = m;
    });
}

// device pointers of the current view: rows64 (n x 64 B, a ready train set), keypoints (n x 28 B), table row ids, image ids
int apds_db_view(void* db, void** rows64, void** kps, void** row_ids, void** image_ids, int* n) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t, APDS_ERR_BAD_ARG, "null table");
        if (rows64) *rows64 = t->view_desc64;
        if (kps) *kps = t->view_kps;
        if (row_ids) *row_ids = t->view_rows;
        if (image_ids) *image_ids = t->view_image_id;
        if (n) *n = (int)t->view_n;
    });
}

// BFMatcher.knnMatch of host query descriptors against the CURRENT VIEW (resident on the device): idx = position in the view
int apds_db_knn_match(void* db, const uint8_t* query_desc, int n_query, int desc_bytes, int k, int32_t* idx, int32_t* dist) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t && idx && dist && n_query >= 0, APDS_ERR_BAD_ARG, "bad argument");
        APDS_REQUIRE(desc_bytes >= 1 && desc_bytes <= 64, APDS_ERR_ASSERT, "descriptor length must be 1..64 bytes");
        APDS_REQUIRE(k >= 1, APDS_ERR_ASSERT, "k >= 1");   // (any k apds_dev_hamming_topk serves: the keys come from the same scan)
        if (!n_query) return;
        ThreadCtx& c = ctx();
        c.ws_reset();
        hipStream_t s = c.stream;
        uint8_t* raw = c.alloc_n<uint8_t>((size_t)n_query * desc_bytes);
        uint8_t* q64 = c.alloc_n<uint8_t>((size_t)n_query * 64);
        uint64_t* keys = c.alloc_n<uint64_t>((size_t)n_query * k);
        HIP_CHECK(hipMemcpyAsync(raw, query_desc, (size_t)n_query * desc_bytes, hipMemcpyHostToDevice, s));
        pack_rows_device(raw, n_query, desc_bytes, desc_bytes, q64, s);
        hamming_topk_device(q64, n_query, t->view_desc64, t->view_n, 0, k, keys, s);
        std::vector<uint64_t> h((size_t)n_query * k);
        HIP_CHECK(hipMemcpyAsync(h.data(), keys, h.size() * 8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        for (size_t i = 0; i < h.size(); i++) {
            if (h[i] == EMPTY_KEY) idx[i] = -1, dist[i] = 0x7fffffff;
            else idx[i] = (int32_t)(uint32_t)h[i], dist[i] = (int32_t)(h[i] >> 32);
        }
    });
}

// host copy of the current view: what the reference's Vec<models::Keypoint> holds (id: the table's id column, a SERIAL column's values:
// row + 1 on a table that never saw a delete)
int apds_db_view_download(void* db, apds_keypoint* kps, uint8_t* desc61, int32_t* ids, int32_t* image_ids) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t, APDS_ERR_BAD_ARG, "null table");
        const int m = (int)t->view_n;
        if (!m) return;
        ThreadCtx& c = ctx();
        c.ws_reset();
        hipStream_t s = c.stream;
        if (kps) HIP_CHECK(hipMemcpyAsync(kps, t->view_kps, (size_t)m * sizeof(apds_keypoint), hipMemcpyDeviceToHost, s));
        if (image_ids) HIP_CHECK(hipMemcpyAsync(image_ids, t->view_image_id, (size_t)m * 4, hipMemcpyDeviceToHost, s));
        if (ids) {
            int* view_ids = c.alloc_n<int>(m);
            hipLaunchKernelGGL(table_ids_of_rows_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, s, (const int*)t->id, (const int*)t->view_rows, m, view_ids);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(ids, view_ids, (size_t)m * 4, hipMemcpyDeviceToHost, s));
        }
        if (desc61) {
            uint8_t* d61 = c.alloc_n<uint8_t>((size_t)m * 61);
            HIP_CHECK(hipMemcpy2DAsync(d61, 61, t->view_desc64, 64, 61, m, hipMemcpyDeviceToDevice, s));
            HIP_CHECK(hipMemcpyAsync(desc61, d61, (size_t)m * 61, hipMemcpyDeviceToHost, s));
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

// ---- view objects: keypointdb.rs:50-90 once per frame, on the caller's stream ------------------------------------------------------
int apds_db_view_create(void* db, int capacity, void** view) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t && view, APDS_ERR_BAD_ARG, "null argument");
        *view = nullptr;
        APDS_REQUIRE(t->device == ctx().device, APDS_ERR_BAD_ARG, "the table lives on another device than the calling thread's");
        TableView* v = new TableView();
        v->t = t;
        v->limit = (int)(capacity <= 0 ? std::min<int64_t>(APDS_MAX_POINTS, t->capacity) : std::min<int64_t>(capacity, APDS_MAX_POINTS));
        v->sort_cap = SORT_B;
        while (v->sort_cap < v->limit) v->sort_cap <<= 1;
        const size_t nblocks = (size_t)ceil_div(t->capacity, TB) + 1, lim = (size_t)v->limit;
        try {
            dev_alloc(v->block_counts, nblocks); dev_alloc(v->cut_counts, nblocks);
            dev_alloc(v->keys, (size_t)t->capacity); dev_alloc(v->sorted, (size_t)v->sort_cap);
            dev_alloc(v->state, 1);
            dev_alloc(v->rows, lim); dev_alloc(v->image_id, lim); dev_alloc(v->kps, lim); dev_alloc(v->desc64, lim * 64); dev_alloc(v->xyz, lim * 3);
            HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&v->host_count), sizeof(int), hipHostMallocDefault));
        } catch (...) {
            view_free(v);
            throw;
        }
        *view = v;
    });
}

int apds_db_view_destroy(void* view) {
    return guarded([&] {
        if (view) view_free(static_cast<TableView*>(view));
    });
}

// apds_db_select's rows into the view, everything on `stream` (NULL: the calling thread's). The one host synchronisation is the count
// of qualifying rows; the kernels that cut, sort and gather are queued behind it and the call returns: *n_out is final, the view's
// buffers are complete once the stream has run (any later work on the same stream sees them).
int apds_db_view_select(void* view, int mode, int value, float x_start, float y_start, float x_end, float y_end, int with_xyz, void* stream, int* n_out) {
    return guarded([&] {
        TableView* v = static_cast<TableView*>(view);
        APDS_REQUIRE(v && n_out && mode >= 0 && mode <= 2, APDS_ERR_BAD_ARG, "bad argument");
        KeypointTable* t = v->t;
        *n_out = 0;
        APDS_REQUIRE(!with_xyz || (t->xyz && t->xyz_rows == t->n), APDS_ERR_BAD_ARG,
                     "the table's world points are absent or older than its rows (apds_db_world_coordinates)");
        APDS_REQUIRE(t->device == ctx().device, APDS_ERR_BAD_ARG, "the table lives on another device than the calling thread's");
        hipStream_t s = pick_stream(stream);
        v->n = 0;
        v->has_xyz = false;
        const int n = (int)t->n;
        if (!n) return;
        const SelectArgs a{mode, value, floorf(x_start), floorf(y_start), ceilf(x_end), ceilf(y_end)};
        const TableColumns c = columns_of(t);
        const int nb = ceil_div(n, TB);
        hipLaunchKernelGGL(view_count_rows_kernel, dim3(nb), dim3(TB), 0, s, c, n, a, v->block_counts);
        hipLaunchKernelGGL(view_offsets_kernel, dim3(1), dim3(1024), 0, s, v->block_counts, nb);
        HIP_CHECK(hipMemcpyAsync(v->host_count, v->block_counts + nb, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        int m = *v->host_count;
        if (!m) return;
        hipLaunchKernelGGL(view_emit_keys_kernel, dim3(nb), dim3(TB), 0, s, c, n, a, (const int*)v->block_counts, v->keys);
        const uint64_t* unsorted = v->keys;
        if (m > v->limit) {
            // radix select of the limit-th smallest key, most significant byte first; each byte's bucket is decided on the device
            hipLaunchKernelGGL(view_radix_init_kernel, dim3(1), dim3(256), 0, s, v->state, (unsigned int)(v->limit - 1));
            for (int shift = 56; shift >= 0; shift -= 8) {
                hipLaunchKernelGGL(view_radix_hist_kernel, dim3(256), dim3(256), 0, s, (const uint64_t*)v->keys, m, shift, v->state);
                hipLaunchKernelGGL(view_radix_decide_kernel, dim3(1), dim3(256), 0, s, v->state, shift);
            }
            const int mb = ceil_div(m, TB);
            hipLaunchKernelGGL(view_cut_count_kernel, dim3(mb), dim3(TB), 0, s, (const uint64_t*)v->keys, m, (const ViewSelectState*)v->state, v->cut_counts);
            hipLaunchKernelGGL(view_offsets_kernel, dim3(1), dim3(1024), 0, s, v->cut_counts, mb);
            hipLaunchKernelGGL(view_cut_compact_kernel, dim3(mb), dim3(TB), 0, s, (const uint64_t*)v->keys, m, (const ViewSelectState*)v->state,
                               (const int*)v->cut_counts, v->limit, v->sorted);
            unsorted = v->sorted;
            m = v->limit;
        }
        // bitonic sort of the m surviving keys, padded to p2 (a power of two, at least one block) with keys above every real one
        unsigned int p2 = SORT_B;
        while (p2 < (unsigned int)m) p2 <<= 1;
        hipLaunchKernelGGL(view_block_sort_kernel, dim3(p2 / SORT_B), dim3(SORT_B / 2), 0, s, unsorted, m, v->sorted);
        for (unsigned int k = 2 * SORT_B; k <= p2; k <<= 1) {
            for (unsigned int j = k >> 1; j >= (unsigned int)SORT_B; j >>= 1)
                hipLaunchKernelGGL(view_merge_step_kernel, dim3(p2 / 2 / 256), dim3(256), 0, s, v->sorted, p2 / 2, k, j);
            hipLaunchKernelGGL(view_merge_tail_kernel, dim3(p2 / SORT_B), dim3(SORT_B / 2), 0, s, v->sorted, k);
        }
        hipLaunchKernelGGL(view_gather_kernel, dim3(ceil_div((long long)m * 16, 256)), dim3(256), 0, s, (const uint64_t*)v->sorted, m, c,
                           (const double*)(with_xyz ? t->xyz : nullptr), v->rows, v->kps, v->image_id, reinterpret_cast<uint32_t*>(v->desc64), v->xyz);
        HIP_CHECK(hipGetLastError());
        v->n = m;
        v->has_xyz = with_xyz != 0;
        *n_out = m;
    });
}

// device pointers of the view's last selection (*xyz_dev: NULL unless it ran with_xyz)
int apds_db_view_pointers(const void* view, void** rows64_dev, void** kps_dev, void** row_ids_dev, void** image_ids_dev, void** xyz_dev, int* n) {
    return guarded([&] {
        const TableView* v = static_cast<const TableView*>(view);
        APDS_REQUIRE(v, APDS_ERR_BAD_ARG, "null view");
        if (rows64_dev) *rows64_dev = v->desc64;
        if (kps_dev) *kps_dev = v->kps;
        if (row_ids_dev) *row_ids_dev = v->rows;
        if (image_ids_dev) *image_ids_dev = v->image_id;
        if (xyz_dev) *xyz_dev = v->has_xyz ? v->xyz : nullptr;
        if (n) *n = v->n;
    });
}

// ---- ids and deletes: keypointdb.rs:28-36 (read_keypoint_from_id) and 92-97 (delete_keypoint) ----------------------------------------
int apds_db_ids(void* db, void** ids_dev) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t && ids_dev, APDS_ERR_BAD_ARG, "null argument");
        *ids_dev = t->id;
    });
}

int apds_db_read_keypoint_from_id(void* db, int id, apds_keypoint* kp, uint8_t* desc61, int* image_id, int64_t* row) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t, APDS_ERR_BAD_ARG, "null table");
        APDS_REQUIRE(t->n > 0 && id >= 1, APDS_ERR_OUT_OF_RANGE, "no keypoint has this id");
        ThreadCtx& c = ctx();
        APDS_REQUIRE(t->device == c.device, APDS_ERR_BAD_ARG, "the table lives on another device than the calling thread's");
        c.ws_reset();
        hipStream_t s = c.stream;
        FoundRow* out = c.alloc_n<FoundRow>(1);
        hipLaunchKernelGGL(table_read_id_kernel, dim3(1), dim3(64), 0, s, columns_of(t), (long long)t->n, id, out);
        HIP_CHECK(hipGetLastError());
        FoundRow h;
        HIP_CHECK(hipMemcpyAsync(&h, out, sizeof(h), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        APDS_REQUIRE(h.row >= 0, APDS_ERR_OUT_OF_RANGE, "no keypoint has this id");
        if (kp) *kp = h.kp;
        if (desc61) memcpy(desc61, h.desc, 61);
        if (image_id) *image_id = h.image_id;
        if (row) *row = h.row;
    });
}

int apds_db_delete_where(void* db, int mode, int value, float x_start, float y_start, float x_end, float y_end, int64_t* n_deleted) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t && mode >= 0 && mode <= 2, APDS_ERR_BAD_ARG, "bad argument");
        if (n_deleted) *n_deleted = 0;
        if (!t->n) return;
        ThreadCtx& c = ctx();
        APDS_REQUIRE(t->device == c.device, APDS_ERR_BAD_ARG, "the table lives on another device than the calling thread's");
        c.ws_reset();
        const SelectArgs a{mode, value, floorf(x_start), floorf(y_start), ceilf(x_end), ceilf(y_end)};
        const int64_t m = table_delete_rows(t, c, a, c.alloc_n<uint8_t>((size_t)t->n));
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
        APDS_REQUIRE(t->device == c.device, APDS_ERR_BAD_ARG, "the table lives on another device than the calling thread's");
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
