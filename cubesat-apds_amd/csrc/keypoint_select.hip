// csrc/keypoint_select.hip — the reads of the keypoint table (feature_database/src/keypointdb.rs:38-90): by image id / by level of detail
// / by bounding box at a level of detail, each `ORDER BY response DESC LIMIT 262143` (OPENCV_KEYPOINT_LIMIT, keypointdb.rs:12).
// ONE engine (select_rows): rows per block that satisfy the predicate -> block offsets -> ordered compaction of u64 keys
// (order_key: ~response_bits << 32 | row) -> radix select of the LIMIT-th key when more rows qualify -> bitonic sort of the survivors ->
// row gather. Ties in response are ordered by insertion order (row), which SQL leaves unspecified. Two fronts hand it their buffers:
// apds_db_select (the table's current view, scratch from the thread's workspace, synchronised) and apds_db_view_select (a view object
// that owns outputs and scratch, on the caller's stream). A selection is directly usable as a train set: 64-byte descriptor rows, and
// `train_idx` = position in the selection (the index the reference would get from the returned Vec). On a float table the rows are 64
// floats, and a view object's gather also writes the L2 screen's train side of the selection (apds_db_view_l2_train).
#include <cstring>
#include <vector>

#include "bf16_round.h"
#include "keypoint_table.h"
#include "topk_keys.h"

namespace apds {

// One host synchronisation per selection (the count of qualifying rows, right after the offsets: every later grid is sized by it); the
// radix select keeps its prefix and remaining rank in device memory; the sort does every stride below SORT_B in LDS.
static constexpr int SORT_B = 2048;             // keys one workgroup sorts / merges in LDS: 16 KB of u64, two per thread of 1024
static constexpr uint64_t PAD_KEY = ~0ull;      // strictly above every real key (order_key: the row is below 2^31)

struct SelectState {
    unsigned int hist[256];
    unsigned long long prefix, mask_hi;   // the bytes of the limit-th key decided so far, and the mask that covers them
    unsigned int rank, pad;               // rank of that key among the keys that share the prefix
};

__global__ __launch_bounds__(TB) void select_count_rows_kernel(TableColumns c, int n, SelectArgs a, int* __restrict__ block_counts) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * TB + threadIdx.x;
    int total;
    (void)block_rank(i < n && row_selected(c, i, a), &total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// one block: block_counts[0 .. nblocks) -> exclusive offsets in place, the sum to block_counts[nblocks]
__global__ __launch_bounds__(1024) void block_offsets_kernel(int* __restrict__ block_counts, int nblocks) {
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

void block_offsets_device(int* counts, int nblocks, hipStream_t s) { hipLaunchKernelGGL(block_offsets_kernel, dim3(1), dim3(1024), 0, s, counts, nblocks); }

__global__ __launch_bounds__(TB) void select_emit_keys_kernel(TableColumns c, int n, SelectArgs a, const int* __restrict__ block_offsets,
                                                              uint64_t* __restrict__ keys) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * TB + threadIdx.x;
    const int f = i < n && row_selected(c, i, a);
    int total;
    const int pos = block_rank(f, &total);
    if (f) keys[block_offsets[blockIdx.x] + pos] = order_key(c.response[i], (uint32_t)i);
}

__global__ __launch_bounds__(256) void select_radix_init_kernel(SelectState* __restrict__ st, unsigned int rank) {
    st->hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) st->prefix = 0, st->mask_hi = 0, st->rank = rank, st->pad = 0;
}

// one radix-select pass: histogram of byte `shift/8` over the keys that match the state's prefix on the bits above it
__global__ __launch_bounds__(256) void select_radix_hist_kernel(const uint64_t* __restrict__ keys, int m, int shift, SelectState* __restrict__ st) {
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
__global__ __launch_bounds__(256) void select_radix_decide_kernel(SelectState* __restrict__ st, int shift) {
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
__global__ __launch_bounds__(TB) void select_cut_count_kernel(const uint64_t* __restrict__ keys, int m, const SelectState* __restrict__ st,
                                                              int* __restrict__ block_counts) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * TB + threadIdx.x;
    int total;
    (void)block_rank(i < m && keys[i] <= st->prefix, &total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(TB) void select_cut_compact_kernel(const uint64_t* __restrict__ keys, int m, const SelectState* __restrict__ st,
                                                                const int* __restrict__ block_offsets, int limit, uint64_t* __restrict__ out) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * TB + threadIdx.x;
    const uint64_t k = i < m ? keys[i] : PAD_KEY;
    const int f = i < m && k <= st->prefix;
    int total;
    const int pos = block_offsets[blockIdx.x] + block_rank(f, &total);
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
__global__ __launch_bounds__(SORT_B / 2) void select_block_sort_kernel(const uint64_t* src, int m, uint64_t* dst) {
    APDS_RAISE_WAVE_PRIORITY();
    __shared__ uint64_t s[SORT_B];
    const unsigned int base = blockIdx.x * SORT_B;
    for (unsigned int e = threadIdx.x; e < SORT_B; e += SORT_B / 2) s[e] = base + e < (unsigned int)m ? src[base + e] : PAD_KEY;
    __syncthreads();
    for (unsigned int k = 2; k <= SORT_B; k <<= 1) lds_bitonic_steps(s, base, k, k >> 1);
    for (unsigned int e = threadIdx.x; e < SORT_B; e += SORT_B / 2) dst[base + e] = s[e];
}

// every step of merge stage k (> SORT_B) whose stride is below SORT_B, in one launch
__global__ __launch_bounds__(SORT_B / 2) void select_merge_tail_kernel(uint64_t* __restrict__ keys, unsigned int k) {
    APDS_RAISE_WAVE_PRIORITY();
    __shared__ uint64_t s[SORT_B];
    const unsigned int base = blockIdx.x * SORT_B;
    for (unsigned int e = threadIdx.x; e < SORT_B; e += SORT_B / 2) s[e] = keys[base + e];
    __syncthreads();
    lds_bitonic_steps(s, base, k, SORT_B / 2);
    for (unsigned int e = threadIdx.x; e < SORT_B; e += SORT_B / 2) keys[base + e] = s[e];
}

// one step of stride j >= SORT_B: a thread per pair
__global__ __launch_bounds__(256) void select_merge_step_kernel(uint64_t* __restrict__ keys, unsigned int pairs, unsigned int k, unsigned int j) {
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

// the train side of an L2 screen over a selection of float rows (kernels.h: L2Train), written by the gather; all null on a byte table
struct TrainSideOut {
    float* norms;              // |row|^2, row_norms_kernel's value bit for bit
    uint16_t* rows_bf;         // bf16 of -2 * row, 64 per row
    unsigned int* tmax_bits;   // bits of the largest norm: cleared on the stream in front of the launch
};

// everything a selection holds, in one launch: a lane per dword of a descriptor row (16 lanes per row of a byte table, one whole wave per
// row of a float table: the row is read as one coalesced 256 bytes); lane 0 also writes the keypoint, row id and image id, lanes 1..3 one
// coordinate of the world point each when xyz is asked for.
// A float view (ts.norms != null; a wave per row) also gets its train side here, from the row it holds in registers: the norm is
// row_norms_kernel's at dim 64 - one element per lane squared (its `0 + v * v` is v * v), then the same xor butterfly 32, 16, .., 1 -
// the bf16 value is to_bf16_rows_kernel's at scale -2, and the largest norm max_norm_kernel's (fmaxf from 0 drops a NaN norm as it does).
__global__ __launch_bounds__(256) void select_gather_kernel(const uint64_t* __restrict__ keys, int m, TableColumns c, const double* __restrict__ xyz,
                                                            int* __restrict__ rows, apds_keypoint* __restrict__ kps, int* __restrict__ out_img,
                                                            uint32_t* __restrict__ out_desc, double* __restrict__ out_xyz, TrainSideOut ts) {
    APDS_RAISE_WAVE_PRIORITY();
    const int W = c.row_dwords();
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)m * W) return;   // (a float row: the whole wave leaves together)
    const int i = (int)(t >> c.row_shift), w = (int)(t & (W - 1));
    const uint32_t r = (uint32_t)keys[i];
    const uint32_t bits = c.desc64[(size_t)r * W + w];
    out_desc[(size_t)i * W + w] = bits;
    if (ts.norms) {
        const float v = __uint_as_float(bits);
        float s = v * v;
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        const uint32_t h = f32_to_bf16_rne(v * -2.0f);
        const uint32_t up = (uint32_t)__shfl_down((int)h, 1);
        if ((w & 1) == 0) reinterpret_cast<uint32_t*>(ts.rows_bf)[((size_t)i * 64 + w) >> 1] = h | (up << 16);
        if (w == 0) {
            ts.norms[i] = s;
            // non-negative floats order like their bits. The value only grows, so a row that a relaxed read shows to be no larger has
            // nothing to add: all but a few of a large selection's rows skip the atomic on the one shared word.
            const unsigned int nb = __float_as_uint(fmaxf(0.f, s));
            if (nb > __atomic_load_n(ts.tmax_bits, __ATOMIC_RELAXED)) atomicMax(ts.tmax_bits, nb);
        }
    }
    if (w == 0) {
        rows[i] = (int)r;
        kps[i] = load_keypoint(c, r);
        out_img[i] = c.image_id[r];
    } else if (w <= 3 && xyz) {
        out_xyz[(size_t)i * 3 + (w - 1)] = xyz[(size_t)r * 3 + (w - 1)];
    }
}

__global__ void table_ids_of_rows_kernel(const int* __restrict__ ids, const int* __restrict__ rows, int m, int* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) out[i] = ids[rows[i]];
}

// what a selection over n table rows with a limit works in; nothing in it outlives the call
struct SelectScratch {
    int *block_counts = nullptr, *cut_counts = nullptr;   // ceil(n / TB) + 1 each
    uint64_t *keys = nullptr, *sorted = nullptr;          // n; sort_capacity(min(n, limit))
    SelectState* state = nullptr;
    int* host_count = nullptr;                            // where the count of qualifying rows lands on the host
};
// where a selection of at most `limit` rows lands (device)
struct SelectOutputs {
    int *rows = nullptr, *image_id = nullptr;
    apds_keypoint* kps = nullptr;
    uint8_t* desc64 = nullptr;   // rows of the table's kind: 64 bytes, or 64 floats
    double* xyz = nullptr;       // null: the world points are not gathered
    TrainSideOut train{nullptr, nullptr, nullptr};   // a float view's L2 train side; all null: not written
};

// keys the sort buffer of a selection of at most m rows holds: the power of two that holds them, at least one LDS block
static int64_t sort_capacity(int64_t m) {
    int64_t p2 = SORT_B;
    while (p2 < m) p2 <<= 1;
    return p2;
}

// The rows of t that `a` selects, best response first, at most `limit`, into o; everything on s. The one host synchronisation is the
// count of qualifying rows; the kernels that cut, sort and gather are queued behind it when this returns the row count.
static int select_rows(KeypointTable* t, const SelectArgs& a, int limit, hipStream_t s, const SelectScratch& w, const SelectOutputs& o) {
    const int n = (int)t->n;
    if (!n) return 0;
    const TableColumns c = columns_of(t);
    const int nb = ceil_div(n, TB);
    hipLaunchKernelGGL(select_count_rows_kernel, dim3(nb), dim3(TB), 0, s, c, n, a, w.block_counts);
    block_offsets_device(w.block_counts, nb, s);
    HIP_CHECK(hipMemcpyAsync(w.host_count, w.block_counts + nb, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    int m = *w.host_count;
    if (!m) return 0;
    hipLaunchKernelGGL(select_emit_keys_kernel, dim3(nb), dim3(TB), 0, s, c, n, a, (const int*)w.block_counts, w.keys);
    const uint64_t* unsorted = w.keys;
    if (m > limit) {
        // radix select of the limit-th smallest key, most significant byte first; each byte's bucket is decided on the device
        hipLaunchKernelGGL(select_radix_init_kernel, dim3(1), dim3(256), 0, s, w.state, (unsigned int)(limit - 1));
        for (int shift = 56; shift >= 0; shift -= 8) {
            hipLaunchKernelGGL(select_radix_hist_kernel, dim3(256), dim3(256), 0, s, (const uint64_t*)w.keys, m, shift, w.state);
            hipLaunchKernelGGL(select_radix_decide_kernel, dim3(1), dim3(256), 0, s, w.state, shift);
        }
        const int mb = ceil_div(m, TB);
        hipLaunchKernelGGL(select_cut_count_kernel, dim3(mb), dim3(TB), 0, s, (const uint64_t*)w.keys, m, (const SelectState*)w.state, w.cut_counts);
        block_offsets_device(w.cut_counts, mb, s);
        hipLaunchKernelGGL(select_cut_compact_kernel, dim3(mb), dim3(TB), 0, s, (const uint64_t*)w.keys, m, (const SelectState*)w.state,
                           (const int*)w.cut_counts, limit, w.sorted);
        unsorted = w.sorted;
        m = limit;
    }
    // bitonic sort of the m surviving keys, padded to p2 (a power of two, at least one block) with keys above every real one
    const unsigned int p2 = (unsigned int)sort_capacity(m);
    hipLaunchKernelGGL(select_block_sort_kernel, dim3(p2 / SORT_B), dim3(SORT_B / 2), 0, s, unsorted, m, w.sorted);
    for (unsigned int k = 2 * SORT_B; k <= p2; k <<= 1) {
        for (unsigned int j = k >> 1; j >= (unsigned int)SORT_B; j >>= 1)
            hipLaunchKernelGGL(select_merge_step_kernel, dim3(p2 / 2 / 256), dim3(256), 0, s, w.sorted, p2 / 2, k, j);
        hipLaunchKernelGGL(select_merge_tail_kernel, dim3(p2 / SORT_B), dim3(SORT_B / 2), 0, s, w.sorted, k);
    }
    if (o.train.norms) HIP_CHECK(hipMemsetAsync(o.train.tmax_bits, 0, 16, s));
    KernelTimer timer("db_select_gather", s);   // (apds_dev_last_kernel_ms; free unless timing is on)
    hipLaunchKernelGGL(select_gather_kernel, dim3(ceil_div((long long)m * t->row_dwords, 256)), dim3(256), 0, s, (const uint64_t*)w.sorted, m, c,
                       (const double*)(o.xyz ? t->xyz : nullptr), o.rows, o.kps, o.image_id, reinterpret_cast<uint32_t*>(o.desc64), o.xyz, o.train);
    HIP_CHECK(hipGetLastError());
    return m;
}

// A view of one table: the outputs of a selection and all the scratch it takes, sized by the table's capacity and allocated once
// (apds_db_view_create).
struct TableView {
    KeypointTable* t = nullptr;
    int limit = 0, n = 0;
    bool has_xyz = false;
    SelectScratch scratch;   // host_count: pinned
    SelectOutputs out;       // xyz always allocated; a selection without world points does not write it
    // a float table's view: the train side of the current selection as the handle apds_dev_l2_train_top2 takes (apds_db_view_l2_train).
    // rows = out.desc64 and the three buffers of out.train, all allocated at create for `limit` rows; n and screen_ready follow each select.
    L2Train train;
};

}  // namespace apds

using namespace apds;

namespace {
void view_free(TableView* v) {
    const SelectScratch& w = v->scratch;
    const SelectOutputs& o = v->out;
    for (void* p : {(void*)w.block_counts, (void*)w.cut_counts, (void*)w.keys, (void*)w.sorted, (void*)w.state, (void*)o.rows, (void*)o.image_id,
                    (void*)o.kps, (void*)o.desc64, (void*)o.xyz, (void*)o.train.norms, (void*)o.train.rows_bf, (void*)o.train.tmax_bits})
        if (p) (void)hipFree(p);
    if (w.host_count) (void)hipHostFree(w.host_count);
    delete v;
}
}  // namespace

extern "C" {

// Result (ordered by response desc, at most 262143 rows) stays on the device as the table's current view; *n_out is its row count.
// The scratch is the thread's workspace, sized by the table's rows: what a select of every row has always taken there.
int apds_db_select(void* db, int mode, int value, float x_start, float y_start, float x_end, float y_end, int* n_out) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t && n_out && mode >= 0 && mode <= 2, APDS_ERR_BAD_ARG, "bad argument");
        *n_out = 0;
        t->view_n = 0;
        if (!t->n) return;
        ThreadCtx& c = ctx();
        c.ws_reset();
        hipStream_t s = c.stream;
        const int limit = (int)std::min<int64_t>(APDS_MAX_POINTS, t->view_cap);
        const size_t nblocks = (size_t)ceil_div(t->n, TB) + 1;
        int count = 0;
        SelectScratch w;   // (every workspace request is 256-byte aligned: the keys and the state need 8)
        w.keys = c.alloc_n<uint64_t>((size_t)t->n);
        w.sorted = c.alloc_n<uint64_t>((size_t)sort_capacity(std::min<int64_t>(t->n, limit)));
        w.state = c.alloc_n<SelectState>(1);
        w.block_counts = c.alloc_n<int>(nblocks);
        w.cut_counts = c.alloc_n<int>(nblocks);
        w.host_count = &count;
        const int m = select_rows(t, select_args(mode, value, x_start, y_start, x_end, y_end), limit, s, w,
                                  SelectOutputs{t->view_rows, t->view_image_id, t->view_kps, t->view_desc64, nullptr, {}});
        if (!m) return;
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
        require_table_kind(t, false);
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

// apds_l2_knn_match of host query rows (64 floats each) against the CURRENT VIEW of a float table: the exact kernel over the view's rows
int apds_db_l2_knn_match(void* db, const float* query, int n_query, int k, int32_t* idx, float* dist) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t && idx && dist && n_query >= 0 && (query || !n_query), APDS_ERR_BAD_ARG, "bad argument");
        require_table_kind(t, true);
        APDS_REQUIRE(k >= 1, APDS_ERR_ASSERT, "bad sizes");
        APDS_REQUIRE(k <= 2, APDS_ERR_ASSERT, "k > 2 is not implemented");
        if (!n_query) return;
        if (!t->view_n) {
            for (long long i = 0; i < (long long)n_query * k; i++) idx[i] = -1, dist[i] = INFINITY;
            return;
        }
        ThreadCtx& c = ctx();
        require_table_device(t);
        c.ws_reset();
        hipStream_t s = c.stream;
        float* dq = c.alloc_n<float>((size_t)n_query * APDS_DESC_FLOAT_DIM);
        uint64_t* keys = c.alloc_n<uint64_t>((size_t)n_query * k);
        HIP_CHECK(hipMemcpyAsync(dq, query, (size_t)n_query * APDS_DESC_FLOAT_DIM * sizeof(float), hipMemcpyHostToDevice, s));
        l2_topk_device(dq, n_query, reinterpret_cast<const float*>(t->view_desc64), t->view_n, APDS_DESC_FLOAT_DIM, 0, k, keys, s);
        std::vector<uint64_t> h((size_t)n_query * k);
        HIP_CHECK(hipMemcpyAsync(h.data(), keys, h.size() * 8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        for (size_t i = 0; i < h.size(); i++) {
            if (h[i] == EMPTY_KEY) idx[i] = -1, dist[i] = INFINITY;
            else {
                const uint32_t d2_bits = (uint32_t)(h[i] >> 32);
                float d2;
                memcpy(&d2, &d2_bits, sizeof(d2));
                idx[i] = (int32_t)(uint32_t)h[i];
                dist[i] = sqrtf(d2);   // BFMatcher(NORM_L2) reports the distance, not its square
            }
        }
    });
}

namespace {
// both downloads of the current view: desc receives host_row bytes of every row (61 of a byte row, 256 of a float row)
int view_download(void* db, bool want_float, apds_keypoint* kps, void* desc, int32_t* ids, int32_t* image_ids) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t, APDS_ERR_BAD_ARG, "null table");
        require_table_kind(t, want_float);
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
        if (desc && want_float) {
            HIP_CHECK(hipMemcpyAsync(desc, t->view_desc64, (size_t)m * t->row_bytes(), hipMemcpyDeviceToHost, s));
        } else if (desc) {
            uint8_t* d61 = c.alloc_n<uint8_t>((size_t)m * 61);
            HIP_CHECK(hipMemcpy2DAsync(d61, 61, t->view_desc64, 64, 61, m, hipMemcpyDeviceToDevice, s));
            HIP_CHECK(hipMemcpyAsync(desc, d61, (size_t)m * 61, hipMemcpyDeviceToHost, s));
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}
}  // namespace

// host copy of the current view: what the reference's Vec<models::Keypoint> holds (id: the table's id column, a SERIAL column's values:
// row + 1 on a table that never saw a delete)
int apds_db_view_download(void* db, apds_keypoint* kps, uint8_t* desc61, int32_t* ids, int32_t* image_ids) {
    return view_download(db, false, kps, desc61, ids, image_ids);
}

int apds_db_view_download_float(void* db, apds_keypoint* kps, float* desc64f, int32_t* ids, int32_t* image_ids) {
    return view_download(db, true, kps, desc64f, ids, image_ids);
}

// ---- view objects: keypointdb.rs:50-90 once per frame, on the caller's stream ------------------------------------------------------
int apds_db_view_create(void* db, int capacity, void** view) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t && view, APDS_ERR_BAD_ARG, "null argument");
        *view = nullptr;
        require_table_device(t);
        TableView* v = new TableView();
        v->t = t;
        v->train.borrowed = true;
        v->limit = (int)(capacity <= 0 ? std::min<int64_t>(APDS_MAX_POINTS, t->capacity) : std::min<int64_t>(capacity, APDS_MAX_POINTS));
        const size_t nblocks = (size_t)ceil_div(t->capacity, TB) + 1, lim = (size_t)v->limit;
        SelectScratch& w = v->scratch;
        SelectOutputs& o = v->out;
        try {
            dev_alloc(w.block_counts, nblocks); dev_alloc(w.cut_counts, nblocks);
            dev_alloc(w.keys, (size_t)t->capacity); dev_alloc(w.sorted, (size_t)sort_capacity(v->limit));
            dev_alloc(w.state, 1);
            dev_alloc(o.rows, lim); dev_alloc(o.image_id, lim); dev_alloc(o.kps, lim); dev_alloc(o.desc64, lim * t->row_bytes()); dev_alloc(o.xyz, lim * 3);
            if (t->is_float()) {
                dev_alloc(o.train.norms, lim); dev_alloc(o.train.rows_bf, lim * APDS_DESC_FLOAT_DIM); dev_alloc(o.train.tmax_bits, 4);
                v->train.device = t->device;
                v->train.rows = reinterpret_cast<const float*>(o.desc64);
                v->train.dim = APDS_DESC_FLOAT_DIM;
                v->train.norms = o.train.norms;
                v->train.rows_bf = o.train.rows_bf;
                v->train.tmax_bits = o.train.tmax_bits;
            }
            HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&w.host_count), sizeof(int), hipHostMallocDefault));
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
        require_table_device(t);
        hipStream_t s = pick_stream(stream);
        v->n = 0;
        v->has_xyz = false;
        v->train.n = 0;
        v->train.screen_ready = false;
        SelectOutputs o = v->out;
        if (!with_xyz) o.xyz = nullptr;
        const int m = select_rows(t, select_args(mode, value, x_start, y_start, x_end, y_end), v->limit, s, v->scratch, o);
        v->n = m;
        v->train.n = m;
        v->train.screen_ready = t->is_float() && m >= 2;   // (what l2_train_create asks of a handle: dim 64, rows from hipMalloc, two rows)
        v->has_xyz = m && with_xyz;
        *n_out = m;
    });
}

// device pointers of the view's last selection (*xyz_dev: NULL unless it ran with_xyz)
int apds_db_view_pointers(const void* view, void** rows64_dev, void** kps_dev, void** row_ids_dev, void** image_ids_dev, void** xyz_dev, int* n) {
    return guarded([&] {
        const TableView* v = static_cast<const TableView*>(view);
        APDS_REQUIRE(v, APDS_ERR_BAD_ARG, "null view");
        if (rows64_dev) *rows64_dev = v->out.desc64;
        if (kps_dev) *kps_dev = v->out.kps;
        if (row_ids_dev) *row_ids_dev = v->out.rows;
        if (image_ids_dev) *image_ids_dev = v->out.image_id;
        if (xyz_dev) *xyz_dev = v->has_xyz ? v->out.xyz : nullptr;
        if (n) *n = v->n;
    });
}

// The train side of a float view's current selection as an L2 train set: borrowed (never apds_l2_train_destroy), valid until the view is
// destroyed, contents those of the last select once its stream has run. Index base 0: a key's row is the position in the view.
int apds_db_view_l2_train(void* view, void** set) {
    return guarded([&] {
        TableView* v = static_cast<TableView*>(view);
        APDS_REQUIRE(v && set, APDS_ERR_BAD_ARG, "null argument");
        *set = nullptr;
        require_table_kind(v->t, true);
        *set = &v->train;
    });
}

}  // extern "C"
