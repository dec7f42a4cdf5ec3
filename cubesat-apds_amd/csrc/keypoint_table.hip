// csrc/keypoint_table.hip — GPU-resident keypoint table: what fills the descriptor database the matcher scans
// (SURVEY §8f-1). Mirrors the reference's `keypoint` table and its access paths, without Postgres:
//   insert  : preprocessor/src/main.rs:296-324 (to_db_type + level-of-detail rescale of x,y, one INSERT per tile)
//   read    : feature_database/src/keypointdb.rs:28-90 - by id here; the ordered, limited selections in keypoint_select.hip
//   delete  : keypointdb.rs:92-97, in keypoint_delete.hip
// Columns are stored SoA (coalesced predicate scans); descriptors as 64-byte rows, i.e. already in the layout the
// Hamming kernel streams - or, on a float table (apds_db_create_float), as rows of 64 floats, the layout the L2 matchers read. The kind
// is fixed at create; the kernels receive the row width with the columns. The table, its columns and what the three sources share:
// keypoint_table.h.
#include <cstring>
#include <vector>

#include "keypoint_table.h"

namespace apds {

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

// The same rows from the device buffers an extraction has written (28-byte keypoints, descriptor rows of the table's kind: 64 bytes or
// 64 floats; tile i at i * capacity rows), every tile of a batch in one launch: a lane per dword of a table row (16 or 64 of them).
// tile_offsets[i] = rows of the tiles < i (tile_offsets[n_tiles] = all rows), copied to LDS; a row group finds its tile by binary search
// (empty tiles repeat an offset: the last tile whose offset is <= the row is the one that holds it). tile_xy_off[i] = that tile's
// (xoff, yoff). Bytes 61-63 of a 64-byte source row are not trusted: word 15 keeps byte 60 alone. A float row is stored whole.
__global__ __launch_bounds__(256) void table_insert_dev_kernel(const apds_keypoint* __restrict__ kps, const uint32_t* __restrict__ desc_src, int n_tiles,
                                                               int capacity, const int* __restrict__ tile_offsets, const float2* __restrict__ tile_xy_off,
                                                               int first_image_id, int lod, float scale, long long base, int first_id, TableColumns c) {
    APDS_RAISE_WAVE_PRIORITY();
    extern __shared__ int offs[];   // n_tiles + 1
    for (int i = threadIdx.x; i <= n_tiles; i += blockDim.x) offs[i] = tile_offsets[i];
    __syncthreads();
    const int W = c.row_dwords();
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)offs[n_tiles] * W) return;
    const int r = (int)(t >> c.row_shift), w = (int)(t & (W - 1));
    int lo = 0, hi = n_tiles - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offs[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    const long long src = (long long)lo * capacity + (r - offs[lo]);
    uint32_t v = desc_src[src * W + w];
    if (W == 16 && w == 15) v &= 0xFFu;
    c.desc64[(base + r) * W + w] = v;
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
    out[r] = load_keypoint(c, r);
}

struct FoundRow {
    long long row;   // -1: no row has the id
    apds_keypoint kp;
    int image_id;
    uint32_t desc[64];   // the row's dwords: the first 16 of a byte table, all 64 of a float table
};

// one wave: lane 0 searches the id column, a lane per dword copies the descriptor row
__global__ __launch_bounds__(64) void table_read_id_kernel(TableColumns c, long long n, int id, FoundRow* __restrict__ out) {
    __shared__ long long found;
    if (threadIdx.x == 0) found = find_id_row(c.id, n, id);
    __syncthreads();
    const long long r = found;
    if (threadIdx.x == 0) out->row = r;
    if (r < 0) return;
    const int W = c.row_dwords();
    if ((int)threadIdx.x < W) out->desc[threadIdx.x] = c.desc64[r * W + threadIdx.x];
    if (threadIdx.x == 0) {
        out->kp = load_keypoint(c, r);
        out->image_id = c.image_id[r];
    }
}

}  // namespace apds

using namespace apds;

namespace {
void table_free(KeypointTable* t) {
    for (void* p : {(void*)t->x, (void*)t->y, (void*)t->size, (void*)t->angle, (void*)t->response, (void*)t->octave, (void*)t->class_id,
                    (void*)t->image_id, (void*)t->lod, (void*)t->desc64, (void*)t->view_rows, (void*)t->view_kps, (void*)t->view_image_id,
                    (void*)t->view_desc64, (void*)t->all_kps, (void*)t->xyz, (void*)t->id, (void*)t->stage})
        if (p) (void)hipFree(p);
    delete t;
}
float lift_offset(uint64_t index, uint64_t tile, int lod) { return (float)(index * tile * (1ull << lod)); }   // (u64 product) as f32
}  // namespace

namespace apds {

int table_device(const void* db) {
    APDS_REQUIRE(db, APDS_ERR_BAD_ARG, "null table");
    return static_cast<const KeypointTable*>(db)->device;
}

// n_tiles tiles of an extraction's device output appended in tile order by one launch on s; the small tile table comes from the calling
// thread's workspace (no ws_reset here: the extraction's buffers may live there). Everything is checked before anything is written.
// Synchronises s.
// (Index: u32 for the batch entries, u64 for apds_db_insert_image_float's one tile, which takes the column and row apds_db_insert_image takes)
template <class Index>
static void table_insert_tiles(KeypointTable* t, const void* kps_dev, const void* desc64_dev, int n_tiles, int capacity, const int32_t* counts, int first_image_id,
                               int lod, const Index* columns_rows, uint64_t tile_w, uint64_t tile_h, hipStream_t s) {
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
    hipLaunchKernelGGL(table_insert_dev_kernel, dim3(ceil_div(total * t->row_dwords, 256)), dim3(256), ((size_t)n_tiles + 1) * sizeof(int), s,
                       static_cast<const apds_keypoint*>(kps_dev), static_cast<const uint32_t*>(desc64_dev), n_tiles, capacity, (const int*)dtab,
                       reinterpret_cast<const float2*>(dtab + xy_at), first_image_id, lod, ldexpf(1.0f, lod), (long long)t->n, (int)t->next_id, columns_of(t));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
    t->n += total;
    t->next_id += total;
}

void table_insert_batch_device(void* db, const void* kps_dev, const void* desc64_dev, int n_tiles, int capacity, const int32_t* counts, int first_image_id,
                               int lod, const uint32_t* columns_rows, uint64_t tile_w, uint64_t tile_h, hipStream_t s) {
    table_insert_tiles(static_cast<KeypointTable*>(db), kps_dev, desc64_dev, n_tiles, capacity, counts, first_image_id, lod, columns_rows, tile_w, tile_h, s);
}

int table_descriptor(const void* db) {
    APDS_REQUIRE(db, APDS_ERR_BAD_ARG, "null table");
    return static_cast<const KeypointTable*>(db)->is_float() ? APDS_AKAZE_DESCRIPTOR_KAZE : APDS_AKAZE_DESCRIPTOR_MLDB;
}

}  // namespace apds

extern "C" {

namespace {
int table_create(void** db, int64_t capacity, int row_dwords) {
    return guarded([&] {
        APDS_REQUIRE(db && capacity > 0 && capacity < (1ll << 31), APDS_ERR_BAD_ARG, "bad capacity");
        ThreadCtx& c = ctx();
        KeypointTable* t = new KeypointTable();
        t->device = c.device;
        t->capacity = capacity;
        t->row_dwords = row_dwords;
        try {
            dev_alloc(t->x, capacity); dev_alloc(t->y, capacity); dev_alloc(t->size, capacity); dev_alloc(t->angle, capacity);
            dev_alloc(t->response, capacity); dev_alloc(t->octave, capacity); dev_alloc(t->class_id, capacity);
            dev_alloc(t->image_id, capacity); dev_alloc(t->lod, capacity); dev_alloc(t->desc64, (size_t)capacity * t->row_bytes());
            dev_alloc(t->id, capacity);
            t->view_cap = std::min<int64_t>(capacity, APDS_MAX_POINTS);
            dev_alloc(t->view_rows, t->view_cap); dev_alloc(t->view_kps, t->view_cap); dev_alloc(t->view_image_id, t->view_cap);
            dev_alloc(t->view_desc64, (size_t)t->view_cap * t->row_bytes());
        } catch (...) {
            table_free(t);
            throw;
        }
        *db = t;
    });
}
}  // namespace

int apds_db_create(void** db, int64_t capacity) { return table_create(db, capacity, 16); }

// the same table with a descriptor column of 64 x f32 (M-SURF rows, APDS_AKAZE_DESCRIPTOR_KAZE)
int apds_db_create_float(void** db, int64_t capacity) { return table_create(db, capacity, APDS_DESC_FLOAT_DIM); }

int apds_db_info(const void* db, int* descriptor, int* row_bytes) {
    return guarded([&] {
        const KeypointTable* t = static_cast<const KeypointTable*>(db);
        APDS_REQUIRE(t, APDS_ERR_BAD_ARG, "null table");
        if (descriptor) *descriptor = table_descriptor(t);
        if (row_bytes) *row_bytes = (int)t->row_bytes();
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
        require_table_kind(t, false);
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

// The float table's host insert: n rows of 64 floats. The rows are uploaded as they are and go through the device insert's launch, so a
// row reaches the table by one path whichever side it comes from.
int apds_db_insert_image_float(void* db, const apds_keypoint* kps, const float* desc64f, int n, int image_id, int lod, uint64_t column, uint64_t row,
                               uint64_t tile_w, uint64_t tile_h) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t && n >= 0 && lod >= 0 && lod < 31, APDS_ERR_BAD_ARG, "bad argument");
        require_table_kind(t, true);
        APDS_REQUIRE(t->n + n <= t->capacity, APDS_ERR_NOMEM, "keypoint table is full");
        APDS_REQUIRE(t->next_id + n <= (1ll << 31), APDS_ERR_NOMEM, "keypoint table has given out every 32-bit id");
        if (!n) return;
        APDS_REQUIRE(kps && desc64f, APDS_ERR_BAD_ARG, "null argument");
        ThreadCtx& c = ctx();
        c.ws_reset();
        hipStream_t s = c.stream;
        apds_keypoint* dk = c.alloc_n<apds_keypoint>(n);
        float* dd = c.alloc_n<float>((size_t)n * APDS_DESC_FLOAT_DIM);
        HIP_CHECK(hipMemcpyAsync(dk, kps, (size_t)n * sizeof(apds_keypoint), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(dd, desc64f, (size_t)n * APDS_DESC_FLOAT_DIM * sizeof(float), hipMemcpyHostToDevice, s));
        const int32_t counts[1] = {n};
        const uint64_t cr[2] = {column, row};
        table_insert_tiles(t, dk, dd, 1, n, counts, image_id, lod, cr, tile_w, tile_h, s);
    });
}

// the same rows from what apds_dev_akaze_extract has written on the device (no upload, no repack): one tile, then a batch of them
// (a float table: from what apds_dev_akaze_extract_float has written)
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
        require_table_device(t);
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
            require_table_device(t);
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

// ---- ids: keypointdb.rs:28-36 (read_keypoint_from_id) -------------------------------------------------------------------------------
int apds_db_ids(void* db, void** ids_dev) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t && ids_dev, APDS_ERR_BAD_ARG, "null argument");
        *ids_dev = t->id;
    });
}

namespace {
// both reads by id: desc receives desc_bytes of the row (61 of a byte row, 256 of a float row)
int table_read_id(void* db, bool want_float, int id, apds_keypoint* kp, void* desc, size_t desc_bytes, int* image_id, int64_t* row) {
    return guarded([&] {
        KeypointTable* t = static_cast<KeypointTable*>(db);
        APDS_REQUIRE(t, APDS_ERR_BAD_ARG, "null table");
        require_table_kind(t, want_float);
        APDS_REQUIRE(t->n > 0 && id >= 1, APDS_ERR_OUT_OF_RANGE, "no keypoint has this id");
        ThreadCtx& c = ctx();
        require_table_device(t);
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
        if (desc) memcpy(desc, h.desc, desc_bytes);
        if (image_id) *image_id = h.image_id;
        if (row) *row = h.row;
    });
}
}  // namespace

int apds_db_read_keypoint_from_id(void* db, int id, apds_keypoint* kp, uint8_t* desc61, int* image_id, int64_t* row) {
    return table_read_id(db, false, id, kp, desc61, APDS_DESC_BYTES, image_id, row);
}

int apds_db_read_keypoint_from_id_float(void* db, int id, apds_keypoint* kp, float* desc64f, int* image_id, int64_t* row) {
    return table_read_id(db, true, id, kp, desc64f, APDS_DESC_FLOAT_DIM * sizeof(float), image_id, row);
}

}  // extern "C"
