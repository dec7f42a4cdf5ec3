// csrc/akaze_mask_sat.hip — the zero-count summed-area table of a detection mask on gfx950: S[y][x] = the number of zero mask bytes in
// rows < y and columns < x, (rows + 1) x (cols + 1) u32, exact (a side is < 65536, so a count is < 2^32). With it "is there a masked pixel
// in this square?" is four reads (akaze_compact.hip: masked_out), whatever the square's size - what the mask support of
// apds_akaze_extract_masked_support needs, where a keypoint's square depends on its level.
//
// Two launches, no atomics, the mask read once:
//   1. sat_rows_kernel: a wave per table row. A lane takes 16 consecutive mask bytes (one 16-byte load from a plane, four from the alpha
//      bytes of a BGRA image), counts their zeros, the wave scans the 64 lane totals, and a carry runs over the row's 1024-pixel chunks.
//      The 1024 prefixes go through the wave's own LDS rows so that the stores are lane-consecutive. Row 0 and column 0 are zeros.
//   2. sat_cols_kernel: the column prefix in place. A block owns 32 columns and walks the rows in chunks of 256: 32 segments of 8 rows, a
//      thread per (column, segment), the segment totals through LDS, a carry per column from chunk to chunk.
// Any PixelMask layout (common.h): a plane with any row stride, any pixel stride, a batch (img_stride) or one mask for all (one table).
#include "akaze.h"

namespace apds {

namespace {

constexpr int SAT_LANE_PX = 16;                          // mask bytes a lane takes per chunk
constexpr int SAT_WAVE_PX = 64 * SAT_LANE_PX;            // pixels of a row a wave takes per chunk
constexpr int SAT_ROW_WAVES = 4;                         // rows (waves) per block of the row pass
constexpr int SAT_LDS_PITCH = SAT_LANE_PX + 1;           // a lane's 16 prefixes + one pad word: ds_write_b32 of lane l, word j hits bank (17 l + j) % 32
constexpr int SAT_COLS = 32, SAT_SEGS = 32, SAT_SEG_ROWS = 8;   // the column pass: 32 x 32 threads, 8 rows each = chunks of 256 rows

__device__ __forceinline__ uint32_t is_zero_byte(uint32_t word, int shift) { return ((word >> shift) & 0xFFu) == 0 ? 1u : 0u; }

// z[j] = 1 iff pixel x0 + j of the row at `row` is masked (its byte is zero); pixels at or past `cols` count as unmasked
__device__ __forceinline__ void load_zero_flags(const uint8_t* __restrict__ row, size_t pix_stride, int x0, int cols, uint32_t (&z)[SAT_LANE_PX]) {
    if (x0 + SAT_LANE_PX <= cols && pix_stride == 1) {
        uint32_t w[4];
        __builtin_memcpy(w, row + x0, 16);   // (any alignment: a row of a strided plane starts anywhere)
#pragma unroll
        for (int j = 0; j < SAT_LANE_PX; j++) z[j] = is_zero_byte(w[j >> 2], 8 * (j & 3));
    } else if (x0 + SAT_LANE_PX <= cols && pix_stride == 4) {
        // the aligned dword that holds each byte (for the alpha of a BGRA image: the pixel itself), 64 bytes per lane
        const uint8_t* __restrict__ p = row + (size_t)x0 * 4;
        const int byte = (int)(reinterpret_cast<uintptr_t>(p) & 3);
        const int shift = 8 * byte;
        uint32_t w[SAT_LANE_PX];
        __builtin_memcpy(w, p - byte, 64);
#pragma unroll
        for (int j = 0; j < SAT_LANE_PX; j++) z[j] = is_zero_byte(w[j], shift);
    } else {
#pragma unroll
        for (int j = 0; j < SAT_LANE_PX; j++) z[j] = x0 + j < cols && row[(size_t)(x0 + j) * pix_stride] == 0 ? 1u : 0u;
    }
}

// Table row r of image blockIdx.z: zeros for r == 0, else column 0 = 0 and S[r][x + 1] = the zero bytes of mask row r - 1 in columns <= x
__global__ __launch_bounds__(64 * SAT_ROW_WAVES) void sat_rows_kernel(PixelMask M, uint32_t* __restrict__ sat, size_t sat_img_stride) {
    __shared__ uint32_t lds[SAT_ROW_WAVES][64 * SAT_LDS_PITCH];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = blockIdx.x * SAT_ROW_WAVES + wv;
    const bool live = r <= M.rows;                                      // (wave-uniform; dead waves only keep the block's barriers)
    const int pitch = M.cols + 1;
    uint32_t* __restrict__ out = sat + (size_t)blockIdx.z * sat_img_stride + (size_t)(live ? r : 0) * pitch;
    const uint8_t* __restrict__ row = M.base + (size_t)blockIdx.z * M.img_stride + (size_t)(r >= 1 && live ? r - 1 : 0) * M.row_stride;
    if (live && lane == 0) out[0] = 0;
    uint32_t carry = 0;
    for (int c0 = 0; c0 < M.cols; c0 += SAT_WAVE_PX) {
        const int x0 = c0 + lane * SAT_LANE_PX;
        uint32_t z[SAT_LANE_PX];
#pragma unroll
        for (int j = 0; j < SAT_LANE_PX; j++) z[j] = 0;
        if (live && r >= 1 && x0 < M.cols) load_zero_flags(row, M.pix_stride, x0, M.cols, z);
#pragma unroll
        for (int j = 1; j < SAT_LANE_PX; j++) z[j] += z[j - 1];          // inclusive inside the lane
        uint32_t incl = z[SAT_LANE_PX - 1];                              // inclusive over the wave's lanes
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const uint32_t before = carry + incl - z[SAT_LANE_PX - 1];      // zeros of the row in front of this lane's pixels
#pragma unroll
        for (int j = 0; j < SAT_LANE_PX; j++) lds[wv][lane * SAT_LDS_PITCH + j] = before + z[j];
        carry += __shfl(incl, 63);
        __syncthreads();
        if (live) {
#pragma unroll
            for (int k = 0; k < SAT_LANE_PX; k++) {
                const int i = k * 64 + lane;                             // pixel c0 + i: word i + i / 16 of the padded rows
                if (c0 + i < M.cols) out[1 + c0 + i] = lds[wv][i + (i >> 4)];
            }
        }
        __syncthreads();
    }
}

// In place: S[r][c] <- the sum of S[1 .. r][c], for columns 1 .. cols (row 0 and column 0 hold zeros already)
__global__ __launch_bounds__(SAT_COLS * SAT_SEGS) void sat_cols_kernel(uint32_t* __restrict__ sat, size_t sat_img_stride, int rows, int cols) {
    __shared__ uint32_t tot[SAT_SEGS][SAT_COLS];
    const int cx = threadIdx.x % SAT_COLS, seg = threadIdx.x / SAT_COLS;
    const int c = 1 + blockIdx.x * SAT_COLS + cx;
    const bool col_ok = c <= cols;
    const size_t pitch = (size_t)cols + 1;
    uint32_t* __restrict__ S = sat + (size_t)blockIdx.z * sat_img_stride + (col_ok ? c : 0);
    constexpr int CHUNK = SAT_SEGS * SAT_SEG_ROWS;
    uint32_t carry = 0;
    uint32_t nxt[SAT_SEG_ROWS];
#pragma unroll
    for (int k = 0; k < SAT_SEG_ROWS; k++) {
        const int r = 1 + seg * SAT_SEG_ROWS + k;
        nxt[k] = col_ok && r <= rows ? S[(size_t)r * pitch] : 0u;
    }
    for (int r0 = 1; r0 <= rows; r0 += CHUNK) {
        uint32_t v[SAT_SEG_ROWS];
#pragma unroll
        for (int k = 0; k < SAT_SEG_ROWS; k++) v[k] = nxt[k];
        // the next chunk's rows are on their way while this one is summed (nobody writes them before this thread does)
#pragma unroll
        for (int k = 0; k < SAT_SEG_ROWS; k++) {
            const int r = r0 + CHUNK + seg * SAT_SEG_ROWS + k;
            nxt[k] = col_ok && r <= rows ? S[(size_t)r * pitch] : 0u;
        }
#pragma unroll
        for (int k = 1; k < SAT_SEG_ROWS; k++) v[k] += v[k - 1];
        tot[seg][cx] = v[SAT_SEG_ROWS - 1];
        __syncthreads();
        uint32_t above = carry, all = 0;
#pragma unroll
        for (int q = 0; q < SAT_SEGS; q++) {
            const uint32_t t = tot[q][cx];
            above += q < seg ? t : 0u;
            all += t;
        }
        carry += all;
#pragma unroll
        for (int k = 0; k < SAT_SEG_ROWS; k++) {
            const int r = r0 + seg * SAT_SEG_ROWS + k;
            if (col_ok && r <= rows) S[(size_t)r * pitch] = above + v[k];
        }
        __syncthreads();
    }
}

}  // namespace

size_t mask_zero_sat_elems(int rows, int cols) { return ((size_t)rows + 1) * ((size_t)cols + 1); }

// The tables of `n_tables` masks (image i's mask M.img_stride bytes after image i - 1's) to sat + i * sat_img_stride (elements)
void mask_zero_sat_device(const PixelMask& M, int n_tables, uint32_t* sat, size_t sat_img_stride, hipStream_t s) {
    APDS_REQUIRE(M.base && sat, APDS_ERR_BAD_ARG, "null mask or table");
    APDS_REQUIRE(M.rows >= 1 && M.cols >= 1 && M.rows < 65536 && M.cols < 65536, APDS_ERR_ASSERT, "mask side must be 1 .. 65535");
    APDS_REQUIRE(M.pix_stride >= 1 && M.row_stride >= (size_t)(M.cols - 1) * M.pix_stride + 1, APDS_ERR_ASSERT, "mask row stride smaller than a row");
    APDS_REQUIRE(n_tables >= 1 && n_tables <= 65535, APDS_ERR_BAD_ARG, "1 .. 65535 tables");
    APDS_REQUIRE(n_tables == 1 || sat_img_stride >= mask_zero_sat_elems(M.rows, M.cols), APDS_ERR_ASSERT, "table stride smaller than a table");
    hipLaunchKernelGGL(sat_rows_kernel, dim3(ceil_div(M.rows + 1, SAT_ROW_WAVES), 1, n_tables), dim3(64 * SAT_ROW_WAVES), 0, s, M, sat, sat_img_stride);
    hipLaunchKernelGGL(sat_cols_kernel, dim3(ceil_div(M.cols, SAT_COLS), 1, n_tables), dim3(SAT_COLS * SAT_SEGS), 0, s, sat, sat_img_stride, M.rows, M.cols);
    HIP_CHECK(hipGetLastError());
}

}  // namespace apds
