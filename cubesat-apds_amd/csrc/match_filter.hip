// csrc/match_filter.hip — what follows a finished match (feature_extraction/src/lib.rs:104-126): the ratio test on the two nearest, the
// cross-check of a roles-swapped top-1, and the ordered compaction both end in - matches leave in query order, as BFMatcher's do.
#include "kernels.h"
#include "topk_keys.h"

namespace apds {

__global__ void ratio_flag_kernel(const uint64_t* __restrict__ keys, int nq, int K, float fs, uint8_t* __restrict__ flags) {
    APDS_RAISE_WAVE_PRIORITY();
    const int qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    const uint64_t k0 = keys[(size_t)qi * K], k1 = keys[(size_t)qi * K + 1];
    const float d0 = (float)(uint32_t)(k0 >> 32), d1 = (float)(uint32_t)(k1 >> 32);
    flags[qi] = (k0 != EMPTY_KEY && k1 != EMPTY_KEY && d0 < d1 * fs) ? 1 : 0;
}

__global__ void crosscheck_scatter_kernel(const uint64_t* __restrict__ train_best, long long n_train, unsigned long long* __restrict__ best_per_query) {
    APDS_RAISE_WAVE_PRIORITY();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_train) return;
    const uint64_t key = train_best[i];
    if (key == EMPTY_KEY) return;
    const uint32_t qidx = (uint32_t)key;
    const uint64_t cand = (key & 0xFFFFFFFF00000000ull) | (uint64_t)(uint32_t)i;
    atomicMin(&best_per_query[qidx], (unsigned long long)cand);
}

__global__ void nonempty_flag_kernel(const uint64_t* __restrict__ keys, int n, uint8_t* __restrict__ flags) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[i] = keys[i] != EMPTY_KEY;
}

// ---- ordered compaction: flags -> exclusive positions (3 small kernels, no host round trip) -------------
static constexpr int SCAN_BLOCK = 1024;

__global__ __launch_bounds__(SCAN_BLOCK) void scan_block_counts_kernel(const uint8_t* __restrict__ flags, int n, int* __restrict__ block_counts) {
    APDS_RAISE_WAVE_PRIORITY();
    __shared__ int wsum[SCAN_BLOCK / 64];
    const int i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    const int f = i < n ? (flags[i] != 0) : 0;
    const unsigned long long b = __ballot(f);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < SCAN_BLOCK / 64; w++) s += wsum[w];
        block_counts[blockIdx.x] = s;
    }
}

// single block: exclusive scan of block_counts in place, total to *total
__global__ __launch_bounds__(1024) void scan_offsets_kernel(int* __restrict__ block_counts, int nblocks, int* __restrict__ total) {
    APDS_RAISE_WAVE_PRIORITY();
    __shared__ int buf[1024];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nblocks; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < nblocks ? block_counts[i] : 0;
        buf[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            int add = threadIdx.x >= off ? buf[threadIdx.x - off] : 0;
            __syncthreads();
            buf[threadIdx.x] += add;
            __syncthreads();
        }
        const int incl = buf[threadIdx.x];
        if (i < nblocks) block_counts[i] = carry + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

__device__ __forceinline__ int block_exclusive_pos(int f, int block_offset) {
    __shared__ int wsum[SCAN_BLOCK / 64];
    const unsigned long long b = __ballot(f);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wsum[w] = __popcll(b);
    __syncthreads();
    int before = 0;
    for (int k = 0; k < w; k++) before += wsum[k];
    return block_offset + before + __popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(SCAN_BLOCK) void emit_ratio_matches_kernel(const uint64_t* __restrict__ keys, int nq, int K, const uint8_t* __restrict__ flags,
                                                                        const int* __restrict__ block_offsets, apds_dmatch* __restrict__ out) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    const int f = i < nq ? (flags[i] != 0) : 0;
    const int pos = block_exclusive_pos(f, block_offsets[blockIdx.x]);
    if (f) {
        const uint64_t k0 = keys[(size_t)i * K];
        apds_dmatch m;
        m.query_idx = i;
        m.train_idx = (int32_t)(uint32_t)k0;
        m.img_idx = 0;
        m.distance = (float)(uint32_t)(k0 >> 32);
        out[pos] = m;
    }
}

// flags (n bytes) -> block offsets; returns device pointers for the emit kernel; *total_dev holds the count
int* scan_flags_device(const uint8_t* flags, int n, int** total_dev, hipStream_t s) {
    ThreadCtx& c = ctx();
    const int nblocks = std::max(1, ceil_div(n, SCAN_BLOCK));
    int* block_counts = c.alloc_n<int>(nblocks + 1);
    int* total = block_counts + nblocks;
    hipLaunchKernelGGL(scan_block_counts_kernel, dim3(nblocks), dim3(SCAN_BLOCK), 0, s, flags, n, block_counts);
    hipLaunchKernelGGL(scan_offsets_kernel, dim3(1), dim3(1024), 0, s, block_counts, nblocks, total);
    HIP_CHECK(hipGetLastError());
    *total_dev = total;
    return block_counts;
}

// The tail of both filters: positions of the flagged queries, their matches (keys[q * K]: the nearest of query q) in query order, and the
// count read back. Synchronises s.
static int emit_flagged_device(const uint64_t* keys, int nq, int K, const uint8_t* flags, apds_dmatch* out, hipStream_t s) {
    int* total_dev = nullptr;
    int* offs = scan_flags_device(flags, nq, &total_dev, s);
    hipLaunchKernelGGL(emit_ratio_matches_kernel, dim3(ceil_div(nq, SCAN_BLOCK)), dim3(SCAN_BLOCK), 0, s, keys, nq, K, flags, offs, out);
    HIP_CHECK(hipGetLastError());
    int total = 0;
    HIP_CHECK(hipMemcpyAsync(&total, total_dev, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return total;
}

int ratio_filter_device(const uint64_t* keys, int nq, int k, float fs, apds_dmatch* out, hipStream_t s) {
    if (nq <= 0) return 0;
    uint8_t* flags = ctx().alloc_n<uint8_t>(nq);
    hipLaunchKernelGGL(ratio_flag_kernel, dim3(ceil_div(nq, 256)), dim3(256), 0, s, keys, nq, k, fs, flags);
    return emit_flagged_device(keys, nq, k, flags, out, s);
}

// ---- the ratio test on L2 keys (f32 bits of d^2 << 32 | row: l2_match.hip, l2_screen.hip) ----------------------------------------------
// The distance of a key is sqrtf(d^2), correctly rounded: the value apds_l2_knn_match computes on the host from the same bits and
// get_knn_matches_l2 compares. It is taken in binary64 and rounded once more: a square root of a binary32 value is never within 2^-49
// (relative) of the midpoint of two binary32 numbers, so the second rounding of a binary64 root, even one that is an ulp off, gives the
// correctly rounded binary32 root (53 >= 2 * 24 + 2). (__fsqrt_rn is NOT that root here: unless the HIP math header is compiled
// with OCML_BASIC_ROUNDED_OPERATIONS it is __ocml_native_sqrt_f32, the hardware's v_sqrt_f32 of 1 ulp, whatever the build's flags; it
// measured one ulp below the host's root on 2 of 500 distances.) d1 * fs is one f32 product (no contraction: nothing is added to it), the test a strict f32 `<`.
__device__ __forceinline__ float l2_key_distance(uint64_t key) { return (float)sqrt((double)__uint_as_float((uint32_t)(key >> 32))); }

__global__ void l2_ratio_flag_kernel(const uint64_t* __restrict__ keys, int nq, int K, float fs, uint8_t* __restrict__ flags) {
    APDS_RAISE_WAVE_PRIORITY();
    const int qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    const uint64_t k0 = keys[(size_t)qi * K], k1 = keys[(size_t)qi * K + 1];
    const float d0 = l2_key_distance(k0), d1 = l2_key_distance(k1);
    flags[qi] = (k0 != EMPTY_KEY && k1 != EMPTY_KEY && d0 < d1 * fs) ? 1 : 0;
}

__global__ __launch_bounds__(SCAN_BLOCK) void emit_l2_ratio_matches_kernel(const uint64_t* __restrict__ keys, int nq, int K, const uint8_t* __restrict__ flags,
                                                                           const int* __restrict__ block_offsets, apds_dmatch* __restrict__ out) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    const int f = i < nq ? (flags[i] != 0) : 0;
    const int pos = block_exclusive_pos(f, block_offsets[blockIdx.x]);
    if (f) {
        const uint64_t k0 = keys[(size_t)i * K];
        apds_dmatch m;
        m.query_idx = i;
        m.train_idx = (int32_t)(uint32_t)k0;
        m.img_idx = 0;
        m.distance = l2_key_distance(k0);
        out[pos] = m;
    }
}

int l2_ratio_filter_device(const uint64_t* keys, int nq, int k, float fs, apds_dmatch* out, hipStream_t s) {
    if (nq <= 0) return 0;
    uint8_t* flags = ctx().alloc_n<uint8_t>(nq);
    hipLaunchKernelGGL(l2_ratio_flag_kernel, dim3(ceil_div(nq, 256)), dim3(256), 0, s, keys, nq, k, fs, flags);
    int* total_dev = nullptr;
    int* offs = scan_flags_device(flags, nq, &total_dev, s);
    hipLaunchKernelGGL(emit_l2_ratio_matches_kernel, dim3(ceil_div(nq, SCAN_BLOCK)), dim3(SCAN_BLOCK), 0, s, keys, nq, k, (const uint8_t*)flags, (const int*)offs, out);
    HIP_CHECK(hipGetLastError());
    int total = 0;
    HIP_CHECK(hipMemcpyAsync(&total, total_dev, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return total;
}

int cross_check_device(const uint64_t* train_best, long long n_train, int nq, apds_dmatch* out, hipStream_t s) {
    if (nq <= 0 || n_train <= 0) return 0;
    ThreadCtx& c = ctx();
    uint64_t* best = c.alloc_n<uint64_t>(nq);
    HIP_CHECK(hipMemsetAsync(best, 0xFF, (size_t)nq * 8, s));
    hipLaunchKernelGGL(crosscheck_scatter_kernel, dim3(ceil_div(n_train, 256)), dim3(256), 0, s, train_best, n_train,
                       reinterpret_cast<unsigned long long*>(best));
    uint8_t* flags = c.alloc_n<uint8_t>(nq);
    hipLaunchKernelGGL(nonempty_flag_kernel, dim3(ceil_div(nq, 256)), dim3(256), 0, s, best, nq, flags);
    return emit_flagged_device(best, nq, 1, flags, out, s);
}

// ---- the cross-check with an index base (apds_dev_crosscheck_match, the pipeline's cross-check mode) ----
// The scatter, the flags and the scan are cross_check_device's; the emit adds index_base to the train row (a shard's or a batch's global
// row, as the keys of apds_dev_hamming_topk carry it). best_per_query[q] = (distance << 32 | train row), EMPTY where nobody chose q.
__global__ __launch_bounds__(SCAN_BLOCK) void emit_crosscheck_matches_kernel(const uint64_t* __restrict__ best_per_query, int nq, uint32_t index_base,
                                                                             const uint8_t* __restrict__ flags, const int* __restrict__ block_offsets,
                                                                             apds_dmatch* __restrict__ out) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    const int f = i < nq ? (flags[i] != 0) : 0;
    const int pos = block_exclusive_pos(f, block_offsets[blockIdx.x]);
    if (f) {
        const uint64_t k0 = best_per_query[i];
        apds_dmatch m;
        m.query_idx = i;
        m.train_idx = (int32_t)((uint32_t)k0 + index_base);
        m.img_idx = 0;
        m.distance = (float)(uint32_t)(k0 >> 32);
        out[pos] = m;
    }
}

int cross_check_base_device(const uint64_t* train_best, long long n_train, int nq, uint32_t index_base, apds_dmatch* out, hipStream_t s) {
    if (nq <= 0 || n_train <= 0) return 0;
    ThreadCtx& c = ctx();
    uint64_t* best = c.alloc_n<uint64_t>(nq);
    HIP_CHECK(hipMemsetAsync(best, 0xFF, (size_t)nq * 8, s));
    hipLaunchKernelGGL(crosscheck_scatter_kernel, dim3(ceil_div(n_train, 256)), dim3(256), 0, s, train_best, n_train,
                       reinterpret_cast<unsigned long long*>(best));
    uint8_t* flags = c.alloc_n<uint8_t>(nq);
    hipLaunchKernelGGL(nonempty_flag_kernel, dim3(ceil_div(nq, 256)), dim3(256), 0, s, best, nq, flags);
    int* total_dev = nullptr;
    int* offs = scan_flags_device(flags, nq, &total_dev, s);
    hipLaunchKernelGGL(emit_crosscheck_matches_kernel, dim3(ceil_div(nq, SCAN_BLOCK)), dim3(SCAN_BLOCK), 0, s, best, nq, index_base, flags, offs, out);
    HIP_CHECK(hipGetLastError());
    int total = 0;
    HIP_CHECK(hipMemcpyAsync(&total, total_dev, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return total;
}

}  // namespace apds
