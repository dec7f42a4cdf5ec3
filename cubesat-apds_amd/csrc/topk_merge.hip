// csrc/topk_merge.hip — merges of sorted key lists (topk_keys.h). Every matcher that splits its train rows ends here: the matrix-core
// Hamming matcher (hamming_mfma.hip), both L2 matchers (l2_match.hip, l2_screen.hip) and the sharded matcher (shard.cpp); the vector-ALU
// scan merges its own compact records (match_hamming.hip: merge_records_kernel).
// Lists are [parts][nq][k]: ascending, an EMPTY_KEY tail where a part held fewer than k rows. All keys of a query are distinct.
#include "kernels.h"
#include "topk_keys.h"

namespace apds {

// merge `parts` sorted candidate lists per query into the k smallest keys
template <int K>
__global__ void merge_topk_kernel(const uint64_t* __restrict__ parts_keys, int parts, int nq, uint64_t* __restrict__ out) {
    APDS_RAISE_WAVE_PRIORITY();
    const int qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    uint64_t best[K];
#pragma unroll
    for (int k = 0; k < K; k++) best[k] = EMPTY_KEY;
    constexpr int U = K <= 2 ? 8 : 2;   // independent loads in flight per lane
    int p = 0;
    for (; p + U <= parts; p += U) {
        uint64_t v[U][K];
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int k = 0; k < K; k++) v[u][k] = parts_keys[((size_t)(p + u) * nq + qi) * K + k];
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int k = 0; k < K; k++) topk_insert<K>(best, v[u][k]);
    }
    for (; p < parts; p++)
#pragma unroll
        for (int k = 0; k < K; k++) topk_insert<K>(best, parts_keys[((size_t)p * nq + qi) * K + k]);
#pragma unroll
    for (int k = 0; k < K; k++) out[(size_t)qi * K + k] = best[k];
}

// The same for any k (the sharded matcher above 16 neighbours, and k not a power of two): every list is ascending and all keys are distinct
// (a key carries its global row), so output j is the smallest key above output j - 1: each lane walks a cursor per list. parts <= 64.
__global__ void merge_topk_any_kernel(const uint64_t* __restrict__ parts_keys, int parts, int nq, int k, uint64_t* __restrict__ out) {
    APDS_RAISE_WAVE_PRIORITY();
    const int qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    uint16_t cur[64];   // cursor of every list
    for (int p = 0; p < parts; p++) cur[p] = 0;
    for (int j = 0; j < k; j++) {
        uint64_t best = EMPTY_KEY;
        int arg = -1;
        for (int p = 0; p < parts; p++) {
            if (cur[p] >= k) continue;
            const uint64_t v = parts_keys[((size_t)p * nq + qi) * k + cur[p]];
            if (v < best) best = v, arg = p;
        }
        out[(size_t)qi * k + j] = best;
        if (arg >= 0) cur[arg]++;
    }
}

__global__ void take_first_columns_kernel(const uint64_t* __restrict__ in, int nq, int kin, int kout, uint64_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)nq * kout) return;
    const int q = (int)(i / kout), c = (int)(i - (long long)q * kout);
    out[i] = in[(size_t)q * kin + c];
}

template <int K>
static void merge_launch(const uint64_t* parts, int nparts, int nq, uint64_t* out, hipStream_t s) {
    hipLaunchKernelGGL((merge_topk_kernel<K>), dim3(ceil_div(nq, 256)), dim3(256), 0, s, parts, nparts, nq, out);
}

void merge_topk_device(const uint64_t* parts, int nparts, int nq, int k, uint64_t* out, hipStream_t s) {
    if (nq <= 0) return;
    switch (k) {
        case 1: merge_launch<1>(parts, nparts, nq, out, s); break;
        case 2: merge_launch<2>(parts, nparts, nq, out, s); break;
        case 4: merge_launch<4>(parts, nparts, nq, out, s); break;
        case 8: merge_launch<8>(parts, nparts, nq, out, s); break;
        case 16: merge_launch<16>(parts, nparts, nq, out, s); break;
        default:
            APDS_REQUIRE(k >= 1 && k <= 4096 && nparts <= 64, APDS_ERR_ASSERT, "merge supports 1 <= k <= 4096 over at most 64 lists");
            hipLaunchKernelGGL(merge_topk_any_kernel, dim3(ceil_div(nq, 64)), dim3(64), 0, s, parts, nparts, nq, k, out);
    }
    HIP_CHECK(hipGetLastError());
}

void take_first_columns_device(const uint64_t* in, int nq, int kin, int kout, uint64_t* out, hipStream_t s) {
    if (nq <= 0) return;
    hipLaunchKernelGGL(take_first_columns_kernel, dim3(ceil_div((long long)nq * kout, 256)), dim3(256), 0, s, in, nq, kin, kout, out);
}

}  // namespace apds
