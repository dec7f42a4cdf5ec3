// csrc/topk_keys.h — the 64-bit keys every matcher ranks by, and sorted lists of them.
//
// A key is (rank << 32 | train row): rank is the Hamming distance, or the bit pattern of a non-negative float distance (which orders
// like the float). Unsigned 64-bit order is then BFMatcher's order (distance, then the lower train row), a key carries its row, so all
// keys of a query are distinct, and all ones - above every key a row can have - marks a list slot without a row.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace apds {

static constexpr uint64_t EMPTY_KEY = ~0ull;

__host__ __device__ __forceinline__ uint64_t make_key(uint32_t rank, uint32_t index) { return ((uint64_t)rank << 32) | index; }
__host__ __device__ __forceinline__ uint32_t key_rank(uint64_t key) { return (uint32_t)(key >> 32); }
__host__ __device__ __forceinline__ uint32_t key_index(uint64_t key) { return (uint32_t)key; }

// Insert into an ascending list of K keys (static register indices only). Strict '<': a key equal to one in the list goes behind it, and
// one that is not below the K-th is dropped.
template <int K>
__device__ __forceinline__ void topk_insert(uint64_t (&best)[K], uint64_t key) {
    if (key < best[K - 1]) {
        bool placed = false;
#pragma unroll
        for (int j = K - 1; j > 0; j--) {
            if (!placed) {
                if (best[j - 1] > key) best[j] = best[j - 1];
                else {
                    best[j] = key;
                    placed = true;
                }
            }
        }
        if (!placed) best[0] = key;
    }
}

}  // namespace apds
