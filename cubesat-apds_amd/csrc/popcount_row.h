// csrc/popcount_row.h — a packed descriptor row as the vector-ALU scan reads it, and the scan's one inner instruction. Shared by the
// scan (match_hamming.hip) and by the microbenchmark that replays its issue pattern (valu_peak.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace apds {

typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));   // one 64-byte row: a wave-uniform address loads it into 16 SGPRs

// acc + popcount(x) in ONE VALU op. hipcc otherwise splits the accumulate into v_bcnt(x,0) + v_add3 (5 ops per
// two dwords instead of 4), so the accumulate form is spelled out.
__device__ __forceinline__ int bcnt_acc(uint32_t x, int acc) {
    int r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

}  // namespace apds
