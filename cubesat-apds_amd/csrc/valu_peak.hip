// csrc/valu_peak.hip — register-only VALU microbenchmark: the denominator of the popcount roofline (bench.py divides the vector-ALU scan
// by valu_popcount_peak_device) and the issue-order experiments behind the scan's inner loop (match_hamming.hip: row_distances).
#include <utility>

#include "kernels.h"
#include "popcount_row.h"

namespace apds {

// One instruction kind per MODE, eight independent chains per lane, nothing but that instruction in the loop body (the loop
// counter is scalar). Modes 0-3 and 8-10 are 32-bit integer ops, 4-7 and 11 are FP32 ops issued by the same waves on the same
// SIMDs, so one run shows whether the integer ops the match kernel is made of issue at the FP32 rate or at half of it.
//   0 v_xor_b32(sgpr, vgpr) + v_bcnt_u32_b32 accumulate: the match kernel's inner pair (two lane-ops per pair)
//   1 v_xor_b32 (sgpr operand)   2 v_bcnt_u32_b32 accumulate   3 v_add_u32 (sgpr operand)
//   4 v_fma_f32   5 v_add_f32   6 v_pk_fma_f32 (two FMAs per lane per instruction)   7 v_pk_add_f32 (two adds)
//   8 v_xor_b32 (vgpr, vgpr)   9 v_bfi_b32 (VOP3, three vgprs)   10 v_and_b32 (vgpr, vgpr)   11 v_mul_f32
// Modes 12-17 replay the ISSUE PATTERN of the match kernel's inner loop (one train row in 15 SGPRs against 4 queries of 15 dwords
// in VGPRs = 60 xor + 60 bcnt per row) in different instruction orders, to find the order the SIMD issues fastest:
//   12 query-sequential, one dependent chain per query (xor t,s_j,q_cj ; bcnt a_c,t,a_c for j = 0..14, then the next query): the
//      order hipcc emits for row_distances()        13 dword-major (the four queries' chains interleaved round-robin)
//   14 = 13 with the xor of step i+1 issued before the bcnt of step i (two temporaries)      15 = 13 with the row first copied to
//   VGPRs (15 v_mov per row, not counted) so the xor has no SGPR operand      16 = 12 skewed like 14      17 = 13 with two xors
//   ahead (three temporaries)
// Every wave also leaves its s_memtime span, so the host can state cycles per wave-instruction per SIMD without assuming a clock.
typedef float f32x2 __attribute__((ext_vector_type(2)));
static constexpr int VALU_MODES = 28;
static constexpr int VALU_CHAINS = 8, VALU_UNROLL = 16;

template <int MODE>
__global__ __launch_bounds__(256) void valu_peak_kernel(uint32_t* __restrict__ sink, unsigned long long* __restrict__ spans, int iters,
                                                        const u32x16* __restrict__ rowp) {
    extern __shared__ uint32_t occupancy_pad[];   // dynamic LDS request only bounds the workgroups per CU
    if (MODE >= 12) {
        uint32_t q4[4][15];
        int a[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            a[c] = c;
#pragma unroll
            for (int j = 0; j < 15; j++) q4[c][j] = threadIdx.x * 2654435761u + (c * 16 + j) * 40503u + 1u;
        }
        // the row is reloaded every iteration (wave-uniform address: s_load_dwordx16, as in the match kernel), one row ahead; the
        // xor is plain C and the accumulate is bcnt_acc(), as in row_distances(); sched_barrier(0) pins the order under test
        // (two adjacent inline-asm VALU ops make hipcc insert an s_nop between them, which the match kernel's loop does not have)
        u32x16 row = rowp[blockIdx.x & 7];
        const unsigned long long t0 = __builtin_readcyclecounter();
        for (int it = 0; it < iters; it++) {
            const u32x16 next = rowp[(blockIdx.x + it + 1) & 7];
#define APDS_X(tmp, j, c) { tmp = row[j] ^ q4[c][j]; __builtin_amdgcn_sched_barrier(0); }
#define APDS_XV(tmp, j, c) { tmp = rv[j] ^ q4[c][j]; __builtin_amdgcn_sched_barrier(0); }
#define APDS_B(tmp, c) { a[c] = bcnt_acc(tmp, a[c]); __builtin_amdgcn_sched_barrier(0); }
            __builtin_amdgcn_sched_barrier(0);
            if (MODE == 12) {
#pragma unroll
                for (int c = 0; c < 4; c++)
#pragma unroll
                    for (int j = 0; j < 15; j++) { uint32_t t; APDS_X(t, j, c); APDS_B(t, c); }
            } else if (MODE == 18) {      // 12 with an s_nop between every xor and the bcnt that consumes it
#pragma unroll
                for (int c = 0; c < 4; c++)
#pragma unroll
                    for (int j = 0; j < 15; j++) { uint32_t t; APDS_X(t, j, c); asm volatile("s_nop 0"); __builtin_amdgcn_sched_barrier(0); APDS_B(t, c); }
            } else if (MODE == 19) {      // 13 with the s_nop
#pragma unroll
                for (int j = 0; j < 15; j++)
#pragma unroll
                    for (int c = 0; c < 4; c++) { uint32_t t; APDS_X(t, j, c); asm volatile("s_nop 0"); __builtin_amdgcn_sched_barrier(0); APDS_B(t, c); }
            } else if (MODE == 20) {      // 12 with an s_nop after EVERY instruction
#pragma unroll
                for (int c = 0; c < 4; c++)
#pragma unroll
                    for (int j = 0; j < 15; j++) {
                        uint32_t t;
                        APDS_X(t, j, c); asm volatile("s_nop 0"); __builtin_amdgcn_sched_barrier(0);
                        APDS_B(t, c); asm volatile("s_nop 0"); __builtin_amdgcn_sched_barrier(0);
                    }
            } else if (MODE == 22) {      // bcnt only (the xor hoisted: 15 xors, then 60 bcnt with an s_nop after each) - is bcnt 4 cycles whatever the phase?
                uint32_t t[15];
#pragma unroll
                for (int j = 0; j < 15; j++) APDS_X(t[j], j, 0);
#pragma unroll
                for (int c = 0; c < 4; c++)
#pragma unroll
                    for (int j = 0; j < 15; j++) { APDS_B(t[j], c); asm volatile("s_nop 0"); __builtin_amdgcn_sched_barrier(0); }
            } else if (MODE == 23) {      // X X nop B B
#pragma unroll
                for (int c = 0; c < 4; c += 2)
#pragma unroll
                    for (int j = 0; j < 15; j++) {
                        uint32_t t0, t1;
                        APDS_X(t0, j, c); APDS_X(t1, j, c + 1); asm volatile("s_nop 0"); __builtin_amdgcn_sched_barrier(0);
                        APDS_B(t0, c); APDS_B(t1, c + 1);
                    }
            } else if (MODE == 24) {      // X s_nop 1 B
#pragma unroll
                for (int c = 0; c < 4; c++)
#pragma unroll
                    for (int j = 0; j < 15; j++) { uint32_t t; APDS_X(t, j, c); asm volatile("s_nop 1"); __builtin_amdgcn_sched_barrier(0); APDS_B(t, c); }
            } else if (MODE == 25) {      // B nop X (the nop after the bcnt instead of before it): X0, then [B nop X] ...
                uint32_t t[60];
                APDS_X(t[0], 0, 0);
#pragma unroll
                for (int i = 0; i < 60; i++) {
                    APDS_B(t[i], i / 15);
                    asm volatile("s_nop 0"); __builtin_amdgcn_sched_barrier(0);
                    if (i + 1 < 60) APDS_X(t[i + 1], (i + 1) % 15, (i + 1) / 15);
                }
            } else if (MODE == 26) {      // X nop B where the nop is an s_sleep-free scalar ALU op (s_add on a dummy) instead of s_nop
                int dummy = it;
#pragma unroll
                for (int c = 0; c < 4; c++)
#pragma unroll
                    for (int j = 0; j < 15; j++) {
                        uint32_t t;
                        APDS_X(t, j, c);
                        asm volatile("s_add_u32 %0, %0, 1" : "+s"(dummy));
                        __builtin_amdgcn_sched_barrier(0);
                        APDS_B(t, c);
                    }
                if (dummy == 0x7ffffff0) a[0]++;
            } else if (MODE == 27) {      // X nop B with a second independent pair stream interleaved: X0 X1 nop B0 B1 on two queries at a time, dword-major
#pragma unroll
                for (int j = 0; j < 15; j++) {
                    uint32_t t0, t1, t2, t3;
                    APDS_X(t0, j, 0); asm volatile("s_nop 0"); __builtin_amdgcn_sched_barrier(0); APDS_B(t0, 0);
                    APDS_X(t1, j, 1); asm volatile("s_nop 0"); __builtin_amdgcn_sched_barrier(0); APDS_B(t1, 1);
                    APDS_X(t2, j, 2); asm volatile("s_nop 0"); __builtin_amdgcn_sched_barrier(0); APDS_B(t2, 2);
                    APDS_X(t3, j, 3); asm volatile("s_nop 0"); __builtin_amdgcn_sched_barrier(0); APDS_B(t3, 3);
                }
            } else if (MODE == 21) {      // 12 with ONE SGPR for the whole row (row[0]) instead of fifteen
#pragma unroll
                for (int c = 0; c < 4; c++)
#pragma unroll
                    for (int j = 0; j < 15; j++) { uint32_t t; t = row[0] ^ q4[c][j]; __builtin_amdgcn_sched_barrier(0); APDS_B(t, c); }
            } else if (MODE == 13) {
#pragma unroll
                for (int j = 0; j < 15; j++)
#pragma unroll
                    for (int c = 0; c < 4; c++) { uint32_t t; APDS_X(t, j, c); APDS_B(t, c); }
            } else if (MODE == 14 || MODE == 17) {
                constexpr int AHEAD = MODE == 17 ? 2 : 1;
                uint32_t t[60];
#pragma unroll
                for (int i = 0; i < 60 + AHEAD; i++) {
                    if (i < 60) APDS_X(t[i], i >> 2, i & 3);
                    if (i >= AHEAD) APDS_B(t[i - AHEAD], (i - AHEAD) & 3);
                }
            } else if (MODE == 15) {
                uint32_t rv[15];
#pragma unroll
                for (int j = 0; j < 15; j++) { asm volatile("v_mov_b32 %0, %1" : "=v"(rv[j]) : "s"(row[j])); }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 15; j++)
#pragma unroll
                    for (int c = 0; c < 4; c++) { uint32_t t; APDS_XV(t, j, c); APDS_B(t, c); }
            } else {   // 16: query-sequential, skewed by one
                uint32_t t[60];
#pragma unroll
                for (int i = 0; i < 61; i++) {
                    if (i < 60) APDS_X(t[i], i % 15, i / 15);
                    if (i >= 1) APDS_B(t[i - 1], (i - 1) / 15);
                }
            }
#undef APDS_X
#undef APDS_XV
#undef APDS_B
            row = next;
        }
        const unsigned long long t1 = __builtin_readcyclecounter();
        if ((a[0] + a[1] + a[2] + a[3]) == 0x7fffffff) sink[0] = 1;
        if ((threadIdx.x & 63) == 0) spans[(size_t)blockIdx.x * 4 + (threadIdx.x >> 6)] = t1 - t0;
        return;
    }
    uint32_t q[VALU_UNROLL];
#pragma unroll
    for (int j = 0; j < VALU_UNROLL; j++) q[j] = threadIdx.x * 2654435761u + j * 40503u + 1u;
    uint32_t acc[VALU_CHAINS];
    float facc[VALU_CHAINS];
    f32x2 pacc[VALU_CHAINS];
#pragma unroll
    for (int c = 0; c < VALU_CHAINS; c++) {
        acc[c] = c + threadIdx.x;
        facc[c] = 1.0f + 0.001f * (float)(c + (threadIdx.x & 7));
        pacc[c] = f32x2{facc[c], facc[c] * 0.5f};
    }
    const float fm = 0.99999f, fa = 1e-6f;
    const f32x2 pm = {0.99999f, 0.99998f}, pa = {1e-6f, 2e-6f};
    uint32_t s = blockIdx.x * 97u + 1u;
    const unsigned long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int j = 0; j < VALU_UNROLL; j++) {
#pragma unroll
            for (int c = 0; c < VALU_CHAINS; c++) {
                if (MODE == 0) {
                    uint32_t x;
                    asm volatile("v_xor_b32 %0, %1, %2" : "=v"(x) : "s"(s), "v"(q[j]));
                    asm volatile("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc[c]) : "v"(x));
                } else if (MODE == 1) asm volatile("v_xor_b32 %0, %1, %0" : "+v"(acc[c]) : "s"(s));
                else if (MODE == 2) asm volatile("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc[c]) : "v"(q[j]));
                else if (MODE == 3) asm volatile("v_add_u32 %0, %1, %0" : "+v"(acc[c]) : "s"(s));
                else if (MODE == 4) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(facc[c]) : "v"(fm), "v"(fa));
                else if (MODE == 5) asm volatile("v_add_f32 %0, %1, %0" : "+v"(facc[c]) : "v"(fa));
                else if (MODE == 6) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(pacc[c]) : "v"(pm), "v"(pa));
                else if (MODE == 7) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(pacc[c]) : "v"(pa));
                else if (MODE == 8) asm volatile("v_xor_b32 %0, %1, %0" : "+v"(acc[c]) : "v"(q[j]));
                else if (MODE == 9) asm volatile("v_bfi_b32 %0, %0, %1, %2" : "+v"(acc[c]) : "v"(q[j]), "v"(q[(j + 1) & (VALU_UNROLL - 1)]));
                else if (MODE == 10) asm volatile("v_and_b32 %0, %1, %0" : "+v"(acc[c]) : "v"(q[j]));
                else asm volatile("v_mul_f32 %0, %1, %0" : "+v"(facc[c]) : "v"(fm));
            }
        }
        s = s * 1664525u + 1013904223u;
    }
    const unsigned long long t1 = __builtin_readcyclecounter();
    uint32_t fold = 0;
#pragma unroll
    for (int c = 0; c < VALU_CHAINS; c++) fold += acc[c] + __float_as_uint(facc[c]) + __float_as_uint(pacc[c].x) + __float_as_uint(pacc[c].y);
    if (fold == 0x7fffffffu) sink[0] = 1;
    if ((threadIdx.x & 63) == 0) spans[(size_t)blockIdx.x * 4 + (threadIdx.x >> 6)] = t1 - t0;
}

// One launch configuration of the microbenchmark: `waves_per_simd` workgroups of 256 threads resident per CU (one wave of each
// on every SIMD; bounded through an unused dynamic-LDS request), a grid eight rounds deep.
struct ValuPeak {
    double lane_ops_per_s;      // wall clock (HIP events), lane-ops as defined per mode (a packed instruction counts two)
    double cycles_per_inst;     // s_memtime cycles per wave-instruction per SIMD = mean wave span / (instructions per wave * waves per SIMD)
};

template <int MODE>
static ValuPeak run_valu_peak(int waves_per_simd, hipStream_t st) {
    ThreadCtx& c = ctx();
    const int w = std::min(std::max(waves_per_simd, 1), 8);
    const int iters = 2048, cus = 256, blocks = cus * w * 8;
    uint32_t* sink = c.alloc_n<uint32_t>(64);
    unsigned long long* spans = c.alloc_n<unsigned long long>((size_t)blocks * 4);
    // 160 KB of LDS per CU: a request of 160 KB / w (minus the granule) admits exactly w workgroups
    const size_t lds = w >= 8 ? 0 : (size_t)(160 * 1024 / w) - (w == 1 ? 0 : 1024);
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&valu_peak_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipEvent_t a, b;
    HIP_CHECK(hipEventCreate(&a));
    HIP_CHECK(hipEventCreate(&b));
    u32x16* rowp = reinterpret_cast<u32x16*>(c.alloc_n<uint32_t>(16 * 8));
    {
        uint32_t h[16 * 8];
        for (int i = 0; i < 16 * 8; i++) h[i] = 0x9E3779B9u * (uint32_t)(i + 1);
        HIP_CHECK(hipMemcpyAsync(rowp, h, sizeof(h), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    hipLaunchKernelGGL((valu_peak_kernel<MODE>), dim3(blocks), dim3(256), lds, st, sink, spans, 32, rowp);
    ValuPeak best{0, 0};
    std::vector<unsigned long long> host((size_t)blocks * 4);
    const double per_inst = MODE == 0 ? 1 : ((MODE == 6 || MODE == 7) ? 2 : 1);   // lane-ops per instruction per lane
    const double insts_per_wave = MODE >= 12 ? (double)iters * 120 : (double)iters * VALU_UNROLL * VALU_CHAINS * (MODE == 0 ? 2 : 1);
    for (int rep = 0; rep < 3; rep++) {
        HIP_CHECK(hipEventRecord(a, st));
        hipLaunchKernelGGL((valu_peak_kernel<MODE>), dim3(blocks), dim3(256), lds, st, sink, spans, iters, rowp);
        HIP_CHECK(hipEventRecord(b, st));
        HIP_CHECK(hipEventSynchronize(b));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, a, b));
        const double ops = (double)blocks * 256 * insts_per_wave * per_inst;
        if (ops / (ms * 1e-3) > best.lane_ops_per_s) {
            HIP_CHECK(hipMemcpy(host.data(), spans, host.size() * 8, hipMemcpyDeviceToHost));
            double sum = 0;
            for (unsigned long long v : host) sum += (double)v;
            best.lane_ops_per_s = ops / (ms * 1e-3);
            best.cycles_per_inst = sum / (double)host.size() / (insts_per_wave * w);
        }
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return best;
}

// One entry per mode, all three from VALU_MODES: the count the API reports, the names, and the table of run_valu_peak<0 .. VALU_MODES - 1>.
static const char* const VALU_MODE_NAMES[] = {"v_xor_b32(s,v)+v_bcnt_u32_b32", "v_xor_b32(s,v)", "v_bcnt_u32_b32", "v_add_u32(s,v)", "v_fma_f32", "v_add_f32",
                                              "v_pk_fma_f32", "v_pk_add_f32", "v_xor_b32(v,v)", "v_bfi_b32", "v_and_b32(v,v)", "v_mul_f32",
                                              "row x 4 queries: query-sequential", "row x 4 queries: dword-major", "dword-major, xor 1 ahead",
                                              "dword-major, row in VGPRs", "query-sequential, xor 1 ahead", "dword-major, xor 2 ahead",
                                              "query-sequential + s_nop before each bcnt", "dword-major + s_nop before each bcnt",
                                              "query-sequential + s_nop after every op", "query-sequential, one SGPR",
                                              "bcnt + s_nop only (75 ops counted as 120)", "X X nop B B", "X s_nop(1) B", "B nop X", "X s_add B", "dword-major X nop B"};
static_assert(sizeof(VALU_MODE_NAMES) / sizeof(VALU_MODE_NAMES[0]) == VALU_MODES, "one name per mode");

template <size_t... MODE>
static ValuPeak run_valu_mode(int mode, int waves_per_simd, hipStream_t st, std::index_sequence<MODE...>) {
    static constexpr ValuPeak (*run[])(int, hipStream_t) = {&run_valu_peak<(int)MODE>...};
    return run[mode](waves_per_simd, st);
}

int valu_peak_modes() { return VALU_MODES; }

const char* valu_peak_mode_name(int mode) { return mode >= 0 && mode < VALU_MODES ? VALU_MODE_NAMES[mode] : "?"; }

void valu_peak_device(int mode, int waves_per_simd, double* lane_ops_per_s, double* cycles_per_inst) {
    APDS_REQUIRE(mode >= 0 && mode < VALU_MODES, APDS_ERR_BAD_ARG, "valu peak: mode out of range");
    const ValuPeak r = run_valu_mode(mode, waves_per_simd, ctx().stream, std::make_index_sequence<VALU_MODES>{});
    if (lane_ops_per_s) *lane_ops_per_s = r.lane_ops_per_s;
    if (cycles_per_inst) *cycles_per_inst = r.cycles_per_inst;
}

// lane-ops/s of the xor+bcnt pair at full occupancy: the denominator bench.py divides the match kernel by
double valu_popcount_peak_device() {
    double v = 0;
    valu_peak_device(0, 8, &v, nullptr);
    return v;
}

}  // namespace apds
