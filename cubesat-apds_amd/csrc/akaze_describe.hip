// csrc/akaze_describe.hip — AKAZE main orientation and the 486-bit M-LDB descriptor on gfx950, one wave per keypoint.
//
// Replaces OpenCV AKAZEFeatures::Compute_Main_Orientation and MLDB_Full_Descriptor_Invoker behind feature_extraction/src/lib.rs:79.
#include "akaze.h"
#include "akaze_describe.h"
#include "config.h"

namespace apds {

__device__ __forceinline__ int clampi2(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// ---- a1.8 main orientation: one wave per keypoint ---------------------------------------------------------------
__constant__ float c_gauss25[7][7] = {
    {0.02546481f, 0.02350698f, 0.01849125f, 0.01239505f, 0.00708017f, 0.00344629f, 0.00142946f},
    {0.02350698f, 0.02169968f, 0.01706957f, 0.01144208f, 0.00653582f, 0.00318132f, 0.00131956f},
    {0.01849125f, 0.01706957f, 0.01342740f, 0.00900066f, 0.00514126f, 0.00250252f, 0.00103800f},
    {0.01239505f, 0.01144208f, 0.00900066f, 0.00603332f, 0.00344629f, 0.00167749f, 0.00069579f},
    {0.00708017f, 0.00653582f, 0.00514126f, 0.00344629f, 0.00196855f, 0.00095820f, 0.00039744f},
    {0.00344629f, 0.00318132f, 0.00250252f, 0.00167749f, 0.00095820f, 0.00046640f, 0.00019346f},
    {0.00142946f, 0.00131956f, 0.00103800f, 0.00069579f, 0.00039744f, 0.00019346f, 0.00008024f}};

struct OrientTable {
    int8_t dx[109], dy[109];
};
constexpr OrientTable make_orient_table() {
    OrientTable t{};
    int k = 0;
    for (int i = -6; i <= 6; ++i)
        for (int j = -6; j <= 6; ++j)
            if (i * i + j * j < 36) {
                t.dy[k] = (int8_t)i;
                t.dx[k] = (int8_t)j;
                ++k;
            }
    return t;
}
__constant__ OrientTable c_orient = make_orient_table();

__device__ __forceinline__ float fast_atan2_deg(float y, float x) {
    const float p1 = 0.9997878412794807f * (float)(180 / 3.14159265358979323846);
    const float p3 = -0.3258083974640975f * (float)(180 / 3.14159265358979323846);
    const float p5 = 0.1555786518463281f * (float)(180 / 3.14159265358979323846);
    const float p7 = -0.04432655554792128f * (float)(180 / 3.14159265358979323846);
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + (float)2.2204460492503131e-16);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + (float)2.2204460492503131e-16);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

__global__ __launch_bounds__(256) void orientation_kernel(LevelTable T, apds_keypoint* __restrict__ kps, const int* __restrict__ range, int n_cap, size_t kp_bstride,
                                                          float ang_step, int nkeys, int xcd_ranges) {
    APDS_RAISE_WAVE_PRIORITY();
    const int begin = range ? bofs(range, T.bstride)[0] : 0;
    const int n = range ? min(bofs(range, T.bstride)[1], n_cap) : n_cap;
    kps = bofs(kps, kp_bstride);
    __shared__ float s_x[4][112], s_y[4][112];
    __shared__ float s_xs[4][112], s_ys[4][112];   // the same, in sorted order
    __shared__ uint8_t s_bin[4][112];
    __shared__ int s_start[4][44];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    KP_GROUP_LOOP(kb, begin, n, xcd_ranges) {   // block-uniform trip count
    const int ki = kb + wv;
    const bool live = ki < n;
    const apds_keypoint kp = kps[live ? ki : kb];
    const int lvl = kp.class_id;
    const int w = T.w[lvl], h = T.h[lvl];
    const float ratio = T.ratio[lvl];
    const int scale = __float2int_rn(0.5f * kp.size / ratio);
    const int x0 = __float2int_rn(kp.x / ratio), y0 = __float2int_rn(kp.y / ratio);
    const float2* __restrict__ Lxy = bofs(T.Lxy[lvl], T.bstride);
    const float rad = (float)(3.14159265358979323846 / 180);
    {
        // both of a lane's samples: table entries, then the two gathers, are in flight together (one round trip each)
        int si[2], sj[2];
        float wgt[2];
        float2 d[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int k = min(lane + 64 * u, 108);
            si[u] = c_orient.dy[k];
            sj[u] = c_orient.dx[k];
            wgt[u] = c_gauss25[si[u] < 0 ? -si[u] : si[u]][sj[u] < 0 ? -sj[u] : sj[u]];
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int y = clampi2(y0 + si[u] * scale, h), x = clampi2(x0 + sj[u] * scale, w);
            d[u] = Lxy[(size_t)y * w + x];
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int k = lane + 64 * u;
            if (k < 109) {
                const float rx = wgt[u] * d[u].x, ry = wgt[u] * d[u].y;
                const float ang = fast_atan2_deg(ry, rx) * rad;
                int b = (int)(ang / ang_step);
                if (b < 0 || b >= nkeys) b = 0;
                s_x[wv][k] = rx;
                s_y[wv][k] = ry;
                s_bin[wv][k] = (uint8_t)b;
            }
        }
    }
    wave_lds_phase();
    // counting sort, identical to idx[--cum[b]] = i for ascending i: within a bin the larger sample index comes first. Every lane
    // holds the bins of its samples lane and lane + 64. Which samples share a lane's bin comes from six bit-sliced ballots per sample
    // set (a bin is six bits: the lanes whose bin equals mine are the AND, over the bits, of the ballot or its complement) instead
    // of one ballot pair per bin (43 iterations): the masked population counts give a sample's place inside its bin and the bin's
    // size; the bins' sizes go through LDS (every sample of a bin writes the same number) to a 42-lane prefix scan -> the bins' starts.
    {
        const int bin0 = s_bin[wv][lane];
        const int bin1 = lane + 64 < 109 ? (int)s_bin[wv][lane + 64] : 63;   // 63: no sample (equal to no bin: they are < 42)
        unsigned long long eq00 = ~0ull, eq01 = ~0ull, eq10 = ~0ull, eq11 = ~0ull;   // eqXY: the lanes of set Y whose bin equals my binX
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const unsigned long long b0 = __ballot((bin0 >> k) & 1), b1 = __ballot((bin1 >> k) & 1);
            const unsigned long long n0 = ((bin0 >> k) & 1) ? 0ull : ~0ull, n1 = ((bin1 >> k) & 1) ? 0ull : ~0ull;   // complement unless my bit is set
            eq00 &= b0 ^ n0;
            eq01 &= b1 ^ n0;
            eq10 &= b0 ^ n1;
            eq11 &= b1 ^ n1;
        }
        const unsigned long long higher = ~((2ull << lane) - 1);   // lanes above this one (none for lane 63)
        const int in0 = __popcll(eq00 & higher) + __popcll(eq01);  // same-bin samples with a larger index: every sample lane' + 64 has one
        const int in1 = __popcll(eq11 & higher);
        if (lane < 44) s_start[wv][lane] = 0;
        wave_lds_phase();
        s_start[wv][bin0] = __popcll(eq00) + __popcll(eq01);       // the bin's size (the same number from every sample of the bin)
        if (bin1 < 42) s_start[wv][bin1] = __popcll(eq10) + __popcll(eq11);
        wave_lds_phase();
        int incl = lane < 42 ? s_start[wv][lane] : 0;
        const int mine = incl;
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        wave_lds_phase();
        if (lane < 43) s_start[wv][lane] = incl - mine;            // exclusive prefix: bin 42 (no sample) holds the total
        wave_lds_phase();
        // the samples' values go straight to their sorted places: the window sums below then read consecutive elements
        const int p0 = s_start[wv][bin0] + in0;
        s_xs[wv][p0] = s_x[wv][lane];
        s_ys[wv][p0] = s_y[wv][lane];
        if (bin1 < 42) {
            const int p1 = s_start[wv][bin1] + in1;
            s_xs[wv][p1] = s_x[wv][lane + 64];
            s_ys[wv][p1] = s_y[wv][lane + 64];
        }
    }
    wave_lds_phase();
    float sumX = 0.0f, sumY = 0.0f, norm = -1.0f;
    if (lane < 42) {
        const int sn = lane, win = 7, slices = 42;
        const int* st = s_start[wv];
        if (sn <= slices - win) {
            for (int i = st[sn]; i < st[sn + win]; i++) {
                sumX += s_xs[wv][i];
                sumY += s_ys[wv][i];
            }
        } else {
            const int remain = sn + win - slices;
            for (int i = st[sn]; i < st[slices]; i++) {
                sumX += s_xs[wv][i];
                sumY += s_ys[wv][i];
            }
            for (int i = st[0]; i < st[remain]; i++) {
                sumX += s_xs[wv][i];
                sumY += s_ys[wv][i];
            }
        }
        norm = sumX * sumX + sumY * sumY;
    }
    // arg max over windows, the first window wins ties (the reference only replaces on strictly greater)
    int best = lane;
    for (int off = 32; off > 0; off >>= 1) {
        const float on = __shfl_xor(norm, off);
        const int ob = __shfl_xor(best, off);
        const float ox = __shfl_xor(sumX, off), oy = __shfl_xor(sumY, off);
        if (on > norm || (on == norm && ob < best)) {
            norm = on;
            best = ob;
            sumX = ox;
            sumY = oy;
        }
    }
    if (live && lane == 0) kps[ki].angle = fast_atan2_deg(sumY, sumX);
    wave_lds_phase();   // the next keypoint reuses the wave's LDS slices
    }
}

// ---- a1.9 M-LDB 486-bit descriptor: one wave per keypoint ----------------------------------------------------------
struct MldbLut {
    uint8_t a[488], b[488];
};
constexpr MldbLut make_mldb_lut() {
    MldbLut L{};
    int dpos = 0, base = 0;
    for (int g = 0; g < 3; g++) {
        const int cnt = (g + 2) * (g + 2);
        for (int pos = 0; pos < 3; pos++)
            for (int i = 0; i < cnt; i++)
                for (int j = i + 1; j < cnt; j++) {
                    L.a[dpos] = (uint8_t)(base + 3 * i + pos);
                    L.b[dpos] = (uint8_t)(base + 3 * j + pos);
                    dpos++;
                }
        base += 3 * cnt;
    }
    return L;
}
__constant__ MldbLut c_mldb = make_mldb_lut();

// One wave per keypoint. The three grids (2x2, 3x3, 4x4 cells of 10^2, 7^2, 5^2 samples) take their samples from the same
// lattice of offsets (k, l) in [-10, 11)^2 around the keypoint -- the 2x2 and 4x4 grids use its [-10, 10)^2 part, the 3x3 grid
// all of it -- and a sample depends on (k, l) only. So the 441 lattice samples (Lt, rotated Lx/Ly) are gathered ONCE into LDS
// by all 64 lanes (they were gathered 1241 times, once per grid), then 29 lanes, one per cell of any grid, add their cell's
// samples in the reference's order (k-major, l-minor; float sums are order dependent), and the 486 comparisons are done 32
// per lane.
// What bounds it (4096^2 frame, 35 k keypoints, 237 us; profiles/r03/mldb_decomposition.txt): with every gather pointed at one cache line
// the kernel takes 92 us, without the cell sums it still takes 239, with neither 67 - the 145 us are gather misses and everything else
// hides behind them. The patches of 25 k octave-0 keypoints (42 - 63 pixels square, one sample every 2 - 3 pixels) cover most of the four
// octave-0 levels, so the kernel reads nearly all of their Lt and Lx/Ly planes (~0.9 GB) once, in scattered 128-byte lines: ~3.8 TB/s of
// HBM. Walking the lattice in the direction closest to the image's rows for the keypoint's angle (fewer lines per load) changed nothing,
// and neither did dropping the block-wide barriers: the bytes have to come from HBM whatever the order.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 8))) void mldb_kernel(LevelTable T, const apds_keypoint* __restrict__ kps, const int* __restrict__ range, int n_cap, size_t kp_bstride,
                                                   uint32_t* __restrict__ desc64, size_t desc_bstride, int xcd_ranges) {
    APDS_RAISE_WAVE_PRIORITY();
    const int begin = range ? bofs(range, T.bstride)[0] : 0;
    const int n = range ? min(bofs(range, T.bstride)[1], n_cap) : n_cap;
    kps = bofs(kps, kp_bstride);
    desc64 = bofs(desc64, desc_bstride);
    constexpr int LW = 21;                     // lattice width: offsets -10 .. 10
    // per wave: the three sampled values of every lattice point as separate planes (an invalid point holds zeros) and the validity bitmap.
    // A plane has 25 rows (+): the cell loops below run over a fixed 10 x 10 window whatever the cell's size and mask what lies outside it.
    constexpr int PL = 25 * LW + 6;            // plane pitch (odd: the three planes of a point sit in different banks); the last window read is 24 * 21 + 24
    __shared__ float s_samp[4][3 * PL];
    __shared__ uint32_t s_bits[4][16];
    __shared__ int s_val[4][88];
    __shared__ uint8_t s_lut[976];              // c_mldb: a[488] then b[488]
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // the comparison table goes to LDS once per block (lane-indexed reads of __constant__ data are global loads)
    for (int i = threadIdx.x; i < 244; i += 256) reinterpret_cast<uint32_t*>(s_lut)[i] = reinterpret_cast<const uint32_t*>(&c_mldb)[i];
    for (int i = lane; i < 3 * PL; i += 64) s_samp[wv][i] = 0.0f;   // the rows past the lattice stay zero
    if (lane < 16) s_bits[wv][lane] = 0;
    __syncthreads();
    // chain = (cell, component): cells 0..3 the 2x2 grid (10 x 10 samples each), 4..12 the 3x3 grid (7 x 7), 13..28 the 4x4 grid (5 x 5);
    // 87 chains: lanes take chains 0..63 in a first pass (all sizes), chains 64..86 (4x4 cells only) in a second
    auto chain_geometry = [](int chain, int& step, int& base) {
        const int cell_all = chain / 3, comp = chain - 3 * cell_all;
        const int g = cell_all < 4 ? 0 : (cell_all < 13 ? 1 : 2);
        const int cell = cell_all - (g == 0 ? 0 : (g == 1 ? 4 : 13));
        const int side = g + 2;
        step = g == 0 ? 10 : (g == 1 ? 7 : 5);
        base = comp * PL + ((cell / side) * step) * LW + (cell % side) * step;
    };
    int step1, base1, step2, base2;
    chain_geometry(lane, step1, base1);
    chain_geometry(min(64 + lane, 86), step2, base2);
    KP_GROUP_LOOP(kb, begin, n, xcd_ranges) {   // block-uniform trip count
    const int ki = kb + wv;
    const bool live = ki < n;
    const apds_keypoint kp = kps[live ? ki : kb];
    const int lvl = kp.class_id;
    const int w = T.w[lvl], h = T.h[lvl];
    const float* __restrict__ Lt = bofs(T.Lt[lvl], T.bstride);
    const float2* __restrict__ Lxy = bofs(T.Lxy[lvl], T.bstride);
    const float ratio = (float)(1 << kp.octave);
    const float scale = (float)__float2int_rn(0.5f * kp.size / ratio);
    const float xf = kp.x / ratio, yf = kp.y / ratio;
    const float angle = kp.angle * (float)(3.14159265358979323846 / 180.f);
    double sd, cd;
    det_sincos((double)angle, sd, cd);
    const float co = (float)cd, si = (float)sd;
    {
        // all of a lane's lattice gathers are issued before the first LDS store: one memory round trip per keypoint, not seven
        constexpr int NS = (LW * LW + 63) / 64;
        float2 d[NS];
        float li[NS];
        bool ok[NS];
#pragma unroll
        for (int j = 0; j < NS; j++) {
            const int sidx = min(lane + 64 * j, LW * LW - 1);
            const int k = -10 + sidx / LW, l = -10 + sidx % LW;
            const float sample_y = yf + (l * co * scale + k * si * scale);
            const float sample_x = xf + (-l * si * scale + k * co * scale);
            const int y1 = __float2int_rn(sample_y), x1 = __float2int_rn(sample_x);
            ok[j] = !(y1 < 0 || y1 >= h || x1 < 0 || x1 >= w);
            const size_t o = ok[j] ? (size_t)y1 * w + x1 : 0;
            d[j] = Lxy[o];
            li[j] = Lt[o];
        }
#pragma unroll
        for (int j = 0; j < NS; j++) {
            const int sidx = lane + 64 * j;
            const bool in = sidx < LW * LW;
            const unsigned long long m = __ballot(in && ok[j]);
            if (lane == 0) {
                s_bits[wv][2 * j] = (uint32_t)m;
                s_bits[wv][2 * j + 1] = (uint32_t)(m >> 32);
            }
            if (in) {
                float vi = 0.f, vx = 0.f, vy = 0.f;
                if (ok[j]) {
                    const float rx = d[j].x, ry = d[j].y;
                    vi = li[j];
                    vx = -rx * si + ry * co;   // rrx
                    vy = rx * co + ry * si;    // rry
                }
                s_samp[wv][sidx] = vi;
                s_samp[wv][PL + sidx] = vx;
                s_samp[wv][2 * PL + sidx] = vy;
            }
        }
    }
    wave_lds_phase();
    // Cell sums in the reference's order (row-major over the cell's samples, one running sum per value). An invalid sample contributes
    // +0: a running sum that starts at +0 is never -0 (x + y is -0 only if both are), so adding +0 never changes it — the reference
    // skips those samples. The loops run over a fixed 10 x 10 window with static LDS offsets; a chain masks what is outside its cell.
    {
        float acc1 = 0.0f, acc2 = 0.0f;
        const float* p1 = &s_samp[wv][base1];
        const float* p2 = &s_samp[wv][base2];
#pragma unroll 1
        for (int a = 0; a < 10; a++) {      // (a row at a time: fully unrolled, the compiler hoists all hundred loads and spills)
            const float* row = p1 + a * LW;
            const bool row_in = a < step1;
#pragma unroll
            for (int b = 0; b < 10; b++) {
                const float v = row[b];
                acc1 += (row_in && b < step1) ? v : 0.0f;
            }
        }
#pragma unroll
        for (int a = 0; a < 5; a++)
#pragma unroll
            for (int b = 0; b < 5; b++) acc2 += p2[a * LW + b];
        // the number of valid samples of a cell, from the validity bitmap (lane = cell)
        int nsamples = 0;
        if (lane < 29) {
            int st, bs;
            chain_geometry(3 * lane, st, bs);
            for (int a = 0; a < st; a++) {
                const int pos = bs + a * LW;          // (component 0: bs is the cell's first lattice index)
                const unsigned long long two = (unsigned long long)s_bits[wv][(pos >> 5) + 1] << 32 | s_bits[wv][pos >> 5];
                nsamples += __popcll((two >> (pos & 31)) & ((1ull << st) - 1));
            }
        }
        // chain c's cell count sits in lane c / 3
        const int n1 = __shfl(nsamples, lane / 3), n2 = __shfl(nsamples, min(64 + lane, 86) / 3);
        if (n1 > 0) acc1 *= 1.0f / n1;
        if (n2 > 0) acc2 *= 1.0f / n2;
        const int v1 = __float_as_int(acc1), v2 = __float_as_int(acc2);
        s_val[wv][lane] = v1 ^ (v1 < 0 ? 0x7fffffff : 0);   // CV_TOGGLE_FLT: int order == float order
        if (lane < 23) s_val[wv][64 + lane] = v2 ^ (v2 < 0 ? 0x7fffffff : 0);
    }
    wave_lds_phase();
    // 486 comparisons: lane tests bits lane, lane + 64, ...; a ballot is two words of the descriptor
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int pos = 64 * j + lane;
        const bool bit = pos < 486 && s_val[wv][s_lut[min(pos, 487)]] > s_val[wv][s_lut[488 + min(pos, 487)]];
        const unsigned long long m = __ballot(bit);
        if (live && lane == 0) {
            desc64[(size_t)ki * 16 + 2 * j] = (uint32_t)m;      // 61 payload bytes + 3 zero bytes per 64-byte row
            desc64[(size_t)ki * 16 + 2 * j + 1] = (uint32_t)(m >> 32);
        }
    }
    wave_lds_phase();   // the next keypoint reuses the wave's LDS slices
    }
}

__global__ void pack_desc61_kernel(const uint8_t* __restrict__ d64, int n, uint8_t* __restrict__ d61) {
    APDS_RAISE_WAVE_PRIORITY();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * 61) return;
    const long long r = i / 61;
    d61[i] = d64[r * 64 + (i - r * 61)];
}

void pack_desc61_device(const uint8_t* d64, int n, uint8_t* d61, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(pack_desc61_kernel, dim3(ceil_div((long long)n * 61, 256)), dim3(256), 0, s, d64, n, d61);
}

void describe_keypoints(const LevelTable& T, apds_keypoint* kps, const int* range, int n_cap, size_t kp_bstride, uint8_t* desc, size_t desc_bstride,
                        int blocks, int batch, int xcd_ranges, hipStream_t s, int descriptor) {
    const float ang_step = (float)(2.0 * M_PI / 42);
    const int nkeys = (int)((float)(2.0 * M_PI) / ang_step);
    hipLaunchKernelGGL(orientation_kernel, dim3(blocks, 1, batch), dim3(256), 0, s, T, kps, range, n_cap, kp_bstride, ang_step, nkeys, xcd_ranges);
    if (descriptor == APDS_AKAZE_DESCRIPTOR_KAZE) {
        launch_msurf(T, kps, range, n_cap, kp_bstride, reinterpret_cast<float*>(desc), desc_bstride, blocks, batch, xcd_ranges, -1, s);
        return;
    }
    hipLaunchKernelGGL(mldb_kernel, dim3(blocks, 1, batch), dim3(256), 0, s, T, (const apds_keypoint*)kps, range, n_cap, kp_bstride,
                       reinterpret_cast<uint32_t*>(desc), desc_bstride, xcd_ranges);
}
}  // namespace apds
