// csrc/homography.hip — findHomography (least squares / RANSAC / LMEDS) on gfx950.
//
// Replaces opencv::calib3d::find_homography behind homographier/src/homographier/mod.rs:243-250.
//
// Split of the work (speculative batched RANSAC that reproduces OpenCV's sequential result exactly):
//   host   : cv::RNG sample stream + subset checks (control flow, O(iterations)), replay of the adaptive
//            termination rule over per-hypothesis inlier counts, and the O(1)-size linear algebra of the final
//            refit (9x9 Jacobi, 8x8 Levenberg-Marquardt solves);
//   device : one thread per hypothesis solves the normalised 4-point DLT in f64 (same operation order as the
//            scalar algorithm => bit-identical models); the scoring kernel evaluates hypotheses x points
//            reprojection errors in f32 (points streamed from L2, 8 hypotheses held in SGPRs per block, inlier
//            counts by wave ballot + popcount, integer atomics => deterministic); inlier mask; all per-point
//            sums of the refit (centroids, scales, 9x9 normal equations, J^T J, J^T r, residuals) as
//            deterministic two-stage reductions.
// This file: the kernels of the estimators and the driver, one function per method. The sample stream, the termination rule and the
// speculative loop are host arithmetic shared with pnp.hip (ransac_loop.h); the refit is homography_refit.hip (homography.h).
// Everything sequential in OpenCV stays sequential in meaning: hypotheses are scored speculatively in batches
// and the winner is chosen by replaying `goodCount > max(best, 3)` / RANSACUpdateNumIters in iteration order.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "config.h"
#include "homography.h"
#include "kernels.h"
#include "ransac_loop.h"

namespace apds {

// ---- device kernels ------------------------------------------------------------------------------------------
// The 4-point solve, 16 lanes per sample (four samples per wave). The matrices stay in LDS, but
// the work inside one Jacobi rotation -- the row/column updates, the eigenvector update, the four pivot-index rescans -- is
// spread over the lanes, and every lane evaluates the (cheap, uniform) pivot scan and rotation parameters itself. Each
// element goes through exactly the operations of jacobi_eigen<9> in the same order, so the result is bit-identical to one
// thread running jacobi_eigen<9> alone (the host refit, the oracle). What it cannot change is the rotation COUNT: the stopping rule
// is |pivot| <= DBL_EPSILON in absolute terms, which the rounding noise of a 9x9 system with O(10) entries rarely reaches, so
// most samples run the full 9*9*30 = 2430 rotations (as they do in OpenCV); a rotation costs ~0.2 us here against ~0.3 us.
static constexpr int COOP_LANES = 16, COOP_PER_BLOCK = 16;

struct CoopSlot {
    double A[81], V[81], W[9];
    int indR[9], indC[9];
    int pad[2];
};

__device__ __forceinline__ double coop_l_entry(int row, int j, double x, double y, double X, double Y) {
    // row 0: Lx = {X, Y, 1, 0, 0, 0, -x*X, -x*Y, -x}; row 1: Ly = {0, 0, 0, X, Y, 1, -y*X, -y*Y, -y}
    const double u = row == 0 ? x : y;
    const int jj = row == 0 ? j : j - 3;
    if (j >= 6) return j == 6 ? -u * X : (j == 7 ? -u * Y : -u);
    if (jj < 0 || jj > 2) return 0.0;
    return jj == 0 ? X : (jj == 1 ? Y : 1.0);
}

__global__ __launch_bounds__(COOP_LANES* COOP_PER_BLOCK) void hypothesis_coop_kernel(const P2* __restrict__ M, const P2* __restrict__ m,
                                                                                    const int* __restrict__ idx4, int B, double* __restrict__ models,
                                                                                    uint8_t* __restrict__ valid) {
    APDS_RAISE_WAVE_PRIORITY();
    __shared__ CoopSlot s_slot[COOP_PER_BLOCK];
    const int g = threadIdx.x / COOP_LANES, li = threadIdx.x % COOP_LANES;
    const int h = blockIdx.x * COOP_PER_BLOCK + g;
    const bool live = h < B;
    volatile double* A = s_slot[g].A;
    volatile double* V = s_slot[g].V;
    volatile double* W = s_slot[g].W;
    volatile int* indR = s_slot[g].indR;
    volatile int* indC = s_slot[g].indC;
    constexpr int N = 9;
    const double eps = 2.2204460492503131e-16;
    // every lane of the group reads the four correspondences and normalises them (uniform work, identical results)
    P2 ms1[4], ms2[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int id = live ? idx4[h * 4 + j] : 0;
        ms1[j] = M[id];
        ms2[j] = m[id];
    }
    double cMx = 0, cMy = 0, cmx = 0, cmy = 0, sMx = 0, sMy = 0, smx = 0, smy = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        cmx += ms2[i].x; cmy += ms2[i].y;
        cMx += ms1[i].x; cMy += ms1[i].y;
    }
    cmx /= 4; cmy /= 4; cMx /= 4; cMy /= 4;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        smx += fabs(ms2[i].x - cmx); smy += fabs(ms2[i].y - cmy);
        sMx += fabs(ms1[i].x - cMx); sMy += fabs(ms1[i].y - cMy);
    }
    const bool ok = live && !(fabs(smx) < eps || fabs(smy) < eps || fabs(sMx) < eps || fabs(sMy) < eps);
    smx = 4 / smx; smy = 4 / smy;
    sMx = 4 / sMx; sMy = 4 / sMy;
    // normal equations: 45 upper-triangle entries over 16 lanes, each summed over the points in order
    for (int e = li; e < 45; e += COOP_LANES) {
        int j = 0, rem = e;
        while (rem >= N - j) {
            rem -= N - j;
            j++;
        }
        const int k = j + rem;
        double acc = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const double x = (ms2[i].x - cmx) * smx, y = (ms2[i].y - cmy) * smy;
            const double X = (ms1[i].x - cMx) * sMx, Y = (ms1[i].y - cMy) * sMy;
            acc += coop_l_entry(0, j, x, y, X, Y) * coop_l_entry(0, k, x, y, X, Y) + coop_l_entry(1, j, x, y, X, Y) * coop_l_entry(1, k, x, y, X, Y);
        }
        A[j * N + k] = acc;
        A[k * N + j] = acc;
    }
    for (int e = li; e < 81; e += COOP_LANES) V[e] = (e % 10 == 0) ? 1.0 : 0.0;
    __builtin_amdgcn_wave_barrier();
    if (li < N) {   // initial eigenvalues and pivot indices, one row / column per lane
        const int k = li;
        W[k] = A[(N + 1) * k];
        if (k < N - 1) {
            int mi = k + 1;
            double mv = fabs(A[N * k + mi]);
            for (int i = k + 2; i < N; i++) {
                const double val = fabs(A[N * k + i]);
                if (mv < val) mv = val, mi = i;
            }
            indR[k] = mi;
        }
        if (k > 0) {
            int mi = 0;
            double mv = fabs(A[k]);
            for (int i = 1; i < k; i++) {
                const double val = fabs(A[N * i + k]);
                if (mv < val) mv = val, mi = i;
            }
            indC[k] = mi;
        }
    }
    __builtin_amdgcn_wave_barrier();
    bool done = !ok;
    for (int iters = 0; iters < N * N * 30; iters++) {
        if (!__any(!done)) break;   // wave-uniform exit: every group of this wave has converged
        if (!done) {
            // pivot: the sequential scan of jacobi_eigen, evaluated by every lane (broadcast LDS reads). All loads of a level
            // are issued before the first compare, so the scan costs two LDS latencies instead of sixteen.
            int ir[N - 1], ic[N];
            double vr[N - 1], vc[N];
#pragma unroll
            for (int i = 0; i < N - 1; i++) ir[i] = indR[i];
#pragma unroll
            for (int i = 1; i < N; i++) ic[i] = indC[i];
#pragma unroll
            for (int i = 0; i < N - 1; i++) vr[i] = A[N * i + ir[i]];
#pragma unroll
            for (int i = 1; i < N; i++) vc[i] = A[N * ic[i] + i];
            int k = 0;
            double mv = fabs(vr[0]);
#pragma unroll
            for (int i = 1; i < N - 1; i++) {
                const double val = fabs(vr[i]);
                if (mv < val) mv = val, k = i;
            }
            int l = 0;
#pragma unroll
            for (int i = 0; i < N - 1; i++)
                if (i == k) l = ir[i];
#pragma unroll
            for (int i = 1; i < N; i++) {
                const double val = fabs(vc[i]);
                if (mv < val) mv = val, k = ic[i], l = i;
            }
            const double p = A[N * k + l];
            if (fabs(p) <= eps) {
                done = true;
            } else {
                const double y = (W[l] - W[k]) * 0.5;
                double t = fabs(y) + hypot_cv(p, y);
                double sn = hypot_cv(p, t);
                const double c = t / sn;
                sn = p / sn;
                t = (p / t) * p;
                if (y < 0) sn = -sn, t = -t;
                __builtin_amdgcn_wave_barrier();   // all lanes have read the pivot data before anything is modified
                if (li == 0) {
                    A[N * k + l] = 0;
                    W[k] = W[k] - t;
                    W[l] = W[l] + t;
                }
                if (li < N) {
                    const int i = li;
                    double a0, b0;
                    if (i < k) {
                        a0 = A[N * i + k], b0 = A[N * i + l];
                        A[N * i + k] = a0 * c - b0 * sn;
                        A[N * i + l] = a0 * sn + b0 * c;
                    } else if (i > k && i < l) {
                        a0 = A[N * k + i], b0 = A[N * i + l];
                        A[N * k + i] = a0 * c - b0 * sn;
                        A[N * i + l] = a0 * sn + b0 * c;
                    } else if (i > l) {
                        a0 = A[N * k + i], b0 = A[N * l + i];
                        A[N * k + i] = a0 * c - b0 * sn;
                        A[N * l + i] = a0 * sn + b0 * c;
                    }
                    a0 = V[N * k + i], b0 = V[N * l + i];
                    V[N * k + i] = a0 * c - b0 * sn;
                    V[N * l + i] = a0 * sn + b0 * c;
                }
                __builtin_amdgcn_wave_barrier();
                if (li < 4) {   // lanes 0..3: indR[k], indC[k], indR[l], indC[l]; loads first, then the scan in registers
                    const int idx = li < 2 ? k : l;
                    const bool rows = (li & 1) == 0;
                    double v[N - 1];
#pragma unroll
                    for (int q = 0; q < N - 1; q++) {
                        // row scan: elements (idx, q + 1) with q + 1 > idx; column scan: elements (q, idx) with q < idx
                        const int e = rows ? N * idx + min(max(q + 1, idx + 1), N - 1) : N * min(q, max(idx - 1, 0)) + idx;
                        v[q] = A[e];
                    }
                    if (rows) {
                        if (idx < N - 1) {
                            int mi = idx + 1;
                            double mv2 = 0;
                            bool first = true;
#pragma unroll
                            for (int q = 0; q < N - 1; q++) {
                                const int i = q + 1;
                                if (i > idx) {
                                    const double val = fabs(v[q]);
                                    if (first) mv2 = val, mi = i, first = false;
                                    else if (mv2 < val) mv2 = val, mi = i;
                                }
                            }
                            indR[idx] = mi;
                        }
                    } else if (idx > 0) {
                        int mi = 0;
                        double mv2 = fabs(v[0]);
#pragma unroll
                        for (int q = 1; q < N - 1; q++) {
                            if (q < idx) {
                                const double val = fabs(v[q]);
                                if (mv2 < val) mv2 = val, mi = q;
                            }
                        }
                        indC[idx] = mi;
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    // eigenvalues descending: selection sort, the row swaps of V spread over the lanes
    if (ok) {
        for (int k = 0; k < N - 1; k++) {
            int mi = k;
            for (int i = k + 1; i < N; i++)
                if (W[mi] < W[i]) mi = i;
            __builtin_amdgcn_wave_barrier();
            if (k != mi) {
                if (li == 0) {
                    const double tw = W[mi];
                    W[mi] = W[k];
                    W[k] = tw;
                }
                if (li < N) {
                    const double tv = V[N * mi + li];
                    V[N * mi + li] = V[N * k + li];
                    V[N * k + li] = tv;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (!live) return;
    double H[9];
    if (ok) {
        double H0[9];
        for (int i = 0; i < 9; i++) H0[i] = V[72 + i];
        const double invHnorm[9] = {1. / smx, 0, cmx, 0, 1. / smy, cmy, 0, 0, 1};
        const double Hnorm2[9] = {sMx, 0, -cMx * sMx, 0, sMy, -cMy * sMy, 0, 0, 1};
        double Ht[9], Hd[9];
        for (int r = 0; r < 3; r++)
            for (int cc = 0; cc < 3; cc++) {
                double sacc = 0;
                for (int kk = 0; kk < 3; kk++) sacc += invHnorm[r * 3 + kk] * H0[kk * 3 + cc];
                Ht[r * 3 + cc] = sacc;
            }
        for (int r = 0; r < 3; r++)
            for (int cc = 0; cc < 3; cc++) {
                double sacc = 0;
                for (int kk = 0; kk < 3; kk++) sacc += Ht[r * 3 + kk] * Hnorm2[kk * 3 + cc];
                Hd[r * 3 + cc] = sacc;
            }
        const double sc = 1. / Hd[8];
        for (int i = 0; i < 9; i++) H[i] = Hd[i] * sc;
    }
    if (li == 0) valid[h] = ok ? 1 : 0;
    if (li < 9) models[(size_t)h * 9 + li] = ok ? H[li] : 0.0;
}

__device__ __forceinline__ float reproj_err(const float (&Hf)[8], float Mx, float My, float mx, float my) {
    const float ww = 1.f / (Hf[6] * Mx + Hf[7] * My + 1.f);
    const float dx = (Hf[0] * Mx + Hf[1] * My + Hf[2]) * ww - mx;
    const float dy = (Hf[3] * Mx + Hf[4] * My + Hf[5]) * ww - my;
    return dx * dx + dy * dy;
}

static constexpr int HT = 8;   // hypotheses per block of the scoring kernel

// grid: x = ceil(B / HT), y = point parts. good[h] += #points with err <= t
__global__ __launch_bounds__(256) void score_kernel(const P2* __restrict__ M, const P2* __restrict__ m, int n, const double* __restrict__ models, int B,
                                                    float t, int* __restrict__ good) {
    APDS_RAISE_WAVE_PRIORITY();
    const int h0 = blockIdx.x * HT;
    float Hf[HT][8];
#pragma unroll
    for (int h = 0; h < HT; h++) {
        const int hh = min(h0 + h, B - 1);
#pragma unroll
        for (int j = 0; j < 8; j++) Hf[h][j] = (float)models[(size_t)hh * 9 + j];   // wave-uniform -> scalar registers
    }
    int cnt[HT];
#pragma unroll
    for (int h = 0; h < HT; h++) cnt[h] = 0;
    const int per = (n + gridDim.y - 1) / gridDim.y;
    const int i0 = blockIdx.y * per, i1 = min(n, i0 + per);
    for (int base = i0; base < i1; base += 256) {
        const int i = base + threadIdx.x;
        const bool in = i < i1;
        const P2 a = M[in ? i : i0], b = m[in ? i : i0];
#pragma unroll
        for (int h = 0; h < HT; h++) {
            const float e = reproj_err(Hf[h], a.x, a.y, b.x, b.y);
            cnt[h] += __popcll(__ballot(in && e <= t));
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int h = 0; h < HT; h++)
            if (h0 + h < B && cnt[h]) atomicAdd(&good[h0 + h], cnt[h]);
    }
}

__global__ void inlier_mask_kernel(const P2* __restrict__ M, const P2* __restrict__ m, int n, const double* __restrict__ model, float t,
                                   uint8_t* __restrict__ mask) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float Hf[8];
#pragma unroll
    for (int j = 0; j < 8; j++) Hf[j] = (float)model[j];
    mask[i] = reproj_err(Hf, M[i].x, M[i].y, m[i].x, m[i].y) <= t;
}

// all errors of one hypothesis (LMEDS): err[h*n + i]
__global__ void errors_kernel(const P2* __restrict__ M, const P2* __restrict__ m, int n, const double* __restrict__ models, float* __restrict__ err) {
    APDS_RAISE_WAVE_PRIORITY();
    const int h = blockIdx.y;
    float Hf[8];
#pragma unroll
    for (int j = 0; j < 8; j++) Hf[j] = (float)models[(size_t)h * 9 + j];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        err[(size_t)h * n + i] = reproj_err(Hf, M[i].x, M[i].y, m[i].x, m[i].y);
}

// exact k-th smallest of n non-negative floats per hypothesis (radix select on the bit pattern, 3 passes of 11/11/10 bits)
__global__ __launch_bounds__(1024) void kth_select_kernel(const float* __restrict__ err, int n, int kth, float* __restrict__ out) {
    APDS_RAISE_WAVE_PRIORITY();
    __shared__ unsigned int hist[2048];
    __shared__ unsigned int s_prefix, s_k;
    const unsigned int* e = reinterpret_cast<const unsigned int*>(err + (size_t)blockIdx.x * n);
    if (threadIdx.x == 0) {
        s_prefix = 0;
        s_k = (unsigned int)kth;
    }
    const int shifts[3] = {21, 10, 0};
    const int bits[3] = {11, 11, 10};
    unsigned int mask_hi = 0;
    for (int pass = 0; pass < 3; pass++) {
        for (int i = threadIdx.x; i < 2048; i += 1024) hist[i] = 0;
        __syncthreads();
        const unsigned int prefix = s_prefix;
        const int sh = shifts[pass];
        const unsigned int bm = (1u << bits[pass]) - 1;
        for (int i = threadIdx.x; i < n; i += 1024) {
            const unsigned int v = e[i];
            if ((v & mask_hi) == prefix) atomicAdd(&hist[(v >> sh) & bm], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int k = s_k, b = 0;
            for (; b <= bm; b++) {
                if (k < hist[b]) break;
                k -= hist[b];
            }
            s_k = k;
            s_prefix = prefix | (b << sh);
        }
        __syncthreads();
        mask_hi |= bm << sh;
    }
    if (threadIdx.x == 0) out[blockIdx.x] = __uint_as_float(s_prefix);
}

// ---- host side ----------------------------------------------------------------------------------------------------
namespace {

// One call's points: on the device, and a host copy that is fetched once, when a method needs it (the cv::RNG sample stream's subset checks
// read the coordinates; small refits run on the host).
struct Points {
    const P2 *M, *m;   // device
    int n;
    uint8_t* mask;     // device, n bytes
    hipStream_t s;
    std::vector<P2> hM, hm;

    void fetch() {
        if (!hM.empty()) return;
        hM.resize(n);
        hm.resize(n);
        HIP_CHECK(hipMemcpyAsync(hM.data(), M, (size_t)n * sizeof(P2), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(hm.data(), m, (size_t)n * sizeof(P2), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
};

void launch_hypotheses(const P2* M, const P2* m, const int* idx_dev, int B, double* models_dev, uint8_t* valid_dev, hipStream_t s) {
    hipLaunchKernelGGL(hypothesis_coop_kernel, dim3(ceil_div(B, COOP_PER_BLOCK)), dim3(COOP_LANES * COOP_PER_BLOCK), 0, s, M, m, idx_dev, B, models_dev, valid_dev);
}

// mask[i] = point i lies within t (squared pixels) of model H; model_dev: room for 9 doubles
void launch_mask(const Points& p, const double* H, float t, double* model_dev) {
    HIP_CHECK(hipMemcpyAsync(model_dev, H, 9 * sizeof(double), hipMemcpyHostToDevice, p.s));
    hipLaunchKernelGGL(inlier_mask_kernel, dim3(ceil_div(p.n, 256)), dim3(256), 0, p.s, p.M, p.m, p.n, (const double*)model_dev, t, p.mask);
}

// Few points: the refit runs on the host, over the pairs mask_dev selects (all pairs when null), compressed, in index order
void refit_on_host(Points& p, Refit& refit, const uint8_t* mask_dev) {
    p.fetch();
    std::vector<uint8_t> hmask(p.n, 1);
    if (mask_dev) {
        HIP_CHECK(hipMemcpyAsync(hmask.data(), mask_dev, p.n, hipMemcpyDeviceToHost, p.s));
        HIP_CHECK(hipStreamSynchronize(p.s));
    }
    refit.host = true;
    refit.selM.clear();
    refit.selm.clear();
    for (int i = 0; i < p.n; i++)
        if (hmask[i]) {
            refit.selM.push_back(p.hM[i]);
            refit.selm.push_back(p.hm[i]);
        }
}

// The methods: each leaves its model in H and the inlier mask in p.mask, and returns how many points the final refit runs over
// (-1: no model).

int least_squares(Points& p, Refit& refit, double* H) {
    HIP_CHECK(hipMemsetAsync(p.mask, 1, p.n, p.s));
    if (p.n <= HOST_REFIT_MAX) refit_on_host(p, refit, nullptr);
    return refit.run_kernel(H) > 0 ? p.n : -1;
}

int ransac(Points& p, double thr, int max_iters, double confidence, double* H) {
    p.fetch();
    CvRng rng((uint64_t)-1);
    const float t = (float)(thr * thr);
    // First batch: config().ransac_batch samples (with a fair inlier ratio the budget collapses to a few dozen iterations after the
    // first good model). Later batches cover the whole remaining budget, up to 4096 at once: a batch costs about the
    // same wall time whatever its size (one thread per sample, latency-bound), so low-inlier inputs that keep the
    // full budget finish in two round trips instead of max_iters / 512.
    const int first_batch = std::max(8, std::min(config().ransac_batch, std::max(max_iters, 8)));
    const int max_batch = std::max(first_batch, std::min(4096, std::max(max_iters, 8)));
    ThreadCtx& c = ctx();
    int* idx_dev = c.alloc_n<int>((size_t)max_batch * 4);
    double* models_dev = c.alloc_n<double>((size_t)max_batch * 9);
    uint8_t* valid_dev = c.alloc_n<uint8_t>(max_batch);
    int* good_dev = c.alloc_n<int>(max_batch);
    const hipStream_t s = p.s;
    auto draw = [&](int* idx) { return get_subset(p.hM.data(), p.hm.data(), p.n, idx, rng, 10000); };
    auto evaluate = [&](const int* idx, int B, int* good, uint8_t* valid, double* models) {
        HIP_CHECK(hipMemcpyAsync(idx_dev, idx, (size_t)B * 4 * sizeof(int), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(good_dev, 0, (size_t)B * sizeof(int), s));
        launch_hypotheses(p.M, p.m, idx_dev, B, models_dev, valid_dev, s);
        {
            KernelTimer timer("ransac_score", s);
            const int parts = std::max(1, std::min(64, ceil_div(256 * 8, ceil_div(B, HT))));
            hipLaunchKernelGGL(score_kernel, dim3(ceil_div(B, HT), parts), dim3(256), 0, s, p.M, p.m, p.n, (const double*)models_dev, B, t, good_dev);
        }
        HIP_CHECK(hipMemcpyAsync(good, good_dev, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(valid, valid_dev, (size_t)B, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(models, models_dev, (size_t)B * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    };
    const RansacResult r = speculative_ransac(p.n, 4, 9, max_iters, confidence, first_batch, max_batch, draw, evaluate);
    if (!r.found) return -1;
    std::memcpy(H, r.model.data(), 9 * sizeof(double));
    launch_mask(p, H, t, models_dev);
    return r.max_good;
}

// LMedSPointSetRegistrator::run: the budget is fixed before the first sample, so every sample is drawn and solved at once and the winner
// is the first model with the least median error (radix select per model); no controller.
int lmeds(Points& p, Refit& refit, int max_iters, double confidence, double* H) {
    p.fetch();
    CvRng rng((uint64_t)-1);
    const int n = p.n;
    const hipStream_t s = p.s;
    const double outlierRatio = 0.45;
    const int niters = std::max(update_num_iters(confidence, outlierRatio, 4, max_iters), 3);
    std::vector<int> idx((size_t)niters * 4);
    int B = 0;
    for (; B < niters; B++)
        if (!get_subset(p.hM.data(), p.hm.data(), n, &idx[(size_t)B * 4], rng, 1000)) break;
    if (B == 0) return -1;
    ThreadCtx& c = ctx();
    int* idx_dev = c.alloc_n<int>((size_t)B * 4);
    double* models_dev = c.alloc_n<double>((size_t)B * 9);
    uint8_t* valid_dev = c.alloc_n<uint8_t>(B);
    float* err_dev = c.alloc_n<float>((size_t)B * n);
    float* med_dev = c.alloc_n<float>(B);
    HIP_CHECK(hipMemcpyAsync(idx_dev, idx.data(), (size_t)B * 4 * sizeof(int), hipMemcpyHostToDevice, s));
    launch_hypotheses(p.M, p.m, idx_dev, B, models_dev, valid_dev, s);
    hipLaunchKernelGGL(errors_kernel, dim3(std::min(64, ceil_div(n, 256)), B), dim3(256), 0, s, p.M, p.m, n, (const double*)models_dev, err_dev);
    hipLaunchKernelGGL(kth_select_kernel, dim3(B), dim3(1024), 0, s, (const float*)err_dev, n, n / 2, med_dev);
    std::vector<float> med(B);
    std::vector<uint8_t> valid(B);
    std::vector<double> models((size_t)B * 9);
    HIP_CHECK(hipMemcpyAsync(med.data(), med_dev, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(valid.data(), valid_dev, (size_t)B, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(models.data(), models_dev, (size_t)B * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    double minMedian = DBL_MAX;
    for (int b = 0; b < B; b++) {
        if (!valid[b]) continue;
        const double median = med[b];
        if (median < minMedian) {
            minMedian = median;
            std::memcpy(H, &models[(size_t)b * 9], 9 * sizeof(double));
        }
    }
    if (!(minMedian < DBL_MAX)) return -1;
    double sigma = 2.5 * 1.4826 * (1 + 5. / (n - 4)) * std::sqrt(minMedian);
    sigma = std::max(sigma, 0.001);
    launch_mask(p, H, (float)(sigma * sigma), models_dev);
    refit.mask = p.mask;
    const int inliers = refit.selected();
    return inliers >= 4 ? inliers : -1;
}

}  // namespace

// returns 1 (model found; H_host filled, mask_dev filled if non-null) or 0 (none)
int find_homography_device(const float* src, const float* dst, int n, int method, double thr, int max_iters, double confidence, double* H_host,
                           uint8_t* mask_dev, hipStream_t s) {
    APDS_REQUIRE(src && dst && H_host, APDS_ERR_BAD_ARG, "null argument");
    APDS_REQUIRE(n >= 4, APDS_ERR_ASSERT, "at least 4 point pairs are required");
    APDS_REQUIRE(method == 0 || method == APDS_HOMOGRAPHY_LMEDS || method == APDS_HOMOGRAPHY_RANSAC || method == APDS_HOMOGRAPHY_RHO, APDS_ERR_BAD_ARG,
                 "unknown homography method");
    APDS_REQUIRE(confidence > 0 && confidence < 1, APDS_ERR_ASSERT, "confidence must be in (0,1)");
    if (method == APDS_HOMOGRAPHY_RHO && n > 4)   // its own estimator and refinement (homography_rho.hip); n == 4 is the plain solve, as in OpenCV
        return find_homography_rho_device(src, dst, n, thr, max_iters, confidence, H_host, mask_dev, s);
    if (thr <= 0) thr = 3;
    Points p{reinterpret_cast<const P2*>(src), reinterpret_cast<const P2*>(dst), n, mask_dev ? mask_dev : ctx().alloc_n<uint8_t>(n), s, {}, {}};
    Refit refit(p.M, p.m, n, s);

    int selected;   // points the final refit runs over (inliers), -1: no model
    if (method == 0 || n == 4)
        selected = least_squares(p, refit, H_host);
    else if (method == APDS_HOMOGRAPHY_RANSAC)
        selected = ransac(p, thr, max_iters, confidence, H_host);
    else
        selected = lmeds(p, refit, max_iters, confidence, H_host);
    HIP_CHECK(hipGetLastError());

    if (selected >= 0 && n > 4) {
        refit.mask = p.mask;
        if (!refit.host && selected <= HOST_REFIT_MAX) refit_on_host(p, refit, p.mask);   // few inliers: refit on the host in index order
        if (method == APDS_HOMOGRAPHY_RANSAC || method == APDS_HOMOGRAPHY_LMEDS) refit.run_kernel(H_host);
        refit.lm_refine(H_host, 10);
    }
    if (selected < 0) {
        HIP_CHECK(hipMemsetAsync(p.mask, 0, n, s));
        for (int i = 0; i < 9; i++) H_host[i] = 0;
    }
    HIP_CHECK(hipStreamSynchronize(s));
    return selected >= 0 ? 1 : 0;
}

}  // namespace apds
