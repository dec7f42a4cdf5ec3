// csrc/homography_refit.hip — the final refit of findHomography (homography.h: Refit): HomographyEstimatorCallback::runKernel over all
// selected points and the Levenberg-Marquardt polish (HomographyRefineCallback, LMSolver), on gfx950.
//
// The per-point sums (centroids, scales, 9x9 normal equations, J^T J, J^T r, residuals) are deterministic two-stage reductions on the
// device, or a plain host loop for small selections; the O(1)-size linear algebra (9x9 Jacobi, 8x8 solves) runs on the host.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "homography.h"

namespace apds {

// Array accessor of the dense helpers below (which take any indexable)
template <class T>
struct PlainArr {
    T* p;
    __host__ __device__ T& operator[](int i) const { return p[i]; }
};

// Symmetric eigen decomposition, pivoted Jacobi rotations (cv::eigen's JacobiImpl_ restated). A: N x N, upper
// triangle used and destroyed. W: eigenvalues descending. V rows: eigenvectors. indR/indC: N ints of scratch each.
template <int N, class MA, class MW, class MV, class MI>
__host__ __device__ inline void jacobi_eigen(MA A, MW W, MV V, MI indR, MI indC) {
    const double eps = 2.2204460492503131e-16;
    for (int i = 0; i < N; i++) {
        for (int j = 0; j < N; j++) V[i * N + j] = 0;
        V[i * N + i] = 1;
    }
    for (int k = 0; k < N; k++) {
        W[k] = A[(N + 1) * k];
        if (k < N - 1) {
            int m = k + 1;
            double mv = fabs(A[N * k + m]);
            for (int i = k + 2; i < N; i++) {
                const double val = fabs(A[N * k + i]);
                if (mv < val) mv = val, m = i;
            }
            indR[k] = m;
        }
        if (k > 0) {
            int m = 0;
            double mv = fabs(A[k]);
            for (int i = 1; i < k; i++) {
                const double val = fabs(A[N * i + k]);
                if (mv < val) mv = val, m = i;
            }
            indC[k] = m;
        }
    }
    const int maxIters = N * N * 30;
    for (int iters = 0; iters < maxIters; iters++) {
        int k = 0;
        double mv = fabs(A[indR[0]]);
        for (int i = 1; i < N - 1; i++) {
            const double val = fabs(A[N * i + indR[i]]);
            if (mv < val) mv = val, k = i;
        }
        int l = indR[k];
        for (int i = 1; i < N; i++) {
            const double val = fabs(A[N * indC[i] + i]);
            if (mv < val) mv = val, k = indC[i], l = i;
        }
        const double p = A[N * k + l];
        if (fabs(p) <= eps) break;
        const double y = (W[l] - W[k]) * 0.5;
        double t = fabs(y) + hypot_cv(p, y);
        double s = hypot_cv(p, t);
        const double c = t / s;
        s = p / s;
        t = (p / t) * p;
        if (y < 0) s = -s, t = -t;
        A[N * k + l] = 0;
        W[k] -= t;
        W[l] += t;
        double a0, b0;
#define APDS_ROT(v0, v1) a0 = v0, b0 = v1, v0 = a0 * c - b0 * s, v1 = a0 * s + b0 * c
        for (int i = 0; i < k; i++) APDS_ROT(A[N * i + k], A[N * i + l]);
        for (int i = k + 1; i < l; i++) APDS_ROT(A[N * k + i], A[N * i + l]);
        for (int i = l + 1; i < N; i++) APDS_ROT(A[N * k + i], A[N * l + i]);
        for (int i = 0; i < N; i++) APDS_ROT(V[N * k + i], V[N * l + i]);
#undef APDS_ROT
        for (int j = 0; j < 2; j++) {
            const int idx = j == 0 ? k : l;
            if (idx < N - 1) {
                int m = idx + 1;
                double mv2 = fabs(A[N * idx + m]);
                for (int i = idx + 2; i < N; i++) {
                    const double val = fabs(A[N * idx + i]);
                    if (mv2 < val) mv2 = val, m = i;
                }
                indR[idx] = m;
            }
            if (idx > 0) {
                int m = 0;
                double mv2 = fabs(A[idx]);
                for (int i = 1; i < idx; i++) {
                    const double val = fabs(A[N * i + idx]);
                    if (mv2 < val) mv2 = val, m = i;
                }
                indC[idx] = m;
            }
        }
    }
    for (int k = 0; k < N - 1; k++) {
        int m = k;
        for (int i = k + 1; i < N; i++)
            if (W[m] < W[i]) m = i;
        if (k != m) {
            const double tw = W[m];
            W[m] = W[k];
            W[k] = tw;
            for (int i = 0; i < N; i++) {
                const double tv = V[N * m + i];
                V[N * m + i] = V[N * k + i];
                V[N * k + i] = tv;
            }
        }
    }
}

// smallest eigenvector of LtL -> denormalised H with H[8] == 1
template <class MA, class MW, class MV, class MI>
__host__ __device__ inline void homography_from_ltl(MA LtL /*81, full symmetric*/, MW W, MV V, MI indR, MI indC,
                                                    const double* norm /*cmx,cmy,cMx,cMy,smx,smy,sMx,sMy*/, double* Hout) {
    jacobi_eigen<9>(LtL, W, V, indR, indC);
    double H0[9];
    for (int i = 0; i < 9; i++) H0[i] = V[72 + i];
    const double invHnorm[9] = {1. / norm[4], 0, norm[0], 0, 1. / norm[5], norm[1], 0, 0, 1};
    const double Hnorm2[9] = {norm[6], 0, -norm[2] * norm[6], 0, norm[7], -norm[3] * norm[7], 0, 0, 1};
    double Ht[9], H[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += invHnorm[r * 3 + k] * H0[k * 3 + c];
            Ht[r * 3 + c] = s;
        }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += Ht[r * 3 + k] * Hnorm2[k * 3 + c];
            H[r * 3 + c] = s;
        }
    const double sc = 1. / H[8];
    for (int i = 0; i < 9; i++) Hout[i] = H[i] * sc;
}

// ---- deterministic reductions over (masked) points: per-block partial sums of K doubles ---------------------------
static constexpr int RED_BLOCKS = 64, RED_THREADS = 256, RED_MAXK = 46;

struct RedParams {
    int kind;        // 0 centroid sums, 1 abs deviations, 2 LtL, 3 LM normal equations, 4 LM residual only
    double p[8];     // kind 1: centroids (cmx,cmy,cMx,cMy); kind 2: cmx,cmy,cMx,cMy,smx,smy,sMx,sMy; kind 3/4: h[8]
};

template <int K, class F>
__device__ __forceinline__ void block_reduce_store(double (&acc)[K], double* __restrict__ partials, F) {
    __shared__ double s_part[RED_THREADS / 64][RED_MAXK];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; k++) {
        double v = acc[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) s_part[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double v = 0;
        for (int w = 0; w < RED_THREADS / 64; w++) v += s_part[w][threadIdx.x];
        partials[(size_t)blockIdx.x * RED_MAXK + threadIdx.x] = v;
    }
}

__device__ __forceinline__ void block_reduce_max_store(double v, double* __restrict__ partials, int slot) {
    __shared__ double s_max[RED_THREADS / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off));
    if (lane == 0) s_max[wv] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = 0;
        for (int w = 0; w < RED_THREADS / 64; w++) r = fmax(r, s_max[w]);
        partials[(size_t)blockIdx.x * RED_MAXK + slot] = r;
    }
}

__global__ __launch_bounds__(RED_THREADS) void reduce_kernel(const P2* __restrict__ M, const P2* __restrict__ m, const uint8_t* __restrict__ mask, int n,
                                                             RedParams P, double* __restrict__ partials) {
    APDS_RAISE_WAVE_PRIORITY();
    const int stride = gridDim.x * RED_THREADS;
    const int first = blockIdx.x * RED_THREADS + threadIdx.x;
    if (P.kind == 0) {
        double acc[5] = {0, 0, 0, 0, 0};
        for (int i = first; i < n; i += stride)
            if (!mask || mask[i]) {
                acc[0] += m[i].x; acc[1] += m[i].y; acc[2] += M[i].x; acc[3] += M[i].y; acc[4] += 1.0;
            }
        block_reduce_store<5>(acc, partials, 0);
    } else if (P.kind == 1) {
        double acc[4] = {0, 0, 0, 0};
        for (int i = first; i < n; i += stride)
            if (!mask || mask[i]) {
                acc[0] += fabs(m[i].x - P.p[0]); acc[1] += fabs(m[i].y - P.p[1]);
                acc[2] += fabs(M[i].x - P.p[2]); acc[3] += fabs(M[i].y - P.p[3]);
            }
        block_reduce_store<4>(acc, partials, 0);
    } else if (P.kind == 2) {
        double acc[45];
#pragma unroll
        for (int k = 0; k < 45; k++) acc[k] = 0;
        for (int i = first; i < n; i += stride)
            if (!mask || mask[i]) {
                const double x = (m[i].x - P.p[0]) * P.p[4], y = (m[i].y - P.p[1]) * P.p[5];
                const double X = (M[i].x - P.p[2]) * P.p[6], Y = (M[i].y - P.p[3]) * P.p[7];
                const double Lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x};
                const double Ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
                int q = 0;
#pragma unroll
                for (int j = 0; j < 9; j++)
#pragma unroll
                    for (int k = j; k < 9; k++) acc[q++] += Lx[j] * Lx[k] + Ly[j] * Ly[k];
            }
        block_reduce_store<45>(acc, partials, 0);
    } else {
        // HomographyRefineCallback::compute: residuals and Jacobian rows of the 8-parameter model
        double acc[45];
#pragma unroll
        for (int k = 0; k < 45; k++) acc[k] = 0;
        const double* h = P.p;
        double rinf = 0;
        for (int i = first; i < n; i += stride)
            if (!mask || mask[i]) {
                const double Mx = M[i].x, My = M[i].y;
                double ww = h[6] * Mx + h[7] * My + 1.;
                ww = fabs(ww) > 2.2204460492503131e-16 ? 1. / ww : 0;
                const double xi = (h[0] * Mx + h[1] * My + h[2]) * ww;
                const double yi = (h[3] * Mx + h[4] * My + h[5]) * ww;
                const double r0 = xi - m[i].x, r1 = yi - m[i].y;
                acc[44] += r0 * r0 + r1 * r1;
                rinf = fmax(rinf, fmax(fabs(r0), fabs(r1)));
                if (P.kind == 3) {
                    const double J0[8] = {Mx * ww, My * ww, ww, 0, 0, 0, -Mx * ww * xi, -My * ww * xi};
                    const double J1[8] = {0, 0, 0, Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi};
                    int q = 0;
#pragma unroll
                    for (int a = 0; a < 8; a++)
#pragma unroll
                        for (int b = a; b < 8; b++) acc[q++] += J0[a] * J0[b] + J1[a] * J1[b];
#pragma unroll
                    for (int a = 0; a < 8; a++) acc[36 + a] += J0[a] * r0 + J1[a] * r1;
                }
            }
        block_reduce_store<45>(acc, partials, 0);
        block_reduce_max_store(rinf, partials, 45);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
namespace {

// sum the per-block partials in block order (deterministic)
void run_reduce(const P2* M, const P2* m, const uint8_t* mask, int n, const RedParams& P, int K, double* out, double* partials_dev,
                double* partials_host, hipStream_t s) {
    hipLaunchKernelGGL(reduce_kernel, dim3(RED_BLOCKS), dim3(RED_THREADS), 0, s, M, m, mask, n, P, partials_dev);
    HIP_CHECK(hipMemcpyAsync(partials_host, partials_dev, sizeof(double) * RED_BLOCKS * RED_MAXK, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (int k = 0; k < K; k++) {
        double v = 0;
        for (int b = 0; b < RED_BLOCKS; b++) v += partials_host[b * RED_MAXK + k];
        out[k] = v;
    }
    if (P.kind >= 3) {   // slot 45 carries max |r| instead of a sum
        double v = 0;
        for (int b = 0; b < RED_BLOCKS; b++) v = std::max(v, partials_host[b * RED_MAXK + 45]);
        out[45] = v;
    }
}

// x = sum_i (v_i . b / w_i) v_i over eigenpairs with |w_i| > 2 eps sum(w)  (cv::solve / cv::invert, DECOMP_EIG)
void eig_solve8(const double* Asym, const double* b, int nb, double* x) {
    double A[64], W[8], V[64];
    int indR[8], indC[8];
    std::memcpy(A, Asym, sizeof(A));
    jacobi_eigen<8>(PlainArr<double>{A}, PlainArr<double>{W}, PlainArr<double>{V}, PlainArr<int>{indR}, PlainArr<int>{indC});
    double threshold = 0;
    for (int i = 0; i < 8; i++) threshold += W[i];
    threshold *= DBL_EPSILON * 2;
    for (int i = 0; i < 8 * nb; i++) x[i] = 0;
    for (int i = 0; i < 8; i++) {
        double wi = W[i];
        if (std::fabs(wi) <= threshold) continue;
        wi = 1 / wi;
        for (int c = 0; c < nb; c++) {
            double sdot = 0;
            for (int j = 0; j < 8; j++) sdot += V[i * 8 + j] * b[j * nb + c];
            sdot *= wi;
            for (int j = 0; j < 8; j++) x[j * nb + c] += sdot * V[i * 8 + j];
        }
    }
}

}  // namespace

Refit::Refit(const P2* M_, const P2* m_, int n_, hipStream_t s_)
    : M(M_), m(m_), n(n_), s(s_), pd(ctx().alloc_n<double>((size_t)RED_BLOCKS * RED_MAXK)), ph((size_t)RED_BLOCKS * RED_MAXK) {}

int Refit::selected() {
    RedParams P{};
    P.kind = 0;
    double r[8];
    run_reduce(M, m, mask, n, P, 5, r, pd, ph.data(), s);
    return (int)r[4];
}

void Refit::sums(const RedParams& P, int K, double* r) {
    if (!host) {
        run_reduce(M, m, mask, n, P, K, r, pd, ph.data(), s);
        return;
    }
    for (int k = 0; k < 46; k++) r[k] = 0;
    double rinf = 0;
    const double* h = P.p;
    for (size_t i = 0; i < selM.size(); i++) {
        const P2 Mi = selM[i], mi = selm[i];
        if (P.kind == 0) {
            r[0] += mi.x; r[1] += mi.y; r[2] += Mi.x; r[3] += Mi.y; r[4] += 1.0;
        } else if (P.kind == 1) {
            r[0] += std::fabs(mi.x - P.p[0]); r[1] += std::fabs(mi.y - P.p[1]);
            r[2] += std::fabs(Mi.x - P.p[2]); r[3] += std::fabs(Mi.y - P.p[3]);
        } else if (P.kind == 2) {
            const double x = (mi.x - P.p[0]) * P.p[4], y = (mi.y - P.p[1]) * P.p[5];
            const double X = (Mi.x - P.p[2]) * P.p[6], Y = (Mi.y - P.p[3]) * P.p[7];
            const double Lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x};
            const double Ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
            int q = 0;
            for (int j = 0; j < 9; j++)
                for (int k = j; k < 9; k++) r[q++] += Lx[j] * Lx[k] + Ly[j] * Ly[k];
        } else {
            const double Mx = Mi.x, My = Mi.y;
            double ww = h[6] * Mx + h[7] * My + 1.;
            ww = std::fabs(ww) > DBL_EPSILON ? 1. / ww : 0;
            const double xi = (h[0] * Mx + h[1] * My + h[2]) * ww;
            const double yi = (h[3] * Mx + h[4] * My + h[5]) * ww;
            const double r0 = xi - mi.x, r1 = yi - mi.y;
            r[44] += r0 * r0;
            r[44] += r1 * r1;
            rinf = std::max(rinf, std::max(std::fabs(r0), std::fabs(r1)));
            if (P.kind == 3) {
                const double J0[8] = {Mx * ww, My * ww, ww, 0, 0, 0, -Mx * ww * xi, -My * ww * xi};
                const double J1[8] = {0, 0, 0, Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi};
                int q = 0;
                for (int a = 0; a < 8; a++)
                    for (int b = a; b < 8; b++) {
                        r[q] += J0[a] * J0[b];
                        r[q] += J1[a] * J1[b];
                        q++;
                    }
                for (int a = 0; a < 8; a++) {
                    r[36 + a] += J0[a] * r0;
                    r[36 + a] += J1[a] * r1;
                }
            }
        }
    }
    r[45] = rinf;
}

// runKernel over the masked points: returns 0 when degenerate
int Refit::run_kernel(double* H) {
    RedParams P{};
    double r[46];
    P.kind = 0;
    sums(P, 5, r);
    const double count = r[4];
    if (count < 1) return 0;
    const double cmx = r[0] / count, cmy = r[1] / count, cMx = r[2] / count, cMy = r[3] / count;
    P.kind = 1;
    P.p[0] = cmx; P.p[1] = cmy; P.p[2] = cMx; P.p[3] = cMy;
    sums(P, 4, r);
    double smx = r[0], smy = r[1], sMx = r[2], sMy = r[3];
    if (std::fabs(smx) < DBL_EPSILON || std::fabs(smy) < DBL_EPSILON || std::fabs(sMx) < DBL_EPSILON || std::fabs(sMy) < DBL_EPSILON) return 0;
    smx = count / smx; smy = count / smy; sMx = count / sMx; sMy = count / sMy;
    P.kind = 2;
    P.p[4] = smx; P.p[5] = smy; P.p[6] = sMx; P.p[7] = sMy;
    sums(P, 45, r);
    double LtL[81];
    int q = 0;
    for (int j = 0; j < 9; j++)
        for (int k = j; k < 9; k++) LtL[j * 9 + k] = LtL[k * 9 + j] = r[q++];
    const double norm[8] = {cmx, cmy, cMx, cMy, smx, smy, sMx, sMy};
    double W9[9], V81[81];
    int indR[9], indC[9];
    homography_from_ltl(PlainArr<double>{LtL}, PlainArr<double>{W9}, PlainArr<double>{V81}, PlainArr<int>{indR}, PlainArr<int>{indC}, norm, H);
    return 1;
}

// kind 3: A = J^T J, v = J^T r, S = |r|^2 ; kind 4: S only
void Refit::normal_eq(const double* h, double* A, double* v, double& S, bool need_J) {
    RedParams P{};
    P.kind = need_J ? 3 : 4;
    for (int i = 0; i < 8; i++) P.p[i] = h[i];
    double r[46];
    sums(P, 45, r);
    S = r[44];
    rinf_last = r[45];
    if (need_J) {
        int q = 0;
        for (int a = 0; a < 8; a++)
            for (int b = a; b < 8; b++) A[a * 8 + b] = A[b * 8 + a] = r[q++];
        for (int a = 0; a < 8; a++) v[a] = r[36 + a];
    }
}

// LMSolver::run (levmarq.cpp), 8 parameters, maxIters 10, eps FLT_EPSILON
void Refit::lm_refine(double* H, int maxIters) {
    const int lx = 8;
    double x[8], xd[8], A[64], Ap[64], v[8], d[8], temp_d[8], D[8];
    for (int i = 0; i < 8; i++) x[i] = H[i];
    double S;
    normal_eq(x, A, v, S, true);
    double rinf = rinf_last;
    for (int i = 0; i < lx; i++) D[i] = A[i * 8 + i];
    const double Rlo = 0.25, Rhi = 0.75;
    double lambda = 1, lc = 0.75;
    int iter = 0;
    for (;;) {
        std::memcpy(Ap, A, sizeof(A));
        for (int i = 0; i < lx; i++) Ap[i * 8 + i] += lambda * D[i];
        eig_solve8(Ap, v, 1, d);
        for (int i = 0; i < lx; i++) xd[i] = x[i] - d[i];
        double Sd, dummyA[1], dummyv[1];
        normal_eq(xd, dummyA, dummyv, Sd, false);
        for (int a = 0; a < 8; a++) {
            double sacc = 0;
            for (int b = 0; b < 8; b++) sacc += A[a * 8 + b] * d[b];
            temp_d[a] = -sacc + 2 * v[a];
        }
        double dS = 0;
        for (int a = 0; a < 8; a++) dS += d[a] * temp_d[a];
        const double R = (S - Sd) / (std::fabs(dS) > DBL_EPSILON ? dS : 1);
        if (R > Rhi) {
            lambda *= 0.5;
            if (lambda < lc) lambda = 0;
        } else if (R < Rlo) {
            double t = 0;
            for (int a = 0; a < 8; a++) t += d[a] * v[a];
            double nu = (Sd - S) / (std::fabs(t) > DBL_EPSILON ? t : 1) + 2;
            nu = std::min(std::max(nu, 2.), 10.);
            if (lambda == 0) {
                double I8[64] = {0};
                for (int i = 0; i < 8; i++) I8[i * 8 + i] = 1;
                eig_solve8(A, I8, 8, Ap);
                double maxval = DBL_EPSILON;
                for (int i = 0; i < lx; i++) maxval = std::max(maxval, std::fabs(Ap[i * 8 + i]));
                lambda = lc = 1. / maxval;
                nu *= 0.5;
            }
            lambda *= nu;
        }
        if (Sd < S) {
            std::memcpy(x, xd, sizeof(x));
            normal_eq(x, A, v, S, true);
            rinf = rinf_last;
        }
        iter++;
        double dinf = 0;
        for (int i = 0; i < 8; i++) dinf = std::max(dinf, std::fabs(d[i]));
        const bool proceed = iter < maxIters && dinf >= FLT_EPSILON && rinf >= FLT_EPSILON;
        if (!proceed) break;
    }
    for (int i = 0; i < 8; i++) H[i] = x[i];
}

}  // namespace apds
