// csrc/homography.h — what homography.hip (kernels of the estimators, driver) and homography_refit.hip (the final refit) share.
#pragma once
#include <vector>

#include "common.h"

namespace apds {

struct P2 {
    float x, y;
};

// the one dense helper both the cooperative 4-point solve and the refit's Jacobi use
__host__ __device__ inline double hypot_cv(double a, double b) {
    a = fabs(a);
    b = fabs(b);
    if (a > b) {
        b /= a;
        return a * sqrt(1 + b * b);
    }
    if (b > 0) {
        a /= b;
        return b * sqrt(1 + a * a);
    }
    return 0;
}

// Sums over the selected points. Large selections: two-stage parallel f64 reductions on the device (reduce_kernel). Small
// ones (<= HOST_REFIT_MAX points, where the refit is poorly conditioned and every rounding shows): a plain loop on the host
// over the compressed points in index order, with the associations of the sequential algorithm (J^T J and |r|^2 accumulate
// row by row, i.e. the x and y residual of a point in two steps), which makes the result bit-identical to the CPU restatement.
constexpr int HOST_REFIT_MAX = 256;

struct RedParams;

// The refit of a model over the points `mask` selects (all of them when null): on the device, or, once `host` is set, over selM / selm.
struct Refit {
    const P2 *M, *m;   // device
    int n;
    hipStream_t s;
    const uint8_t* mask = nullptr;   // device
    bool host = false;
    std::vector<P2> selM, selm;   // host: the selected (inlier) pairs, compressed, index order

    Refit(const P2* M, const P2* m, int n, hipStream_t s);   // takes its reduction scratch from the calling thread's workspace
    int selected();                                          // how many points the mask selects (a device reduction)
    int run_kernel(double* H);                               // HomographyEstimatorCallback::runKernel over the selection; 0 when degenerate
    void lm_refine(double* H, int maxIters);                 // LMSolver::run (levmarq.cpp), 8 parameters, eps FLT_EPSILON

private:
    double* pd;   // per-block partial sums, device
    std::vector<double> ph;
    double rinf_last = 0;   // |r|_inf of the last normal_eq call
    void sums(const RedParams& P, int K, double* r);
    void normal_eq(const double* h, double* A, double* v, double& S, bool need_J);
};

}  // namespace apds
