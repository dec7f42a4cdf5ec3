// csrc/ransac_loop.h — the part of the robust estimators that has to agree with OpenCV iteration by iteration, written once and host only:
// cv::RNG, RANSACUpdateNumIters, the subset draws of findHomography and solvePnPRansac (ptsetreg.cpp, fundam.cpp) and the speculative
// RANSAC loop that homography.hip and pnp.hip both run. No HIP header and no HIP call: g++ compiles it into the host library of
// tests/test_ransac_loop_cpu.py (tests/cpp/ransac_loop_host.cpp), which pins it to the oracle without a device.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#ifdef __HIPCC__
#define APDS_RANSAC_HD __host__ __device__
#else
#define APDS_RANSAC_HD
#endif

namespace apds {

// cv::RNG (multiply-with-carry). A zero seed is mapped as cv::RNG's constructor maps it. Also used in device code (pnp_core.h).
struct CvRng {
    uint64_t state;
    APDS_RANSAC_HD explicit CvRng(uint64_t s) : state(s ? s : 0xffffffffULL) {}
    APDS_RANSAC_HD unsigned next() {
        state = (uint64_t)(unsigned)state * 4164903690U + (unsigned)(state >> 32);
        return (unsigned)state;
    }
    int uniform(int a, int b) { return a == b ? a : (int)(next() % (unsigned)(b - a) + a); }
};

// ptsetreg.cpp RANSACUpdateNumIters
inline int update_num_iters(double p, double ep, int modelPoints, int maxIters) {
    p = std::min(std::max(p, 0.), 1.);
    ep = std::min(std::max(ep, 0.), 1.);
    double num = std::max(1. - p, DBL_MIN);
    double denom = 1. - std::pow(1. - ep, modelPoints);
    if (denom < DBL_MIN) return 0;
    num = std::log(num);
    denom = std::log(denom);
    return denom >= 0 || -num >= maxIters * (-denom) ? maxIters : (int)lrint(num / denom);
}

// ---- solvePnPRansac's draw: getSubset with the default checkSubset, `model_points` distinct indices (one attempt of findHomography's) -----
inline void next_sample(int count, int* idx, CvRng& rng, int model_points) {
    for (int i = 0; i < model_points; ++i) {
        int v;
        for (v = rng.uniform(0, count); std::find(idx, idx + i, v) != idx + i; v = rng.uniform(0, count)) {
        }
        idx[i] = v;
    }
}

// ---- findHomography's draw: four distinct indices that pass HomographyEstimatorCallback::checkSubset, within an attempt limit ------------
// P: a point with float members x, y
template <class P>
bool have_collinear(const P* ptr, int count) {
    const int i = count - 1;
    for (int j = 0; j < i; j++) {
        const double dx1 = ptr[j].x - ptr[i].x, dy1 = ptr[j].y - ptr[i].y;
        for (int k = 0; k < j; k++) {
            const double dx2 = ptr[k].x - ptr[i].x, dy2 = ptr[k].y - ptr[i].y;
            if (std::fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (std::fabs(dx1) + std::fabs(dy1) + std::fabs(dx2) + std::fabs(dy2))) return true;
        }
    }
    return false;
}

inline double det3(const double* a) {
    return a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
}

template <class P>
bool check_subset(const P* s, const P* d, int count) {
    if (have_collinear(s, count) || have_collinear(d, count)) return false;
    if (count == 4) {
        static const int tt[][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
        int negative = 0;
        for (int i = 0; i < 4; i++) {
            const int* t = tt[i];
            const double A[9] = {s[t[0]].x, s[t[0]].y, 1., s[t[1]].x, s[t[1]].y, 1., s[t[2]].x, s[t[2]].y, 1.};
            const double B[9] = {d[t[0]].x, d[t[0]].y, 1., d[t[1]].x, d[t[1]].y, 1., d[t[2]].x, d[t[2]].y, 1.};
            negative += det3(A) * det3(B) < 0;
        }
        if (negative != 0 && negative != 4) return false;
    }
    return true;
}

template <class P>
bool get_subset(const P* m1, const P* m2, int count, int* idx, CvRng& rng, int maxAttempts) {
    P ms1[4], ms2[4];
    for (int iters = 0; iters < maxAttempts; ++iters) {
        next_sample(count, idx, rng, 4);
        for (int i = 0; i < 4; ++i) ms1[i] = m1[idx[i]], ms2[i] = m2[idx[i]];
        if (check_subset(ms1, ms2, 4)) return true;
    }
    return false;
}

// ---- the loop --------------------------------------------------------------------------------------------------------------------------
struct RansacResult {
    bool found = false;
    int max_good = 0;            // inlier count of the best model
    int iters = 0;               // iterations of the sequential loop that were replayed
    std::vector<double> model;   // model_doubles values of the best model (zeros when none was found)
};

// RANSACPointSetRegistrator::run, speculated: the sample stream does not depend on the scores, so the samples of a whole batch are drawn
// ahead and scored at once, and the sequential loop (`good > max(maxGood, model_points - 1)`, RANSACUpdateNumIters) is replayed over the
// batch's counts in iteration order. Samples speculated beyond a shortened budget are discarded, so the model, its count and the
// iteration the loop ends on are those of the sequential loop.
//   draw(int* idx) -> bool                               one sample of model_points indices; false: no admissible subset (getSubset failed)
//   evaluate(const int* idx, int B, int* good, uint8_t* valid, double* models)
//                                                        the B drawn samples -> inlier counts, whether a sample has a model, the models
// The first batch holds up to first_batch samples, every later one up to later_batch. A draw that fails at iteration 0 gives no model; a
// later one ends the loop after the samples drawn before it are scored, with the best model so far.
template <class Draw, class Evaluate>
RansacResult speculative_ransac(int n, int model_points, int model_doubles, int max_iters, double confidence, int first_batch, int later_batch, Draw&& draw,
                                Evaluate&& evaluate) {
    RansacResult r;
    r.model.assign(model_doubles, 0.0);
    int niters = std::max(max_iters, 1);
    const size_t cap = (size_t)std::max(first_batch, later_batch);
    std::vector<int> idx(cap * model_points), good(cap);
    std::vector<uint8_t> valid(cap);
    std::vector<double> models(cap * model_doubles);
    bool draw_failed = false;
    while (!draw_failed && r.iters < niters) {
        const int batch = r.iters == 0 ? first_batch : later_batch;
        int B = 0;
        for (; B < batch && r.iters + B < niters; B++)
            if (!draw(&idx[(size_t)B * model_points])) {
                draw_failed = true;
                break;
            }
        if (B == 0) break;
        evaluate(idx.data(), B, good.data(), valid.data(), models.data());
        for (int b = 0; b < B && r.iters < niters; b++, r.iters++) {
            if (!valid[b] || good[b] <= std::max(r.max_good, model_points - 1)) continue;
            std::memcpy(r.model.data(), &models[(size_t)b * model_doubles], sizeof(double) * model_doubles);
            r.max_good = good[b];
            r.found = true;
            niters = update_num_iters(confidence, (double)(n - good[b]) / n, model_points, niters);
        }
    }
    return r;
}

}  // namespace apds
