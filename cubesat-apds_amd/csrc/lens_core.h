// csrc/lens_core.h — the lens model: OpenCV's radial-tangential (Brown-Conrady) distortion with the rational denominator, written once
// for the host and the device. Everything is binary64; the build has -ffp-contract=off, so every operation written below is ONE IEEE
// operation, rounded to nearest even, in exactly the order the parentheses give. No libm. tests/lens_reference.py restates these
// expressions in numpy, operation for operation, and the kernels are held to its bits.
//
// Coefficients in OpenCV's order (k1, k2, p1, p2[, k3[, k4, k5, k6]]); a shorter vector is padded with zeros and goes through the SAME
// expressions (adding a +0.0 product changes no bit of a non-zero sum), so there is one code path for 4, 5 and 8 coefficients.
// The camera matrix contributes fx = K[0], cx = K[2], fy = K[4], cy = K[5]; the skew K[1] is ignored, as OpenCV ignores it.
//
// Evaluation order (x, y normalised coordinates):
//   xx  = x * x                     yy  = y * y
//   r2  = xx + yy                   r4  = r2 * r2                  r6 = r4 * r2
//   num = ((1 + k1 * r2) + k2 * r4) + k3 * r6
//   den = ((1 + k4 * r2) + k5 * r4) + k6 * r6
//   rc  = num / den
//   a1  = (2 * x) * y               a2  = r2 + 2 * xx              a3 = r2 + 2 * yy
//   dx  = p1 * a1 + p2 * a2         dy  = p1 * a3 + p2 * a1        (the tangential part)
// normalise (pixel -> normalised):  x = (u - cx) / fx              y = (v - cy) / fy
// forward (ideal -> distorted):     xd = x * rc + dx               yd = y * rc + dy
// to pixels:                        u' = fx * xd + cx              v' = fy * yd + cy
// inverse (distorted -> ideal), cv::undistortPoints' fixed-point iteration: x0 = x = normalised distorted point; then exactly `iters`
// times, no early exit, with rc, dx, dy evaluated at the current (x, y) and both coordinates updated from the same evaluation:
//                                   x <- (x0 - dx) / rc            y <- (y0 - dy) / rc
// and to pixels with the same camera matrix (P = cameraMatrix): u = fx * x + cx, v = fy * y + cy.
#pragma once
#include <hip/hip_runtime.h>

namespace apds {
namespace lens {

constexpr int DEFAULT_ITERS = 5;   // cv::undistortPoints: TermCriteria(COUNT, 5, 0.01)

struct Lens {
    double fx, fy, cx, cy;
    double k1, k2, p1, p2, k3, k4, k5, k6;
};

// rc, dx, dy at the normalised point (x, y)
__host__ __device__ inline void terms(const Lens& L, double x, double y, double& rc, double& dx, double& dy) {
    const double xx = x * x, yy = y * y;
    const double r2 = xx + yy;
    const double r4 = r2 * r2;
    const double r6 = r4 * r2;
    const double num = ((1.0 + L.k1 * r2) + L.k2 * r4) + L.k3 * r6;
    const double den = ((1.0 + L.k4 * r2) + L.k5 * r4) + L.k6 * r6;
    rc = num / den;
    const double a1 = (2.0 * x) * y;
    const double a2 = r2 + 2.0 * xx;
    const double a3 = r2 + 2.0 * yy;
    dx = L.p1 * a1 + L.p2 * a2;
    dy = L.p1 * a3 + L.p2 * a1;
}

// normalised ideal point -> distorted pixel
__host__ __device__ inline void forward_normalised(const Lens& L, double x, double y, double& ud, double& vd) {
    double rc, dx, dy;
    terms(L, x, y, rc, dx, dy);
    const double xd = x * rc + dx;
    const double yd = y * rc + dy;
    ud = L.fx * xd + L.cx;
    vd = L.fy * yd + L.cy;
}

// ideal pixel -> distorted pixel
__host__ __device__ inline void distort_pixel(const Lens& L, double u, double v, double& ud, double& vd) {
    forward_normalised(L, (u - L.cx) / L.fx, (v - L.cy) / L.fy, ud, vd);
}

// distorted pixel -> ideal pixel; iters >= 1
__host__ __device__ inline void undistort_pixel(const Lens& L, double ud, double vd, int iters, double& u, double& v) {
    const double x0 = (ud - L.cx) / L.fx, y0 = (vd - L.cy) / L.fy;
    double x = x0, y = y0;
    for (int i = 0; i < iters; i++) {
        double rc, dx, dy;
        terms(L, x, y, rc, dx, dy);
        x = (x0 - dx) / rc;
        y = (y0 - dy) / rc;
    }
    u = L.fx * x + L.cx;
    v = L.fy * y + L.cy;
}

}  // namespace lens
}  // namespace apds
