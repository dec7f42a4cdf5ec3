// csrc/akaze_describe.h — what the one-wave-per-keypoint kernels share (akaze_describe.hip: main orientation and M-LDB;
// akaze_describe_msurf.hip: the 64-float M-SURF descriptor): the per-wave LDS phase boundary, the loop over groups of four keypoints and
// the deterministic sine / cosine of the keypoint angle. Device code only.
#pragma once
#include "akaze.h"

namespace apds {

// The per-keypoint kernels give every wave its own slices of the block's LDS arrays: what one phase writes, only the same wave reads in
// the next. The LDS unit executes a wave's instructions in issue order, so a later read sees an earlier write without any wait; all that is
// needed between two phases is that the compiler does not move LDS accesses across the boundary. (Round 2 used __syncthreads() here: three
// block-wide rendezvous per keypoint in the descriptor kernel and seven in the orientation kernel tied four independent waves together.
// Same time either way - the descriptor kernel waits for HBM, see below - but nothing is left that needs the block to move in step.)
__device__ __forceinline__ void wave_lds_phase() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Keypoints [range[0], min(range[1], n_cap)) of this image (range: two consecutive ints of the image's slab, written by the stage's
// scan; nullptr: [0, n_cap)): the counts stay on the device, and the blocks stride over the range, so the grid need not match it.
// Which groups of four keypoints a block takes. Plain: block b takes groups b, b + gridDim.x, ... XCD-aware (xcd_ranges): workgroups are
// dealt round-robin over the 8 XCDs, so block b runs on XCD b % 8; that XCD gets ONE contiguous eighth of the groups and its blocks walk
// it in order. Keypoints are in level-major, row-major order: neighbours in the list are neighbours in the image, their sample patches
// overlap, and one XCD's L2 then serves both instead of two L2s fetching the same lines.
#define KP_GROUP_LOOP(kb, begin, n, xcd_ranges)                                                                                          \
    const int kp_groups_ = ((n) - (begin) + 3) >> 2, kp_nbx_ = ((int)gridDim.x + 7) >> 3;                                               \
    const int kp_x_ = (int)blockIdx.x & 7, kp_lo_ = (int)((long long)kp_groups_ * kp_x_ >> 3), kp_hi_ = (int)((long long)kp_groups_ * (kp_x_ + 1) >> 3); \
    const int kp_first_ = (xcd_ranges) ? kp_lo_ + ((int)blockIdx.x >> 3) : (int)blockIdx.x, kp_end_ = (xcd_ranges) ? kp_hi_ : kp_groups_; \
    const int kp_stride_ = (xcd_ranges) ? kp_nbx_ : (int)gridDim.x;                                                                       \
    for (int kg_ = kp_first_, kb = (begin) + 4 * kg_; kg_ < kp_end_; kg_ += kp_stride_, kb = (begin) + 4 * kg_)

// deterministic double sin/cos on [0, 2pi] (Cody-Waite reduction + Taylor/Horner; same arithmetic as the oracle)
__device__ __forceinline__ void det_sincos(double a, double& s, double& c) {
    const double two_over_pi = 0.63661977236758134308;
    const double pio2_hi = 1.57079632673412561417e+00, pio2_lo = 6.07710050650619224932e-11;
    const int k = (int)(a * two_over_pi + 0.5);
    const double r = (a - k * pio2_hi) - k * pio2_lo;
    const double r2 = r * r;
    double ps = -7.6471637318198164759e-13;          // -1/15!
    ps = ps * r2 + 1.6059043836821614599e-10;        //  1/13!
    ps = ps * r2 + -2.5052108385441718775e-08;       // -1/11!
    ps = ps * r2 + 2.7557319223985890653e-06;        //  1/9!
    ps = ps * r2 + -1.9841269841269841270e-04;       // -1/7!
    ps = ps * r2 + 8.3333333333333333333e-03;        //  1/5!
    ps = ps * r2 + -1.6666666666666666667e-01;       // -1/3!
    const double sr = r + r * (r2 * ps);
    double pc = 4.7794773323873852974e-14;           //  1/16!
    pc = pc * r2 + -1.1470745597729724714e-11;       // -1/14!
    pc = pc * r2 + 2.0876756987868098979e-09;        //  1/12!
    pc = pc * r2 + -2.7557319223985890653e-07;       // -1/10!
    pc = pc * r2 + 2.4801587301587301587e-05;        //  1/8!
    pc = pc * r2 + -1.3888888888888888889e-03;       // -1/6!
    pc = pc * r2 + 4.1666666666666666667e-02;        //  1/4!
    pc = pc * r2 + -0.5;
    const double cr = 1.0 + r2 * pc;
    switch (k & 3) {
        case 0: s = sr; c = cr; break;
        case 1: s = cr; c = -sr; break;
        case 2: s = -sr; c = -cr; break;
        default: s = -cr; c = sr; break;
    }
}

}  // namespace apds
