// csrc/lens.hip — lens distortion (the model: lens_core.h) where the pose chain meets a real camera:
//   * points: ideal <-> distorted pixels on f64 host arrays, and the in-place undistort of f32 pairs on the device (a point array, or the
//     x, y of 28-byte keypoints) that the pipeline's homography and pose stages run on their matched image points;
//   * frames: cv::undistort's shape - per destination pixel the forward model gives the source position, then the warp's fixed-point
//     bilinear tail (warp_sample.h) with border value 0. One thread per destination pixel, one destination row per blockIdx.y, whole
//     pixels as uint32_t for four channels, no LDS: a streaming store and a gather whose 2x2 footprints of neighbouring lanes overlap.
// A lens without distortion (no coefficients, or all of them exactly zero) launches nothing: (u - cx) / fx * fx + cx is no exact identity.
#include <cmath>
#include <cstring>

#include "kernels.h"
#include "warp_sample.h"

namespace apds {

using lens::Lens;

constexpr int UNDISTORT_BORDER = 0;   // cv::undistort: BORDER_CONSTANT with the default Scalar()

// iters == 0: the forward model (ideal -> distorted); iters >= 1: the inverse with that many steps
__global__ __launch_bounds__(256) void lens_points_f64_kernel(const double* __restrict__ xy, int n, Lens L, int iters, double* __restrict__ out) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double u, v;
    if (iters == 0) lens::distort_pixel(L, xy[2 * (size_t)i], xy[2 * (size_t)i + 1], u, v);
    else lens::undistort_pixel(L, xy[2 * (size_t)i], xy[2 * (size_t)i + 1], iters, u, v);
    out[2 * (size_t)i] = u;
    out[2 * (size_t)i + 1] = v;
}

// in place on the f32 pair at the head of every `stride` bytes: widened to f64, undistorted, rounded once on the store
__global__ __launch_bounds__(256) void lens_undistort_points_f32_kernel(uint8_t* __restrict__ base, int n, size_t stride, Lens L, int iters) {
    APDS_RAISE_WAVE_PRIORITY();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float* p = reinterpret_cast<float*>(base + (size_t)i * stride);
    double u, v;
    lens::undistort_pixel(L, (double)p[0], (double)p[1], iters, u, v);
    p[0] = (float)u;
    p[1] = (float)v;
}

// destination pixel (x, y) of the ideal image with camera matrix (nfx, nfy, ncx, ncy) -> its position in the distorted source -> sample
template <int CH>
__global__ __launch_bounds__(256) void undistort_image_kernel(const uint8_t* __restrict__ src, int rows, int cols, Lens L, double nfx, double nfy, double ncx,
                                                              double ncy, const short* __restrict__ tab, uint8_t* __restrict__ dst) {
    APDS_RAISE_WAVE_PRIORITY();
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    const double xn = ((double)x - ncx) / nfx, yn = ((double)y - ncy) / nfy;
    double us, vs;
    lens::forward_normalised(L, xn, yn, us, vs);
    const int X = sat_int_rn(us * 32.0), Y = sat_int_rn(vs * 32.0);
    sample_bilinear_u8<CH>(src, rows, cols, X, Y, tab, UNDISTORT_BORDER, dst + ((size_t)y * cols + x) * CH);
}

namespace {

bool focal_ok(const double* K) { return std::isfinite(K[0]) && std::isfinite(K[4]) && K[0] > 0 && K[4] > 0; }

}  // namespace

// The argument checks of every lens entry, before any device work. Returns whether the lens distorts at all (false: nothing to launch).
bool lens_from_args(const double* K, const double* dist, int n_dist, Lens* out) {
    APDS_REQUIRE(K, APDS_ERR_BAD_ARG, "null camera matrix");
    APDS_REQUIRE(n_dist != 12 && n_dist != 14, APDS_ERR_NOT_IMPLEMENTED, "thin-prism and tilt coefficients (12 or 14 distortion coefficients) are not built");
    APDS_REQUIRE(n_dist == 0 || n_dist == 4 || n_dist == 5 || n_dist == 8, APDS_ERR_BAD_ARG, "distortion coefficients: 0, 4, 5 or 8 of them");
    if (!dist) n_dist = 0;
    double k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool any = false;
    for (int i = 0; i < n_dist; i++) {
        APDS_REQUIRE(std::isfinite(dist[i]), APDS_ERR_BAD_ARG, "a distortion coefficient is not finite");
        k[i] = dist[i];
        any = any || dist[i] != 0.0;
    }
    APDS_REQUIRE(focal_ok(K), APDS_ERR_BAD_ARG, "the focal lengths must be finite and positive");
    *out = Lens{K[0], K[4], K[2], K[5], k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7]};
    return any;
}

void lens_points_f64_device(const double* xy_dev, int n, const Lens& L, int iters, double* out_dev, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(lens_points_f64_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, xy_dev, n, L, iters, out_dev);
    HIP_CHECK(hipGetLastError());
}

void lens_undistort_points_f32_device(void* xy_dev, int n, size_t stride_bytes, const Lens& L, int iters, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(lens_undistort_points_f32_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, static_cast<uint8_t*>(xy_dev), n, stride_bytes, L,
                       iters > 0 ? iters : lens::DEFAULT_ITERS);
    HIP_CHECK(hipGetLastError());
}

// host arrays through the calling thread's workspace (not reset here); returns when out is written
void lens_points_host(const double* xy, int n, const Lens& L, int iters, double* out, hipStream_t s) {
    ThreadCtx& c = ctx();
    double* din = c.alloc_n<double>((size_t)n * 2);
    double* dout = c.alloc_n<double>((size_t)n * 2);
    HIP_CHECK(hipMemcpyAsync(din, xy, (size_t)n * 16, hipMemcpyHostToDevice, s));
    lens_points_f64_device(din, n, L, iters, dout, s);
    HIP_CHECK(hipMemcpyAsync(out, dout, (size_t)n * 16, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

// src, dst: device images of rows x cols x channels u8, packed; the weight table comes from the calling thread's workspace
void undistort_image_device(const uint8_t* src, int rows, int cols, int channels, const Lens& L, const double* new_K, uint8_t* dst, hipStream_t s) {
    const double nfx = new_K ? new_K[0] : L.fx, nfy = new_K ? new_K[4] : L.fy, ncx = new_K ? new_K[2] : L.cx, ncy = new_K ? new_K[5] : L.cy;
    short* tab = ctx().alloc_n<short>(32 * 32 * 4);
    HIP_CHECK(hipMemcpyAsync(tab, bilinear_tab_host(), sizeof(short) * 32 * 32 * 4, hipMemcpyHostToDevice, s));
    const dim3 grid(ceil_div(cols, 256), rows), block(256);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, s, src, rows, cols, L, nfx, nfy, ncx, ncy, (const short*)tab, dst); };
    if (channels == 1) go(undistort_image_kernel<1>);
    else if (channels == 3) go(undistort_image_kernel<3>);
    else go(undistort_image_kernel<4>);
    HIP_CHECK(hipGetLastError());
}

namespace {

// the checks the two image entries share; returns whether a kernel has to run (false: dst is a copy of src)
bool image_args(const void* src, int rows, int cols, int channels, const double* K, const double* dist, int n_dist, const double* new_K, const void* dst, Lens* L) {
    APDS_REQUIRE(src && dst, APDS_ERR_BAD_ARG, "null argument");
    const bool distorts = lens_from_args(K, dist, n_dist, L);
    APDS_REQUIRE(!new_K || focal_ok(new_K), APDS_ERR_BAD_ARG, "the focal lengths of new_K must be finite and positive");
    APDS_REQUIRE(rows > 0 && cols > 0, APDS_ERR_ASSERT, "empty image");
    APDS_REQUIRE(rows <= 65535, APDS_ERR_ASSERT, "undistort_image serves at most 65535 rows (one destination row per grid row)");
    APDS_REQUIRE(channels == 1 || channels == 3 || channels == 4, APDS_ERR_ASSERT, "undistort_image serves 1-, 3- and 4-channel u8 images");
    return distorts || new_K;
}

int points_host(const double* xy, int n, const double* K, const double* dist, int n_dist, int iters, double* out) {
    return guarded([&] {
        Lens L;
        const bool distorts = lens_from_args(K, dist, n_dist, &L);
        APDS_REQUIRE(n >= 0, APDS_ERR_ASSERT, "negative count");
        if (n == 0) return;
        APDS_REQUIRE(xy && out, APDS_ERR_BAD_ARG, "null argument");
        if (!distorts) {   // the input's bits
            if (out != xy) std::memmove(out, xy, (size_t)n * 16);
            return;
        }
        ThreadCtx& c = ctx();
        c.ws_reset();
        lens_points_host(xy, n, L, iters, out, c.stream);
    });
}

}  // namespace

}  // namespace apds

using namespace apds;

extern "C" {

int apds_distort_points(const double* xy, int n, const double* K, const double* dist, int n_dist, double* out) {
    return points_host(xy, n, K, dist, n_dist, 0, out);
}

int apds_undistort_points(const double* xy, int n, const double* K, const double* dist, int n_dist, int iters, double* out) {
    return points_host(xy, n, K, dist, n_dist, iters > 0 ? iters : lens::DEFAULT_ITERS, out);
}

int apds_dev_undistort_points(void* xy_dev, int n, int stride_bytes, const double* K, const double* dist, int n_dist, int iters, void* stream) {
    return guarded([&] {
        Lens L;
        const bool distorts = lens_from_args(K, dist, n_dist, &L);
        APDS_REQUIRE(n >= 0, APDS_ERR_ASSERT, "negative count");
        APDS_REQUIRE(stride_bytes >= 8 && stride_bytes % 4 == 0, APDS_ERR_BAD_ARG, "stride_bytes: at least 8 and a multiple of 4");
        if (n == 0 || !distorts) return;
        APDS_REQUIRE(xy_dev && reinterpret_cast<uintptr_t>(xy_dev) % 4 == 0, APDS_ERR_BAD_ARG, "xy_dev: a 4-byte aligned device pointer");
        lens_undistort_points_f32_device(xy_dev, n, (size_t)stride_bytes, L, iters, pick_stream(stream));   // (no workspace: nothing to order but the stream)
    });
}

int apds_undistort_image(const uint8_t* src, int rows, int cols, int channels, const double* K, const double* dist, int n_dist, const double* new_K,
                         uint8_t* dst) {
    return guarded([&] {
        Lens L;
        const size_t bytes = (size_t)(rows > 0 ? rows : 0) * (size_t)(cols > 0 ? cols : 0) * (size_t)(channels > 0 ? channels : 0);
        if (!image_args(src, rows, cols, channels, K, dist, n_dist, new_K, dst, &L)) {
            if (dst != src) std::memmove(dst, src, bytes);
            return;
        }
        ThreadCtx& c = ctx();
        c.ws_reset();
        hipStream_t s = c.stream;
        uint8_t* ds = c.alloc_n<uint8_t>(bytes);
        uint8_t* dd = c.alloc_n<uint8_t>(bytes);
        HIP_CHECK(hipMemcpyAsync(ds, src, bytes, hipMemcpyHostToDevice, s));
        undistort_image_device(ds, rows, cols, channels, L, new_K, dd, s);
        HIP_CHECK(hipMemcpyAsync(dst, dd, bytes, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int apds_dev_undistort_image(const void* src_dev, int rows, int cols, int channels, const double* K, const double* dist, int n_dist, const double* new_K,
                             void* dst_dev, void* stream) {
    return guarded([&] {
        Lens L;
        const bool run = image_args(src_dev, rows, cols, channels, K, dist, n_dist, new_K, dst_dev, &L);
        const size_t bytes = (size_t)rows * cols * channels;
        if (!run) {
            if (dst_dev != src_dev) HIP_CHECK(hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, pick_stream(stream)));
            return;
        }
        const uintptr_t a = reinterpret_cast<uintptr_t>(src_dev), b = reinterpret_cast<uintptr_t>(dst_dev);
        APDS_REQUIRE(a + bytes <= b || b + bytes <= a, APDS_ERR_BAD_ARG, "the destination overlaps the source (the kernel gathers: not in place)");
        APDS_REQUIRE(channels != 4 || (a % 4 == 0 && b % 4 == 0), APDS_ERR_BAD_ARG, "four-channel images: 4-byte aligned device pointers");
        QueuedWorkspaceCall call(pick_stream(stream));   // (the weight table lives in the workspace and the kernel is queued on return)
        undistort_image_device(static_cast<const uint8_t*>(src_dev), rows, cols, channels, L, new_K, static_cast<uint8_t*>(dst_dev), call.s);
    });
}

}  // extern "C"
