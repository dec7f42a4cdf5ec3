// csrc/api_pnp.cpp — C-ABI entry points of homographier::pnp_solver_ransac (mod.rs:320-369).
#include "kernels.h"

using namespace apds;

extern "C" {

int apds_pnp_solver_ransac(const double* obj_xyz, const double* img_xy, int n, const double* camera_intrinsic, int iter_count, float reproj_thres,
                           double confidence, int method, double* rvec, double* tvec, int32_t* inliers, int* n_inliers, int* found) {
    APDS_RANGE("apds_pnp_solver_ransac");
    return guarded([&] {
        APDS_REQUIRE(found, APDS_ERR_BAD_ARG, "null argument");
        *found = 0;
        ThreadCtx& c = ctx();
        c.ws_reset();
        *found = pnp_ransac_device(obj_xyz, img_xy, n, camera_intrinsic, iter_count, reproj_thres, confidence, method, rvec, tvec, inliers, n_inliers, c.stream);
    });
}

int apds_pnp_solver_ransac_dist(const double* obj_xyz, const double* img_xy, int n, const double* camera_intrinsic, int iter_count, float reproj_thres,
                                double confidence, int method, const double* dist, int n_dist, double* rvec, double* tvec, int32_t* inliers,
                                int* n_inliers, int* found) {
    APDS_RANGE("apds_pnp_solver_ransac_dist");
    return guarded([&] {
        APDS_REQUIRE(found, APDS_ERR_BAD_ARG, "null argument");
        *found = 0;
        // argument errors before any device work: the lens, then what the plain call checks
        lens::Lens L;
        const bool distorts = lens_from_args(camera_intrinsic, dist, n_dist, &L);
        APDS_REQUIRE(n_inliers, APDS_ERR_BAD_ARG, "null argument");
        *n_inliers = 0;
        APDS_REQUIRE(obj_xyz && img_xy && rvec && tvec && inliers, APDS_ERR_BAD_ARG, "null argument");
        (void)pnp_checked_method(n, method);
        ThreadCtx& c = ctx();
        c.ws_reset();
        if (!distorts) {   // apds_pnp_solver_ransac itself
            *found = pnp_ransac_device(obj_xyz, img_xy, n, camera_intrinsic, iter_count, reproj_thres, confidence, method, rvec, tvec, inliers, n_inliers, c.stream);
            return;
        }
        // the image points to ideal pixels in f64 (cv::undistortPoints' five steps, P = cameraMatrix), then the f32 conversion and the loop
        std::vector<double> ideal((size_t)n * 2);
        lens_points_host(img_xy, n, L, lens::DEFAULT_ITERS, ideal.data(), c.stream);
        *found = pnp_ransac_device(obj_xyz, ideal.data(), n, camera_intrinsic, iter_count, reproj_thres, confidence, method, rvec, tvec, inliers, n_inliers, c.stream);
    });
}

int apds_dev_pnp_solver_ransac(const void* obj_xyz_dev, const void* img_xy_dev, int n, const double* camera_intrinsic, int iter_count, float reproj_thres,
                               double confidence, int method, double* rvec, double* tvec, int32_t* inliers, int* n_inliers, int* found, void* stream) {
    APDS_RANGE("apds_dev_pnp_solver_ransac");
    return guarded([&] {
        APDS_REQUIRE(found && n_inliers, APDS_ERR_BAD_ARG, "null argument");
        *found = 0;
        *n_inliers = 0;
        APDS_REQUIRE(obj_xyz_dev && img_xy_dev && camera_intrinsic && rvec && tvec, APDS_ERR_BAD_ARG, "null argument");
        (void)pnp_checked_method(n, method);   // (argument errors before any device work)
        hipStream_t s = pick_stream(stream);
        ctx().ws_reset(s);   // (every solve starts from an empty workspace: a pipeline thread calls this once per frame)
        *found = pnp_ransac_core(static_cast<const float*>(obj_xyz_dev), static_cast<const float*>(img_xy_dev), n, camera_intrinsic, iter_count, reproj_thres,
                                 confidence, method, rvec, tvec, inliers, n_inliers, s);
    });
}

int apds_dev_pnp_correspondences(const void* kps, int n_kps, const void* db_xyz, int64_t n_db, const double* origin, const void* matches, int n_matches,
                                 void* img_xy, void* obj_xyz, void* stream) {
    APDS_RANGE("apds_dev_pnp_correspondences");
    return guarded([&] {
        APDS_REQUIRE(n_kps >= 0 && n_db >= 0 && n_matches >= 0, APDS_ERR_ASSERT, "negative count");
        if (n_matches == 0) return;
        APDS_REQUIRE(kps && db_xyz && origin && matches && img_xy && obj_xyz, APDS_ERR_BAD_ARG, "null argument");
        ThreadCtx& c = ctx();
        hipStream_t s = pick_stream(stream);
        c.ws_reset(s);
        int* err = c.alloc_n<int>(1);
        HIP_CHECK(hipMemsetAsync(err, 0, sizeof(int), s));
        pnp_correspondences_device(static_cast<const apds_keypoint*>(kps), n_kps, static_cast<const double*>(db_xyz), (long long)n_db, origin,
                                   static_cast<const apds_dmatch*>(matches), n_matches, static_cast<float*>(img_xy), static_cast<float*>(obj_xyz), err, s);
        int* herr = c.pinned_ints(1);
        HIP_CHECK(hipMemcpyAsync(herr, err, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        APDS_REQUIRE(herr[0] == 0, APDS_ERR_OUT_OF_RANGE, "match index outside the keypoint vector or the DB's world points");
    });
}

int apds_pnp_hypotheses(const double* obj_xyz, const double* img_xy, int n, const double* camera_intrinsic, const int32_t* idx5, int n_samples,
                        int model_points, double* models) {
    return guarded([&] {
        ThreadCtx& c = ctx();
        c.ws_reset();
        pnp_hypotheses_device(obj_xyz, img_xy, n, camera_intrinsic, idx5, n_samples, model_points, models, c.stream);
    });
}

int apds_pnp_sqpnp(const double* obj_xyz, const double* img_xy, int n, const double* camera_intrinsic, double* rvec, double* tvec, int* found) {
    return guarded([&] {
        APDS_REQUIRE(found, APDS_ERR_BAD_ARG, "null argument");
        *found = 0;
        *found = pnp_sqpnp_host(obj_xyz, img_xy, n, camera_intrinsic, rvec, tvec);
    });
}

int apds_pnp_ippe(const double* obj_xyz, const double* img_xy, int n, const double* camera_intrinsic, double* rvec, double* tvec, int* found) {
    return guarded([&] {
        APDS_REQUIRE(found, APDS_ERR_BAD_ARG, "null argument");
        *found = 0;
        *found = pnp_ippe_host(obj_xyz, img_xy, n, camera_intrinsic, rvec, tvec);
    });
}

int apds_get_world_coordinates(const double* xy, int n, const double* dataset_gt, const double* elevation_gt, const double* elevation, int ew, int eh,
                               double* xyz) {
    return guarded([&] {
        APDS_REQUIRE(n >= 0 && (n == 0 || (xy && xyz)) && dataset_gt, APDS_ERR_BAD_ARG, "null argument");
        APDS_REQUIRE(!elevation_gt || (elevation && ew > 0 && eh > 0), APDS_ERR_BAD_ARG, "elevation geotransform without a raster");
        if (n == 0) return;
        ThreadCtx& c = ctx();
        c.ws_reset();
        hipStream_t s = c.stream;
        double* dxy = c.alloc_n<double>((size_t)n * 2);
        double* dxyz = c.alloc_n<double>((size_t)n * 3);
        double* del = nullptr;
        HIP_CHECK(hipMemcpyAsync(dxy, xy, (size_t)n * 16, hipMemcpyHostToDevice, s));
        if (elevation_gt) {
            del = c.alloc_n<double>((size_t)ew * eh);
            HIP_CHECK(hipMemcpyAsync(del, elevation, (size_t)ew * eh * 8, hipMemcpyHostToDevice, s));
        }
        const int missing = world_coordinates_device(dxy, n, dataset_gt, elevation_gt, del, ew, eh, dxyz, s);
        HIP_CHECK(hipMemcpyAsync(xyz, dxyz, (size_t)n * 24, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (missing) fail(APDS_ERR_OUT_OF_RANGE, "an elevation lookup fell outside the elevation table (those points are NaN)");
    });
}

}  // extern "C"
