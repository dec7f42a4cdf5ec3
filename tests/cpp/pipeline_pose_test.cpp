// tests/cpp/pipeline_pose_test.cpp — a host that is NOT Python streams frames through the library's pipeline with the pose stage on
// (apds_pipeline_create -> apds_pipeline_enable_pose -> apds_pipeline_submit / apds_pipeline_poll_pose -> apds_pipeline_destroy,
// include/apds.h) and must get, frame by frame, the pose the one-call entry points give: apds_dev_akaze_extract -> apds_dev_hamming_topk
// (k = 2) -> apds_dev_ratio_filter -> the pairs built on the host -> apds_pnp_solver_ransac. Built by g++ against libapds_hip.so
// (tests/test_pipeline_pose_cpu.py compiles it, tests/test_pipeline_pose_gpu.py runs it), no torch, no HIP headers. The DB's world points
// are the DB keypoints back-projected from a camera with R = I, f = 500 px, at depth 1000 m, so the frames (the DB image shifted by
// (-23, -19) px) are seen from that camera moved sideways by (46 m, 38 m); the bounds follow test_pipeline_pose_gpu.py's anchor for this
// narrower field (th = 256 / 500 at the edge).
#include <apds.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

namespace {

int failures = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                       \
            fprintf(stderr, "\n");                              \
            failures++;                                         \
        }                                                       \
    } while (0)
#define OK(call)                                                                                               \
    do {                                                                                                       \
        const int rc_ = (call);                                                                                \
        if (rc_ != 0) {                                                                                        \
            fprintf(stderr, "FAIL %s:%d: %s -> %d (%s)\n", __FILE__, __LINE__, #call, rc_, apds_last_error()); \
            failures++;                                                                                        \
        }                                                                                                      \
    } while (0)

struct SplitMix {
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

// a grey BGRA image of Gaussian blobs (enough structure for a few thousand AKAZE keypoints)
std::vector<uint8_t> blob_frame(int T, uint64_t seed) {
    std::vector<float> v((size_t)T * T, 128.f);
    SplitMix g{seed};
    const int blobs = 2200 * T / 1024 * T / 1024 + 300;
    for (int b = 0; b < blobs; b++) {
        const double cx = g.uni() * T, cy = g.uni() * T, sg = 1.5 + g.uni() * 7.0, amp = -80 + g.uni() * 160;
        const int r = (int)(3 * sg) + 1;
        for (int y = std::max(0, (int)cy - r); y <= std::min(T - 1, (int)cy + r); y++)
            for (int x = std::max(0, (int)cx - r); x <= std::min(T - 1, (int)cx + r); x++) {
                const double d2 = (x - cx) * (x - cx) + (y - cy) * (y - cy);
                v[(size_t)y * T + x] += (float)(amp * std::exp(-d2 / (2 * sg * sg)));
            }
    }
    std::vector<uint8_t> img((size_t)T * T * 4);
    for (size_t i = 0; i < v.size(); i++) {
        const uint8_t u = (uint8_t)std::min(255.f, std::max(0.f, v[i] + 0.5f));
        img[i * 4] = img[i * 4 + 1] = img[i * 4 + 2] = u;
        img[i * 4 + 3] = 255;
    }
    return img;
}

std::vector<uint8_t> rolled(const std::vector<uint8_t>& img, int T, int dy, int dx) {
    std::vector<uint8_t> out(img.size());
    for (int y = 0; y < T; y++)
        for (int x = 0; x < T; x++) std::memcpy(&out[((size_t)((y + dy) % T) * T + (x + dx) % T) * 4], &img[((size_t)y * T + x) * 4], 4);
    return out;
}

struct DevBuf {
    void* p = nullptr;
    explicit DevBuf(size_t bytes) { OK(apds_dev_alloc(bytes, &p)); }
    ~DevBuf() { apds_dev_release(p); }
    DevBuf(const DevBuf&) = delete;
};

}  // namespace

int main() {
    if (apds_device_count() < 1) {
        fprintf(stderr, "no HIP device\n");
        return 2;
    }
    OK(apds_set_device(0));
    const int T = 512, NF = 3, NDB = 40000, CAP = 20000;
    const float ratio = 0.3f;
    const double f = 500.0, c = 256.0, Z0 = 1000.0;
    std::vector<std::vector<uint8_t>> frames;
    for (int i = 0; i < NF - 1; i++) frames.push_back(blob_frame(T, 0xFACE + (uint64_t)i));
    frames.emplace_back((size_t)T * T * 4, 0);   // a blank frame: no keypoints, no matches -> pose status APDS_ERR_ASSERT
    for (size_t i = 3; i < frames.back().size(); i += 4) frames.back()[i] = 255;
    const size_t fbytes = (size_t)T * T * 4;
    std::vector<std::unique_ptr<DevBuf>> dframes;
    for (auto& fr : frames) {
        dframes.emplace_back(new DevBuf(fbytes));
        OK(apds_dev_upload(dframes.back()->p, fr.data(), fbytes, nullptr));
    }
    // the train set: descriptors, keypoints and world points of a shifted copy of every textured frame, then random rows
    DevBuf kps((size_t)CAP * 28), desc((size_t)CAP * 64), tmp(fbytes), db((size_t)NDB * 64), dbk((size_t)NDB * 28), dbx((size_t)NDB * 24);
    std::vector<uint8_t> db_rows((size_t)NDB * 64, 0);
    std::vector<apds_keypoint> db_kps((size_t)NDB);
    std::vector<double> xyz((size_t)NDB * 3, 0.0);
    int P = 0;
    for (int i = 0; i < NF - 1; i++) {
        std::vector<uint8_t> r = rolled(frames[(size_t)i], T, 19, 23);
        OK(apds_dev_upload(tmp.p, r.data(), fbytes, nullptr));
        int n = 0;
        OK(apds_dev_akaze_extract(tmp.p, T, T, 4, (size_t)T * 4, CAP, kps.p, desc.p, CAP, &n, nullptr));
        CHECK(n > 300 && P + n < NDB, "shifted frame %d gives %d keypoints", i, n);
        OK(apds_dev_download(&db_rows[(size_t)P * 64], desc.p, (size_t)n * 64, nullptr));
        OK(apds_dev_download(&db_kps[(size_t)P], kps.p, (size_t)n * 28, nullptr));
        P += n;
    }
    SplitMix g{0xDB};
    for (int i = P; i < NDB; i++) {
        uint64_t* w = reinterpret_cast<uint64_t*>(&db_rows[(size_t)i * 64]);
        for (int j = 0; j < 8; j++) w[j] = g.next();
        db_rows[(size_t)i * 64 + 60] &= 0x3F;
        db_rows[(size_t)i * 64 + 61] = db_rows[(size_t)i * 64 + 62] = db_rows[(size_t)i * 64 + 63] = 0;
        db_kps[(size_t)i] = apds_keypoint{0, 0, 0, 0, 0, 0, 0};
    }
    for (int i = 0; i < NDB; i++) {   // back-projection from the DB camera, depth with a 0.2 % relief
        const double u = db_kps[(size_t)i].x, v = db_kps[(size_t)i].y, Z = Z0 * (1 + 0.002 * std::sin(u / 41.0) * std::cos(v / 29.0));
        xyz[(size_t)i * 3] = (u - c) * Z / f;
        xyz[(size_t)i * 3 + 1] = (v - c) * Z / f;
        xyz[(size_t)i * 3 + 2] = Z;
    }
    double origin[3] = {0, 0, Z0};
    OK(apds_dev_upload(db.p, db_rows.data(), db_rows.size(), nullptr));
    OK(apds_dev_upload(dbk.p, db_kps.data(), db_kps.size() * 28, nullptr));
    OK(apds_dev_upload(dbx.p, xyz.data(), xyz.size() * 8, nullptr));
    OK(apds_stream_synchronize(nullptr));

    apds_pipeline_pose_params pose;
    std::memset(&pose, 0, sizeof(pose));
    pose.db_xyz_dev = dbx.p;
    std::memcpy(pose.origin, origin, sizeof(origin));
    const double K[9] = {f, 0, c, 0, f, c, 0, 0, 1};
    std::memcpy(pose.camera_intrinsic, K, sizeof(K));
    pose.method = APDS_SOLVEPNP_ITERATIVE;   // (EPnP is ill-conditioned on points this close to a plane: the anchor below needs a refined pose)
    pose.reproj_thres = 3.0f;
    pose.iter_count = 500;

    // what the one-call entry points give per frame
    std::vector<apds_frame_pose> want((size_t)NF);
    {
        DevBuf keys((size_t)CAP * 16), matches((size_t)CAP * 16);
        for (int i = 0; i < NF; i++) {
            apds_frame_pose& e = want[(size_t)i];
            std::memset(&e, 0, sizeof(e));
            int nk = 0, M = 0;
            OK(apds_dev_akaze_extract(dframes[(size_t)i]->p, T, T, 4, (size_t)T * 4, CAP, kps.p, desc.p, CAP, &nk, nullptr));
            if (nk > 0) {
                OK(apds_dev_hamming_topk(desc.p, nk, db.p, NDB, 0, 2, keys.p, nullptr));
                OK(apds_dev_ratio_filter(keys.p, nk, 2, ratio, matches.p, &M, nullptr));
            }
            std::vector<apds_keypoint> fk((size_t)std::max(nk, 1));
            std::vector<apds_dmatch> fm((size_t)std::max(M, 1));
            if (nk) OK(apds_dev_download(fk.data(), kps.p, (size_t)nk * 28, nullptr));
            if (M) OK(apds_dev_download(fm.data(), matches.p, (size_t)M * 16, nullptr));
            std::vector<double> obj((size_t)std::max(M, 1) * 3), img((size_t)std::max(M, 1) * 2);
            for (int m = 0; m < M; m++) {
                for (int k = 0; k < 3; k++) obj[(size_t)m * 3 + k] = xyz[(size_t)fm[(size_t)m].train_idx * 3 + k] - origin[k];
                img[(size_t)m * 2] = fk[(size_t)fm[(size_t)m].query_idx].x;
                img[(size_t)m * 2 + 1] = fk[(size_t)fm[(size_t)m].query_idx].y;
            }
            std::vector<int32_t> inl((size_t)std::max(M, 1));
            e.n_correspondences = M;
            e.status = apds_pnp_solver_ransac(obj.data(), img.data(), M, K, pose.iter_count, pose.reproj_thres, 0.99, pose.method, e.rvec, e.tvec, inl.data(),
                                              &e.n_inliers, &e.found);
            if (e.status != 0) {
                e.found = e.n_inliers = 0;
                std::memset(e.rvec, 0, sizeof(e.rvec));
                std::memset(e.tvec, 0, sizeof(e.tvec));
            }
        }
        CHECK(want[0].status == 0 && want[0].found && want[0].n_inliers > 100, "serial frame 0: status %d found %d inliers %d", want[0].status, want[0].found,
              want[0].n_inliers);
        // the anchor: R close to I, camera centre -R^T t + origin close to (23, 19, 0) m (R^T t = t - th (k x t) + (1 - cos th) k x (k x t)
        // to first order in the small angle th, which the check bounds anyway)
        const double* t = want[0].tvec;
        const double* w = want[0].rvec;
        const double angle = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        const double wxt[3] = {w[1] * t[2] - w[2] * t[1], w[2] * t[0] - w[0] * t[2], w[0] * t[1] - w[1] * t[0]};
        const double cx = -(t[0] - wxt[0]) + origin[0], cy = -(t[1] - wxt[1]) + origin[1], cz = -(t[2] - wxt[2]) + origin[2];
        CHECK(angle < 3.5e-3 && std::fabs(cx - 46) < 4.5 && std::fabs(cy - 38) < 4.5 && std::fabs(cz) < 2.0, "frame 0 pose: angle %.2e centre (%.2f, %.2f, %.2f)", angle,
              cx, cy, cz);
        CHECK(want[(size_t)NF - 1].status == APDS_ERR_ASSERT, "the blank frame's pose status is %d", want[(size_t)NF - 1].status);
    }

    apds_pipeline_params pp;
    std::memset(&pp, 0, sizeof(pp));
    pp.rows = pp.cols = T;
    pp.channels = 4;
    pp.max_points = CAP;
    pp.filter_strength = ratio;
    pp.homography_method = APDS_HOMOGRAPHY_RANSAC;
    void* pipe = nullptr;
    OK(apds_pipeline_create(&pipe, db.p, NDB, 0, nullptr, dbk.p, NDB, &pp));
    if (!pipe) return 1;
    apds_pipeline_pose_params bad = pose;
    bad.method = 9;
    CHECK(apds_pipeline_enable_pose(pipe, &bad) == APDS_ERR_NOT_IMPLEMENTED, "an unknown method must be refused");
    bad = pose;
    bad.camera_intrinsic[4] = 0;
    CHECK(apds_pipeline_enable_pose(pipe, &bad) == APDS_ERR_BAD_ARG, "a zero focal length must be refused");
    OK(apds_pipeline_enable_pose(pipe, &pose));
    const int count = 12;
    for (int i = 0; i < count; i++) OK(apds_pipeline_submit(pipe, dframes[(size_t)(i % NF)]->p, (size_t)T * 4, 1, nullptr));
    CHECK(apds_pipeline_enable_pose(pipe, &pose) == APDS_ERR_BAD_ARG, "enable_pose after the first submit must be refused");
    for (int i = 0; i < count; i++) {
        apds_frame_result r;
        apds_frame_pose q;
        if (i == 5) {   // apds_pipeline_poll on a pipeline with pose: the pose is dropped, the result is the same
            OK(apds_pipeline_poll(pipe, &r, 1));
            CHECK(r.frame == i && r.status == 0, "plain poll: frame %lld status %d", (long long)r.frame, r.status);
            continue;
        }
        OK(apds_pipeline_poll_pose(pipe, &r, &q, 1));
        const apds_frame_pose& e = want[(size_t)(i % NF)];
        CHECK(r.frame == i && q.frame == i && r.status == 0, "result %d: frame %lld / %lld status %d", i, (long long)r.frame, (long long)q.frame, r.status);
        CHECK(q.status == e.status && q.found == e.found && q.n_correspondences == e.n_correspondences && q.n_inliers == e.n_inliers &&
                  std::memcmp(q.rvec, e.rvec, sizeof(e.rvec)) == 0 && std::memcmp(q.tvec, e.tvec, sizeof(e.tvec)) == 0,
              "frame %d: pipeline pose (status %d found %d pairs %d inliers %d) != one-call (%d %d %d %d)", i, q.status, q.found, q.n_correspondences, q.n_inliers,
              e.status, e.found, e.n_correspondences, e.n_inliers);
    }
    printf("%d frames with pose ... %s\n", count, failures ? "FAILED" : "ok");
    OK(apds_pipeline_destroy(pipe));
    // frames in flight at destroy are drained through the pose stage, not dropped mid-kernel
    OK(apds_pipeline_create(&pipe, db.p, NDB, 0, nullptr, dbk.p, NDB, &pp));
    OK(apds_pipeline_enable_pose(pipe, &pose));
    for (int i = 0; i < 5; i++) OK(apds_pipeline_submit(pipe, dframes[(size_t)(i % NF)]->p, (size_t)T * 4, 1, nullptr));
    OK(apds_pipeline_destroy(pipe));
    OK(apds_thread_release());
    printf("%d failed\n", failures);
    return failures ? 1 : 0;
}
