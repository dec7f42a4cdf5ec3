// tests/cpp/pipeline_table_view_test.cpp — a host that is NOT Python drives the per-frame-view pipeline through the C ABI
// (apds_db_view_*, apds_pipeline_create_table, apds_pipeline_submit_select; include/apds.h) and must get, frame by frame, what the
// calls that existed before give: apds_dev_akaze_extract -> apds_db_select + apds_db_view -> apds_dev_hamming_topk (k = 2) ->
// apds_dev_ratio_filter -> apds_dev_points_from_matches -> apds_dev_find_homography. Built by g++ against libapds_hip.so
// (tests/test_pipeline_table_view_native.py), no torch, no HIP headers; run on the GPU box.
#include <apds.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

// a grey BGRA image of Gaussian blobs
std::vector<uint8_t> blob_frame(int T, uint64_t seed) {
    std::vector<float> v((size_t)T * T, 128.f);
    SplitMix g{seed};
    for (int b = 0; b < 900; b++) {
        const double cx = g.uni() * T, cy = g.uni() * T, sg = 1.5 + g.uni() * 5.0, amp = -80 + g.uni() * 160;
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

void* dev(size_t bytes) {
    void* p = nullptr;
    OK(apds_dev_alloc(bytes, &p));
    return p;
}

struct Expect {
    int status = 0, K = 0, M = 0, inliers = 0, found = 0;
    double H[9] = {0};
};

}  // namespace

int main() {
    if (apds_device_count() < 1) {
        fprintf(stderr, "no HIP device\n");
        return 2;
    }
    OK(apds_set_device(0));
    const int T = 256, CAP = 4096, NF = 2;
    const float ratio = 0.8f;
    const size_t fbytes = (size_t)T * T * 4;
    void *kps = dev((size_t)CAP * 28), *desc = dev((size_t)CAP * 64), *keys = dev((size_t)CAP * 16), *matches = dev((size_t)CAP * 16);
    void *p1 = dev((size_t)CAP * 8), *p2 = dev((size_t)CAP * 8), *mask = dev(CAP), *scratch = dev(fbytes);
    void* db = nullptr;
    OK(apds_db_create(&db, 4 * CAP));
    std::vector<void*> dframes;
    // the table: frame f rolled by (19, 23) is image f + 1 at level of detail 0, tile column f; the same rows again at level 1
    for (int f = 0; f < NF; f++) {
        const std::vector<uint8_t> img = blob_frame(T, 0xBEEF + (uint64_t)f), roll = rolled(img, T, 19, 23);
        dframes.push_back(dev(fbytes));
        OK(apds_dev_upload(dframes.back(), img.data(), fbytes, nullptr));
        OK(apds_dev_upload(scratch, roll.data(), fbytes, nullptr));
        int n = 0;
        OK(apds_dev_akaze_extract(scratch, T, T, 4, (size_t)T * 4, CAP, kps, desc, CAP, &n, nullptr));
        CHECK(n >= 30, "frame %d: only %d keypoints", f, n);
        OK(apds_db_insert_dev(db, kps, desc, n, f + 1, 0, (uint64_t)f, 0, T, T, nullptr));
        OK(apds_db_insert_dev(db, kps, desc, n, f + 11, 1, (uint64_t)f, 0, T, T, nullptr));
    }
    const apds_db_selection sels[] = {{2, 0, 0.f, 0.f, 255.5f, 255.5f}, {2, 0, 257.f, 0.f, 511.5f, 255.5f}, {1, 1, 0, 0, 0, 0}, {0, 12, 0, 0, 0, 0},
                                      {1, 7, 0, 0, 0, 0}, {1, 0, 0, 0, 0, 0}};
    const int NS = (int)(sizeof(sels) / sizeof(sels[0])), N = 2 * NS;

    printf("serial composition ...");
    std::vector<Expect> want((size_t)N);
    for (int i = 0; i < N; i++) {
        Expect& e = want[(size_t)i];
        const apds_db_selection& s = sels[i % NS];
        OK(apds_dev_akaze_extract(dframes[(size_t)(i % NF)], T, T, 4, (size_t)T * 4, CAP, kps, desc, CAP, &e.K, nullptr));
        int nv = 0;
        OK(apds_db_select(db, s.mode, s.value, s.x_start, s.y_start, s.x_end, s.y_end, &nv));
        void *rows64 = nullptr, *vkps = nullptr;
        OK(apds_db_view(db, &rows64, &vkps, nullptr, nullptr, &nv));
        if (nv < 2) {
            e.status = APDS_ERR_ASSERT;
            continue;
        }
        OK(apds_dev_hamming_topk(desc, e.K, rows64, nv, 0, 2, keys, nullptr));
        OK(apds_dev_ratio_filter(keys, e.K, 2, ratio, matches, &e.M, nullptr));
        if (e.M < 4) continue;
        OK(apds_dev_points_from_matches(kps, e.K, vkps, nv, matches, e.M, 0, p1, p2, nullptr));
        const int rc = apds_dev_find_homography(p1, p2, e.M, APDS_HOMOGRAPHY_RANSAC, 3.0, 2000, 0.995, e.H, mask, nullptr);
        CHECK(rc == APDS_OK || rc == APDS_ERR_EMPTY, "find_homography -> %d", rc);
        if (rc != APDS_OK) continue;
        e.found = 1;
        std::vector<uint8_t> hm((size_t)e.M);
        OK(apds_dev_download(hm.data(), mask, hm.size(), nullptr));
        for (uint8_t b : hm) e.inliers += b != 0;
    }
    int with_h = 0;
    for (const Expect& e : want) with_h += e.found;
    CHECK(with_h >= 4, "only %d frames of the serial run found a homography", with_h);
    printf(failures ? " FAILED\n" : " ok\n");

    printf("table pipeline ...");
    const int before = failures;
    apds_pipeline_params pp;
    std::memset(&pp, 0, sizeof pp);
    pp.rows = pp.cols = T;
    pp.channels = 4;
    pp.max_points = CAP;
    pp.n_slots = 4;
    pp.filter_strength = ratio;
    pp.homography_method = APDS_HOMOGRAPHY_RANSAC;
    void* pipe = nullptr;
    OK(apds_pipeline_create_table(&pipe, db, 0, &pp));
    CHECK(apds_pipeline_submit(pipe, dframes[0], (size_t)T * 4, 1, nullptr) == APDS_ERR_BAD_ARG, "submit on a table pipeline");
    CHECK(apds_pipeline_submit_select(pipe, dframes[0], (size_t)T * 4, 1, nullptr, nullptr) == APDS_ERR_BAD_ARG, "null selection");
    int polled = 0;
    auto take = [&](int wait) {
        apds_frame_result r;
        while (polled < N && apds_pipeline_poll(pipe, &r, wait) == APDS_OK) {
            const Expect& e = want[(size_t)polled];
            CHECK(r.frame == polled, "frame %d arrived as %lld", polled, (long long)r.frame);
            CHECK(r.status == e.status && r.n_keypoints == e.K && r.n_matches == e.M && r.n_inliers == e.inliers && r.homography_found == e.found,
                  "frame %d: status %d/%d K %d/%d M %d/%d inliers %d/%d found %d/%d", polled, r.status, e.status, r.n_keypoints, e.K, r.n_matches, e.M,
                  r.n_inliers, e.inliers, r.homography_found, e.found);
            if (e.found) CHECK(std::memcmp(r.H, e.H, sizeof e.H) == 0, "frame %d: H differs", polled);
            polled++;
        }
    };
    for (int i = 0; i < N; i++) {
        int64_t id = -1;
        OK(apds_pipeline_submit_select(pipe, dframes[(size_t)(i % NF)], (size_t)T * 4, 1, &sels[i % NS], &id));
        CHECK(id == i, "frame id %lld", (long long)id);
        take(0);
    }
    take(1);
    CHECK(polled == N, "%d of %d results", polled, N);
    OK(apds_pipeline_destroy(pipe));
    printf(failures > before ? " FAILED\n" : " ok\n");

    OK(apds_db_destroy(db));
    for (void* p : dframes) apds_dev_release(p);
    for (void* p : {kps, desc, keys, matches, p1, p2, mask, scratch}) apds_dev_release(p);
    printf("%d failed\n", failures);
    return failures ? 1 : 0;
}
