// tests/cpp/pipeline_crosscheck_test.cpp — a host that is NOT Python sets the pipeline's matcher to the cross-check
// (apds_pipeline_set_matcher, include/apds.h), streams frames and must get, frame by frame, what the one-call functions give:
// apds_dev_akaze_extract -> apds_dev_crosscheck_match (and, on the downloaded rows, apds_get_bruteforce_matches) ->
// apds_dev_points_from_matches -> apds_dev_find_homography. Built by g++ against libapds_hip.so (tests/test_pipeline_crosscheck_native.py),
// no torch, no HIP headers; run on the GPU box.
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
    int K = 0, M = 0, inliers = 0, found = 0;
    double H[9] = {0};
};

}  // namespace

int main() {
    if (apds_device_count() < 1) {
        fprintf(stderr, "no HIP device\n");
        return 2;
    }
    OK(apds_set_device(0));
    const int T = 256, CAP = 4096, NF = 2, FILL = 700, N = 10;
    const size_t fbytes = (size_t)T * T * 4;
    void *kps = dev((size_t)CAP * 28), *desc = dev((size_t)CAP * 64), *matches = dev((size_t)CAP * 16);
    void *p1 = dev((size_t)CAP * 8), *p2 = dev((size_t)CAP * 8), *mask = dev(CAP), *scratch = dev(fbytes);
    // the train set: the rows (and keypoints) of every frame rolled by (19, 23), then random rows
    std::vector<uint8_t> db_rows, db_kps;
    std::vector<void*> dframes;
    for (int f = 0; f < NF; f++) {
        const std::vector<uint8_t> img = blob_frame(T, 0xC0DE + (uint64_t)f), roll = rolled(img, T, 19, 23);
        dframes.push_back(dev(fbytes));
        OK(apds_dev_upload(dframes.back(), img.data(), fbytes, nullptr));
        OK(apds_dev_upload(scratch, roll.data(), fbytes, nullptr));
        int n = 0;
        OK(apds_dev_akaze_extract(scratch, T, T, 4, (size_t)T * 4, CAP, kps, desc, CAP, &n, nullptr));
        CHECK(n >= 30, "frame %d: only %d keypoints", f, n);
        OK(apds_stream_synchronize(nullptr));
        const size_t r0 = db_rows.size(), k0 = db_kps.size();
        db_rows.resize(r0 + (size_t)n * 64);
        db_kps.resize(k0 + (size_t)n * 28);
        OK(apds_dev_download(db_rows.data() + r0, desc, (size_t)n * 64, nullptr));
        OK(apds_dev_download(db_kps.data() + k0, kps, (size_t)n * 28, nullptr));
    }
    SplitMix g{0xF111};
    for (int i = 0; i < FILL; i++) {
        uint8_t row[64] = {0};
        for (int b = 0; b < 61; b++) row[b] = (uint8_t)g.next();
        db_rows.insert(db_rows.end(), row, row + 64);
        float kp[7] = {(float)(g.uni() * T), (float)(g.uni() * T), 0, 0, 0, 0, 0};
        const uint8_t* kb = reinterpret_cast<const uint8_t*>(kp);
        db_kps.insert(db_kps.end(), kb, kb + 28);
    }
    const int ND = (int)(db_rows.size() / 64);
    void *ddb = dev(db_rows.size()), *ddb_kps = dev(db_kps.size());
    OK(apds_dev_upload(ddb, db_rows.data(), db_rows.size(), nullptr));
    OK(apds_dev_upload(ddb_kps, db_kps.data(), db_kps.size(), nullptr));

    printf("serial composition ...");
    std::vector<Expect> want((size_t)NF);
    for (int f = 0; f < NF; f++) {
        Expect& e = want[(size_t)f];
        OK(apds_dev_akaze_extract(dframes[(size_t)f], T, T, 4, (size_t)T * 4, CAP, kps, desc, CAP, &e.K, nullptr));
        OK(apds_dev_crosscheck_match(desc, e.K, ddb, ND, 0, matches, &e.M, nullptr));
        // the host one-call matcher on the same rows gives the same list
        std::vector<uint8_t> hq((size_t)e.K * 64), hm((size_t)e.M * 16);
        OK(apds_dev_download(hq.data(), desc, hq.size(), nullptr));
        OK(apds_dev_download(hm.data(), matches, hm.size(), nullptr));
        apds_dmatch* bf = nullptr;
        int nbf = -1;
        OK(apds_get_bruteforce_matches(hq.data(), e.K, db_rows.data(), ND, 64, &bf, &nbf));
        CHECK(nbf == e.M && bf && std::memcmp(bf, hm.data(), hm.size()) == 0, "frame %d: apds_get_bruteforce_matches gives %d matches, the device call %d", f, nbf, e.M);
        apds_free(bf);
        // ... and it is not the ratio matcher's answer
        int ratio_m = 0;
        void *keys = dev((size_t)CAP * 16), *ratio_matches = dev((size_t)CAP * 16);
        OK(apds_dev_hamming_topk(desc, e.K, ddb, ND, 0, 2, keys, nullptr));
        OK(apds_dev_ratio_filter(keys, e.K, 2, 0.8f, ratio_matches, &ratio_m, nullptr));
        apds_dev_release(keys);
        apds_dev_release(ratio_matches);
        CHECK(ratio_m != e.M, "frame %d: ratio %d, cross-check %d matches of %d keypoints", f, ratio_m, e.M, e.K);
        if (e.M < 4) continue;
        OK(apds_dev_points_from_matches(kps, e.K, ddb_kps, ND, matches, e.M, 0, p1, p2, nullptr));
        const int rc = apds_dev_find_homography(p1, p2, e.M, APDS_HOMOGRAPHY_RANSAC, 3.0, 2000, 0.995, e.H, mask, nullptr);
        CHECK(rc == APDS_OK || rc == APDS_ERR_EMPTY, "find_homography -> %d", rc);
        if (rc != APDS_OK) continue;
        e.found = 1;
        std::vector<uint8_t> inl((size_t)e.M);
        OK(apds_dev_download(inl.data(), mask, inl.size(), nullptr));
        for (uint8_t b : inl) e.inliers += b != 0;
    }
    CHECK(want[0].found && want[0].M >= 30, "the serial run found no homography (%d matches)", want[0].M);
    printf(failures ? " FAILED\n" : " ok\n");

    printf("cross-check pipeline ...");
    const int before = failures;
    apds_pipeline_params pp;
    std::memset(&pp, 0, sizeof pp);
    pp.rows = pp.cols = T;
    pp.channels = 4;
    pp.max_points = CAP;
    pp.n_slots = 4;
    pp.filter_strength = 0.8f;
    pp.homography_method = APDS_HOMOGRAPHY_RANSAC;
    void* pipe = nullptr;
    OK(apds_pipeline_create(&pipe, ddb, ND, 0, nullptr, ddb_kps, ND, &pp));
    CHECK(apds_pipeline_set_matcher(pipe, 2) == APDS_ERR_BAD_ARG, "matcher 2");
    CHECK(apds_pipeline_set_matcher(pipe, -1) == APDS_ERR_BAD_ARG, "matcher -1");
    OK(apds_pipeline_set_matcher(pipe, APDS_PIPELINE_MATCH_CROSSCHECK));
    int polled = 0;
    auto take = [&](int wait) {
        apds_frame_result r;
        while (polled < N && apds_pipeline_poll(pipe, &r, wait) == APDS_OK) {
            const Expect& e = want[(size_t)(polled % NF)];
            CHECK(r.frame == polled, "frame %d arrived as %lld", polled, (long long)r.frame);
            CHECK(r.status == 0 && r.n_keypoints == e.K && r.n_matches == e.M && r.n_inliers == e.inliers && r.homography_found == e.found,
                  "frame %d: status %d K %d/%d M %d/%d inliers %d/%d found %d/%d", polled, r.status, r.n_keypoints, e.K, r.n_matches, e.M, r.n_inliers, e.inliers,
                  r.homography_found, e.found);
            if (e.found) CHECK(std::memcmp(r.H, e.H, sizeof e.H) == 0, "frame %d: H differs", polled);
            polled++;
        }
    };
    for (int i = 0; i < N; i++) {
        int64_t id = -1;
        OK(apds_pipeline_submit(pipe, dframes[(size_t)(i % NF)], (size_t)T * 4, 1, &id));
        CHECK(id == i, "frame id %lld", (long long)id);
        if (i == 0) CHECK(apds_pipeline_set_matcher(pipe, APDS_PIPELINE_MATCH_RATIO) == APDS_ERR_BAD_ARG, "set_matcher after the first submit");
        take(0);
    }
    take(1);
    CHECK(polled == N, "%d of %d results", polled, N);
    OK(apds_pipeline_destroy(pipe));
    printf(failures > before ? " FAILED\n" : " ok\n");

    for (void* p : dframes) apds_dev_release(p);
    for (void* p : {kps, desc, matches, p1, p2, mask, scratch, ddb, ddb_kps}) apds_dev_release(p);
    printf("%d failed\n", failures);
    return failures ? 1 : 0;
}
