// tests/cpp/db_float_table_test.cpp — a host that is NOT Python builds, reads, streams against and edits a FLOAT keypoint table through
// the C ABI (apds_db_create_float and its twins, apds_db_view_l2_train, apds_pipeline_create_table on a float table; include/apds.h):
//   build    : apds_dev_akaze_extract_float -> apds_db_insert_dev, and the same rows again through apds_db_insert_image_float; the kind
//              (apds_db_info) and the wrong-kind calls
//   select   : apds_db_select + apds_db_view_download_float against the rows that went in; a view object's train handle
//              (apds_db_view_l2_train) in both modes against apds_dev_l2_topk over the view's rows, bit for bit
//   pipeline : every frame equals apds_db_select -> apds_dev_akaze_extract_float -> apds_dev_l2_topk -> apds_dev_l2_ratio_filter ->
//              apds_dev_points_from_matches -> apds_dev_find_homography; the matcher cannot be changed
//   delete   : an image leaves; the survivors keep order, ids and every bit (apds_db_read_keypoint_from_id_float)
// Built by g++ against libapds_hip.so (tests/test_db_float_table_native.py), no torch, no HIP headers; run on the GPU box.
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
    void *kps = dev((size_t)CAP * 28), *desc = dev((size_t)CAP * 256), *keys = dev((size_t)CAP * 16), *keys2 = dev((size_t)CAP * 16), *matches = dev((size_t)CAP * 16);
    void *p1 = dev((size_t)CAP * 8), *p2 = dev((size_t)CAP * 8), *mask = dev(CAP), *scratch = dev(fbytes);
    void *db = nullptr, *bytes_db = nullptr;

    printf("build ...");
    OK(apds_db_create_float(&db, 4 * CAP));
    OK(apds_db_create(&bytes_db, 16));
    int descriptor = 0, row_bytes = 0;
    OK(apds_db_info(db, &descriptor, &row_bytes));
    CHECK(descriptor == APDS_AKAZE_DESCRIPTOR_KAZE && row_bytes == 256, "float table reports %d / %d", descriptor, row_bytes);
    OK(apds_db_info(bytes_db, &descriptor, &row_bytes));
    CHECK(descriptor == APDS_AKAZE_DESCRIPTOR_MLDB && row_bytes == 64, "byte table reports %d / %d", descriptor, row_bytes);
    std::vector<void*> dframes;
    std::vector<std::vector<apds_keypoint>> hk((size_t)NF);
    std::vector<std::vector<float>> hd((size_t)NF);
    // the table: frame f rolled by (19, 23) is image f + 1 at level of detail 0, tile column f (from the device); the same rows again as
    // image f + 11 at level 1 (from the host)
    for (int f = 0; f < NF; f++) {
        const std::vector<uint8_t> img = blob_frame(T, 0xBEEF + (uint64_t)f), roll = rolled(img, T, 19, 23);
        dframes.push_back(dev(fbytes));
        OK(apds_dev_upload(dframes.back(), img.data(), fbytes, nullptr));
        OK(apds_dev_upload(scratch, roll.data(), fbytes, nullptr));
        int n = 0;
        OK(apds_dev_akaze_extract_float(scratch, T, T, 4, (size_t)T * 4, nullptr, 0, 0, CAP, kps, desc, CAP, &n, nullptr));
        CHECK(n >= 30, "frame %d: only %d keypoints", f, n);
        OK(apds_db_insert_dev(db, kps, desc, n, f + 1, 0, (uint64_t)f, 0, T, T, nullptr));
        hk[(size_t)f].resize((size_t)n);
        hd[(size_t)f].resize((size_t)n * 64);
        OK(apds_dev_download(hk[(size_t)f].data(), kps, (size_t)n * 28, nullptr));
        OK(apds_dev_download(hd[(size_t)f].data(), desc, (size_t)n * 256, nullptr));
        OK(apds_db_insert_image_float(db, hk[(size_t)f].data(), hd[(size_t)f].data(), n, f + 11, 1, (uint64_t)f, 0, T, T));
    }
    const int n0 = (int)hk[0].size(), n1 = (int)hk[1].size(), total = 2 * (n0 + n1);
    CHECK(apds_db_rows(db) == total, "rows %lld, want %d", (long long)apds_db_rows(db), total);
    {   // the wrong kind in both directions changes nothing
        std::vector<uint8_t> d61(61 * 2);
        CHECK(apds_db_insert_image(db, hk[0].data(), d61.data(), 2, 9, 0, 0, 0, T, T) == APDS_ERR_BAD_ARG, "byte insert into a float table");
        CHECK(apds_db_insert_image_float(bytes_db, hk[0].data(), hd[0].data(), 2, 9, 0, 0, 0, T, T) == APDS_ERR_BAD_ARG, "float insert into a byte table");
        int32_t idx[2];
        int32_t di[2];
        CHECK(apds_db_knn_match(db, d61.data(), 1, 61, 2, idx, di) == APDS_ERR_BAD_ARG, "Hamming knn on a float table");
        void* sh = nullptr;
        CHECK(apds_db_shard(db, 0, 1, APDS_TRANSPORT_LOOPBACK, nullptr, nullptr, &sh) == APDS_ERR_BAD_ARG && !sh, "shard of a float table");
        CHECK(apds_db_rows(db) == total && apds_db_rows(bytes_db) == 0, "a refused call changed a table");
    }
    printf(failures ? " FAILED\n" : " ok\n");

    printf("select ...");
    int before = failures;
    {
        // image 12 = frame 1's rows from the host at level 1: x lifted by 2 and by one tile column (256 * 2); best response first, ties by row
        int nv = 0;
        OK(apds_db_select(db, 0, 12, 0, 0, 0, 0, &nv));
        CHECK(nv == n1, "image 12 has %d rows, want %d", nv, n1);
        std::vector<apds_keypoint> vk((size_t)nv);
        std::vector<float> vd((size_t)nv * 64);
        std::vector<int32_t> ids((size_t)nv), imgs((size_t)nv);
        OK(apds_db_view_download_float(db, vk.data(), vd.data(), ids.data(), imgs.data()));
        std::vector<uint8_t> d61((size_t)nv * 61);
        CHECK(apds_db_view_download(db, vk.data(), d61.data(), nullptr, nullptr) == APDS_ERR_BAD_ARG, "byte download of a float view");
        const int first_id = 2 * n0 + n1 + 1;   // ids: frame 0 device, frame 0 host, frame 1 device, frame 1 host
        std::vector<int> order((size_t)n1);
        for (int i = 0; i < n1; i++) order[(size_t)i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return hk[1][(size_t)a].response > hk[1][(size_t)b].response; });
        for (int i = 0; i < nv && i < n1; i++) {
            const int r = order[(size_t)i];
            const apds_keypoint& s = hk[1][(size_t)r];
            CHECK(ids[(size_t)i] == first_id + r && imgs[(size_t)i] == 12, "view row %d: id %d image %d", i, ids[(size_t)i], imgs[(size_t)i]);
            CHECK(vk[(size_t)i].x == s.x * 2.0f + 512.0f && vk[(size_t)i].y == s.y * 2.0f && vk[(size_t)i].response == s.response, "view row %d: keypoint", i);
            CHECK(std::memcmp(&vd[(size_t)i * 64], &hd[1][(size_t)r * 64], 256) == 0, "view row %d: descriptor", i);
        }
        // a view object: rows and train side from one gather; the handle's keys in both modes are the exact kernel's over the view's rows
        void *view = nullptr, *train = nullptr, *vrows = nullptr;
        OK(apds_db_view_create(db, 0, &view));
        OK(apds_db_view_l2_train(view, &train));
        CHECK(apds_l2_train_destroy(train) == APDS_ERR_BAD_ARG, "a borrowed train set was destroyed");
        int K = 0;
        OK(apds_dev_akaze_extract_float(dframes[0], T, T, 4, (size_t)T * 4, nullptr, 0, 0, CAP, kps, desc, CAP, &K, nullptr));
        const apds_db_selection vs[] = {{1, 0, 0, 0, 0, 0}, {0, 99, 0, 0, 0, 0}, {2, 1, 0.f, 0.f, 300.f, 300.f}};
        for (const apds_db_selection& s : vs) {
            OK(apds_db_view_select(view, s.mode, s.value, s.x_start, s.y_start, s.x_end, s.y_end, 0, nullptr, &nv));
            OK(apds_db_view_pointers(view, &vrows, nullptr, nullptr, nullptr, nullptr, nullptr));
            int64_t tn = -1;
            int dim = 0, ready = -1;
            OK(apds_l2_train_info(train, &tn, &dim, &ready));
            CHECK(tn == nv && dim == 64 && ready == (nv >= 2), "train handle: %lld rows, dim %d, ready %d for a view of %d", (long long)tn, dim, ready, nv);
            OK(apds_dev_l2_topk(desc, K, vrows, nv, 64, 0, 2, keys, nullptr));
            std::vector<uint64_t> want((size_t)K * 2), got((size_t)K * 2);
            OK(apds_dev_download(want.data(), keys, want.size() * 8, nullptr));
            for (int mode : {APDS_L2_SCREEN, APDS_L2_EXACT}) {
                int used = -1;
                OK(apds_dev_l2_train_top2(train, desc, K, mode, keys2, nullptr, &used, nullptr));
                OK(apds_dev_download(got.data(), keys2, got.size() * 8, nullptr));
                CHECK(used == (mode == APDS_L2_SCREEN && nv >= 2 ? APDS_L2_SCREEN : APDS_L2_EXACT), "mode %d ran as %d on %d rows", mode, used, nv);
                CHECK(got == want, "view of %d rows, mode %d: keys differ from the exact kernel's", nv, mode);
            }
        }
        OK(apds_db_view_destroy(view));
        void* bview = nullptr;
        OK(apds_db_view_create(bytes_db, 0, &bview));
        CHECK(apds_db_view_l2_train(bview, &train) == APDS_ERR_BAD_ARG && !train, "train handle of a byte view");
        OK(apds_db_view_destroy(bview));
    }
    printf(failures > before ? " FAILED\n" : " ok\n");

    const apds_db_selection sels[] = {{2, 0, 0.f, 0.f, 255.5f, 255.5f}, {2, 0, 257.f, 0.f, 511.5f, 255.5f}, {1, 1, 0, 0, 0, 0}, {0, 12, 0, 0, 0, 0},
                                      {1, 7, 0, 0, 0, 0}, {1, 0, 0, 0, 0, 0}};
    const int NS = (int)(sizeof(sels) / sizeof(sels[0])), N = 2 * NS;

    printf("serial composition ...");
    before = failures;
    std::vector<Expect> want((size_t)N);
    for (int i = 0; i < N; i++) {
        Expect& e = want[(size_t)i];
        const apds_db_selection& s = sels[i % NS];
        OK(apds_dev_akaze_extract_float(dframes[(size_t)(i % NF)], T, T, 4, (size_t)T * 4, nullptr, 0, 0, CAP, kps, desc, CAP, &e.K, nullptr));
        int nv = 0;
        OK(apds_db_select(db, s.mode, s.value, s.x_start, s.y_start, s.x_end, s.y_end, &nv));
        void *rows = nullptr, *vkps = nullptr;
        OK(apds_db_view(db, &rows, &vkps, nullptr, nullptr, &nv));
        if (nv < 2) {
            e.status = APDS_ERR_ASSERT;
            continue;
        }
        OK(apds_dev_l2_topk(desc, e.K, rows, nv, 64, 0, 2, keys, nullptr));
        OK(apds_dev_l2_ratio_filter(keys, e.K, 2, ratio, matches, &e.M, nullptr));
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
    printf(failures > before ? " FAILED\n" : " ok\n");

    printf("table pipeline ...");
    before = failures;
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
    CHECK(apds_pipeline_set_matcher(pipe, APDS_PIPELINE_MATCH_CROSSCHECK) == APDS_ERR_BAD_ARG, "cross-check on a float table pipeline");
    CHECK(apds_pipeline_set_matcher(pipe, APDS_PIPELINE_MATCH_RATIO) == APDS_ERR_BAD_ARG, "Hamming ratio on a float table pipeline");
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

    printf("delete ...");
    before = failures;
    {
        // image 11 (rows n0 .. 2 n0, ids n0 + 1 .. 2 n0) leaves: the rows behind it move down by n0 and keep ids and bits
        int64_t gone = -1, row = -1;
        OK(apds_db_delete_where(db, 0, 11, 0, 0, 0, 0, &gone));
        CHECK(gone == n0 && apds_db_rows(db) == total - n0, "deleted %lld rows, %lld left", (long long)gone, (long long)apds_db_rows(db));
        apds_keypoint k;
        std::vector<float> d(64);
        int image = 0;
        CHECK(apds_db_read_keypoint_from_id_float(db, n0 + 1, &k, d.data(), &image, &row) == APDS_ERR_OUT_OF_RANGE, "a deleted id was found");
        for (int r : {0, n1 - 1}) {   // frame 1's device rows: ids 2 n0 + 1 + r, now at row n0 + r
            OK(apds_db_read_keypoint_from_id_float(db, 2 * n0 + 1 + r, &k, d.data(), &image, &row));
            CHECK(row == n0 + r && image == 2, "id %d is at row %lld of image %d", 2 * n0 + 1 + r, (long long)row, image);
            CHECK(k.x == hk[1][(size_t)r].x + 256.0f && k.y == hk[1][(size_t)r].y && std::memcmp(d.data(), &hd[1][(size_t)r * 64], 256) == 0, "id %d: row changed", 2 * n0 + 1 + r);
        }
        OK(apds_db_read_keypoint_from_id_float(db, 1, &k, d.data(), &image, &row));
        CHECK(row == 0 && image == 1 && std::memcmp(d.data(), hd[0].data(), 256) == 0, "the first row changed");
        uint8_t d61[61];
        CHECK(apds_db_read_keypoint_from_id(db, 1, &k, d61, nullptr, nullptr) == APDS_ERR_BAD_ARG, "byte read of a float row");
        const int32_t victims[] = {1, total};   // the first and the last id, by id
        OK(apds_db_delete_ids(db, victims, 2, &gone));
        CHECK(gone == 2 && apds_db_rows(db) == total - n0 - 2, "delete by id removed %lld", (long long)gone);
        OK(apds_db_read_keypoint_from_id_float(db, 2, &k, d.data(), &image, &row));
        CHECK(row == 0 && std::memcmp(d.data(), &hd[0][64], 256) == 0, "id 2 did not move to row 0 intact");
        // ids go on behind the highest ever given
        OK(apds_db_insert_image_float(db, hk[0].data(), hd[0].data(), 1, 20, 0, 0, 0, T, T));
        OK(apds_db_read_keypoint_from_id_float(db, total + 1, &k, d.data(), &image, &row));
        CHECK(image == 20 && row == apds_db_rows(db) - 1, "the new row has image %d at row %lld", image, (long long)row);
    }
    printf(failures > before ? " FAILED\n" : " ok\n");

    OK(apds_db_destroy(db));
    OK(apds_db_destroy(bytes_db));
    for (void* p : dframes) apds_dev_release(p);
    for (void* p : {kps, desc, keys, keys2, matches, p1, p2, mask, scratch}) apds_dev_release(p);
    printf("%d failed\n", failures);
    return failures ? 1 : 0;
}
