// tests/cpp/akaze_plan_host.cpp — the PRODUCT's extraction plan (csrc/akaze_plan.h: levels, FED step sizes, area tap tables, launch plan,
// slab layout) compiled by g++ without a GPU. As a shared library: the C entry points tests/test_akaze_plan_cpu.py drives. With
// -DAKAZE_PLAN_MAIN: a program that walks every table for the test's image sizes and lays a slab out in real memory, writing the first and
// the last byte of every plane (what an address or undefined-behaviour sanitizer build of it checks).
#include <cstdio>
#include <cstring>

#include "../../cubesat-apds_amd/csrc/akaze_plan.h"

using namespace apds;

extern "C" {

// info[level][6] = w, h, octave, sigma_size, border, nsteps; finfo[level][3] = esigma, etime, ratio; tau[level][64]. Returns the level count.
int akaze_plan_levels(int W, int H, int* info, float* finfo, float* tau) {
    const std::vector<LevelDesc> ev = akaze_levels(W, H);
    for (size_t i = 0; i < ev.size(); i++) {
        const LevelDesc& e = ev[i];
        const int v[6] = {e.w, e.h, e.octave, e.sigma_size, e.border, e.nsteps};
        const float f[3] = {e.esigma, e.etime, e.ratio};
        std::memcpy(info + 6 * i, v, sizeof v);
        std::memcpy(finfo + 3 * i, f, sizeof f);
        std::memcpy(tau + 64 * i, e.tau, sizeof e.tau);
    }
    return (int)ev.size();
}

// ofs / wgt: dsize x 4, cnt: dsize
void akaze_plan_area_tables(int ssize, int dsize, int* ofs, float* wgt, int* cnt) {
    std::vector<int> o, c;
    std::vector<float> w;
    area_tables(ssize, dsize, o, w, c);
    std::memcpy(ofs, o.data(), o.size() * sizeof(int));
    std::memcpy(wgt, w.data(), w.size() * sizeof(float));
    std::memcpy(cnt, c.data(), c.size() * sizeof(int));
}

// out = launches, fuse, fused_level, try_strips, then per pass (first, steps, lands_in_lt); returns launches
int akaze_plan_level(int W, int H, int level, int batch, int level_fuse, int level_strip, int fused_max_steps, int* out) {
    const std::vector<LevelDesc> ev = akaze_levels(W, H);
    const LevelPlan p = plan_level(ev[level], batch, level_fuse, level_strip, fused_max_steps);
    out[0] = p.launches;
    out[1] = p.fuse;
    out[2] = p.fused_level;
    out[3] = p.try_strips;
    for (int q = 0; q < p.launches; q++) {
        out[4 + 3 * q] = p.first[q];
        out[5 + 3 * q] = p.steps[q];
        out[6 + 3 * q] = p.lands_in_lt(q);
    }
    return p.launches;
}

}  // extern "C"

#ifdef AKAZE_PLAN_MAIN
namespace {
int failures = 0;
void expect(bool ok, const char* what, int a, int b) {
    if (ok) return;
    failures++;
    std::fprintf(stderr, "FAILED: %s (%d, %d)\n", what, a, b);
}

template <class T>
void touch(T* p, size_t n, const char* base, size_t bytes) {
    char* b = reinterpret_cast<char*>(p);
    expect(b >= base && b + n * sizeof(T) <= base + bytes, "plane inside the slab", (int)(b - base), (int)n);
    b[0] = 1;
    b[n * sizeof(T) - 1] = 1;
}
}  // namespace

int main() {
    const int sizes[5][2] = {{64, 48}, {160, 80}, {161, 83}, {640, 320}, {641, 321}};
    for (const auto& wh : sizes) {
        const std::vector<LevelDesc> ev = akaze_levels(wh[0], wh[1]);
        for (int batch : {1, 4})
            for (int level_fuse = 0; level_fuse < 3; level_fuse++)
                for (int level_strip = 0; level_strip < 3; level_strip++)
                    for (int fused_max : {29, 3})
                        for (size_t i = 1; i < ev.size(); i++) {
                            const LevelPlan p = plan_level(ev[i], batch, level_fuse, level_strip, fused_max);
                            int sum = 0;
                            for (int q = 0; q < p.launches; q++) {
                                expect(p.first[q] == sum, "passes are consecutive", (int)i, q);
                                expect(p.steps[q] >= 1 && p.steps[q] <= (q == 0 && p.fused_level ? fused_max : p.fuse), "pass within the fuse depth", (int)i, q);
                                sum += p.steps[q];
                            }
                            expect(sum == ev[i].nsteps, "passes cover the level's steps", (int)i, sum);
                            expect(p.launches == 0 || p.lands_in_lt(p.launches - 1), "last pass lands in Lt", (int)i, p.launches);
                        }
        for (size_t i = 1; i < ev.size(); i++)
            if (ev[i].octave > ev[i - 1].octave) {
                const int src[2] = {ev[i - 1].w, ev[i - 1].h}, dst[2] = {ev[i].w, ev[i].h};
                for (int axis = 0; axis < 2; axis++) {
                    std::vector<int> o, c;
                    std::vector<float> w;
                    area_tables(src[axis], dst[axis], o, w, c);
                    for (size_t d = 0; d < c.size(); d++)
                        for (int t = 0; t < c[d]; t++) expect(o[4 * d + t] >= 0 && o[4 * d + t] < src[axis], "area tap inside the source", (int)d, t);
                }
            }
        for (bool per_level : {false, true}) {
            SlabLayout sl{};
            sl.lay_out(nullptr, ev, per_level);
            const size_t bytes = sl.bytes;
            std::vector<char> mem(bytes + 256);
            char* base = mem.data() + (256 - reinterpret_cast<uintptr_t>(mem.data()) % 256) % 256;
            sl.lay_out(base, ev, per_level);
            expect(sl.bytes == bytes, "sizing pass and placing pass agree", (int)sl.bytes, (int)bytes);
            expect(reinterpret_cast<char*>(sl.list_count) == base, "slab starts with list_count", 0, 0);
            const size_t n0 = (size_t)ev[0].w * ev[0].h;
            touch(sl.list_count, AKAZE_MAX_LEVELS, base, bytes);
            touch(sl.hmax_bits, 1, base, bytes);
            touch(sl.hist, 304, base, bytes);
            touch(sl.pend_count, 3 * AKAZE_MAX_LEVELS * PEND_PITCH, base, bytes);
            touch(sl.kp_base, 8, base, bytes);
            touch(sl.fine_counts, sl.n_fine + 1024, base, bytes);
            touch(sl.coarse_counts, (size_t)sl.n_coarse * COARSE_PITCH, base, bytes);
            touch(sl.mask_all, (size_t)sl.total_pix + 128, base, bytes);
            touch(sl.status_all, (size_t)sl.total_pix, base, bytes);
            touch(sl.k_oct, 8, base, bytes);
            touch(sl.block_counts, sl.nblocks + 4, base, bytes);
            touch(sl.gray, n0, base, bytes);
            touch(sl.tmpS, n0, base, bytes);
            touch(sl.tmpF, n0, base, bytes);
            touch(sl.tmpP, n0, base, bytes);
            touch(sl.tmpH, n0 / 4 + 64, base, bytes);
            for (size_t i = 0; i < ev.size(); i++) {
                const size_t n = (size_t)ev[i].w * ev[i].h;
                touch(sl.Lt[i], n, base, bytes);
                touch(sl.Lxy[i], n, base, bytes);
                touch(sl.Ldet[i], n, base, bytes);
                touch(sl.list[i], (size_t)sl.pend_cap[i], base, bytes);
                touch(sl.pend[i], 3 * (size_t)sl.pend_cap[i], base, bytes);
                touch(sl.lsm[i], n, base, bytes);
                expect((sl.lsm[i] == sl.tmpS) == !(per_level && i > 0), "Lsmooth plane per level only when asked", (int)i, per_level);
            }
        }
    }
    const GaussTaps g = gauss_taps(9, 1.6);
    float kside, kmid;
    deriv_weights(2, kside, kmid);
    expect(g.k[0] > g.k[4] && kmid > kside, "taps fall off from the centre", 0, 0);
    std::printf(failures ? "akaze_plan_host: %d failures\n" : "akaze_plan_host: OK\n", failures);
    return failures ? 1 : 0;
}
#endif
