// tests/cpp/akaze_plan_host.cpp — the PRODUCT's extraction plan (csrc/akaze_plan.h: levels, FED step sizes, area tap tables, the kernel
// family of every stage and level, slab layout) compiled by g++ without a GPU. As a shared library: the C entry points tests/test_akaze_plan_cpu.py drives. With
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

namespace {
// sw[9]: nld_strip, sf_strip, base_strip, level_strip, level_fuse, level_stream, doh_strip, half_fuse, fork
PlanSwitches switches(const int* v) { return PlanSwitches{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8] != 0}; }

// per level PLAN_INTS ints: doh_strips, start, start_in_lt, smooth, head, launches, half_pass, then per pass (first, steps, strip_pass, lands_in_lt)
constexpr int PLAN_INTS = 7 + 4 * LevelPlan::MAX_PASSES;
void put_plan(const ExtractionPlan& plan, int* out) {
    for (size_t i = 0; i < plan.level.size(); i++) {
        const LevelPlan& p = plan.level[i];
        int* o = out + PLAN_INTS * i;
        const int head[7] = {p.doh_strips, (int)p.start, p.start_in_lt(), (int)p.smooth, (int)p.head, p.launches, p.half_pass};
        std::memcpy(o, head, sizeof head);
        for (int q = 0; q < p.launches; q++) {
            const int v[4] = {p.first[q], p.steps[q], p.strip_pass[q], p.lands_in_lt(q)};
            std::memcpy(o + 7 + 4 * q, v, sizeof v);
        }
    }
}

// What must hold for every plan, whatever the switches. Returns the number of violations (and says which on stderr).
int check_plan(const std::vector<LevelDesc>& ev, const ExtractionPlan& plan, const PlanSwitches& sw) {
    int bad = 0;
    const auto expect = [&bad](bool ok, const char* what, int level) {
        if (ok) return;
        bad++;
        std::fprintf(stderr, "FAILED: %s (level %d)\n", what, level);
    };
    const int L = (int)ev.size();
    int n_strip = 0;
    for (int i = 0; i < L; i++) {
        const LevelPlan& p = plan.level[i];
        expect(!p.doh_strips || i == 0 || plan.level[i - 1].doh_strips, "strip-Hessian levels are a prefix", i);
        n_strip += p.doh_strips;
        if (i == 0) continue;
        const LevelDesc &e = ev[i], &prev = ev[i - 1];
        int finishing = 0, sum = 0;
        for (int q = 0; q < p.launches; q++) {
            expect(p.first[q] == sum && p.steps[q] >= 1, "passes are consecutive", i);
            sum += p.steps[q];
            finishing += sum == e.nsteps;
            expect(q < p.first_fed_pass() || p.steps[q] <= (p.strip_pass[q] ? 4 : 8), "a FED pass within its kernel's depth", i);
            expect(q == p.launches - 1 || p.lands_in_lt(q) != p.lands_in_lt(q + 1), "passes alternate between Lt and the scratch plane", i);
        }
        expect(sum == e.nsteps && finishing == (e.nsteps > 0), "exactly one pass finishes the level", i);
        expect(p.launches == 0 || p.lands_in_lt(p.launches - 1), "last pass lands in Lt", i);
        expect((p.head == Head::Fused) == p.fused_level, "a fused level has the fused head", i);
        expect(p.head == Head::None || p.steps[0] <= (p.head == Head::Fused ? LEVEL_FUSED_MAX_STEPS : 4), "head within its kernel's depth", i);
        expect(p.head != Head::Stream || (e.w >= 64 && e.h >= 32), "streaming head only from 64 x 32", i);
        expect(!(p.head == Head::Stream || p.head == Head::Strips) || p.smooth == Smooth::None, "a stream or strips head smooths itself", i);
        expect(p.head != Head::None || p.smooth != Smooth::None, "somebody makes Lsmooth", i);
        expect(!(p.head == Head::Fused && p.smooth != Smooth::None) || (sw.fork && i == L - 1), "a fused level smooths apart only when last and forking", i);
        const bool next_is_half = i + 1 < L && ev[i + 1].octave > e.octave && e.w == 2 * ev[i + 1].w && e.h == 2 * ev[i + 1].h;
        expect(p.half_pass == -1 || (p.half_pass == p.launches - 1 && next_is_half && sw.half_fuse), "only the finishing pass writes the half image, only for an exact half", i);
        expect(p.half_pass == -1 || (p.half_pass == 0 && p.head != Head::None ? p.head != Head::Strips : p.strip_pass[p.half_pass]), "level_strip heads and tile passes write no half image", i);
        expect(!(p.head == Head::Stream && p.half_pass == 0) || p.launches == 1, "a stream head that writes the half image writes no conductivity", i);
        const bool resampled = e.octave > prev.octave;
        expect((p.start == Start::PrevLt) == !resampled, "resample exactly at an octave's start", i);
        expect((p.start == Start::Written) == (plan.level[i - 1].half_pass >= 0), "the written start image is used, and only it", i);
        expect(p.start != Start::HalfSample || (prev.w == 2 * e.w && prev.h == 2 * e.h), "half_sample only by exactly two", i);
        // a resampled start image goes to the plane the first pass does NOT land in, so that the passes alternate down to Lt
        expect(!resampled || p.launches == 0 || p.start_in_lt() != p.lands_in_lt(0), "start plane of a resampled level", i);
    }
    expect(n_strip == plan.n_strip_levels, "n_strip_levels counts the prefix", n_strip);
    return bad;
}
}  // namespace

extern "C" {

int akaze_plan_fused_max_steps() { return LEVEL_FUSED_MAX_STEPS; }
int akaze_plan_ints_per_level() { return PLAN_INTS; }

// The whole extraction's plan (out: PLAN_INTS per level, see put_plan). Returns the level count, or -1 - violations of check_plan.
int akaze_plan_extraction(int W, int H, int batch, const int* sw, int* out) {
    const std::vector<LevelDesc> ev = akaze_levels(W, H);
    const ExtractionPlan plan = plan_extraction(ev, batch, switches(sw));
    put_plan(plan, out);
    const int bad = check_plan(ev, plan, switches(sw));
    return bad ? -1 - bad : (int)ev.size();
}

// The plan of a level of any size and step count: level 1 of two levels w x h of one octave (out: 2 x PLAN_INTS).
int akaze_plan_one_level(int w, int h, int sigma_size, int nsteps, int batch, const int* sw, int* out) {
    std::vector<LevelDesc> ev(2);
    for (LevelDesc& d : ev) {
        d = LevelDesc{};
        d.w = w;
        d.h = h;
        d.sigma_size = sigma_size;
    }
    ev[1].nsteps = nsteps;
    ev[1].pix_offset = (long long)w * h;
    const ExtractionPlan plan = plan_extraction(ev, batch, switches(sw));
    put_plan(plan, out);
    const int bad = check_plan(ev, plan, switches(sw));
    return bad ? -1 - bad : 2;
}

// 0: base_strip_kernel, 1: the separate kernels
int akaze_plan_base(int rows, int cols, int channels, long long stride, long long img, long long img_stride, int batch, const int* sw) {
    return (int)plan_base(rows, cols, channels, (size_t)stride, (uintptr_t)img, (size_t)img_stride, batch, switches(sw));
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
    const int sizes[8][2] = {{64, 48}, {160, 80}, {161, 83}, {640, 320}, {641, 321}, {2048, 2048}, {3001, 2003}, {4096, 4096}};
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
        // the whole plan under every switch setting that changes it (each switch 0 / 1 / 2, half_fuse and fork 0 / 1)
        for (int batch : {1, 4})
            for (int code = 0; code < 3 * 3 * 3 * 3 * 3 * 3 * 2 * 2; code++) {
                int v[9], c = code;
                for (int k : {0, 1, 3, 4, 5, 6}) {
                    v[k] = c % 3;
                    c /= 3;
                }
                v[2] = 1;
                v[7] = c % 2;
                v[8] = c / 2;
                const PlanSwitches sw = switches(v);
                expect(check_plan(ev, plan_extraction(ev, batch, sw), sw) == 0, "plan invariants", code, batch);
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
        if ((size_t)wh[0] * wh[1] > (size_t)1 << 20) continue;   // (the large sizes are here for the plan; their slabs are gigabytes)
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
    {
        const int v[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
        expect(plan_base(2048, 2048, 4, 8192, 4096, 0, 1, switches(v)) == BaseStage::Strips, "aligned BGRA takes the strip pass", 0, 0);
        expect(plan_base(2048, 2048, 4, 8192, 4097, 0, 1, switches(v)) == BaseStage::Separate, "misaligned BGRA does not", 0, 0);
    }
    const GaussTaps g = gauss_taps(9, 1.6);
    float kside, kmid;
    deriv_weights(2, kside, kmid);
    expect(g.k[0] > g.k[4] && kmid > kside, "taps fall off from the centre", 0, 0);
    std::printf(failures ? "akaze_plan_host: %d failures\n" : "akaze_plan_host: OK\n", failures);
    return failures ? 1 : 0;
}
#endif
