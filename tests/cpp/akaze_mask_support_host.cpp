// tests/cpp/akaze_mask_support_host.cpp — the mask-support radii of the PRODUCT's extraction plan (csrc/akaze_plan.h) compiled by g++
// without a GPU, as a shared library for tests/test_akaze_mask_support_cpu.py: per level the unit plan_extraction decided (scale * ratio) and
// the radius a support gives it.
#include "../../cubesat-apds_amd/csrc/akaze_plan.h"

using namespace apds;

extern "C" {

// units[level] = the plan's support_unit, octaves[level] = the level's octave; returns the level count (<= 16)
int akaze_mask_support_units(int W, int H, int batch, int* units, int* octaves) {
    const std::vector<LevelDesc> ev = akaze_levels(W, H);
    const ExtractionPlan plan = plan_extraction(ev, batch, PlanSwitches{});
    for (size_t i = 0; i < ev.size(); i++) {
        units[i] = plan.level[i].support_unit;
        octaves[i] = ev[i].octave;
    }
    return (int)ev.size();
}

int akaze_mask_support_radius(int support, int unit) { return mask_support_radius(support, unit); }

}  // extern "C"
