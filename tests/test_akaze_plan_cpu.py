"""CPU: the extraction plan of the product (csrc/akaze_plan.h: the host arithmetic decided before the first launch), compiled by g++ into
a host-only test library (tests/cpp/akaze_plan_host.cpp).

Levels: for each size the plan's level list equals the oracle's (oracle_akaze_level_info / oracle_akaze_level_tau of a whole oracle
extraction of an image of that size) exactly - w, h, octave, sigma_size, border, nsteps as integers, esigma, etime, ratio and every tau as
float bit patterns. The sizes: one octave (the `lw < 80` stop), two octaves with the stop hit from the other side, odd halves, the smallest
image with four octaves, and an odd one with four.

Area tap tables (no oracle accessor): what the construction implies - at most 4 taps per destination, every offset inside the source, the
weights of a destination sum to 1 within 4 ulp of float (<= 4 weights, each the float rounding of a / cell where the a's sum to cell;
every weight is below 1, so its rounding moves the sum by at most a quarter ulp of 1), and on the exact 2 : 1 case two taps of 0.5.

Launch plan: for every level of those sizes and every value of APDS_LEVEL_FUSE / APDS_LEVEL_STRIP, single and batched, the passes' step
counts sum to nsteps, none exceeds its fuse depth, and the last pass lands in Lt."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(64, 48), (160, 80), (161, 83), (640, 320), (641, 321)]
N_OCTAVES = {(64, 48): 1, (160, 80): 2, (161, 83): 2, (640, 320): 4, (641, 321): 4}
LF_MAX_STEPS = 29   # level_fused_kernel's capacity (csrc/akaze_filters.hip)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("akaze_plan") / "libakaze_plan_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "akaze_plan_host.cpp"), "-o", so])
    return C.CDLL(so)


def plan_levels(plan, w, h):
    info, finfo, tau = np.zeros((16, 6), np.int32), np.zeros((16, 3), np.float32), np.zeros((16, 64), np.float32)
    n = plan.akaze_plan_levels(w, h, info.ctypes.data_as(C.c_void_p), finfo.ctypes.data_as(C.c_void_p), tau.ctypes.data_as(C.c_void_p))
    return n, info, finfo, tau


@pytest.mark.parametrize("w,h", SIZES)
def test_levels_equal_the_oracle(plan, w, h):
    import oracle
    rng = np.random.default_rng(w * 1000 + h)
    ref = oracle.akaze((rng.random((h, w)) * 255).astype(np.uint8)).levels
    n, info, finfo, tau = plan_levels(plan, w, h)
    assert n == len(ref) == 4 * N_OCTAVES[(w, h)]
    for i, lv in enumerate(ref):
        got = dict(zip(("w", "h", "octave", "sigma_size", "border", "nsteps"), (int(v) for v in info[i])))
        assert got == {k: lv[k] for k in got}, i
        for j, k in enumerate(("esigma", "etime", "ratio")):
            assert finfo[i, j].view(np.uint32) == np.float32(lv[k]).view(np.uint32), (i, k)
        assert len(lv["tau"]) == lv["nsteps"]
        assert np.array_equal(tau[i, :lv["nsteps"]].view(np.uint32), lv["tau"].view(np.uint32)), i


@pytest.mark.parametrize("ssize,dsize", [(161, 80), (83, 41), (641, 320), (160, 80)])
def test_area_tables(plan, ssize, dsize):
    ofs, wgt, cnt = np.full((dsize, 4), -7, np.int32), np.zeros((dsize, 4), np.float32), np.zeros(dsize, np.int32)
    plan.akaze_plan_area_tables(ssize, dsize, ofs.ctypes.data_as(C.c_void_p), wgt.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p))
    assert cnt.min() >= 1 and cnt.max() <= 4
    ulp = float(np.spacing(np.float32(1.0)))
    for d in range(dsize):
        o, w = ofs[d, :cnt[d]], wgt[d, :cnt[d]]
        assert o.min() >= 0 and o.max() < ssize, d
        assert np.all(np.diff(o) == 1), d                     # consecutive source pixels
        assert abs(float(np.sum(w.astype(np.float64))) - 1.0) <= 4 * ulp, d
        if ssize == 2 * dsize:
            assert list(o) == [2 * d, 2 * d + 1] and list(w) == [0.5, 0.5], d


@pytest.mark.parametrize("w,h", SIZES)
def test_launch_plan(plan, w, h):
    n, info, _, _ = plan_levels(plan, w, h)
    out = np.zeros(4 + 3 * 18, np.int32)
    for level in range(1, n):
        nsteps = int(info[level, 5])
        for batch in (1, 4):
            for level_fuse in (0, 1, 2):
                for level_strip in (0, 1, 2):
                    for fused_max in (LF_MAX_STEPS, 3):
                        launches = plan.akaze_plan_level(w, h, level, batch, level_fuse, level_strip, fused_max, out.ctypes.data_as(C.c_void_p))
                        case = (level, batch, level_fuse, level_strip, fused_max)
                        fuse, fused_level, try_strips = int(out[1]), bool(out[2]), bool(out[3])
                        passes = out[4:4 + 3 * launches].reshape(launches, 3)
                        assert launches >= 1 and int(passes[:, 1].sum()) == nsteps, case
                        assert list(passes[:, 0]) == [int(passes[:q, 1].sum()) for q in range(launches)], case
                        for q in range(launches):
                            depth = fused_max if (q == 0 and fused_level) else fuse
                            assert 1 <= passes[q, 1] <= depth, case
                        assert passes[-1, 2] == 1, case            # the last pass lands in Lt
                        assert list(passes[::-1, 2]) == [(q + 1) % 2 for q in range(launches)], case   # and the passes before it alternate
                        assert fuse in (4, 8) and fused_level == (level_fuse == 2 or (level_fuse == 1 and fuse == 8)), case
                        if try_strips:
                            assert not fused_level and level_strip and passes[0, 1] <= 4, case
