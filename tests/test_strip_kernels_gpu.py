"""GPU: the register-strip kernels (FED steps, smoothing + conductivity, the fused base stage) serve the large levels only; the LDS
tile kernels serve the rest. This runs the whole AKAZE parity file and the random-shape AKAZE fuzz again in a child process with the strips forced on for EVERY
level size (APDS_*_STRIP=2; the switches are read once per process), so their border variants meet the small, odd-sized, strided
and 1/3/4-channel images of those tests and must reproduce the oracle bit for bit there too."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_akaze_parity_with_strips_forced_on_every_level(gpu_pkg):
    env = dict(os.environ, APDS_NLD_STRIP="2", APDS_SF_STRIP="2", APDS_BASE_STRIP="2")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_akaze_gpu.py"),
                        os.path.join("tests", "test_fuzz_gpu.py") + "::test_akaze_random_shapes", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1000:])
    assert " passed" in r.stdout and "failed" not in r.stdout


def _rerun(env_extra):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_akaze_gpu.py"),
                        os.path.join("tests", "test_fuzz_gpu.py") + "::test_akaze_random_shapes", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1000:])
    assert " passed" in r.stdout and "failed" not in r.stdout


def test_akaze_parity_with_level_strips_on_every_level(gpu_pkg):
    """level_strip_kernel (smoothing + conductivity + FED steps on register strips, borders included) normally serves levels of
    1 .. 8 Mpx: here it serves every level of every test image, so its border waves meet the small and odd-sized ones."""
    _rerun({"APDS_LEVEL_STRIP": "2", "APDS_LEVEL_FUSE": "0", "APDS_LEVEL_STREAM": "0"})


def test_akaze_parity_with_lds_fused_levels_on_every_level(gpu_pkg):
    """level_fused_kernel (one launch per level, register patches exchanging through LDS) normally serves levels up to 1 Mpx."""
    _rerun({"APDS_LEVEL_FUSE": "2", "APDS_LEVEL_STRIP": "0"})


def test_akaze_parity_on_the_round_2_path(gpu_pkg):
    """separate smoothing / FED launches per level, keypoints placed by two passes over the masks, the LDS-tile Hessian kernel on every
    level with the masks cleared by the zeroing kernel, default events: none of round 3's streaming kernels"""
    _rerun({"APDS_LEVEL_FUSE": "0", "APDS_LEVEL_STRIP": "0", "APDS_KP_RANKED": "0", "APDS_EVENT_SCOPE": "1", "APDS_DOH_STRIP": "0", "APDS_LEVEL_STREAM": "0",
            "APDS_KP_XCD": "0", "APDS_HALF_FUSE": "0"})


def test_akaze_parity_with_full_fed_sweeps_in_the_fused_levels(gpu_pkg):
    """level_fused_kernel on every level without round 4's shrinking zone (every FED step sweeps the whole halo'd region, as in round 3): the
    default (shrinking) runs in the test above and in test_akaze_gpu.py itself."""
    _rerun({"APDS_LEVEL_FUSE": "2", "APDS_LEVEL_STRIP": "0", "APDS_FED_SHRINK": "0"})


def test_akaze_parity_with_the_streaming_kernels_on_every_level(gpu_pkg):
    """Round 3's streaming kernels - doh_strip_kernel (akaze_doh_strips.hip: determinant of the Hessian + extrema walking down 64-column
    strips, the masks written for every pixel instead of cleared) and level_stream_kernel (akaze_level_stream.hip: Gaussian, Scharr,
    conductivity and the first FED steps of a level, the same way) - normally serve levels of 8 Mpx and more. Here they serve every level
    of at least 64 pixels of every test image: top / bottom bands with reflected or clamped rows, first / last strips with reflected or
    clamped columns, partial last bands; once with 16-row bands and once with tall ones."""
    _rerun({"APDS_DOH_STRIP": "2", "APDS_DOH_STRIP_ROWS": "16", "APDS_LEVEL_STREAM": "2", "APDS_LEVEL_STREAM_ROWS": "16", "APDS_LEVEL_STRIP": "2", "APDS_LEVEL_FUSE": "0"})
    _rerun({"APDS_DOH_STRIP": "2", "APDS_DOH_STRIP_ROWS": "112", "APDS_LEVEL_STREAM": "2", "APDS_LEVEL_STREAM_ROWS": "100", "APDS_LEVEL_STRIP": "2", "APDS_LEVEL_FUSE": "0"})


STREAMING_SET = {"APDS_DOH_STRIP": "2", "APDS_LEVEL_STREAM": "2", "APDS_LEVEL_STRIP": "2", "APDS_LEVEL_FUSE": "0"}
BORDER_SIZES = [(63, 64), (64, 31), (64, 63), (64, 64), (70, 33)]   # w x h


@pytest.mark.parametrize("w,h", BORDER_SIZES)
def test_levels_beside_the_streaming_kernels_smallest_sizes_equal_oracle(gpu_pkg, oracle_mod, w, h):
    """Single-octave images on either side of the streaming kernels' smallest sizes (level_stream_kernel: 64 x 32, doh_strip_kernel:
    64 x 64): Lt and Ldet of every level and the keypoints equal the oracle's exactly (the planes, because such an image may have no
    keypoint at all). Under the process's switches; the test below runs it with the streaming set forced, where the plan hands a level
    below those sizes to level_strip_kernel / doh_fused_kernel."""
    forced = os.environ.get("APDS_TEST_EXPECT_SWITCHES")
    if forced:
        assert all(os.environ.get(k) == v for k, v in STREAMING_SET.items()), "the child process lost its switches"
    tile = gpu_pkg.synth.make_tile(h, w, frame_index=w + h, channels=1)
    ref = oracle_mod.akaze(tile, keep_planes=True)
    assert len(ref.levels) == 4 and all((lv["w"], lv["h"]) == (w, h) for lv in ref.levels)
    lib, ptr = gpu_pkg.lib(), gpu_pkg._lib.ptr
    for level in range(4):
        for name, which in (("Lt", 0), ("Ldet", 4)):
            got = np.zeros((h, w), np.float32)
            gpu_pkg._lib.check(lib.apds_akaze_debug_plane(ptr(tile), h, w, 1, tile.strides[0], level, which, ptr(got)))
            want = ref.plane(level, which)
            assert np.array_equal(got, want), (level, name, np.abs(got - want).max())
    got = gpu_pkg.feature_extraction.akaze_keypoint_descriptor_extraction_def(tile, None)
    assert len(got.keypoints) == len(ref.keypoints)
    for f in ("x", "y", "size", "response", "angle", "octave", "class_id"):
        assert np.array_equal(got.keypoints[f], ref.keypoints[f]), f
    assert np.array_equal(got.descriptors, ref.descriptors)


def test_the_plan_hands_levels_below_the_streaming_sizes_to_the_other_family(gpu_pkg):
    """The test above in a child process with APDS_DOH_STRIP=2 APDS_LEVEL_STREAM=2 APDS_LEVEL_STRIP=2 APDS_LEVEL_FUSE=0: 64 x 64 takes both
    streaming kernels, 70 x 33 and 64 x 63 the streaming level kernel and the LDS-tile Hessian kernel, 63 x 64 and 64 x 31 neither - the
    plan decides, no launcher is asked and refuses."""
    env = dict(os.environ, APDS_TEST_EXPECT_SWITCHES="1", **STREAMING_SET)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_strip_kernels_gpu.py"), "-k",
                        "test_levels_beside_the_streaming_kernels_smallest_sizes_equal_oracle", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1000:])
    assert f"{len(BORDER_SIZES)} passed" in r.stdout and "failed" not in r.stdout


def test_akaze_parity_with_separate_launches_and_the_current_keypoint_kernels(gpu_pkg):
    """separate smoothing / FED launches per level (no fused, strip or streaming level kernel) in front of the current keypoint and Hessian
    kernels: the round-2 test above also turns off the ranked placement, the streaming Hessian kernel, the XCD split and the fused
    half-sample."""
    _rerun({"APDS_LEVEL_FUSE": "0", "APDS_LEVEL_STRIP": "0", "APDS_LEVEL_STREAM": "0"})


def test_akaze_parity_with_the_hessian_fork_forced_off_and_on(gpu_pkg):
    """APDS_AKAZE_FORK=0 (the Hessian kernels stay on the caller's stream) and 2 (always on the side stream), a child process each: by
    default a thread forks only while it holds the process's one library context, so nothing else pins either path. The images of 96x640
    up to 1024^2 and the batches up to 7 are the smallest with several octaves (one fork per level), a level >= 1 Mpx (the strip family), a
    last level whose smoothing pass is separated only when forking, and a batch."""
    for fork in ("0", "2"):
        env = dict(os.environ, APDS_AKAZE_FORK=fork)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_akaze_gpu.py"), "-k",
                            "extraction_equals_oracle or batched_extraction_equals_oracle_per_image or odd_sizes_use_general_area_resize", "-q", "-m", "gpu",
                            "-x", "-p", "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (fork, r.stdout[-3000:], r.stderr[-1000:])
        assert " passed" in r.stdout and "failed" not in r.stdout


def test_match_parity_on_the_vector_alu_matcher(gpu_pkg):
    """APDS_MATCH_MFMA=0: hamming_topk_kernel (xor + popcount on the vector ALU) serves k <= 2 as well - the default sends those to the FP4
    matrix pipe (hamming_mfma.hip). Both must reproduce the oracle's keys: the match tests, the matcher fuzz, the sharded matcher and the
    keypoint table's match run again in a child process on the vector kernel."""
    env = dict(os.environ, APDS_MATCH_MFMA="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_match_gpu.py"), os.path.join("tests", "test_fuzz_gpu.py") + "::test_match_random_shapes",
                        os.path.join("tests", "test_shard_native.py"), os.path.join("tests", "test_keypoint_table_gpu.py"), "-q", "-m", "gpu", "-x", "-p",
                        "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1000:])
    assert " passed" in r.stdout and "failed" not in r.stdout
