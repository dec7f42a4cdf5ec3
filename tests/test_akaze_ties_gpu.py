"""GPU: the AKAZE kernels against the oracle, bit for bit, on images that tie (akaze_tie_cases.py): hundreds of keypoints with the same
response, mirrored and periodic neighbourhoods, hard edges. Nothing else in the suite decides a tie: on the synthetic tiles and on noise
all responses of an image differ. Pinned here: the strict comparisons of the extremum kernels, the order of the cross-level suppression
between equal responses, the max_points cut inside a run of equal responses (rank_select_kernel: ties by detection order), the first
maximum among equal sector sums of orientation_kernel and the degenerate 2 x 2 solve of subpixel_filter_kernel.

The parity tests run in this process under the default switches and again in child processes under the other kernel families (the
switches are read once per process), as test_strip_kernels_gpu.py does with the parity file."""
import os
import subprocess
import sys

import numpy as np
import pytest

import akaze_tie_cases as tc
from test_akaze_gpu import _assert_same_extraction, _plane

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_MAX_POINTS = 31       # inside the runs of equal responses of lattice48 [0, 36), periodic96x4 [30, 42) and lattice32 [0, 100)


@pytest.fixture(scope="module")
def inputs(gpu_pkg):
    return dict(tc.all_inputs(gpu_pkg.synth))


@pytest.fixture(scope="module")
def uncut(inputs, oracle_mod):
    oracle_mod.set_threads(8)
    return {name: oracle_mod.akaze(img) for name, img in inputs.items()}


@pytest.mark.parametrize("name", tc.ALL_NAMES)
def test_uncut_parity(gpu_pkg, inputs, uncut, name):
    ref = uncut[name]
    assert tc.tie_figures(ref.keypoints["response"])[2] >= 2
    _assert_same_extraction(gpu_pkg.feature_extraction.akaze_keypoint_descriptor_extraction_def(inputs[name], None), ref)


@pytest.mark.parametrize("name", tc.ALL_NAMES)
def test_cut_parity(gpu_pkg, inputs, uncut, oracle_mod, name):
    """max_points just before, inside (three places) and just after the longest run of equal responses and a short one"""
    cuts = tc.tie_cuts(uncut[name].keypoints["response"])
    assert sum(inside for _, inside in cuts) >= 2
    for mp, inside in cuts:
        got = gpu_pkg.feature_extraction.akaze_keypoint_descriptor_extraction_def(inputs[name], mp)
        ref = oracle_mod.akaze(inputs[name], max_points=mp)
        assert len(ref.keypoints) == min(mp, len(uncut[name].keypoints))
        try:
            _assert_same_extraction(got, ref)
        except AssertionError as e:
            raise AssertionError(f"{name}: max_points {mp} ({'inside' if inside else 'beside'} a run of equal responses): {e}") from e


@pytest.mark.parametrize("name", ["checker32_256", "kron_binary8"])
def test_planes_equal_oracle_on_ties(gpu_pkg, inputs, oracle_mod, name):
    """Ldet and the keypoint mask of every level: a difference in Ldet or in a mask whose Ldet is equal is a detection tie decided the
    other way (or a suppression one: the mask is the one after suppression)"""
    img = inputs[name]
    ref = oracle_mod.akaze(img, keep_planes=True)
    for level, lv in enumerate(ref.levels):
        got = _plane(gpu_pkg, img, level, 4, (lv["h"], lv["w"]))
        want = ref.plane(level, oracle_mod.PLANE_LDET)
        assert np.array_equal(got, want), (level, "Ldet", np.abs(got - want).max())
        m = _plane(gpu_pkg, img, level, 7, (lv["h"], lv["w"]), np.uint8)
        want = ref.plane(level, oracle_mod.PLANE_MASK1) != 0
        assert np.array_equal(m != 0, want), (level, "mask", np.argwhere((m != 0) != want)[:4].tolist())


@pytest.mark.parametrize("max_points", [None, BATCH_MAX_POINTS])
def test_batch_of_tie_images(gpu_pkg, oracle_mod, uncut, max_points):
    """lattice48, a flat image, periodic96x4, the binary kron image, lattice32 in ONE call: the batched suppression shares its rounds
    across the images, and a tie-heavy neighbour must not disturb another image's order. Each image against the oracle and against
    the single-image call."""
    imgs = tc.batch_images(gpu_pkg.synth)
    names = ["lattice48", None, "periodic96x4", "kron_binary8", "lattice32"]
    if max_points is not None:
        inside = [n for n in names if n and any(a < max_points < b for a, b in tc.runs(uncut[n].keypoints["response"]))]
        assert len(inside) >= 2, inside
    fe = gpu_pkg.feature_extraction
    got = fe.akaze_keypoint_descriptor_extraction_batch(imgs, max_points)
    assert len(got) == 5 and len(got[1].keypoints) == 0
    for i in range(5):
        ref = oracle_mod.akaze(imgs[i]) if max_points is None else oracle_mod.akaze(imgs[i], max_points=max_points)
        assert i == 1 or len(ref.keypoints) > 0
        _assert_same_extraction(got[i], ref)
        one = fe.akaze_keypoint_descriptor_extraction_def(imgs[i], max_points)
        assert np.array_equal(one.keypoints, got[i].keypoints) and np.array_equal(one.descriptors, got[i].descriptors)


@pytest.mark.parametrize("which", sorted(tc.DEEP_IMAGES))
def test_deep_suppression_parity(gpu_pkg, oracle_mod, which):
    """the images whose suppression passes need the most rounds (test_akaze_tie_inputs_cpu.py asserts how many): alone, and as a batch
    of two identical copies"""
    img = tc.DEEP_IMAGES[which]()
    oracle_mod.set_threads(8)
    ref = oracle_mod.akaze(img)
    assert len(ref.keypoints) > 0
    fe = gpu_pkg.feature_extraction
    _assert_same_extraction(fe.akaze_keypoint_descriptor_extraction_def(img, None), ref)
    pair = fe.akaze_keypoint_descriptor_extraction_batch(np.stack([img, img]), None)
    assert len(pair) == 2
    for got in pair:
        _assert_same_extraction(got, ref)


# --- the other kernel families, a child process each ---------------------------------------------------------------------------------
PARITY = "test_uncut_parity or test_cut_parity"
ALL_PARITY = PARITY + " or test_planes_equal_oracle_on_ties or test_batch_of_tie_images or test_deep_suppression_parity"


def _rerun(env_extra, select):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_akaze_ties_gpu.py"), "-k", select, "-q", "-m", "gpu", "-x", "-p",
                        "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1000:])
    assert " passed" in r.stdout and "failed" not in r.stdout


def test_ties_on_the_round_2_path(gpu_pkg):
    """keypoints placed by two passes over the masks (no ranked placement, no XCD split), the LDS-tile Hessian kernel on every level,
    separate smoothing / FED launches: planes, batch and the deep images as well"""
    _rerun({"APDS_LEVEL_FUSE": "0", "APDS_LEVEL_STRIP": "0", "APDS_KP_RANKED": "0", "APDS_EVENT_SCOPE": "1", "APDS_DOH_STRIP": "0", "APDS_LEVEL_STREAM": "0",
            "APDS_KP_XCD": "0", "APDS_HALF_FUSE": "0"}, ALL_PARITY)


def test_ties_with_lds_fused_levels_on_every_level(gpu_pkg):
    _rerun({"APDS_LEVEL_FUSE": "2", "APDS_LEVEL_STRIP": "0"}, PARITY)


def test_ties_with_the_streaming_kernels_on_every_level(gpu_pkg):
    """doh_strip_kernel's extremum test (16-row bands: a band border every 16 rows of a periodic image) and level_stream_kernel"""
    _rerun({"APDS_DOH_STRIP": "2", "APDS_DOH_STRIP_ROWS": "16", "APDS_LEVEL_STREAM": "2", "APDS_LEVEL_STREAM_ROWS": "16", "APDS_LEVEL_STRIP": "2",
            "APDS_LEVEL_FUSE": "0"}, PARITY)


def test_ties_with_the_hessian_fork_always_on(gpu_pkg):
    _rerun({"APDS_AKAZE_FORK": "2"}, PARITY)
