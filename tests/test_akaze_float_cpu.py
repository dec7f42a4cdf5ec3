"""CPU: AKAZE's float descriptor (DESCRIPTOR_KAZE, 64 x f32) - the reference of tests/msurf_reference.py against what is known in closed form,
its committed tolerance against a fresh measurement, and the argument checks of the new entry points that need no device.
The GPU half: tests/test_akaze_float_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import akaze_float_cases as fc
import msurf_reference as ref


@pytest.fixture(scope="module")
def tile_run(pkg, oracle_mod):
    """the oracle's extraction of the 96 x 640 grey tile with its planes, and the reference rows in both precisions"""
    res = oracle_mod.akaze(pkg.synth.make_tile(96, 640, channels=1), keep_planes=True)
    planes = fc.oracle_planes(res)
    return res, ref.describe_levels(planes, res.keypoints, np.float64), ref.describe_levels(planes, res.keypoints, np.float32)


def test_constant_planes_give_the_closed_form():
    cases = fc.constant_cases()
    assert len(cases) == len(fc.HOOK_SHAPES) * len(fc.CONSTANT_ANGLES)
    for name, (lx, ly, kps, angle) in cases.items():
        got = ref.describe_plane(lx, ly, kps, np.float64)
        want = ref.constant_plane_row(angle)
        assert abs(np.linalg.norm(want) - 1) < 1e-12
        # wherever the keypoint lies - at the centre, on a corner, with most of its pattern off the plane - because the clamp keeps a constant constant
        assert np.abs(got - want[None, :]).max() < 1e-12, (name, np.abs(got - want[None, :]).max(axis=1))


def test_reference_rows_have_unit_norm_on_the_tile(tile_run):
    res, d64, _ = tile_run
    assert len(res.keypoints) >= 4
    assert np.abs(np.linalg.norm(d64, axis=1) - 1).max() < 1e-12


def test_committed_tolerance_covers_the_tile(tile_run):
    _, d64, d32 = tile_run
    e = float(np.abs(d32.astype(np.float64) - d64).max())
    print(f"e32 on the 96 x 640 tile: {e:.3e}; committed E32 {ref.E32:.3e}, TOL {ref.TOL:.3e}")
    assert ref.TOL == 4 * ref.E32 and ref.TOL <= 1e-3
    assert 4 * e <= ref.TOL


def test_zero_planes_give_zero_rows_in_the_reference():
    lx, ly, kps = fc.zero_case()
    for dt in (np.float32, np.float64):
        assert not ref.describe_plane(lx, ly, kps, dt).any()


def test_the_scale_is_the_f32_rint_with_ties_to_even():
    k = fc.keypoints([(0, 0, 5.0, 0, 0), (0, 0, 7.0, 0, 0), (0, 0, 20.0, 0, 2), (0, 0, 4.9999995, 0, 0)])
    assert [float(ref._scale_f32(kp)) for kp in k] == [2.0, 4.0, 2.0, 2.0]


def test_the_shifted_views_leave_few_queries_near_a_decision(pkg, oracle_mod):
    """The end-to-end GPU test drops the queries whose reference margins are below 8 TOL and allows 2 % of them: the reference alone, on the
    oracle's planes and keypoints, must stay inside that on this scene."""
    a, b = fc.shifted_views()
    rows = []
    for img in (a, b):
        res = oracle_mod.akaze(img, keep_planes=True)
        rows.append((res.keypoints, ref.describe_levels(fc.oracle_planes(res), res.keypoints, np.float64)))
    (ka, da), (kb, db) = rows
    assert len(ka) > 200 and len(kb) > 200
    _, _, ds, _ = ref.ratio_matches(da, db, fc.RATIO)
    m0, m1 = fc.ratio_margins(ds)
    near = (m0 < 8 * ref.TOL) | (m1 < 8 * ref.TOL)
    print(f"{int(near.sum())} of {len(near)} queries within 8 TOL of a decision")
    assert near.mean() <= 0.02


def test_new_entry_points_check_their_arguments_before_any_device_work(pkg):
    L, ptr, lib_ = pkg.lib(), pkg._lib.ptr, pkg._lib
    fe = pkg.feature_extraction
    tile, mask = np.zeros((8, 8), np.uint8), np.ones((8, 8), np.uint8)
    assert (lib_.AKAZE_DESCRIPTOR_KAZE, lib_.AKAZE_DESCRIPTOR_MLDB, lib_.DESC_FLOAT_DIM) == (3, 5, 64)
    kps, desc, n, dim = C.c_void_p(), C.c_void_p(), C.c_int(0), C.c_int(0)
    counts = (C.c_int * 1)()
    mptrs = (C.c_void_p * 1)(mask.ctypes.data)
    dummy = 4096       # never dereferenced: the argument check comes first
    # a negative mask support
    rc = L.apds_akaze_extract_float(ptr(tile), 8, 8, 1, 8, ptr(mask), 8, -1, 0, C.byref(kps), C.byref(desc), C.byref(n), C.byref(dim))
    assert rc == lib_.ERR_BAD_ARG and n.value == 0
    rc = L.apds_akaze_extract_float(ptr(tile), 8, 8, 1, 8, None, 0, -1, 0, C.byref(kps), C.byref(desc), C.byref(n), C.byref(dim))
    assert rc == lib_.ERR_BAD_ARG
    rc = L.apds_akaze_extract_float_batch(ptr(tile), 1, 64, 8, 8, 1, 8, mptrs, 8, -1, 0, C.byref(kps), C.byref(desc), counts, C.byref(dim))
    assert rc == lib_.ERR_BAD_ARG
    rc = L.apds_dev_akaze_extract_float(dummy, 8, 8, 1, 8, dummy, 8, -1, 0, dummy, dummy, 16, C.byref(n), None)
    assert rc == lib_.ERR_BAD_ARG
    rc = L.apds_dev_akaze_extract_float_batch(dummy, 1, 64, 8, 8, 1, 8, dummy, 8, 0, -1, 0, dummy, dummy, 16, counts, None)
    assert rc == lib_.ERR_BAD_ARG
    # a mask whose rows are shorter than the image's
    rc = L.apds_akaze_extract_float(ptr(tile), 8, 8, 1, 8, ptr(mask), 7, 0, 0, C.byref(kps), C.byref(desc), C.byref(n), C.byref(dim))
    assert rc == lib_.ERR_ASSERT and n.value == 0 and dim.value == 64
    rc = L.apds_dev_akaze_describe_float(dummy, 8, 8, dummy, -1, dummy, None)
    assert rc == lib_.ERR_BAD_ARG
    # the Python front
    with pytest.raises(pkg.ApdsError) as e:
        fe.akaze_keypoint_descriptor_extraction(tile, descriptor="nonsense")
    assert e.value.code == lib_.ERR_BAD_ARG
    with pytest.raises(pkg.ApdsError) as e:
        fe.akaze_keypoint_descriptor_extraction_batch([tile], descriptor="nonsense")
    assert e.value.code == lib_.ERR_BAD_ARG
    with pytest.raises(pkg.ApdsError) as e:
        fe.akaze_keypoint_descriptor_extraction(tile, mask, None, -1, descriptor="kaze")
    assert e.value.code == lib_.ERR_BAD_ARG


def test_l2_ratio_front_has_the_hamming_front_s_errors(pkg):
    fe = pkg.feature_extraction
    q = np.zeros((4, 64), np.float32)
    assert len(fe.get_knn_matches_l2(q[:0], q, 2, 0.7)) == 0 and len(fe.get_knn_matches_l2(q, q[:0], 2, 0.7)) == 0
    for args, code in (((q, q, 1, 0.7), pkg._lib.ERR_OUT_OF_RANGE), ((q, q[:1], 2, 0.7), pkg._lib.ERR_OUT_OF_RANGE), ((q, q, 0, 0.7), pkg._lib.ERR_ASSERT)):
        with pytest.raises(pkg.ApdsError) as e:
            fe.get_knn_matches_l2(*args)
        assert e.value.code == code
