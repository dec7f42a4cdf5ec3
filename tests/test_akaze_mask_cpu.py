"""CPU: the expected-result helper of the mask tests (akaze_mask_cases.py) on hand-made keypoint lists, the preconditions of the GPU
cases on the oracle's own result, and the new entry points' signatures."""
import ctypes as C

import numpy as np

import akaze_mask_cases as mc


def _kps(pkg, rows):
    k = np.zeros(len(rows), pkg._lib.KEYPOINT_DTYPE)
    for i, (x, y, resp) in enumerate(rows):
        k[i]["x"], k[i]["y"], k[i]["response"], k[i]["class_id"] = x, y, resp, i
    return k


def _ext(pkg, rows):
    k = _kps(pkg, rows)
    return mc.Extraction(k, np.arange(len(k) * 61, dtype=np.uint32).astype(np.uint8).reshape(len(k), 61))


def test_rounding_is_add_half_and_truncate_in_f32(pkg):
    below = np.nextafter(np.float32(2.5), np.float32(0))            # the largest f32 below 2.5
    k = _kps(pkg, [(2.5, 1.0, 1), (below, 1.0, 1), (2.49, 3.5, 1), (0.0, 0.49, 1), (16777215.0, 0.0, 1)])
    ys, xs = mc.rounded(k)
    assert xs.tolist() == [3, 2, 2, 0, 16777216] and ys.tolist() == [1, 1, 4, 0, 0]      # the last: 2^24 - 1 + 0.5 rounds to even in f32
    assert ys.dtype == np.int32 and xs.dtype == np.int32
    # 0.49999997 + 0.5 is 1.0 in f32 (0.99999997 is no f32: ties to even), and 0 in double: the rule is the f32 one
    edge = np.float32(0.49999997)
    assert int(np.float32(edge) + np.float32(0.5)) == 1 and int(float(edge) + 0.5) == 0
    assert mc.rounded(_kps(pkg, [(edge, edge, 1)]))[1].tolist() == [1]


def test_mask_lookup_axes_last_row_and_column_and_empty_list(pkg):
    h, w = 5, 9
    m = np.zeros((h, w), np.uint8)
    m[h - 1, w - 1] = 7                                              # any non-zero value keeps
    m[1, 3] = 1
    e = _ext(pkg, [(3.2, 0.8, 5), (0.8, 3.2, 6), (w - 1.4, h - 1.3, 7), (w - 1.6, h - 1.0, 8), (w - 1.0, h - 1.5, 9)])
    keep = mc.survivors(e.keypoints, m)
    assert keep.tolist() == [True, False, True, False, True]        # (x, y) = (3, 1) kept, (1, 3) not: rows are y
    out = mc.masked(e, m)
    assert out.keypoints["class_id"].tolist() == [0, 2, 4] and np.array_equal(out.descriptors, e.descriptors[[0, 2, 4]])
    none = _ext(pkg, [])
    assert len(mc.masked(none, m).keypoints) == 0 and mc.masked(none, m, 3).descriptors.shape == (0, 61)
    assert mc.survivors(none.keypoints, m).shape == (0,)


def test_cut_follows_the_mask_strongest_first_ties_by_detection_order(pkg):
    m = np.ones((4, 8), np.uint8)
    m[:, 0] = 0
    e = _ext(pkg, [(0, 0, 100.0), (1, 0, 3.0), (2, 0, 9.0), (3, 0, 3.0), (4, 0, 9.0), (5, 0, 1.0)])
    assert mc.masked(e, m, 5).keypoints["class_id"].tolist() == [1, 2, 3, 4, 5]       # five survivors, five allowed: detection order
    assert mc.masked(e, m, 4).keypoints["class_id"].tolist() == [2, 4, 1, 3]          # cut: response descending, ties by detection order
    assert mc.masked(e, m, 1).keypoints["class_id"].tolist() == [2]                   # the strongest SURVIVOR, not the strongest keypoint
    assert mc.masked(e, m).keypoints["class_id"].tolist() == [1, 2, 3, 4, 5]


def test_preconditions_of_the_gpu_cases_on_the_oracle(pkg, oracle_mod):
    tile = pkg.synth.make_tile(mc.H, mc.W, frame_index=mc.FRAME, channels=4)
    oracle_mod.set_threads(8)
    ref = oracle_mod.akaze(tile)
    k = ref.keypoints
    assert len(np.unique(k["response"])) == len(k) > 100
    keep = mc.survivors(k, mc.checkerboard())
    per = [(int((keep & (k["octave"] == o)).sum()), int((~keep & (k["octave"] == o)).sum())) for o in range(4)]
    assert all(min(p) >= 1 for p in per[:3]) and per[3] == (0, 0), per
    s, t = int(mc.survivors(k, mc.left_half()).sum()), int(mc.survivors(k, mc.top_half()).sum())
    assert 20 < s < len(k) - 20 and 20 < t < len(k) - 20
    # the helper's cut is the oracle's (all-ones mask), at a cut with distinct responses on either side
    m = s // 3
    byresp = np.sort(k["response"])[::-1]
    assert byresp[m - 2] > byresp[m - 1] > byresp[m] > byresp[m + 1]
    mc.assert_same(mc.masked(ref, np.ones((mc.H, mc.W), np.uint8), m), oracle_mod.akaze(tile, max_points=m))
    k3 = oracle_mod.akaze(mc.octave3_tile(pkg)).keypoints
    assert (k3["octave"] == 3).sum() >= 1 and all((k3["octave"] == o).sum() >= 2 for o in range(3))


def test_new_entry_points_are_bound(pkg):
    L = pkg.lib()
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    pp, ip = C.POINTER(C.c_void_p), C.POINTER(C.c_int)
    assert L.apds_akaze_extract_masked.argtypes == [vp, i, i, i, sz, vp, sz, i, pp, pp, ip, ip]
    assert L.apds_dev_akaze_extract_batch_masked.argtypes == [vp, i, sz, i, i, i, sz, vp, sz, sz, i, vp, vp, i, ip, vp]
    assert len(L.apds_tile_extract_ex.argtypes) == len(L.apds_tile_extract.argtypes) + 1
    assert len(L.apds_tile_extract_batch_ex.argtypes) == len(L.apds_tile_extract_batch.argtypes) + 1
    assert len(L.apds_mosaic_tile_extract_ex.argtypes) == len(L.apds_mosaic_tile_extract.argtypes) + 1
    assert len(L.apds_mosaic_tile_extract_batch_ex.argtypes) == len(L.apds_mosaic_tile_extract_batch.argtypes) + 1
    assert (pkg._lib.TILE_MASK_NONE, pkg._lib.TILE_MASK_ALPHA) == (0, 1)
    # argument errors that need no device
    fe = pkg.feature_extraction
    tile = np.zeros((8, 8), np.uint8)
    for bad in (np.zeros((8, 7), np.uint8), np.zeros((8, 8), np.float32)):
        try:
            fe.akaze_keypoint_descriptor_extraction(tile, bad, None)
        except pkg.ApdsError as e:
            assert e.code == pkg._lib.ERR_ASSERT
        else:
            raise AssertionError("a mask of another size or type was accepted")
