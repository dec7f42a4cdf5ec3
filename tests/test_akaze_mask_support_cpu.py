"""CPU: the expected-result helper of the mask-support tests (akaze_mask_support_cases.py) on hand-made keypoint lists, the radii the
product's plan decides against the formula from keypoint fields, the preconditions of the GPU cases on the oracle's own result, and the new
entry points' signatures."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import akaze_mask_cases as mc
import akaze_mask_support_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kps(pkg, rows):
    """rows: (x, y, octave, size)"""
    k = np.zeros(len(rows), pkg._lib.KEYPOINT_DTYPE)
    for i, (x, y, octave, size) in enumerate(rows):
        k[i]["x"], k[i]["y"], k[i]["octave"], k[i]["size"], k[i]["response"], k[i]["class_id"] = x, y, octave, size, 1.0 + i, i
    return k


def _one_zero(h, w, row, col):
    m = np.ones((h, w), np.uint8)
    m[row, col] = 0
    return m


def test_scale_is_rint_half_to_even_in_f32_and_radius_is_an_integer_product(pkg):
    # size / ratio / 2: 2.5 -> 2, 3.5 -> 4 (half to even), 4.8 / 2 = 2.4 -> 2, octave 2: 19.2 / 8 = 2.4 -> 2, octave 3: 38.4 / 16 -> 2
    k = _kps(pkg, [(0, 0, 0, 5.0), (0, 0, 0, 7.0), (0, 0, 0, 4.8), (0, 0, 2, 19.2), (0, 0, 3, 38.4), (0, 0, 1, 11.416388)])
    assert sc.scales(k).tolist() == [2, 4, 2, 2, 2, 3]
    assert sc.radii(k, 15).tolist() == [30, 60, 30, 120, 240, 90] and sc.radii(k, 0).tolist() == [0] * 6
    assert sc.radii(k, 1).dtype == np.int64


def test_table_is_exclusive_and_rows_are_y():
    m = np.ones((3, 5), np.uint8)
    m[0, 4] = 0
    m[2, 1] = 0
    s = sc.zero_table(m)
    assert s.shape == (4, 6) and (s[0] == 0).all() and (s[:, 0] == 0).all()
    assert s[1].tolist() == [0, 0, 0, 0, 0, 1] and s[3].tolist() == [0, 0, 1, 1, 1, 2] and s[2, 5] == 1


def test_zero_exactly_at_the_radius_removes_and_one_past_it_keeps(pkg):
    h, w = 40, 60
    k = _kps(pkg, [(30.2, 19.7, 0, 4.8)])                    # centre (x, y) = (30, 20), scale 2; support 3: R = 6
    assert mc.rounded(k)[0].tolist() == [20] and mc.rounded(k)[1].tolist() == [30]
    for dy, dx, kept in ((0, 6, False), (0, -6, False), (6, 0, False), (-6, 0, False), (6, 6, False), (-6, -6, False),
                         (0, 7, True), (0, -7, True), (7, 0, True), (-7, 0, True), (7, 7, True), (-6, 7, True)):
        assert sc.survivors(k, _one_zero(h, w, 20 + dy, 30 + dx), 3).tolist() == [kept], (dy, dx)
    # rows are y: a zero 6 columns right and 7 rows down is outside, 7 columns right and 6 rows down as well
    assert sc.survivors(k, _one_zero(h, w, 27, 36), 3).tolist() == [True]
    assert sc.square_zero_counts(k, np.zeros((h, w), np.uint8), 3).tolist() == [13 * 13]


def test_squares_are_clipped_at_all_four_edges(pkg):
    h, w = 30, 50
    zeros = np.zeros((h, w), np.uint8)
    # scale 2, support 2: R = 4, a 9 x 9 square where it fits
    k = _kps(pkg, [(1.0, 15.0, 0, 4.8), (48.0, 15.0, 0, 4.8), (25.0, 2.0, 0, 4.8), (25.0, 28.0, 0, 4.8), (0.0, 0.0, 0, 4.8), (49.0, 29.0, 0, 4.8)])
    assert sc.square_zero_counts(k, zeros, 2).tolist() == [6 * 9, 6 * 9, 9 * 7, 9 * 6, 5 * 5, 5 * 5]
    # outside the image nothing is masked: an all-ones mask keeps every one of them, whatever the radius
    assert sc.survivors(k, np.ones((h, w), np.uint8), 1000).all()
    # a radius beyond the image: the whole image is the square
    assert sc.square_zero_counts(k, zeros, 1000).tolist() == [h * w] * 6
    assert sc.survivors(k, _one_zero(h, w, h - 1, w - 1), 1000).tolist() == [False] * 6


def test_support_0_is_the_pixel_rule_and_the_cut_comes_last(pkg):
    rng = np.random.default_rng(5)
    h, w = 33, 47
    m = (rng.random((h, w)) < 0.6).astype(np.uint8) * 9
    rows = [(float(x), float(y), int(o), 4.8 * 2 ** o) for x, y, o in zip(rng.random(64) * (w - 1), rng.random(64) * (h - 1), rng.integers(0, 4, 64))]
    k = _kps(pkg, rows)
    assert np.array_equal(sc.survivors(k, m, 0), mc.survivors(k, m))
    e = mc.Extraction(k, np.arange(len(k) * 61, dtype=np.uint32).astype(np.uint8).reshape(len(k), 61))
    mc.assert_same(sc.masked(e, m, 0), mc.masked(e, m))
    mc.assert_same(sc.masked(e, m, 0, 5), mc.masked(e, m, 5))
    # support 1 with a sparse mask: the strongest SURVIVORS, strongest first (responses rise with the row index)
    sparse = np.ones((h, w), np.uint8)
    sparse[10:14, 20:24] = 0
    keep = sc.survivors(k, sparse, 1)
    assert 3 < keep.sum() < len(k)
    assert sc.masked(e, sparse, 1, 3).keypoints["class_id"].tolist() == np.flatnonzero(keep)[::-1][:3].tolist()
    none = mc.Extraction(k[:0], e.descriptors[:0])
    assert len(sc.masked(none, m, 15, 3).keypoints) == 0 and sc.survivors(none.keypoints, m, 15).shape == (0,)


@pytest.fixture(scope="module")
def support_plan(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("akaze_mask_support") / "libakaze_mask_support_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "akaze_mask_support_host.cpp"), "-o", so])
    return C.CDLL(so)


def _units(support_plan, w, h, batch=1):
    units, octaves = (C.c_int * 16)(), (C.c_int * 16)()
    n = support_plan.akaze_mask_support_units(w, h, batch, units, octaves)
    return list(units)[:n], list(octaves)[:n]


@pytest.fixture(scope="module")
def oracle_cases(pkg, oracle_mod):
    oracle_mod.set_threads(8)
    small = oracle_mod.akaze(pkg.synth.make_tile(mc.H, mc.W, frame_index=mc.FRAME, channels=4))
    wide = oracle_mod.akaze(mc.octave3_tile(pkg))
    return small, wide


def test_plan_radii_equal_the_formula_from_keypoint_fields(support_plan, oracle_cases):
    seen = set()
    for (h, w), ref in zip(((mc.H, mc.W), (mc.H3, mc.W3)), oracle_cases):
        k = ref.keypoints
        units, octaves = _units(support_plan, w, h)
        assert len(units) == 16 and octaves == [i // 4 for i in range(16)]
        assert units == _units(support_plan, w, h, batch=7)[0]                       # the unit is the level's, whatever the batch
        lvl = k["class_id"].astype(np.int64)
        assert np.array_equal(np.asarray(octaves)[lvl], k["octave"])
        for support in (0, 1, 2, 15, 1000):
            want = sc.radii(k, support)
            got = np.asarray([support_plan.akaze_mask_support_radius(support, units[i]) for i in lvl.tolist()], np.int64)
            assert np.array_equal(got, np.minimum(want, 65536))
        seen |= set(lvl.tolist())
        # every level's unit is scale * ratio with scale in 2 .. 4: 2 .. 4, then doubled per octave
        assert all(units[i] % 2 ** octaves[i] == 0 and 2 <= units[i] >> octaves[i] <= 4 for i in range(16)), units
    assert len(seen) >= 11 and {0, 5, 8, 12} <= seen                              # levels of all four octaves carry a keypoint
    # past the largest image side the radius stops growing (every square is the whole image by then)
    assert support_plan.akaze_mask_support_radius(2 ** 31 - 1, 32) == 65536 and support_plan.akaze_mask_support_radius(0, 32) == 0


def test_preconditions_of_the_gpu_cases_on_the_oracle(oracle_cases):
    small, wide = oracle_cases
    k = small.keypoints
    assert len(k) == 208 and [int((k["octave"] == o).sum()) for o in range(4)] == [142, 62, 4, 0]
    assert set(sc.scales(k).tolist()) == {2, 3, 4}
    count = lambda m, s: int(sc.survivors(k, m, s).sum())      # noqa: E731
    assert (count(mc.left_half(), 0), count(mc.left_half(), 15)) == (83, 66)
    assert (count(mc.top_half(), 0), count(mc.top_half(), 15)) == (85, 41)
    assert [count(sc.hole(), s) for s in (0, 1, 15)] == [208, 206, 147]
    assert [count(sc.single_pixel(176, 320), s) for s in (0, 15)] == [208, 163]
    assert [count(mc.checkerboard(), s) for s in (1, 2, 15)] == [0, 0, 0] and 0 < count(mc.checkerboard(), 0) < 208
    for m in (mc.left_half(), mc.top_half(), sc.hole(), mc.checkerboard()):
        assert np.array_equal(sc.survivors(k, m, 0), mc.survivors(k, m))
    # the cuts of the GPU cases fall among the survivors, at distinct responses
    assert len(np.unique(k["response"])) == len(k)
    # the octave-3 tile: Rmax 240, and the three single pixels
    k3 = wide.keypoints
    assert len(k3) == 462 and int((k3["octave"] == 3).sum()) == 1 and int(sc.radii(k3, 15).max()) == 240
    o3 = k3[k3["octave"] == 3]
    assert (mc.rounded(o3)[0].tolist(), mc.rounded(o3)[1].tolist(), sc.radii(o3, 15).tolist()) == ([255], [233], [240])
    corner = sc.survivors(k3, sc.single_pixel(*sc.PIXEL_CORNER, mc.H3, mc.W3), 15)
    assert corner.sum() == 461 and k3["octave"][~corner].tolist() == [1]
    edge = sc.survivors(k3, sc.single_pixel(*sc.PIXEL_OCT3_EDGE, mc.H3, mc.W3), 15)
    assert edge.sum() == 461 and k3["octave"][~edge].tolist() == [3]
    assert sc.survivors(k3, sc.single_pixel(*sc.PIXEL_OCT3_PAST, mc.H3, mc.W3), 15).all()


def test_new_entry_points_are_bound(pkg):
    L = pkg.lib()
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    pp, ip = C.POINTER(C.c_void_p), C.POINTER(C.c_int)

    def plus_int_after(base, pos):
        return base[:pos] + [i] + base[pos:]

    # each new call is the masked call plus one int in front of max_points
    assert L.apds_akaze_extract_masked_support.argtypes == plus_int_after(list(L.apds_akaze_extract_masked.argtypes), 7)
    assert L.apds_akaze_extract_batch_masked_support.argtypes == plus_int_after(list(L.apds_akaze_extract_batch_masked.argtypes), 9)
    assert L.apds_dev_akaze_extract_masked_support.argtypes == plus_int_after(list(L.apds_dev_akaze_extract_masked.argtypes), 7)
    assert L.apds_dev_akaze_extract_batch_masked_support.argtypes == plus_int_after(list(L.apds_dev_akaze_extract_batch_masked.argtypes), 10)
    assert L.apds_akaze_extract_masked_support.argtypes == [vp, i, i, i, sz, vp, sz, i, i, pp, pp, ip, ip]
    assert L.apds_dev_mask_zero_sat.argtypes == [vp, i, i, sz, sz, vp, vp]
    assert (pkg._lib.TILE_MASK_NONE, pkg._lib.TILE_MASK_ALPHA, pkg._lib.TILE_MASK_ALPHA_SUPPORT, pkg._lib.MASK_SUPPORT_DESCRIPTOR) == (0, 1, 3, 15)
    with open(os.path.join(ROOT, "include", "apds.h")) as f:
        header = f.read()
    assert "#define APDS_MASK_SUPPORT_DESCRIPTOR 15\n" in header and "#define APDS_TILE_MASK_ALPHA_SUPPORT 3\n" in header
    fe = pkg.feature_extraction
    assert fe._mask_mode(False) == 0 and fe._mask_mode(True) == 1 and fe._mask_mode("support") == 3
    with pytest.raises(pkg.ApdsError) as e:
        fe._mask_mode("erode")
    assert e.value.code == pkg._lib.ERR_BAD_ARG


def test_negative_mask_support_is_refused_without_a_device(pkg):
    L, ptr = pkg.lib(), pkg._lib.ptr
    fe = pkg.feature_extraction
    tile, mask = np.zeros((8, 8), np.uint8), np.ones((8, 8), np.uint8)
    for call in (lambda: fe.akaze_keypoint_descriptor_extraction(tile, mask, None, -1),
                 lambda: fe.akaze_keypoint_descriptor_extraction(tile, None, None, mask_support=-1),
                 lambda: fe.akaze_keypoint_descriptor_extraction_batch([tile], None, mask=[mask], mask_support=-3)):
        with pytest.raises(pkg.ApdsError) as e:
            call()
        assert e.value.code == pkg._lib.ERR_BAD_ARG
    # the C entries themselves: the argument is checked in front of anything that needs a device
    kps, desc, n, nb = C.c_void_p(), C.c_void_p(), C.c_int(0), C.c_int(0)
    rc = L.apds_akaze_extract_masked_support(ptr(tile), 8, 8, 1, 8, ptr(mask), 8, -1, 0, C.byref(kps), C.byref(desc), C.byref(n), C.byref(nb))
    assert rc == pkg._lib.ERR_BAD_ARG and n.value == 0
    counts = (C.c_int * 1)()
    mptrs = (C.c_void_p * 1)(mask.ctypes.data)
    rc = L.apds_akaze_extract_batch_masked_support(ptr(tile), 1, 64, 8, 8, 1, 8, mptrs, 8, -1, 0, C.byref(kps), C.byref(desc), counts, C.byref(nb))
    assert rc == pkg._lib.ERR_BAD_ARG
    dummy = 4096       # never dereferenced: the argument check comes first
    rc = L.apds_dev_akaze_extract_masked_support(dummy, 8, 8, 1, 8, dummy, 8, -1, 0, dummy, dummy, 16, C.byref(n), None)
    assert rc == pkg._lib.ERR_BAD_ARG
    rc = L.apds_dev_akaze_extract_batch_masked_support(dummy, 1, 64, 8, 8, 1, 8, dummy, 8, 0, -1, 0, dummy, dummy, 16, counts, None)
    assert rc == pkg._lib.ERR_BAD_ARG
