"""GPU: csrc/ingest.hip at its edges: band merge, perspective warp and world points against the independent references of
tests/ingest_reference.py (the rules and bounds of tests/test_ingest_reference_cpu.py, whose docstring derives them) and, bit for bit,
against the oracle. Inputs: tests/ingest_border_cases.py. Every case is a few hundred pixels or points, except the one band-merge
length that reaches the second trip of the grid-stride loop.

Largest observed fractions of each bound on an MI355X, the same as the oracle's since the results are bit-equal to it: no byte of the
band merge differs outside the near-tie band; warp, projective maps: u8 0.94, f32 0.97; warp, W < 0 columns: 0.50; world points: 0.034."""
import numpy as np
import pytest

import ingest_border_cases as bc
import ingest_reference as ref

pytestmark = pytest.mark.gpu

TYPE_IDS = [f"{d.__name__}x{c}" for d, c in bc.WARP_TYPES]


@pytest.fixture(scope="module")
def band_refs():
    """{case: (bands, minmax, reference rgba, near_tie)}, computed once"""
    out = {}
    for case in bc.BAND_CASES:
        bands, mm = bc.band_case(*case)
        out[case] = (bands, mm) + ref.band_merge_ref(*bands, mm)
    return out


def _warp(pkg, src, M, size):
    hg = pkg.homographier
    ch = 1 if src.ndim == 2 else src.shape[2]
    return hg.warp_image_perspective(hg.Cmat(src, src.dtype.type, ch), hg.Cmat(np.asarray(M, np.float64), np.float64), size).mat


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- band merge ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bgra", [False, True], ids=["rgba", "bgra"])
@pytest.mark.parametrize("case", bc.BAND_CASES, ids=lambda c: f"{c[1]}-{c[0]}")
def test_band_merge_at_its_edges(gpu_pkg, oracle_mod, band_refs, case, bgra):
    ge = gpu_pkg.geotiff_extractor
    bands, mm, want, tie = band_refs[case]
    got = ge.band_merger(list(bands), ge.BandsMinMax(*mm), bgra=bgra)
    bad = ref.band_mismatches(got, want, tie, bgra)
    assert len(bad) == 0, (bad[:5], got[bad[:5, 0]], want[bad[:5, 0]])
    ora = oracle_mod.band_merger(*bands, np.array(mm, np.float64))
    assert np.array_equal(got, ora[:, [2, 1, 0, 3]] if bgra else ora)
    all_nan = np.isnan(bands).all(0)
    assert np.array_equal(got[:, 3], np.where(all_nan, 0, 255))      # alpha 0 for three NaNs only
    red, blue = (2, 0) if bgra else (0, 2)
    if case[1] == "degenerate":
        assert not got[:, red].any()                                  # min == max: every pixel 0
        assert case[0] == 1 or (got[:, 1].any() and got[:, blue].any())
    if case[0] >= 526:
        assert len(np.unique(got[:, blue])) == 256                    # either side of every u8 boundary


# ---- warp, exact -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,channels", bc.WARP_TYPES, ids=TYPE_IDS)
def test_warp_dyadic_shifts_are_exact(gpu_pkg, oracle_mod, dtype, channels):
    """the 2 x 2 footprint across each source edge and corner, and wholly outside; f32 sources are small integers, so bit for bit"""
    for w, h in bc.WARP_SOURCES:
        src = bc.warp_source(dtype, channels, w, h)
        size = (w + 2, h + 2)
        for tx, ty in bc.WARP_SHIFTS + [bc.WARP_SHIFT_OUTSIDE]:
            M = bc.shift_matrix(tx, ty)
            got = _warp(gpu_pkg, src, M, size)
            want = ref.warp_ref_dyadic(src, tx, ty, size)
            assert got.dtype == dtype and np.array_equal(got.astype(ref.LD), want.astype(ref.LD)), (w, h, tx, ty)
            assert _same_bits(got, oracle_mod.warp_perspective(src, M, size)), (w, h, tx, ty)
            if (tx, ty) == bc.WARP_SHIFT_OUTSIDE:
                assert (got == 1).all()


@pytest.mark.parametrize("dtype,channels", bc.WARP_TYPES, ids=TYPE_IDS)
def test_warp_destination_widths_around_the_block(gpu_pkg, oracle_mod, dtype, channels):
    src = bc.warp_source(dtype, channels, 7, 5)
    for dw in bc.WARP_WIDTHS:
        for dh in bc.WARP_HEIGHTS:
            for tx, ty in bc.WARP_WIDTH_SHIFTS:
                M = bc.shift_matrix(tx, ty)
                got = _warp(gpu_pkg, src, M, (dw, dh))
                want = ref.warp_ref_dyadic(src, tx, ty, (dw, dh))
                assert np.array_equal(got.astype(ref.LD), want.astype(ref.LD)), (dw, dh, tx, ty)
                assert _same_bits(got, oracle_mod.warp_perspective(src, M, (dw, dh))), (dw, dh, tx, ty)
                if dw > bc.WARP_BLOCK and (tx, ty) == bc.WARP_WIDTH_SHIFTS[1]:
                    assert (want.reshape(dh, dw, -1)[:, bc.WARP_BLOCK:] != 1).any()      # the second block does read the source


# ---- warp, bounded ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,channels", bc.WARP_TYPES, ids=TYPE_IDS)
def test_warp_projective_within_the_bilinear_bound(gpu_pkg, oracle_mod, dtype, channels):
    src = bc.warp_bounded_source(dtype, channels)
    for minv in bc.WARP_BOUNDED_MINV:
        M = bc.forward_of(minv)
        got = _warp(gpu_pkg, src, M, bc.WARP_BOUNDED_DST)
        ratio = ref.warp_bounded_ratio(got, src, minv, bc.WARP_BOUNDED_DST)
        print("warp bounded", dtype.__name__, channels, ratio)
        assert ratio <= 1.0
        assert _same_bits(got, oracle_mod.warp_perspective(src, M, bc.WARP_BOUNDED_DST))


# ---- warp, structural ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,channels", bc.WARP_TYPES, ids=TYPE_IDS)
def test_warp_w_zero_negative_w_and_saturated_coordinates(gpu_pkg, oracle_mod, dtype, channels):
    src = bc.warp_source(dtype, channels, *bc.WARP_STRUCT_SRC)
    s3 = src.reshape(src.shape[0], src.shape[1], -1)
    got = _warp(gpu_pkg, src, bc.WARP_WZERO_M, bc.WARP_STRUCT_DST)
    g3 = got.reshape(got.shape[0], got.shape[1], -1)
    assert (g3[:, bc.WARP_WZERO_COLUMN] == s3[0, 0]).all()           # W == 0 reads source pixel (0, 0)
    ratio = ref.warp_bounded_ratio(got, src, bc.WARP_WZERO_MINV, bc.WARP_STRUCT_DST)      # W < 0 (columns 0-3) and W > 0 alike
    print("warp W<0", dtype.__name__, channels, ratio)
    assert ratio <= 1.0
    assert _same_bits(got, oracle_mod.warp_perspective(src, bc.WARP_WZERO_M, bc.WARP_STRUCT_DST))
    M = bc.forward_of(bc.WARP_SATURATE_MINV)
    got = _warp(gpu_pkg, src, M, bc.WARP_STRUCT_DST)
    g3 = got.reshape(got.shape[0], got.shape[1], -1)
    assert (g3[:, 1:] == 1).all() and (g3[:, 0] == s3[0, 0]).all()   # saturated coordinates: border; x == 0 has W == 0
    assert _same_bits(got, oracle_mod.warp_perspective(src, M, bc.WARP_STRUCT_DST))


# ---- world points ----------------------------------------------------------------------------------------------------------------------
def _elevation_table(pkg, dgt, egt):
    t = pkg.feature_database.ElevationTable()
    t.create_geotransform("dataset", dgt)
    if egt is not None:
        t.create_geotransform("elevation", egt)
        t.add_elevation_data(bc.ELEV)
    return t


def _host_world(pkg, xy, table):
    """apds_get_world_coordinates, the call under ElevationTable.get_world_coordinates_batch, as it is: (status, xyz). The method itself
    raises on a miss and keeps the points from the caller."""
    xy = np.ascontiguousarray(xy, np.float64)
    out = np.zeros((len(xy), 3), np.float64)
    L, ptr = pkg.lib(), pkg._lib.ptr
    if table.elevation is None:
        rc = L.apds_get_world_coordinates(ptr(xy), len(xy), ptr(table.transforms["dataset"]), None, None, 0, 0, ptr(out))
    else:
        rc = L.apds_get_world_coordinates(ptr(xy), len(xy), ptr(table.transforms["dataset"]), ptr(table.transforms["elevation"]), ptr(table.elevation),
                                          table.elevation.shape[1], table.elevation.shape[0], ptr(out))
    return rc, out


@pytest.mark.parametrize("name", list(bc.WORLD_CASES))
def test_world_points_at_their_edges(gpu_pkg, oracle_mod, name):
    xy, dgt, egt = bc.WORLD_CASES[name]
    elev = bc.ELEV if egt is not None else None
    table = _elevation_table(gpu_pkg, dgt, egt)
    rc, got = _host_world(gpu_pkg, xy, table)
    ratio, miss = ref.world_ratio(got, xy, dgt, egt, elev)           # hits and misses as the reference says; misses NaN, the rest finite
    print("world", name, ratio, int(miss.sum()))
    assert ratio <= 1.0
    assert rc == (gpu_pkg._lib.ERR_OUT_OF_RANGE if miss.any() else 0)
    orc, ora = oracle_mod.world_coordinates(xy, dgt, egt, elev)
    assert orc == rc and got.tobytes() == ora.tobytes()
    if miss.any():
        with pytest.raises(gpu_pkg.ApdsError) as e:
            table.get_world_coordinates_batch(xy)
        assert e.value.code == gpu_pkg._lib.ERR_OUT_OF_RANGE
    else:
        assert table.get_world_coordinates_batch(xy).tobytes() == got.tobytes()


class _Extracted:
    def __init__(self, keypoints, descriptors):
        self.keypoints, self.descriptors = keypoints, descriptors


@pytest.mark.parametrize("n", bc.WORLD_COLUMN_COUNTS)
def test_table_world_points_count_the_misses(gpu_pkg, n):
    """the column kernel on the same edge points as f32 columns: the reference's miss count, over partial waves and a second block"""
    xy = bc.world_edge_points(n)
    want, miss, _, _, h = ref.world_ref(xy, bc.DGT_POW2, bc.EGT_POW2, bc.ELEV)
    k = np.zeros(n, gpu_pkg._lib.KEYPOINT_DTYPE)
    k["x"], k["y"] = xy[:, 0].astype(np.float32), xy[:, 1].astype(np.float32)
    table = gpu_pkg.feature_database.KeypointTable(n)
    try:
        table.create_keypoints(_Extracted(k, np.zeros((n, 61), np.uint8)), 1, 0, 0, 0, (512, 512))
        assert table.world_coordinates(_elevation_table(gpu_pkg, bc.DGT_POW2, bc.EGT_POW2)) == int(miss.sum())
        _, _, xyz, rows = table.device_table()
        assert rows == n and xyz
        got = np.zeros((n, 3), np.float64)
        gpu_pkg._lib.check(gpu_pkg.lib().apds_dev_download(gpu_pkg._lib.ptr(got), xyz, got.nbytes, None))
        ratio, _ = ref.world_ratio(got, xy, bc.DGT_POW2, bc.EGT_POW2, bc.ELEV)
        assert ratio <= 1.0
    finally:
        table.close()
