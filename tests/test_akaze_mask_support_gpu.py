"""GPU: the mask support of the AKAZE detection mask (apds_*_masked_support, apds_dev_mask_zero_sat, APDS_TILE_MASK_ALPHA_SUPPORT,
mask_support= / mask_nodata="support" in the Python fronts).

The table alone is compared with numpy's cumsum, exactly. Extractions are compared bit for bit (seven keypoint fields and the descriptors)
with the expectation akaze_mask_support_cases.py builds from the UNMASKED oracle result; its preconditions (how many keypoints each mask
keeps at each support) are asserted on the oracle by tests/test_akaze_mask_support_cpu.py.

Shapes of the table test: 1 x 1, one row, one column, 63 x 65 (below a lane's 16 bytes times 4 + 1, no full wave), 257 x 1031 (past the 256-row
chunk of the column pass and the 1024-pixel chunk of a wave in the row pass, neither a multiple of 16 or 32), a plane with row stride >
cols whose padding holds zeros, and the alpha of a BGRA image (pixel stride 4) whose colour bytes hold zeros."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import akaze_mask_cases as mc
import akaze_mask_support_cases as sc
from stream_handover import hand_over

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = mc.H, mc.W
SUPPORTS = (0, 1, 15)


def _expect_switch():
    if os.environ.get("APDS_TEST_EXPECT_KP_RANKED") is not None:
        assert os.environ.get("APDS_KP_RANKED") == os.environ["APDS_TEST_EXPECT_KP_RANKED"], "the child process lost its switch"


@pytest.fixture(scope="module")
def dev(gpu_pkg):
    import torch
    return torch, torch.device("cuda:0"), gpu_pkg._lib.lib(), gpu_pkg._lib.check


@pytest.fixture(scope="module")
def case(gpu_pkg, oracle_mod):
    """the 352 x 640 tile and its unmasked oracle result, computed once and never modified"""
    tile = gpu_pkg.synth.make_tile(H, W, frame_index=mc.FRAME, channels=4)
    oracle_mod.set_threads(8)
    ref = oracle_mod.akaze(tile)
    for f in (tile, ref.keypoints, ref.descriptors):
        f.setflags(write=False)
    return tile, ref


@pytest.fixture(scope="module")
def case3(gpu_pkg, oracle_mod):
    """the 544 x 672 tile with one octave-3 keypoint"""
    tile = mc.octave3_tile(gpu_pkg)
    oracle_mod.set_threads(8)
    ref = oracle_mod.akaze(tile)
    for f in (tile, ref.keypoints, ref.descriptors):
        f.setflags(write=False)
    return tile, ref


# ---- the table alone ----------------------------------------------------------------------------------------------------------------------
def _sat(dev, plane_bytes, first, rows, cols, row_stride, pix_stride):
    """apds_dev_mask_zero_sat on the byte buffer `plane_bytes` (mask byte (y, x) at first + y * row_stride + x * pix_stride); the output
    buffer has 64 guard words on either side"""
    torch, d, L, check = dev
    src = torch.from_numpy(plane_bytes).to(d)
    n = (rows + 1) * (cols + 1)
    out = torch.full((n + 128,), 0x5A5A5A5A, dtype=torch.int32, device=d)
    hand_over()
    check(L.apds_dev_mask_zero_sat(src.data_ptr() + first, rows, cols, row_stride, pix_stride, out.data_ptr() + 64 * 4, None))
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[:64] == 0x5A5A5A5A).all() and (got[n + 64:] == 0x5A5A5A5A).all(), "written outside the table"
    return got[64:n + 64].reshape(rows + 1, cols + 1)


def _fills(rows, cols, seed):
    rng = np.random.default_rng(seed)
    sparse = np.full((rows, cols), 255, np.uint8)
    sparse[rng.integers(0, rows), rng.integers(0, cols)] = 0
    return {"zeros": np.zeros((rows, cols), np.uint8), "ones": np.full((rows, cols), 1, np.uint8),
            "random": (rng.integers(0, 3, (rows, cols)) * 100).astype(np.uint8), "one zero": sparse}


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 67), (67, 1), (63, 65), (257, 1031)])
def test_zero_sat_of_a_plane_equals_cumsum(dev, rows, cols):
    for name, m in _fills(rows, cols, rows * 10000 + cols).items():
        got = _sat(dev, m.reshape(-1), 0, rows, cols, cols, 1)
        assert np.array_equal(got, sc.zero_table(m).astype(np.uint32)), name
    if (rows, cols) == (257, 1031):
        assert int(got[-1, -1]) == 1 and int(sc.zero_table(_fills(rows, cols, 0)["zeros"])[-1, -1]) == rows * cols


def test_zero_sat_with_a_row_stride_and_with_the_alpha_of_a_bgra_image(dev):
    rows, cols, stride = 37, 100, 131
    for name, m in _fills(rows, cols, 7).items():
        wide = np.zeros((rows, stride), np.uint8)                      # the padding is all zeros: counting it shows
        wide[:, :cols] = m
        got = _sat(dev, wide.reshape(-1)[: (rows - 1) * stride + cols].copy(), 0, rows, cols, stride, 1)
        assert np.array_equal(got, sc.zero_table(m).astype(np.uint32)), name
    rows, cols = 45, 83
    for name, m in _fills(rows, cols, 8).items():
        bgra = np.zeros((rows, cols, 4), np.uint8)                     # colour bytes all zero
        bgra[..., 3] = m
        got = _sat(dev, bgra.reshape(-1), 3, rows, cols, cols * 4, 4)
        assert np.array_equal(got, sc.zero_table(m).astype(np.uint32)), name
        # the same bytes at pixel stride 4 from byte 1 of the words (an unaligned base) and at a pixel stride that has no wide path
        for first, pix in ((1, 4), (2, 3)):
            buf = np.zeros(rows * cols * pix + 8, np.uint8)
            buf[first: first + rows * cols * pix: pix] = m.reshape(-1)
            got = _sat(dev, buf, first, rows, cols, cols * pix, pix)
            assert np.array_equal(got, sc.zero_table(m).astype(np.uint32)), (name, first, pix)


def test_zero_sat_refuses_bad_arguments(dev):
    torch, d, L, _ = dev
    buf = torch.zeros(64, dtype=torch.uint8, device=d)
    out = torch.zeros(256, dtype=torch.int32, device=d)
    assert L.apds_dev_mask_zero_sat(None, 4, 4, 4, 1, out.data_ptr(), None) != 0
    assert L.apds_dev_mask_zero_sat(buf.data_ptr(), 4, 4, 3, 1, out.data_ptr(), None) != 0       # row stride below a row
    assert L.apds_dev_mask_zero_sat(buf.data_ptr(), 0, 4, 4, 1, out.data_ptr(), None) != 0
    assert L.apds_dev_mask_zero_sat(buf.data_ptr(), 4, 4, 4, 0, out.data_ptr(), None) != 0


# ---- extraction ---------------------------------------------------------------------------------------------------------------------------
def _down(gpu_pkg, kps, desc, n):
    k = kps[:n].cpu().numpy().copy().view(gpu_pkg._lib.KEYPOINT_DTYPE).ravel()
    return mc.Extraction(k, desc[:n, :61].cpu().numpy().copy())


def _dev_single(gpu_pkg, dev, tile, mask, support, max_points=4096, capacity=4096):
    """apds_dev_akaze_extract_masked_support"""
    torch, d, L, check = dev
    t = torch.from_numpy(np.array(tile)).to(d)
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).to(d)
    kps = torch.zeros((capacity, 7), dtype=torch.float32, device=d)
    desc = torch.zeros((capacity, 64), dtype=torch.uint8, device=d)
    n = C.c_int(-1)
    ch = 1 if tile.ndim == 2 else tile.shape[2]
    hand_over()
    check(L.apds_dev_akaze_extract_masked_support(t.data_ptr(), tile.shape[0], tile.shape[1], ch, tile.shape[1] * ch, None if m is None else m.data_ptr(),
                                                  tile.shape[1], support, max_points, kps.data_ptr(), desc.data_ptr(), capacity, C.byref(n), None))
    torch.cuda.synchronize()
    return _down(gpu_pkg, kps, desc, n.value)


MASKS = {"left_half": mc.left_half, "top_half": mc.top_half, "hole": sc.hole, "single_pixel": lambda: sc.single_pixel(176, 320),
         "checkerboard": mc.checkerboard}


@pytest.mark.parametrize("name", list(MASKS))
def test_masks_equal_the_expectation(gpu_pkg, dev, case, name):
    """every mask at support 0, 1 and 15, through the host and the apds_dev_ entry, with and without a max_points cut among the survivors"""
    _expect_switch()
    tile, ref = case
    fe = gpu_pkg.feature_extraction
    mask = MASKS[name]()
    kept = []
    for support in SUPPORTS:
        want = sc.masked(ref, mask, support)
        kept.append(len(want.keypoints))
        mc.assert_same(fe.akaze_keypoint_descriptor_extraction(tile, mask, None, support), want)
        mc.assert_same(_dev_single(gpu_pkg, dev, tile, mask, support), want)
        if len(want.keypoints) >= 4:
            cut = len(want.keypoints) // 2
            cut_want = sc.masked(ref, mask, support, cut)
            assert len(cut_want.keypoints) == cut
            mc.assert_same(fe.akaze_keypoint_descriptor_extraction(tile, mask, cut, support), cut_want)
            mc.assert_same(_dev_single(gpu_pkg, dev, tile, mask, support, max_points=cut, capacity=cut), cut_want)
    print(name, "kept at support 0 / 1 / 15:", kept)
    assert kept[0] >= kept[1] >= kept[2] and kept[0] > kept[2]


def test_octave_3_tile(gpu_pkg, dev, case3):
    _expect_switch()
    tile, ref = case3
    fe = gpu_pkg.feature_extraction
    assert int(sc.radii(ref.keypoints, 15).max()) == 240
    for pos, n_kept, octave_removed in ((sc.PIXEL_CORNER, 461, [1]), (sc.PIXEL_OCT3_EDGE, 461, [3]), (sc.PIXEL_OCT3_PAST, 462, [])):
        mask = sc.single_pixel(*pos, mc.H3, mc.W3)
        keep = sc.survivors(ref.keypoints, mask, 15)
        assert int(keep.sum()) == n_kept and ref.keypoints["octave"][~keep].tolist() == octave_removed
        want = sc.masked(ref, mask, 15)
        mc.assert_same(fe.akaze_keypoint_descriptor_extraction(tile, mask, None, 15), want)
        mc.assert_same(_dev_single(gpu_pkg, dev, tile, mask, 15), want)
    cb = mc.checkerboard(mc.H3, mc.W3)
    assert len(fe.akaze_keypoint_descriptor_extraction(tile, cb, None, 1).keypoints) == 0
    mc.assert_same(fe.akaze_keypoint_descriptor_extraction(tile, cb, None, 0), mc.masked(ref, cb))


def test_both_compaction_forms(gpu_pkg):
    """APDS_KP_RANKED=0 (subpixel_filter_kernel + two passes over the masks) is read once per process: the extraction cases again in a
    child process."""
    env = dict(os.environ, APDS_KP_RANKED="0", APDS_TEST_EXPECT_KP_RANKED="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_akaze_mask_support_gpu.py"), "-k",
                        "test_masks_equal_the_expectation or test_octave_3_tile", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1000:])
    assert "6 passed" in r.stdout and "failed" not in r.stdout


def test_support_0_and_a_null_mask(gpu_pkg, dev, case):
    tile, ref = case
    fe = gpu_pkg.feature_extraction
    L, ptr, take = gpu_pkg.lib(), gpu_pkg._lib.ptr, gpu_pkg._lib.take
    hole = sc.hole()

    def host_c(mask, support):
        kps, desc, n, nb = C.c_void_p(), C.c_void_p(), C.c_int(0), C.c_int(0)
        gpu_pkg._lib.check(L.apds_akaze_extract_masked_support(ptr(tile), H, W, 4, tile.strides[0], None if mask is None else ptr(mask), W, support, 0,
                                                               C.byref(kps), C.byref(desc), C.byref(n), C.byref(nb)))
        k = take(kps, n.value, gpu_pkg._lib.KEYPOINT_DTYPE)
        return mc.Extraction(k, take(desc, n.value * nb.value, np.uint8).reshape(n.value, nb.value))

    pixel_rule = fe.akaze_keypoint_descriptor_extraction(tile, hole, None)           # apds_akaze_extract_masked
    mc.assert_same(host_c(hole, 0), pixel_rule)
    mc.assert_same(_dev_single(gpu_pkg, dev, tile, hole, 0), pixel_rule)
    mc.assert_same(pixel_rule, mc.masked(ref, hole))
    # a NULL mask with a support is the unmasked call
    plain = fe.akaze_keypoint_descriptor_extraction_def(tile, None)
    mc.assert_same(host_c(None, 15), plain)
    mc.assert_same(_dev_single(gpu_pkg, dev, tile, None, 15), plain)
    mc.assert_same(fe.akaze_keypoint_descriptor_extraction(tile, None, None, 15), plain)
    # a support past any image side: one zero byte anywhere removes everything, an all-255 mask nothing
    assert len(fe.akaze_keypoint_descriptor_extraction(tile, sc.single_pixel(H - 1, W - 1), None, 2 ** 31 - 1).keypoints) == 0
    mc.assert_same(fe.akaze_keypoint_descriptor_extraction(tile, np.full((H, W), 255, np.uint8), None, 2 ** 31 - 1), plain)


def test_batches(gpu_pkg, dev, case):
    tile, ref = case
    fe = gpu_pkg.feature_extraction
    imgs = np.stack([tile, tile, tile])
    hole, left, cb = sc.hole(), mc.left_half(), mc.checkerboard()
    for support in (1, 15):
        # host: one image unmasked, two with masks of their own
        got = fe.akaze_keypoint_descriptor_extraction_batch(imgs, None, mask=[None, hole, left], mask_support=support)
        mc.assert_same(got[0], ref)
        mc.assert_same(got[1], sc.masked(ref, hole, support))
        mc.assert_same(got[2], sc.masked(ref, left, support))
    torch, d, L, check = dev
    t = torch.from_numpy(imgs).to(d)
    cap = 512
    kps = torch.zeros((3, cap, 7), dtype=torch.float32, device=d)
    desc = torch.zeros((3, cap, 64), dtype=torch.uint8, device=d)
    counts = (C.c_int * 3)()
    # device: one mask shared by all images (image stride 0: one table)
    tm = torch.from_numpy(hole).to(d)
    hand_over()
    check(L.apds_dev_akaze_extract_batch_masked_support(t.data_ptr(), 3, H * W * 4, H, W, 4, W * 4, tm.data_ptr(), W, 0, 15, cap, kps.data_ptr(), desc.data_ptr(),
                                                        cap, counts, None))
    torch.cuda.synchronize()
    want = sc.masked(ref, hole, 15)
    for i in range(3):
        assert counts[i] == len(want.keypoints) == 147
        mc.assert_same(_down(gpu_pkg, kps[i], desc[i], counts[i]), want)
    # device: a mask per image (a table per image), the first all ones
    stack = np.stack([np.ones((H, W), np.uint8), left, cb])
    ts = torch.from_numpy(stack).to(d)
    for support in (0, 15):
        check(L.apds_dev_akaze_extract_batch_masked_support(t.data_ptr(), 3, H * W * 4, H, W, 4, W * 4, ts.data_ptr(), W, H * W, support, cap, kps.data_ptr(),
                                                            desc.data_ptr(), cap, counts, None))
        torch.cuda.synchronize()
        for i in range(3):
            mc.assert_same(_down(gpu_pkg, kps[i], desc[i], counts[i]), sc.masked(ref, stack[i], support))
    # the cut in a batch: per image, after its own mask
    cut = 40
    got = fe.akaze_keypoint_descriptor_extraction_batch(imgs, cut, mask=[None, hole, left], mask_support=15)
    for g, m in zip(got, (np.ones((H, W), np.uint8), hole, left)):
        mc.assert_same(g, sc.masked(ref, m, 15, cut))


# ---- a tile's alpha as the mask, with the descriptor support --------------------------------------------------------------------------
ALL_NAN = (slice(100, 180), slice(200, 330))      # NaN in all three bands: alpha 0


def _bands(pkg, h, w, frame):
    t = pkg.synth.make_tile(h, w, frame_index=frame, channels=3).astype(np.float32)
    return np.stack([t[:, :, 2] * 3.0 + 10.0, t[:, :, 1] * 2.0 - 5.0, t[:, :, 0] * 1.5])


def _min_max(pkg, bands):
    return pkg.geotiff_extractor.BandsMinMax(*[f(bands[b]) for b in range(3) for f in (np.nanmin, np.nanmax)])


def _bgra(pkg, win, mm):
    out = pkg.geotiff_extractor.band_merger([win[0], win[1], win[2]], mm, bgra=True)
    return out.reshape(win.shape[1], win.shape[2], 4)


def test_alpha_support_through_the_four_ex_calls(gpu_pkg):
    fe = gpu_pkg.feature_extraction
    bands = _bands(gpu_pkg, H, W, mc.FRAME)
    bands[(slice(None),) + ALL_NAN] = np.nan
    mm = _min_max(gpu_pkg, bands)
    bgra = _bgra(gpu_pkg, bands, mm)
    alpha = bgra[..., 3]
    assert (alpha == 0).sum() == 80 * 130
    none = fe.tile_keypoint_descriptor_extraction(bands[0], bands[1], bands[2], mm, None)
    pixel = fe.tile_keypoint_descriptor_extraction(bands[0], bands[1], bands[2], mm, None, mask_nodata=True)
    want = fe.akaze_keypoint_descriptor_extraction(bgra, alpha, None, sc.SUPPORT_DESCRIPTOR)
    mc.assert_same(want, sc.masked(none, alpha, sc.SUPPORT_DESCRIPTOR))
    assert 0 < len(want.keypoints) < len(pixel.keypoints) < len(none.keypoints)
    # apds_tile_extract_ex, apds_tile_extract_batch_ex
    mc.assert_same(fe.tile_keypoint_descriptor_extraction(bands[0], bands[1], bands[2], mm, None, mask_nodata="support"), want)
    clean = _bands(gpu_pkg, H, W, mc.FRAME + 1)
    both = fe.tiles_keypoint_descriptor_extraction([clean, bands], mm, None, mask_nodata="support")
    mc.assert_same(both[1], want)
    mc.assert_same(both[0], fe.tile_keypoint_descriptor_extraction(clean[0], clean[1], clean[2], mm, None))
    # apds_mosaic_tile_extract_ex, apds_mosaic_tile_extract_batch_ex: the tile is the left half of a two-tile mosaic
    dm = gpu_pkg.geotiff_extractor.DeviceMosaic(np.concatenate([bands, clean], axis=2))
    try:
        mc.assert_same(fe.mosaic_tile_keypoint_descriptor_extraction(dm, (0, 0), (W, H), (W, H), "nearest", mm, None, mask_nodata="support"), want)
        pair = fe.mosaic_tiles_keypoint_descriptor_extraction(dm, [(W, 0), (0, 0)], (W, H), (W, H), "nearest", mm, None, mask_nodata="support")
        mc.assert_same(pair[1], want)
        mc.assert_same(pair[0], both[0])
    finally:
        dm.close()
    # mode 2 (a support without a mask) names nothing
    L, ptr = gpu_pkg.lib(), gpu_pkg._lib.ptr
    kps, desc, n, nb = C.c_void_p(), C.c_void_p(), C.c_int(0), C.c_int(0)
    mma = mm.as_array()
    rc = L.apds_tile_extract_ex(bands[0].ctypes.data, bands[1].ctypes.data, bands[2].ctypes.data, H, W, W, ptr(mma), 0, 2, C.byref(kps), C.byref(desc),
                                C.byref(n), C.byref(nb))
    assert rc == gpu_pkg._lib.ERR_BAD_ARG


# ---- the DB build ---------------------------------------------------------------------------------------------------------------------------
MOSAIC_NAN = (slice(0, 120), slice(0, 200))      # a nodata corner of the mosaic: in the upper left tile, and in the lod-1 tile at half size


def test_process_lod_from_mosaic_with_support(gpu_pkg):
    fe, pp, fd = gpu_pkg.feature_extraction, gpu_pkg.preprocessor, gpu_pkg.feature_database
    bands = _bands(gpu_pkg, 2 * H, 2 * W, mc.FRAME + 2)
    bands[(slice(None),) + MOSAIC_NAN] = np.nan
    dm = gpu_pkg.geotiff_extractor.DeviceMosaic(bands)
    try:
        mm = dm.datasets_min_max()
        cells = [(0, (0, 0)), (0, (W, 0)), (0, (0, H)), (0, (W, H)), (1, (0, 0))]                    # row-major tile order, level by level
        wants, masked_tiles = [], 0
        for lod, (x0, y0) in cells:
            span = (W * 2 ** lod, H * 2 ** lod)
            plain = fe.mosaic_tile_keypoint_descriptor_extraction(dm, (x0, y0), span, (W, H), "nearest")
            alpha = _bgra(gpu_pkg, dm.window((x0, y0), span, (W, H)), mm)[..., 3]
            want = sc.masked(plain, alpha, sc.SUPPORT_DESCRIPTOR)
            masked_tiles += len(want.keypoints) < len(mc.masked(plain, alpha).keypoints)
            order = np.lexsort((np.arange(len(want.keypoints)), -want.keypoints["response"].astype(np.float64)))
            k = want.keypoints[order].copy()
            k["x"] = k["x"] * np.float32(2.0 ** lod) + np.float32(x0)
            k["y"] = k["y"] * np.float32(2.0 ** lod) + np.float32(y0)
            wants.append((k, want.descriptors[order]))
        assert masked_tiles == 2                                        # the upper left tile and the lod-1 tile

        def build(mask_nodata, **form):
            table, images = fd.KeypointTable(20000), pp.ImageTable()
            out = pp.process_lod_from_mosaic(table, images, dm, 2, mask_nodata=mask_nodata, **form)
            assert [len(level) for level in out] == [4, 1]
            rows = [table.read_keypoints_from_image_id(r["id"]) for r in images.rows]
            stored = [(r.keypoints.copy(), r.descriptors.copy()) for r in rows]
            table.close()
            return stored

        for form in (dict(batch=4), dict(batch=1), dict(workers=2)):     # batch, single, workers
            stored = build("support", **form)
            for (k, d), (wk, wd) in zip(stored, wants):
                assert len(k) == len(wk) > 20
                assert np.array_equal(k, wk) and np.array_equal(d, wd)
        pixel = build(True, batch=4)
        assert sum(len(k) for k, _ in stored) < sum(len(k) for k, _ in pixel)
        assert all(len(a[0]) <= len(b[0]) for a, b in zip(stored, pixel))
    finally:
        dm.close()
