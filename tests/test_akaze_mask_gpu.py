"""GPU: the AKAZE detection mask (apds_*_masked, the *_ex tile calls, mask= / mask_nodata= in the Python fronts).

Expected results come from the UNMASKED oracle through the numpy helper of akaze_mask_cases.py (the rule restated there); comparisons
are bit-exact on the seven keypoint fields and the descriptors.

Shapes. 352 x 640 is the smallest image with four octaves. At that size octave 3 (80 x 44) cannot hold a keypoint: its border is
lrint(10 sqrt(2) * sigma_size) + 1 >= 29 pixels on every side (sigma_size >= 2 there), more than half its height. So the 352 x 640 cases
assert survivors and removals in octaves 0, 1 and 2 (ratios 1, 2, 4) and that octave 3 is empty, and one more image, 544 x 672 with six
wide blobs added (octave 3: 84 x 68), carries ratio 8: the checkerboard and its complement, one of which keeps and the other removes
each octave-3 keypoint."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import akaze_mask_cases as mc
from stream_handover import hand_over

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = mc.H, mc.W


@pytest.fixture(scope="module")
def case(gpu_pkg, oracle_mod):
    """the tile, its unmasked oracle result and the unmasked library result, computed once and never modified"""
    tile = gpu_pkg.synth.make_tile(H, W, frame_index=mc.FRAME, channels=4)
    oracle_mod.set_threads(8)
    ref = oracle_mod.akaze(tile)
    plain = gpu_pkg.feature_extraction.akaze_keypoint_descriptor_extraction_def(tile, None)
    mc.assert_same(plain, ref)
    k = ref.keypoints
    assert len(k) > 100 and len(np.unique(k["response"])) == len(k)        # distinct responses: every cut is unambiguous
    assert (k["octave"] == 3).sum() == 0 and set(k["octave"].tolist()) == {0, 1, 2}
    for f in (tile, k, ref.descriptors):
        f.setflags(write=False)
    return tile, ref, plain


@pytest.fixture(scope="module")
def dev(gpu_pkg):
    import torch
    return torch, torch.device("cuda:0"), gpu_pkg._lib.lib(), gpu_pkg._lib.check


def _down(gpu_pkg, kps, desc, n):
    k = kps[:n].cpu().numpy().copy().view(gpu_pkg._lib.KEYPOINT_DTYPE).ravel()
    return mc.Extraction(k, desc[:n, :61].cpu().numpy().copy())


def _dev_single(gpu_pkg, dev, tile, mask=None, max_points=4096, capacity=4096):
    """apds_dev_akaze_extract_masked; mask: None or a 2-D uint8 array whose row stride is taken as it is"""
    torch, d, L, check = dev
    t = torch.from_numpy(np.array(tile)).to(d)
    mstride, mptr, keepalive = 0, None, None
    if mask is not None:
        mstride = mask.strides[0]
        flat = np.lib.stride_tricks.as_strided(mask, shape=((mask.shape[0] - 1) * mstride + mask.shape[1],), strides=(1,))
        keepalive = torch.from_numpy(np.ascontiguousarray(flat)).to(d)
        mptr = keepalive.data_ptr()
    kps = torch.zeros((capacity, 7), dtype=torch.float32, device=d)
    desc = torch.zeros((capacity, 64), dtype=torch.uint8, device=d)
    n = C.c_int(-1)
    ch = 1 if tile.ndim == 2 else tile.shape[2]
    hand_over()
    rc = L.apds_dev_akaze_extract_masked(t.data_ptr(), tile.shape[0], tile.shape[1], ch, tile.shape[1] * ch, mptr, mstride, max_points, kps.data_ptr(),
                                         desc.data_ptr(), capacity, C.byref(n), None)
    torch.cuda.synchronize()
    if rc != 0:
        return rc, None
    return 0, _down(gpu_pkg, kps, desc, n.value)


# ---- 1, 2: masks that change nothing, a mask that removes everything --------------------------------------------------------------------
def test_null_and_all_255_masks_equal_the_unmasked_call(gpu_pkg, dev, case):
    tile, ref, plain = case
    fe = gpu_pkg.feature_extraction
    ones = np.full((H, W), 255, np.uint8)
    for got in (fe.akaze_keypoint_descriptor_extraction(tile, None, None), fe.akaze_keypoint_descriptor_extraction(tile, ones, None)):
        assert np.array_equal(got.keypoints, plain.keypoints) and np.array_equal(got.descriptors, plain.descriptors)
    # the C entry itself with a NULL mask
    kps, desc, n, nb = C.c_void_p(), C.c_void_p(), C.c_int(0), C.c_int(0)
    gpu_pkg._lib.check(gpu_pkg.lib().apds_akaze_extract_masked(gpu_pkg._lib.ptr(tile), H, W, 4, tile.strides[0], None, 0, 0, C.byref(kps), C.byref(desc),
                                                               C.byref(n), C.byref(nb)))
    k = gpu_pkg._lib.take(kps, n.value, gpu_pkg._lib.KEYPOINT_DTYPE)
    dd = gpu_pkg._lib.take(desc, n.value * nb.value, np.uint8).reshape(n.value, nb.value)
    assert np.array_equal(k, plain.keypoints) and np.array_equal(dd, plain.descriptors)
    for m in (None, ones):
        rc, got = _dev_single(gpu_pkg, dev, tile, m)
        assert rc == 0
        mc.assert_same(got, plain)


def test_all_zero_mask_removes_everything(gpu_pkg, dev, case):
    tile, _, _ = case
    zeros = np.zeros((H, W), np.uint8)
    got = gpu_pkg.feature_extraction.akaze_keypoint_descriptor_extraction(tile, zeros, None)       # status OK: no exception
    assert len(got.keypoints) == 0 and got.descriptors.shape == (0, 61)
    rc, got = _dev_single(gpu_pkg, dev, tile, zeros)
    assert rc == 0 and len(got.keypoints) == 0


# ---- 3: the pixel checkerboard -----------------------------------------------------------------------------------------------------------
def _per_octave(k, keep):
    return [(int((keep & (k["octave"] == o)).sum()), int((~keep & (k["octave"] == o)).sum())) for o in range(4)]


def test_checkerboard_equals_helper(gpu_pkg, dev, case):
    if os.environ.get("APDS_TEST_EXPECT_KP_RANKED") is not None:
        assert os.environ.get("APDS_KP_RANKED") == os.environ["APDS_TEST_EXPECT_KP_RANKED"], "the child process lost its switch"
    tile, ref, _ = case
    cb = mc.checkerboard()
    per = _per_octave(ref.keypoints, mc.survivors(ref.keypoints, cb))
    print("352 x 640 checkerboard (survivors, removed) per octave:", per)
    assert all(min(p) >= 1 for p in per[:3]) and per[3] == (0, 0), per        # octave 3: see the module docstring
    want = mc.masked(ref, cb)
    mc.assert_same(gpu_pkg.feature_extraction.akaze_keypoint_descriptor_extraction(tile, cb, None), want)
    rc, got = _dev_single(gpu_pkg, dev, tile, cb)
    assert rc == 0
    mc.assert_same(got, want)


def test_checkerboard_reaches_octave_3(gpu_pkg, oracle_mod):
    if os.environ.get("APDS_TEST_EXPECT_KP_RANKED") is not None:
        assert os.environ.get("APDS_KP_RANKED") == os.environ["APDS_TEST_EXPECT_KP_RANKED"], "the child process lost its switch"
    tile = mc.octave3_tile(gpu_pkg)
    ref = oracle_mod.akaze(tile)
    k = ref.keypoints
    cb = mc.checkerboard(*tile.shape)
    inv = (1 - cb).astype(np.uint8)
    per = _per_octave(k, mc.survivors(k, cb))
    print("544 x 672 checkerboard (survivors, removed) per octave:", per)
    assert sum(per[3]) >= 1 and all(min(p) >= 1 for p in per[:3]), per
    for m in (cb, inv):      # an octave-3 keypoint survives one of the two and is removed by the other
        mc.assert_same(gpu_pkg.feature_extraction.akaze_keypoint_descriptor_extraction(tile, m, None), mc.masked(ref, m))
    assert mc.survivors(k, cb).sum() + mc.survivors(k, inv).sum() == len(k)


# ---- 4: axes ---------------------------------------------------------------------------------------------------------------------------------
def test_axis_guard(gpu_pkg, case):
    tile, ref, _ = case
    fe = gpu_pkg.feature_extraction
    left, top = mc.left_half(), mc.top_half()
    got_l, got_t = fe.akaze_keypoint_descriptor_extraction(tile, left, None), fe.akaze_keypoint_descriptor_extraction(tile, top, None)
    mc.assert_same(got_l, mc.masked(ref, left))
    mc.assert_same(got_t, mc.masked(ref, top))
    assert (got_l.keypoints["x"] < W // 2).all() and (got_t.keypoints["y"] < H // 2).all()
    assert (got_l.keypoints["y"] >= H // 2).any() and (got_t.keypoints["x"] >= W // 2).any()
    assert len(got_l.keypoints) != len(got_t.keypoints) or not np.array_equal(got_l.keypoints, got_t.keypoints)


# ---- 5: strides ------------------------------------------------------------------------------------------------------------------------------
def test_strided_mask(gpu_pkg, dev, case):
    tile, ref, _ = case
    cb = mc.checkerboard()
    wide = np.zeros((H, W + 37), np.uint8)
    wide[:, W:] = (1 - cb[:, :37])          # the padding holds the OPPOSITE pattern: reading it shows
    wide[:, :W] = cb
    view = wide[:, :W]
    assert view.strides[0] == W + 37 and not view.flags["C_CONTIGUOUS"]
    want = mc.masked(ref, cb)
    mc.assert_same(gpu_pkg.feature_extraction.akaze_keypoint_descriptor_extraction(tile, view, None), want)
    rc, got = _dev_single(gpu_pkg, dev, tile, view)
    assert rc == 0
    mc.assert_same(got, want)
    # mask_stride < cols: OpenCV's size assertion
    L, ptr = gpu_pkg.lib(), gpu_pkg._lib.ptr
    kps, desc, n, nb = C.c_void_p(), C.c_void_p(), C.c_int(0), C.c_int(0)
    rc = L.apds_akaze_extract_masked(ptr(tile), H, W, 4, tile.strides[0], ptr(cb), W - 1, 0, C.byref(kps), C.byref(desc), C.byref(n), C.byref(nb))
    assert rc == gpu_pkg._lib.ERR_ASSERT and n.value == 0
    torch, d, _, _ = dev
    m = torch.from_numpy(cb).to(d)
    t = torch.from_numpy(np.array(tile)).to(d)
    out_k = torch.zeros((64, 7), dtype=torch.float32, device=d)
    out_d = torch.zeros((64, 64), dtype=torch.uint8, device=d)
    hand_over()
    rc = L.apds_dev_akaze_extract_masked(t.data_ptr(), H, W, 4, W * 4, m.data_ptr(), W - 1, 64, out_k.data_ptr(), out_d.data_ptr(), 64, C.byref(n), None)
    assert rc == gpu_pkg._lib.ERR_ASSERT


# ---- 6: max_points comes after the mask --------------------------------------------------------------------------------------------------
def test_max_points_cut_follows_the_mask(gpu_pkg, oracle_mod, case):
    if os.environ.get("APDS_TEST_EXPECT_KP_RANKED") is not None:
        assert os.environ.get("APDS_KP_RANKED") == os.environ["APDS_TEST_EXPECT_KP_RANKED"], "the child process lost its switch"
    tile, ref, _ = case
    fe = gpu_pkg.feature_extraction
    left = mc.left_half()
    k0, s = len(ref.keypoints), int(mc.survivors(ref.keypoints, left).sum())
    assert 20 < s < k0 - 20
    # S <= m < K0: every survivor, in detection order (a cut in front of the mask would return the strongest m of K0, masked)
    for m in (s, (s + k0) // 2, k0 - 1):
        mc.assert_same(fe.akaze_keypoint_descriptor_extraction(tile, left, m), mc.masked(ref, left))
    early = mc.masked(mc.masked(ref, np.ones((H, W), np.uint8), s), left)
    assert len(early.keypoints) < s          # what the wrong order would give is something else
    # m < S: the strongest m of the survivors
    for m in (1, s // 3, s - 1):
        want = mc.masked(ref, left, m)
        assert len(want.keypoints) == m
        mc.assert_same(fe.akaze_keypoint_descriptor_extraction(tile, left, m), want)
    # the order rule of the helper is the oracle's: all-ones mask against the oracle's own cut, responses around the cut distinct
    m = s // 3
    byresp = np.sort(ref.keypoints["response"])[::-1]
    assert byresp[m - 2] > byresp[m - 1] > byresp[m] > byresp[m + 1]
    mc.assert_same(mc.masked(ref, np.ones((H, W), np.uint8), m), oracle_mod.akaze(tile, max_points=m))


# ---- 7: the mask-scan compaction path --------------------------------------------------------------------------------------------------
def test_both_compaction_paths(gpu_pkg):
    """APDS_KP_RANKED=0 (subpixel_filter_kernel + two passes over the masks) is read once per process: the checkerboard and max_points
    cases again in a child process."""
    env = dict(os.environ, APDS_KP_RANKED="0", APDS_TEST_EXPECT_KP_RANKED="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_akaze_mask_gpu.py"), "-k",
                        "test_checkerboard_equals_helper or test_checkerboard_reaches_octave_3 or test_max_points_cut_follows_the_mask", "-q", "-m", "gpu",
                        "-x", "-p", "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1000:])
    assert "3 passed" in r.stdout and "failed" not in r.stdout


# ---- 8: batches ------------------------------------------------------------------------------------------------------------------------------
def test_batch_masks(gpu_pkg, dev, case):
    tile, ref, plain = case
    fe = gpu_pkg.feature_extraction
    imgs = np.stack([tile, gpu_pkg.synth.make_tile(H, W, frame_index=mc.FRAME + 1, channels=4), tile[::-1].copy()])
    cb, zeros = mc.checkerboard(), np.zeros((H, W), np.uint8)
    masks = [cb, None, zeros]
    got = fe.akaze_keypoint_descriptor_extraction_batch(imgs, None, mask=masks)
    singles = [fe.akaze_keypoint_descriptor_extraction(imgs[i], masks[i], None) for i in range(3)]
    for g, one in zip(got, singles):
        mc.assert_same(g, one)
    mc.assert_same(got[0], mc.masked(ref, cb))
    assert len(got[1].keypoints) > 100 and len(got[2].keypoints) == 0
    # device batch, one mask shared by all images (image stride 0)
    torch, d, L, check = dev
    t = torch.from_numpy(imgs).to(d)
    left = mc.left_half()
    tm = torch.from_numpy(left).to(d)
    cap = 1024
    kps = torch.zeros((3, cap, 7), dtype=torch.float32, device=d)
    desc = torch.zeros((3, cap, 64), dtype=torch.uint8, device=d)
    counts = (C.c_int * 3)()
    hand_over()
    check(L.apds_dev_akaze_extract_batch_masked(t.data_ptr(), 3, H * W * 4, H, W, 4, W * 4, tm.data_ptr(), W, 0, cap, kps.data_ptr(), desc.data_ptr(), cap, counts,
                                                None))
    torch.cuda.synchronize()
    for i in range(3):
        one = fe.akaze_keypoint_descriptor_extraction(imgs[i], left, None)
        assert counts[i] == len(one.keypoints) > 20
        mc.assert_same(_down(gpu_pkg, kps[i], desc[i], counts[i]), one)
    # per-image masks on the device
    stack = np.stack([cb, np.ones((H, W), np.uint8), zeros])
    ts = torch.from_numpy(stack).to(d)
    check(L.apds_dev_akaze_extract_batch_masked(t.data_ptr(), 3, H * W * 4, H, W, 4, W * 4, ts.data_ptr(), W, H * W, cap, kps.data_ptr(), desc.data_ptr(), cap,
                                                counts, None))
    torch.cuda.synchronize()
    for i in range(3):
        mc.assert_same(_down(gpu_pkg, kps[i], desc[i], counts[i]), singles[i])
    # a capacity below the unmasked count, at or above the masked one
    s, k0 = int(mc.survivors(ref.keypoints, left).sum()), len(ref.keypoints)
    assert s + 3 < k0
    rc, got1 = _dev_single(gpu_pkg, dev, tile, left, max_points=s + 3, capacity=s + 3)
    assert rc == 0
    mc.assert_same(got1, mc.masked(ref, left))
    rc, _ = _dev_single(gpu_pkg, dev, tile, None, max_points=k0 + 100, capacity=s + 3)       # unmasked, the same capacity is too small
    assert rc == gpu_pkg._lib.ERR_ASSERT


# ---- 9: a tile's alpha as the mask -----------------------------------------------------------------------------------------------------
ALL_NAN = (slice(100, 180), slice(200, 330))      # NaN in all three bands: alpha 0
ONE_NAN = (slice(220, 300), slice(400, 520))      # NaN in the red band only: alpha stays 255


def _bands(pkg, h, w, frame):
    t = pkg.synth.make_tile(h, w, frame_index=frame, channels=3).astype(np.float32)
    return np.stack([t[:, :, 2] * 3.0 + 10.0, t[:, :, 1] * 2.0 - 5.0, t[:, :, 0] * 1.5])


def _min_max(pkg, bands):
    return pkg.geotiff_extractor.BandsMinMax(*[f(bands[b]) for b in range(3) for f in (np.nanmin, np.nanmax)])


def _bgra(pkg, win, mm):
    out = pkg.geotiff_extractor.band_merger([win[0], win[1], win[2]], mm, bgra=True)
    return out.reshape(win.shape[1], win.shape[2], 4)


def test_tile_alpha_mask(gpu_pkg):
    fe = gpu_pkg.feature_extraction
    bands = _bands(gpu_pkg, H, W, mc.FRAME)
    bands[(slice(None),) + ALL_NAN] = np.nan
    bands[(0,) + ONE_NAN] = np.nan
    mm = _min_max(gpu_pkg, bands)
    bgra = _bgra(gpu_pkg, bands, mm)
    alpha = bgra[..., 3]
    hole = np.zeros((H, W), bool)
    hole[ALL_NAN] = True
    assert np.array_equal(alpha == 0, hole) and (alpha[~hole] == 255).all()
    none = fe.tile_keypoint_descriptor_extraction(bands[0], bands[1], bands[2], mm, None)
    mc.assert_same(none, fe.akaze_keypoint_descriptor_extraction_def(bgra, None))
    got = fe.tile_keypoint_descriptor_extraction(bands[0], bands[1], bands[2], mm, None, mask_nodata=True)
    mc.assert_same(got, fe.akaze_keypoint_descriptor_extraction(bgra, alpha, None))
    mc.assert_same(got, mc.masked(none, alpha))
    assert 0 < len(got.keypoints) < len(none.keypoints)
    assert mc.survivors(got.keypoints, alpha).all()
    ys, xs = mc.rounded(none.keypoints)
    in_one = (ys >= ONE_NAN[0].start) & (ys < ONE_NAN[0].stop) & (xs >= ONE_NAN[1].start) & (xs < ONE_NAN[1].stop)
    assert in_one.sum() >= 1
    gy, gx = mc.rounded(got.keypoints)
    g_one = (gy >= ONE_NAN[0].start) & (gy < ONE_NAN[0].stop) & (gx >= ONE_NAN[1].start) & (gx < ONE_NAN[1].stop)
    assert np.array_equal(got.keypoints[g_one], none.keypoints[in_one])       # the one-band rectangle masks nothing
    # an unknown mask_mode
    L, ptr = gpu_pkg.lib(), gpu_pkg._lib.ptr
    kps, desc, n, nb = C.c_void_p(), C.c_void_p(), C.c_int(0), C.c_int(0)
    mma = mm.as_array()
    for mode in (2, -1):
        rc = L.apds_tile_extract_ex(bands[0].ctypes.data, bands[1].ctypes.data, bands[2].ctypes.data, H, W, W, ptr(mma), 0, mode, C.byref(kps), C.byref(desc),
                                    C.byref(n), C.byref(nb))
        assert rc == gpu_pkg._lib.ERR_BAD_ARG and n.value == 0
    # the batch form: two tiles, the second without nodata
    clean = _bands(gpu_pkg, H, W, mc.FRAME + 1)
    both = fe.tiles_keypoint_descriptor_extraction([bands, clean], mm, None, mask_nodata=True)
    mc.assert_same(both[0], got)
    mc.assert_same(both[1], fe.tile_keypoint_descriptor_extraction(clean[0], clean[1], clean[2], mm, None))


# ---- 10, 11: the device mosaic and the DB build ---------------------------------------------------------------------------------------
MOSAIC_NAN = (slice(100, 180), slice(560, 700))      # spans the two upper tiles of the 2 x 2 grid


@pytest.fixture(scope="module")
def mosaic(gpu_pkg):
    bands = _bands(gpu_pkg, 2 * H, 2 * W, mc.FRAME + 2)
    bands[(slice(None),) + MOSAIC_NAN] = np.nan
    bands.setflags(write=False)
    dm = gpu_pkg.geotiff_extractor.DeviceMosaic(bands)
    yield bands, dm
    dm.close()


ORIGINS = [(0, 0), (W, 0), (0, H), (W, H)]


def test_mosaic_tiles_masked_by_their_nodata(gpu_pkg, mosaic):
    fe = gpu_pkg.feature_extraction
    bands, dm = mosaic
    mm = dm.datasets_min_max()
    batch = fe.mosaic_tiles_keypoint_descriptor_extraction(dm, ORIGINS, (W, H), (W, H), "nearest", mask_nodata=True)
    plain = fe.mosaic_tiles_keypoint_descriptor_extraction(dm, ORIGINS, (W, H), (W, H), "nearest")
    lost = []
    for i, org in enumerate(ORIGINS):
        mc.assert_same(batch[i], fe.mosaic_tile_keypoint_descriptor_extraction(dm, org, (W, H), (W, H), "nearest", mask_nodata=True))
        win = dm.window(org, (W, H), (W, H))
        mc.assert_same(batch[i], fe.tile_keypoint_descriptor_extraction(win[0], win[1], win[2], mm, None, mask_nodata=True))
        alpha = _bgra(gpu_pkg, win, mm)[..., 3]
        mc.assert_same(batch[i], mc.masked(plain[i], alpha))
        lost.append(len(plain[i].keypoints) - len(batch[i].keypoints))
    print("keypoints lost per tile:", lost)
    assert lost[0] > 0 and lost[1] > 0 and lost[2] == 0 and lost[3] == 0
    # one lod-1 tile under Lanczos: the NaN area widens by the filter footprint, and the mask with it
    got = fe.mosaic_tile_keypoint_descriptor_extraction(dm, (0, 0), (2 * W, 2 * H), (W, H), "lanczos", mask_nodata=True)
    win = dm.window((0, 0), (2 * W, 2 * H), (W, H), "lanczos")
    alpha = _bgra(gpu_pkg, win, mm)[..., 3]
    nh, nw = MOSAIC_NAN[0], MOSAIC_NAN[1]
    assert (alpha == 0).sum() > (nh.stop - nh.start) * (nw.stop - nw.start) // 4 and set(np.unique(alpha).tolist()) == {0, 255}
    assert len(got.keypoints) > 50 and mc.survivors(got.keypoints, alpha).all()
    mc.assert_same(got, mc.masked(fe.mosaic_tile_keypoint_descriptor_extraction(dm, (0, 0), (2 * W, 2 * H), (W, H), "lanczos"), alpha))


def test_preprocessor_mask_nodata(gpu_pkg, mosaic):
    fe, pp, fd = gpu_pkg.feature_extraction, gpu_pkg.preprocessor, gpu_pkg.feature_database
    _, dm = mosaic
    tables = []
    for batch in (4, 1):
        table, images = fd.KeypointTable(20000), pp.ImageTable()
        out = pp.process_lod_from_mosaic(table, images, dm, 2, batch=batch, mask_nodata=True)       # four 352 x 640 tiles, then one lod-1 tile
        assert [len(level) for level in out] == [4, 1]
        rows = [table.read_keypoints_from_image_id(r["id"]) for r in images.rows]
        tables.append((out, images.rows, [(r.keypoints.copy(), r.descriptors.copy()) for r in rows]))
        table.close()
    assert tables[0][0] == tables[1][0] and tables[0][1] == tables[1][1]
    for a, b in zip(tables[0][2], tables[1][2]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    cells = [(0, (0, 0)), (0, (W, 0)), (0, (0, H)), (0, (W, H)), (1, (0, 0))]                    # row-major tile order, level by level
    for (lod, (x0, y0)), row, (k, d) in zip(cells, tables[0][1], tables[0][2]):
        assert (row["level_of_detail"], row["x_start"], row["y_start"]) == (lod, x0, y0)
        span = (W * 2 ** lod, H * 2 ** lod)
        ref = fe.mosaic_tile_keypoint_descriptor_extraction(dm, (x0, y0), span, (W, H), "nearest", mask_nodata=True)
        order = np.lexsort((np.arange(len(ref.keypoints)), -ref.keypoints["response"].astype(np.float64)))
        want = ref.keypoints[order].copy()
        want["x"] = want["x"] * np.float32(2.0 ** lod) + np.float32(x0)
        want["y"] = want["y"] * np.float32(2.0 ** lod) + np.float32(y0)
        assert len(k) == len(want) > 50
        assert np.array_equal(k, want) and np.array_equal(d, ref.descriptors[order])
    unmasked = fe.mosaic_tile_keypoint_descriptor_extraction(dm, (0, 0), (W, H), (W, H), "nearest")
    assert len(tables[0][2][0][0]) < len(unmasked.keypoints)
