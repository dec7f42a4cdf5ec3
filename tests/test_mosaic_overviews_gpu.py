"""GPU: the overview pyramid of the resident mosaic (apds_mosaic_build_overviews, csrc/mosaic.hip's fused cascade kernel), the choice of
level and the window mapping of a read on a handle that has overviews, and the extraction chain and database build on top of them.

Level k is compared with Wy . L(k-1) . Wx^T in float64, where L(k-1) is the level below AS THE DEVICE HOLDS IT (so nothing compounds) and
W are this file's own double tables of the cubic cascade step (restated in `tables`). The bound per pixel is the one
tests/test_mosaic_gpu.py derives for a separable f32 filter whose weights are doubles rounded once,

    |out - ref| <= 2 (n + 2) 2^-24 (|Wy| . |src| . |Wx|^T),        n = row taps + column taps,

which holds for every summation order and fused or unfused products. Where a NaN lies under a tap the output must be NaN, elsewhere the
bound applies. Every case prints its worst error / bound ratio (run with -s); a log of them belongs in profiles/mosaic/."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def cubic(x):
    a = abs(x)
    if a <= 1.0:
        return 1.5 * a * a * a - 2.5 * a * a + 1.0
    if a < 2.0:
        return -0.5 * a * a * a + 2.5 * a * a - 4.0 * a + 2.0
    return 0.0


def tables(n_src, n_out):
    """One axis of one cascade step: dense float64 weight matrix [n_out, n_src], the 0/1 footprint matrix, the largest tap count."""
    ratio = n_src / n_out
    sw = min(1.0, 1.0 / ratio)
    radius = 2.0 / sw
    Wm, F, taps = np.zeros((n_out, n_src)), np.zeros((n_out, n_src)), 0
    for i in range(n_out):
        c = (i + 0.5) * ratio
        a = max(int(math.floor(c - radius + 0.5)), 0)
        b = min(int(c + radius + 0.5), n_src)
        w = np.array([cubic((j + 0.5 - c) * sw) for j in range(a, b)])
        total = 0.0
        for v in w:
            total += v
        Wm[i, a:b] = w / total
        F[i, a:b] = 1.0
        taps = max(taps, b - a)
    return Wm, F, taps


def level_sizes(rows, cols, min_size):
    """[(rows, cols)] of level 1, 2, ...: halved (rounded up) while the level below exceeds min_size on either axis"""
    out = []
    while rows > min_size or cols > min_size:
        rows, cols = (rows + 1) // 2, (cols + 1) // 2
        out.append((rows, cols))
    return out


def check_step(got, below, label):
    """got [3, h, w] = one cascade step of below [3, H, W]; returns the worst error / bound."""
    H, Wd = below.shape[1:]
    h, w = got.shape[1:]
    Wx, Fx, nx = tables(Wd, w)
    Wy, Fy, ny = tables(H, h)
    assert nx <= 9 and ny <= 9
    n = nx + ny
    worst = 0.0
    for b in range(3):
        nan = np.isnan(below[b])
        s = np.where(nan, 0.0, below[b].astype(np.float64))
        ref = Wy @ s @ Wx.T
        mag = np.abs(Wy) @ np.abs(s) @ np.abs(Wx).T
        want_nan = (Fy @ nan.astype(np.float64) @ Fx.T) > 0
        assert np.array_equal(np.isnan(got[b]), want_nan), (label, b, "NaN footprint")
        bound = 2 * (n + 2) * U * mag
        err = np.abs(np.where(want_nan, 0.0, got[b].astype(np.float64)) - np.where(want_nan, 0.0, ref))
        frac = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
        worst = max(worst, frac)
        print(f"overview {label} band {b}: taps {nx}+{ny} worst |err| {err.max():.3e} worst err/bound {frac:.3f}")
        assert (err <= bound).all(), (label, b, float(err.max()), frac)
    return worst


def _uniform(h, w, seed=3):
    return (np.random.default_rng(seed).random((3, h, w)) * 3000.0).astype(np.float32) - 500.0


def _full(dm, k, mode="nearest"):
    size = dm.level_size(k)
    return dm.window_level(k, (0, 0), size, size, mode)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- level sizes and count ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(77, 131), (64, 128), (300, 1), (257, 257)])
def test_level_sizes_and_count(gpu_pkg, rows, cols):
    ge = gpu_pkg.geotiff_extractor
    dm = ge.DeviceMosaic(_uniform(rows, cols))
    assert dm.level_size(0) == (cols, rows)
    want = level_sizes(rows, cols, 8)
    assert dm.build_overviews(8) == len(want) >= 1
    for k, (r, c) in enumerate(want, 1):
        assert dm.level_size(k) == (c, r) == (-(-cols // 2 ** k), -(-rows // 2 ** k))
    assert max(want[-1]) <= 8 < max(([(rows, cols)] + want)[-2])
    assert dm.build_overviews(8) == len(want)                                    # the same argument: the same count, nothing rebuilt
    n = C.c_int(-1)
    assert gpu_pkg.lib().apds_mosaic_build_overviews(dm.handle, 16, C.byref(n)) == -5     # another argument
    assert gpu_pkg.lib().apds_mosaic_build_overviews(dm.handle, 8, None) == 0
    assert dm.raster_size() == (cols, rows)
    dm.close()


def test_default_min_size_is_the_cog_block(gpu_pkg):
    ge = gpu_pkg.geotiff_extractor
    host = ge.MosaicedDataset(_uniform(300, 300))
    dm = host.to_device(overviews=True)
    assert dm.build_overviews() == 0 and dm.build_overviews(512) == 0 and dm.build_overviews(0) == 0
    with pytest.raises(gpu_pkg.ApdsError):
        dm.level_size(1)
    dm.close()
    dm = host.to_device(overviews=True, min_size=100)
    assert dm.build_overviews(100) == 2 and dm.level_size(2) == (75, 75)
    dm.close()


# ---- each level against the one below -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(77, 131), (136, 200)], ids=["131x77 odd", "200x136 several blocks"])
def test_each_level_within_the_derived_bound(gpu_pkg, rows, cols):
    ge = gpu_pkg.geotiff_extractor
    src = _uniform(rows, cols, seed=rows)
    dm = ge.DeviceMosaic(src)
    n = dm.build_overviews(8)
    assert n == len(level_sizes(rows, cols, 8)) >= 4
    below = _full(dm, 0)
    assert np.array_equal(_bits(below), _bits(src))
    for k in range(1, n + 1):
        got = _full(dm, k)
        assert np.array_equal(_bits(got), _bits(_full(dm, k, "lanczos")))       # equal sizes copy under both modes
        check_step(got, below, f"{cols}x{rows} level {k}")
        below = got
    mm = dm.datasets_min_max().as_array()                                        # stays a reduction over level 0
    assert np.array_equal(mm, ge.MosaicedDataset(src).datasets_min_max().as_array())
    dm.close()


# ---- anchors that come from the input ----------------------------------------------------------------------------------------------
def test_constant_checkerboard_ramp_and_nan(gpu_pkg):
    ge = gpu_pkg.geotiff_extractor
    H, W = 128, 256
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    const = np.full((H, W), 1234.5, np.float32)
    checker = ((xx + yy) % 2).astype(np.float32)
    ramp = (0.75 * xx + 3.0).astype(np.float32)                 # exact in f32
    dm = ge.DeviceMosaic(np.stack([const, checker, ramp]))
    n = dm.build_overviews(16)
    assert n == 4
    levels = [_full(dm, k) for k in range(n + 1)]
    # constant: sum w = 1, so every level holds the constant within the step's bound (|W| |src| |W|^T = |src| * sum|wy| * sum|wx|)
    for k in range(1, n + 1):
        h, w = levels[k].shape[1:]
        Wx, _, nx = tables(levels[k - 1].shape[2], w)
        Wy, _, ny = tables(levels[k - 1].shape[1], h)
        mag = np.abs(Wy) @ np.abs(levels[k - 1][0].astype(np.float64)) @ np.abs(Wx).T
        bound = 2 * (nx + ny + 2) * U * mag
        err = np.abs(levels[k][0].astype(np.float64) - 1234.5)
        # level k - 1 itself is off the constant by at most its own bound; the step's weights pass that on multiplied by sum|w| per axis
        carried = np.abs(Wy) @ np.abs(levels[k - 1][0].astype(np.float64) - 1234.5) @ np.abs(Wx).T
        print(f"constant level {k}: worst err/bound", float((err / (bound + carried)).max()))
        assert (err <= bound + carried).all(), k
    # the one-pixel checkerboard: the eight taps of a ratio-2 footprint alternate parity and mirror taps have equal weight, so even
    # and odd pixels carry one half each in x, and the rows are then filtered to the same: 0.5 away from the clamped edges
    l1 = levels[1]
    Wx, _, nx = tables(W, W // 2)
    Wy, _, ny = tables(H, H // 2)
    bound = 2 * (nx + ny + 2) * U * (np.abs(Wy) @ np.abs(checker.astype(np.float64)) @ np.abs(Wx).T)
    inner = (slice(2, H // 2 - 2), slice(2, W // 2 - 2))
    err = np.abs(l1[1].astype(np.float64) - 0.5)
    print("checkerboard: worst err/bound", float((err[inner] / bound[inner]).max()))
    assert (err[inner] <= bound[inner]).all()
    # the ramp: the taps are symmetric about the output's centre (i + 0.5) * 2 - 0.5 (in pixel units) when the ratio is exactly 2
    cx = (np.arange(W // 2) + 0.5) * 2 - 0.5
    want = np.broadcast_to(0.75 * cx + 3.0, (H // 2, W // 2))
    bound = 2 * (nx + ny + 2) * U * (np.abs(Wy) @ np.abs(ramp.astype(np.float64)) @ np.abs(Wx).T)
    err = np.abs(l1[2].astype(np.float64) - want)
    print("ramp: worst err/bound", float((err[inner] / bound[inner]).max()))
    assert (err[inner] <= bound[inner]).all()
    dm.close()
    # one NaN pixel: NaN exactly under its 8 x 8 footprint (the 4 x 4 outputs whose taps 2i-3 .. 2i+4 hold it) and nowhere else
    src = _uniform(H, W, seed=5)
    src[1, 61, 100] = np.nan
    dm = ge.DeviceMosaic(src)
    dm.build_overviews(16)
    l1 = _full(dm, 1)
    want_nan = np.zeros((3, H // 2, W // 2), bool)
    want_nan[1, 29:33, 48:52] = True                            # 2i - 3 <= 61 <= 2i + 4: i in 29 .. 32; 2i - 3 <= 100 <= 2i + 4: i in 48 .. 51
    assert np.array_equal(np.isnan(l1), want_nan)
    check_step(l1, src, "nan level 1")
    dm.close()


# ---- selection and mapping ------------------------------------------------------------------------------------------------------------
def _best(dm, rows, cols, win, out):
    """the rule, written out: the largest k whose factor min(cols / cols_k, rows / rows_k) does not exceed min(win / out) of both axes"""
    desired = min(win[0] / out[0], win[1] / out[1])
    if desired < 2:
        return 0
    best, k = 0, 1
    while True:
        try:
            c, r = dm.level_size(k)
        except Exception:   # noqa: BLE001 (past the last level)
            return best
        if min(cols / c, rows / r) <= desired:
            best = k
        k += 1


@pytest.mark.parametrize("rows,cols", [(256, 512), (263, 517)], ids=["even", "odd"])
def test_best_level(gpu_pkg, rows, cols):
    ge = gpu_pkg.geotiff_extractor
    dm = ge.DeviceMosaic(_uniform(rows, cols))
    reads = [((100, 100), (100, 100)), ((190, 190), (100, 100)), ((200, 200), (100, 100)), ((399, 399), (100, 100)), ((400, 400), (100, 100)),
             ((256, 256), (4, 4)), ((400, 200), (100, 100)), ((200, 255), (50, 17)), ((512, 256), (8, 4))]
    for win, out in reads:
        assert dm.best_level(win, out) == 0                     # no overviews
    n = dm.build_overviews(16)
    got = [dm.best_level(win, out) for win, out in reads]
    assert got == [_best(dm, rows, cols, win, out) for win, out in reads]
    if (rows, cols) == (256, 512):                              # ratios 1, 1.9, 2, 3.99, 4, 64, (4, 2), (4, 15), 64
        assert n == 5 and got == [0, 0, 1, 1, 2, 5, 1, 2, 5]
    else:
        # 517 -> 259 -> 130 -> 65 -> 33 -> 17 -> 9 and 263 -> 132 -> 66 -> 33 -> 17 -> 9 -> 5: factor(1) = 263 / 132 = 1.992 <= 2, and
        # factor(2) = 517 / 130 = 3.977 <= 3.99, so an odd raster's level 2 already serves the ratio 3.99
        assert n == 6 and got == [0, 0, 1, 2, 2, 6, 1, 2, 6]
    level = C.c_int(-1)
    L = gpu_pkg.lib()
    assert L.apds_mosaic_best_level(None, 4, 4, 2, 2, C.byref(level)) == -5
    assert L.apds_mosaic_best_level(dm.handle, 4, 4, 2, 2, None) == -5
    assert L.apds_mosaic_best_level(dm.handle, 4, 0, 2, 2, C.byref(level)) == -215
    dm.close()


def _map(n_base, n_level, x0, win):
    f = n_base / n_level
    ox = min(n_level - 1, int(x0 / f + 0.5))
    ow = max(1, int(win / f + 0.5))
    return ox, min(ow, n_level - ox)


def test_reads_are_served_from_the_mapped_window_of_the_best_level(gpu_pkg):
    ge = gpu_pkg.geotiff_extractor
    rows, cols = 256, 384
    src = _uniform(rows, cols, seed=8)
    plain, dm = ge.DeviceMosaic(src), ge.DeviceMosaic(src)
    assert dm.build_overviews(32) == 4
    t = 32
    for mode in ("nearest", "lanczos"):
        # a power-of-two window at an origin divisible by it: a copy of the overview
        for x0, y0 in ((0, 0), (128, 64), (cols - 4 * t, rows - 4 * t)):
            got = dm.window((x0, y0), (4 * t, 4 * t), (t, t), mode)
            assert np.array_equal(_bits(got), _bits(dm.window_level(2, (x0 // 4, y0 // 4), (t, t), (t, t), mode))), (mode, x0, y0)
            assert np.array_equal(_bits(got), _bits(_full(dm, 2)[:, y0 // 4:y0 // 4 + t, x0 // 4:x0 // 4 + t]))
        # ratio 3: level 1 (factor 2 <= 3 < 4), the window mapped per axis and resampled by the caller's mode
        for (x0, y0), (ww, wh), (ow, oh) in (((37, 21), (96, 96), (32, 32)), ((3, 5), (381, 251), (127, 83)), ((cols - 97, rows - 99), (97, 99), (32, 33))):
            assert dm.best_level((ww, wh), (ow, oh)) == 1
            mx, mw = _map(cols, cols // 2, x0, ww)
            my, mh = _map(rows, rows // 2, y0, wh)
            got = dm.window((x0, y0), (ww, wh), (ow, oh), mode)
            assert np.array_equal(_bits(got), _bits(dm.window_level(1, (mx, my), (mw, mh), (ow, oh), mode))), (mode, x0, y0)
            assert not np.array_equal(_bits(got), _bits(plain.window((x0, y0), (ww, wh), (ow, oh), mode)))
        # below a factor of 2 the base raster serves the read, as on the handle without overviews; which gives the bytes it always gave
        for (x0, y0), (ww, wh), (ow, oh) in (((5, 9), (100, 90), (64, 64)), ((0, 0), (64, 64), (64, 64)), ((10, 10), (32, 32), (64, 64))):
            want = plain.window((x0, y0), (ww, wh), (ow, oh), mode)
            assert np.array_equal(_bits(dm.window((x0, y0), (ww, wh), (ow, oh), mode)), _bits(want))
            assert np.array_equal(_bits(plain.window_level(0, (x0, y0), (ww, wh), (ow, oh), mode)), _bits(want))
            assert np.array_equal(_bits(dm.window_level(0, (x0, y0), (ww, wh), (ow, oh), mode)), _bits(want))
        for (x0, y0), (ww, wh), (ow, oh) in (((37, 21), (96, 96), (32, 32)), ((0, 0), (384, 256), (48, 32))):       # ... at every ratio
            assert np.array_equal(_bits(plain.window_level(0, (x0, y0), (ww, wh), (ow, oh), mode)), _bits(plain.window((x0, y0), (ww, wh), (ow, oh), mode)))
    assert np.array_equal(dm.to_rgb((128, 64), (128, 128), (32, 32), "lanczos"),
                          ge.band_merger([x.ravel() for x in dm.window_level(2, (32, 16), (32, 32), (32, 32))], dm.datasets_min_max()))
    plain.close()
    dm.close()


# ---- extraction and the database build ------------------------------------------------------------------------------------------------
def _same(a, b):
    return len(a.keypoints) == len(b.keypoints) and np.array_equal(a.keypoints, b.keypoints) and np.array_equal(a.descriptors, b.descriptors)


def _mosaic(pkg, size):
    t = pkg.synth.make_tile(size, size, frame_index=11, channels=3).astype(np.float32)
    bands = np.stack([t[:, :, 2] * 3.0 + 10.0, t[:, :, 1] * 2.0 - 5.0, t[:, :, 0] * 1.5])
    bands[0, 5:9, 7:12] = np.nan
    return bands


@pytest.fixture(scope="module")
def mosaic512(gpu_pkg):
    return _mosaic(gpu_pkg, 512)


def test_extract_equals_tile_extract_on_the_window_and_batch_equals_singles(gpu_pkg, mosaic512):
    ge, fe = gpu_pkg.geotiff_extractor, gpu_pkg.feature_extraction
    dm = ge.MosaicedDataset(mosaic512).to_device(overviews=True, min_size=64)
    mm = dm.datasets_min_max()
    origins = [(0, 0), (256, 0), (0, 256), (256, 256), (128, 128), (77, 201)]      # the last one is not a multiple of the factor
    for mode in ("lanczos", "nearest"):
        singles = []
        for o in origins:
            assert dm.best_level((256, 256), (128, 128)) == 1
            win = dm.window(o, (256, 256), (128, 128), mode)
            want = fe.tile_keypoint_descriptor_extraction(win[0], win[1], win[2], mm, None)
            got = fe.mosaic_tile_keypoint_descriptor_extraction(dm, o, (256, 256), (128, 128), mode)
            assert _same(got, want), (mode, o)
            singles.append(got)
        assert sum(len(x.keypoints) for x in singles) > 0                       # (tiles of 128 pixels hold few keypoints each)
        batch = fe.mosaic_tiles_keypoint_descriptor_extraction(dm, origins, (256, 256), (128, 128), mode)
        assert len(batch) == len(origins)
        for o, a, b in zip(origins, batch, singles):
            assert _same(a, b), (mode, o)
    # windows the level's edge shortens beside windows it does not: the batch still equals the singles
    edge = [(0, 0), (512 - 195, 3), (5, 512 - 195), (512 - 195, 512 - 195)]
    assert {_map(512, 256, x, 195)[1] for x, _ in edge} == {98, 97}
    singles = [fe.mosaic_tile_keypoint_descriptor_extraction(dm, o, (195, 195), (65, 65), "lanczos") for o in edge]
    for o, a, b in zip(edge, fe.mosaic_tiles_keypoint_descriptor_extraction(dm, edge, (195, 195), (65, 65), "lanczos"), singles):
        assert _same(a, b), o
    dm.close()


def _levels(table, n):
    out = []
    for lod in range(n):
        k = table.read_keypoints_from_lod(lod)
        out.append((k.keypoints.copy(), k.descriptors.copy(), k.image_ids.copy()))
    return out


def _levels_equal(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) for x, y in zip(a, b))


def test_database_build_reads_the_pyramid(gpu_pkg, mosaic512):
    ge, pp, fe, fd = gpu_pkg.geotiff_extractor, gpu_pkg.preprocessor, gpu_pkg.feature_extraction, gpu_pkg.feature_database
    host = ge.MosaicedDataset(mosaic512)
    plain, dm = host.to_device(), host.to_device(overviews=True, min_size=64)
    assert dm.build_overviews(64) == 3

    def build(ds, batch):
        table, images = fd.KeypointTable(100000), pp.ImageTable()
        out = pp.process_lod_from_mosaic(table, images, ds, 3, batch=batch, resample="lanczos")      # 16 + 4 + 1 tiles of 128
        lv = _levels(table, 3)
        table.close()
        return out, images.rows, lv

    ref = build(plain, 4)
    assert [len(level) for level in ref[0]] == [16, 4, 1]
    # the expectation: every tile of level k cut out of overview k as it is, through the single-tile chain
    table, images = fd.KeypointTable(100000), pp.ImageTable()
    mm = dm.datasets_min_max()
    for lod in range(3):
        tile, columns, rows = pp.tile_grid(dm.raster_size(), 3, lod)
        assert tile == (128, 128)
        for i in range(rows):
            for j in range(columns):
                win = dm.window_level(lod, (j * tile[0], i * tile[1]), tile, tile)
                pp.store_tile(table, images, fe.tile_keypoint_descriptor_extraction(win[0], win[1], win[2], mm, None), tile, j, i, lod)
    want = _levels(table, 3)
    table.close()
    for batch in (1, 4):
        got = build(dm, batch)
        assert got[1] == ref[1] == images.rows                                  # the image table does not depend on the resampling
        assert _levels_equal(got[2], want), batch
        assert _levels_equal(got[2][:1], ref[2][:1])                            # level 0 is the table of the handle without overviews
        assert len(got[2][1][0]) + len(got[2][2][0]) > 0                        # ... and above it the pyramid decides
        assert not _levels_equal(got[2][1:], ref[2][1:])
    plain.close()
    dm.close()


# ---- housekeeping ---------------------------------------------------------------------------------------------------------------------
def test_create_build_destroy_does_not_grow_device_memory(gpu_pkg):
    import torch
    ge = gpu_pkg.geotiff_extractor
    bands = _uniform(1024, 1024)                                                # 12 MiB per handle, 4 MiB of overviews

    def cycle():
        dm = ge.DeviceMosaic(bands)
        assert dm.build_overviews(64) == 4
        dm.window((0, 0), (512, 512), (128, 128), "lanczos")
        dm.close()

    cycle()                                                                     # the thread's workspace reaches its size
    torch.cuda.synchronize()
    assert gpu_pkg.lib().apds_release_cached_memory() == 0
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(10):
        cycle()
    assert gpu_pkg.lib().apds_release_cached_memory() == 0
    free1 = torch.cuda.mem_get_info()[0]
    print("free before / after 10 create-build-destroy cycles:", free0, free1)
    assert free0 - free1 < bands.nbytes // 2, (free0, free1)                    # leaked overviews alone would be 10 x 4 MiB


def test_two_threads_read_different_levels_of_one_handle(gpu_pkg):
    ge = gpu_pkg.geotiff_extractor
    dm = ge.DeviceMosaic(_uniform(384, 512, seed=12))
    assert dm.build_overviews(32) == 4
    reads = [(k, (x, y), (64 >> (k // 2), 48 >> (k // 2)), (32, 24), mode) for k in range(4) for x, y in ((0, 0), (3, 5)) for mode in ("nearest", "lanczos")]
    want = [dm.window_level(*r) for r in reads]
    got, errors = {}, []

    def work(idx):
        try:
            for _ in range(3):
                for i in idx:
                    got[i] = dm.window_level(*reads[i])
        except Exception as e:   # noqa: BLE001
            errors.append(e)
        finally:
            gpu_pkg.lib().apds_thread_release()

    half = len(reads) // 2                                                      # levels 0, 1 in one thread, 2, 3 in the other
    threads = [threading.Thread(target=work, args=(range(k * half, (k + 1) * half),)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, w in enumerate(want):
        assert np.array_equal(_bits(got[i]), _bits(w)), reads[i]
    dm.close()


def test_errors(gpu_pkg):
    ge = gpu_pkg.geotiff_extractor
    dm = ge.DeviceMosaic(_uniform(128, 256))
    E, L = gpu_pkg.ApdsError, gpu_pkg.lib()

    def code(fn):
        with pytest.raises(E) as e:
            fn()
        return e.value.code

    assert code(lambda: dm.window_level(1, (0, 0), (8, 8), (8, 8))) == -211                  # no overviews yet
    assert dm.build_overviews(32) == 3                                                       # 128 x 64, 64 x 32, 32 x 16
    for mode in ("nearest", "lanczos"):
        assert code(lambda: dm.window_level(4, (0, 0), (8, 8), (8, 8), mode)) == -211        # a level out of range
        assert code(lambda: dm.window_level(-1, (0, 0), (8, 8), (8, 8), mode)) == -211
        assert code(lambda: dm.window_level(1, (100, 0), (64, 32), (32, 16), mode)) == -211  # a window outside the level
        assert code(lambda: dm.window_level(2, (0, 0), (64, 33), (32, 16), mode)) == -211
        assert code(lambda: dm.window_level(3, (-1, 0), (8, 8), (8, 8), mode)) == -211
        assert dm.window_level(3, (0, 0), (32, 16), (16, 8), mode).shape == (3, 8, 16)
        assert code(lambda: dm.window((200, 0), (128, 128), (32, 32), mode)) == -211         # checked against the base raster as before
    assert code(lambda: dm.level_size(4)) == -211 and code(lambda: dm.level_size(-1)) == -211
    assert code(lambda: dm.window_level(1, (0, 0), (8, 8), (8, 8), "cubic")) == -5           # cubic is not a window mode
    out = np.zeros((3, 8, 8), np.float32)
    n = C.c_int(0)
    assert L.apds_mosaic_window_level(None, 0, 0, 0, 8, 8, 8, 8, 0, out.ctypes.data) == -5   # a null handle
    assert L.apds_mosaic_window_level(dm.handle, 1, 0, 0, 8, 8, 8, 8, 0, None) == -5
    assert L.apds_mosaic_window_level(dm.handle, 1, 0, 0, 8, 8, 8, 8, 2, out.ctypes.data) == -5
    assert L.apds_mosaic_build_overviews(None, 32, C.byref(n)) == -5
    assert L.apds_mosaic_level_info(None, 0, None, None) == -5
    dm.close()
    with pytest.raises(E):
        dm.build_overviews(32)                                                               # closed handle


def test_build_from_a_thread_on_another_device_is_refused(gpu_pkg):
    L = gpu_pkg.lib()
    if L.apds_device_count() < 2:
        pytest.skip("one device only: there is no other device to call from")
    dm = gpu_pkg.geotiff_extractor.DeviceMosaic(_uniform(64, 64))
    rc = []

    def other():
        try:
            assert L.apds_set_device(1) == 0
            rc.append(L.apds_mosaic_build_overviews(dm.handle, 8, None))
        finally:
            L.apds_thread_release()

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert rc == [-5]
    assert dm.build_overviews(8) == 3                                                        # the refused call left the handle as it was
    dm.close()
