"""GPU: the mosaic resident in HBM (apds_mosaic_*, csrc/mosaic.hip) - its min/max reduction, the nearest gather, the separable Lanczos
pair, the extraction chain on top of them and the database build through geotiff_extractor.DeviceMosaic.

The Lanczos window is compared with a float64 reference Wy . src . Wx^T built from this file's own double weights (the rule of DESIGN.md
section 2, restated in `tables`). The bound, per pixel:

    |out - ref| <= 2 (n + 2) 2^-24 (|Wy| . |src| . |Wx|^T),        n = the largest tap count of either axis.

Derivation (u = 2^-24, first order). The kernel's weights are the doubles rounded once: w32 = w (1 + d), |d| <= u. A row-pass value is an
f32 dot product of at most n terms, each product and each addition rounded once (or fused, which rounds less): whatever the order of the
sum, fl(sum w32_j s_j) = sum w_j s_j (1 + e_j) with |e_j| <= (n + 1) u  (1 for the weight, 1 for the product, at most n - 1 for the
additions), so |t - t_exact| <= (n + 1) u sum |w_j| |s_j|. The column pass does the same to the row-pass values: its own error is
(n + 1) u sum |w_k| |t_k|, and it carries the row-pass errors through sum |w_k| (n + 1) u (|Wx| |src|)_k. With |t_k| <= (|Wx| |src|)_k to
first order the total is 2 (n + 1) u (|Wy| |src| |Wx|^T); the issue's (n + 2) leaves one u per pass for the final rounding. The bound
holds for every summation order, so the kernels' order is free. No pixel is excluded: where a NaN lies under a tap (any source pixel of the
footprint rectangle, whatever its weight) the output must be NaN, everywhere else the bound applies.

Figures measured on the MI355X are in profiles/mosaic/pytest_gpu.log (the test prints the worst error / bound ratio of every case)."""
import ctypes as C
import math
import threading
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def lanczos(x):
    if x == 0.0:
        return 1.0
    if not abs(x) < 3.0:
        return 0.0
    a = math.pi * x
    return math.sin(a) * math.sin(a / 3.0) / (a * a / 3.0)


def tables(n_src, offset, span, n_out):
    """Dense float64 weight matrix [n_out, n_src], the 0/1 footprint matrix, and the largest tap count."""
    ratio = span / n_out
    sw = min(1.0, 1.0 / ratio)
    radius = 3.0 / sw
    Wm, F, taps = np.zeros((n_out, n_src)), np.zeros((n_out, n_src)), 0
    for i in range(n_out):
        c = (i + 0.5) * ratio + offset
        a = max(int(math.floor(c - radius + 0.5)), 0)
        b = min(int(c + radius + 0.5), n_src)
        w = np.array([lanczos((j + 0.5 - c) * sw) for j in range(a, b)])
        total = 0.0
        for v in w:
            total += v
        Wm[i, a:b] = w / total
        F[i, a:b] = 1.0
        taps = max(taps, b - a)
    return Wm, F, taps


def check_lanczos(got, src, x0, y0, ww, wh, ow, oh, label):
    """got [3, oh, ow] against Wy . src . Wx^T; returns the worst error / bound."""
    H, Wd = src.shape[1:]
    Wx, Fx, nx = tables(Wd, x0, ww, ow)
    Wy, Fy, ny = tables(H, y0, wh, oh)
    n = max(nx, ny)
    worst = 0.0
    for b in range(3):
        nan = np.isnan(src[b])
        s = np.where(nan, 0.0, src[b].astype(np.float64))
        ref = Wy @ s @ Wx.T
        mag = np.abs(Wy) @ np.abs(s) @ np.abs(Wx).T
        want_nan = (Fy @ nan.astype(np.float64) @ Fx.T) > 0
        assert np.array_equal(np.isnan(got[b]), want_nan), (label, b, "NaN footprint")
        bound = 2 * (n + 2) * U * mag
        err = np.abs(np.where(want_nan, 0.0, got[b].astype(np.float64)) - np.where(want_nan, 0.0, ref))
        ok = err <= bound
        frac = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
        worst = max(worst, frac)
        print(f"lanczos {label} band {b}: taps {n} worst |err| {err.max():.3e} worst err/bound {frac:.3f}")
        assert ok.all(), (label, b, float(err.max()), frac)
    return worst


def _uniform(h, w, seed=3):
    return (np.random.default_rng(seed).random((3, h, w)) * 3000.0).astype(np.float32)


def _mosaic(pkg, size):
    """the synthetic mosaic of tests/test_preprocessor_gpu.py"""
    t = pkg.synth.make_tile(size, size, frame_index=11, channels=3).astype(np.float32)
    bands = np.stack([t[:, :, 2] * 3.0 + 10.0, t[:, :, 1] * 2.0 - 5.0, t[:, :, 0] * 1.5])
    bands[0, 5:9, 7:12] = np.nan
    return bands


# ---- handle ---------------------------------------------------------------------------------------------------------------------------
def test_min_max_equals_nanmin_nanmax(gpu_pkg):
    ge = gpu_pkg.geotiff_extractor
    bands = _uniform(1000, 1537) - 1000.0                      # odd width: the scalar path; negative and positive values
    bands[0, 10:40, 100:900] = np.nan
    bands[1, ::7, ::5] = np.nan
    bands[2, 999, 1536] = np.float32(-12345.5)
    bands[2, 0, 0] = np.float32(54321.25)
    dm = ge.DeviceMosaic(bands)
    assert dm.raster_size() == (1537, 1000)
    got = dm.datasets_min_max().as_array()
    want = ge.MosaicedDataset(bands).datasets_min_max().as_array()
    assert np.array_equal(got, want)
    for b in range(3):
        assert got[2 * b] == float(np.nanmin(bands[b])) and got[2 * b + 1] == float(np.nanmax(bands[b]))
    mm2 = np.zeros(6)
    assert gpu_pkg.lib().apds_mosaic_min_max(dm.handle, mm2.ctypes.data) == 0 and np.array_equal(mm2, want)     # the cached answer
    dm.close()
    even = _uniform(512, 1024, seed=5)                         # width a multiple of four: the 16-byte path
    even[1] = np.nan                                           # a band without a number
    even[0, 3, 3] = np.nan
    dm = ge.DeviceMosaic(even)
    got = dm.datasets_min_max().as_array()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                        # numpy: "All-NaN slice encountered"
        want = ge.MosaicedDataset(even).datasets_min_max().as_array()
    assert np.array_equal(got, want, equal_nan=True) and np.isnan(got[2]) and np.isnan(got[3]) and not np.isnan(got[[0, 1, 4, 5]]).any()
    rows, cols = C.c_int(0), C.c_int(0)
    assert gpu_pkg.lib().apds_mosaic_info(dm.handle, C.byref(rows), C.byref(cols)) == 0 and (rows.value, cols.value) == (512, 1024)
    dm.close()


# ---- nearest --------------------------------------------------------------------------------------------------------------------------
def test_nearest_window_equals_the_host_mirror(gpu_pkg):
    ge = gpu_pkg.geotiff_extractor
    bands = _uniform(1024, 1280)
    bands[1, 100:130, 200:260] = np.nan
    host, dm = ge.MosaicedDataset(bands), ge.DeviceMosaic(bands)
    cases = []
    for lod in (0, 1, 2):
        span = 256 * 2 ** lod
        cases += [((0, 0), (span, span), (256, 256)), ((1280 - span, 1024 - span), (span, span), (256, 256))]
    cases += [((3, 5), (777, 501), (256, 192)), ((100, 7), (300, 300), (200, 150)), ((11, 13), (128, 96), (256, 192)), ((0, 0), (1280, 1024), (100, 99))]
    for window, wsize, size in cases:
        want = host.window(window, wsize, size)
        got = dm.window(window, wsize, size)
        assert got.shape == (3, size[1], size[0])
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (window, wsize, size)
        if wsize == size:                                      # equal sizes copy the window under both modes
            assert np.array_equal(dm.window(window, wsize, size, "lanczos").view(np.uint32), got.view(np.uint32))
    assert np.array_equal(dm.to_rgb((3, 5), (777, 501), (256, 192)), host.to_rgb((3, 5), (777, 501), (256, 192)))
    dm.close()


# ---- Lanczos against the float64 reference -------------------------------------------------------------------------------------------
LANCZOS_CASES = [
    # label, (x0, y0), (win_w, win_h), (out_w, out_h) on a 1024 wide x 768 high raster
    ("interior lod1", (256, 256), (256, 256), (128, 128)),
    ("interior lod2", (256, 256), (512, 256), (128, 64)),
    ("corner top-left lod1", (0, 0), (256, 256), (128, 128)),
    ("corner bottom-right lod1", (768, 512), (256, 256), (128, 128)),
    ("whole raster lod3", (0, 0), (1024, 768), (128, 96)),
    ("unaligned", (37, 101), (301, 203), (128, 96)),
    ("ratio 3", (129, 64), (384, 384), (128, 128)),
    ("ratio 0.5", (300, 200), (64, 48), (128, 96)),
    ("ratio 0.5 corner", (960, 720), (64, 48), (128, 96)),
    ("mixed: x ratio 1, y ratio 2", (100, 100), (128, 256), (128, 128)),
    ("wide: several row-pass blocks", (3, 3), (1011, 100), (700, 50)),
]


@pytest.mark.parametrize("label,window,wsize,size", LANCZOS_CASES, ids=[c[0] for c in LANCZOS_CASES])
def test_lanczos_window_within_the_derived_bound(gpu_pkg, label, window, wsize, size):
    ge = gpu_pkg.geotiff_extractor
    src = _uniform(768, 1024)
    dm = ge.DeviceMosaic(src)
    got = dm.window(window, wsize, size, "lanczos")
    check_lanczos(got, src, window[0], window[1], wsize[0], wsize[1], size[0], size[1], label)
    dm.close()


def test_lanczos_nan_propagates_under_the_footprint_only(gpu_pkg):
    ge = gpu_pkg.geotiff_extractor
    src = _uniform(768, 1024, seed=9)
    src[0, 300:303, 400:420] = np.nan                          # inside the tile
    src[1, 250:252, 500] = np.nan                              # in the NEIGHBOUR above the tile, within the footprint's reach
    src[2, 600, 600] = np.nan                                  # far away: no output may see it
    dm = ge.DeviceMosaic(src)
    got = dm.window((256, 256), (256, 256), (128, 128), "lanczos")
    check_lanczos(got, src, 256, 256, 256, 256, 128, 128, "nan lod1")
    assert np.isnan(got[0]).any() and np.isnan(got[1]).any() and not np.isnan(got[2]).any()
    assert np.isnan(got[1, 0]).any() and not np.isnan(got[1, 8:]).any()      # only the first output rows reach rows 250, 251
    dm.close()


# ---- anchors that come from the input ----------------------------------------------------------------------------------------------
def test_constant_ramp_and_checkerboard(gpu_pkg):
    ge = gpu_pkg.geotiff_extractor
    H = W = 512
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    const = np.full((H, W), 1234.5, np.float32)
    ramp = (0.75 * xx + 0.5 * yy + 3.0).astype(np.float32)     # exact in f32
    checker = ((xx + yy) % 2).astype(np.float32)
    dm = ge.DeviceMosaic(np.stack([const, ramp, checker]))
    x0 = y0 = 128
    near = dm.window((x0, y0), (256, 256), (128, 128))
    lan = dm.window((x0, y0), (256, 256), (128, 128), "lanczos")
    n = 12
    # constant: sum w = 1, so every output is the constant within the bound (|W| |src| |W|^T = const * (sum |w|)^2)
    Wx, _, _ = tables(W, x0, 256, 128)
    absw = np.abs(Wx).sum(1)
    bound = 2 * (n + 2) * U * 1234.5 * absw[:, None] * absw[None, :]
    print("constant: worst err/bound", float((np.abs(lan[0] - 1234.5) / bound).max()))
    assert (np.abs(lan[0].astype(np.float64) - 1234.5) <= bound).all()
    # ramp: an aligned ratio-2 footprint is symmetric about its centre, so the filter reproduces a linear function: pixel j holds the value
    # at j, the centre of output i lies at (2 i + 1) + origin - 0.5 in those units
    cx = 2.0 * np.arange(128) + 1 + x0 - 0.5
    want = 0.75 * cx[None, :] + 0.5 * cx[:, None] + 3.0
    mag = np.abs(Wx) @ np.abs(ramp.astype(np.float64)) @ np.abs(Wx).T      # same tables on both axes (square raster, equal origins)
    err = np.abs(lan[1].astype(np.float64) - want)
    print("ramp: worst err/bound", float((err / (2 * (n + 2) * U * mag)).max()))
    assert (err <= 2 * (n + 2) * U * mag).all()
    # the one-pixel checkerboard: decimation aliases it to a flat 0 or 1, the filter removes it (mirror taps of an aligned ratio-2
    # footprint have opposite parity and equal weight: exactly one half each)
    assert np.isin(near[2], (0.0, 1.0)).all() and (near[2] == near[2][0, 0]).all()
    assert (np.abs(lan[2] - 0.5) <= 0.01).all()
    dm.close()


# ---- chain ----------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return len(a.keypoints) == len(b.keypoints) and np.array_equal(a.keypoints, b.keypoints) and np.array_equal(a.descriptors, b.descriptors)


def test_extract_equals_tile_extract_on_the_window_and_batch_equals_singles(gpu_pkg):
    ge, fe = gpu_pkg.geotiff_extractor, gpu_pkg.feature_extraction
    bands = _mosaic(gpu_pkg, 2048)
    dm = ge.DeviceMosaic(bands)
    mm = dm.datasets_min_max()
    origins = [(0, 0), (1024, 0), (0, 1024), (1024, 1024), (512, 512), (300, 700)]
    for mode in ("lanczos", "nearest"):
        singles = []
        for o in origins:
            win = dm.window(o, (1024, 1024), (512, 512), mode)
            want = fe.tile_keypoint_descriptor_extraction(win[0], win[1], win[2], mm, None)
            got = fe.mosaic_tile_keypoint_descriptor_extraction(dm, o, (1024, 1024), (512, 512), mode)
            assert len(got.keypoints) > 100 and _same(got, want), (mode, o)
            assert _same(fe.mosaic_tile_keypoint_descriptor_extraction(dm, o, (1024, 1024), (512, 512), mode, min_max=mm), want)
            singles.append(got)
        batch = fe.mosaic_tiles_keypoint_descriptor_extraction(dm, origins, (1024, 1024), (512, 512), mode)
        assert len(batch) == len(origins)
        for o, a, b in zip(origins, batch, singles):
            assert _same(a, b), (mode, o)
    # lod 0 (equal sizes) through the batch call equals the host path
    host = fe.tiles_keypoint_descriptor_extraction([bands[:, y:y + 512, x:x + 512] for x, y in origins], mm, None)
    for a, b in zip(fe.mosaic_tiles_keypoint_descriptor_extraction(dm, origins, (512, 512), (512, 512), "lanczos"), host):
        assert _same(a, b)
    dm.close()


# ---- database build -------------------------------------------------------------------------------------------------------------------
def _build(pkg, ds, **kw):
    pp, fd = pkg.preprocessor, pkg.feature_database
    table, images = fd.KeypointTable(400000), pp.ImageTable()
    out = pp.process_lod_from_mosaic(table, images, ds, 3, **kw)                # 16 + 4 + 1 tiles of 512
    levels = []
    for lod in range(3):
        k = table.read_keypoints_from_lod(lod)
        levels.append((k.keypoints.copy(), k.descriptors.copy(), k.image_ids.copy()))
    table.close()
    return out, images.rows, levels


def _levels_equal(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) for x, y in zip(a, b))


def test_database_build_from_a_device_mosaic(gpu_pkg):
    ge, pp, fe, fd = gpu_pkg.geotiff_extractor, gpu_pkg.preprocessor, gpu_pkg.feature_extraction, gpu_pkg.feature_database
    bands = _mosaic(gpu_pkg, 2048)
    host = ge.MosaicedDataset(bands)
    dm = host.to_device()
    ref = _build(gpu_pkg, host)
    assert [len(level) for level in ref[0]] == [16, 4, 1] and all(len(l[0]) > 100 for l in ref[2])
    for batch in (1, 4):
        got = _build(gpu_pkg, dm, batch=batch, resample="nearest")
        assert got[0] == ref[0] and got[1] == ref[1] and _levels_equal(got[2], ref[2]), batch
    # Lanczos: the single-tile chain (window -> apds_tile_extract -> store) as the expectation
    table, images = fd.KeypointTable(400000), pp.ImageTable()
    mm = dm.datasets_min_max()
    for lod in range(3):
        tile, columns, rows = pp.tile_grid(dm.raster_size(), 3, lod)
        span = (tile[0] * 2 ** lod, tile[1] * 2 ** lod)
        for i in range(rows):
            for j in range(columns):
                win = dm.window((j * span[0], i * span[1]), span, tile, "lanczos")
                pp.store_tile(table, images, fe.tile_keypoint_descriptor_extraction(win[0], win[1], win[2], mm, None), tile, j, i, lod)
    want = []
    for lod in range(3):
        k = table.read_keypoints_from_lod(lod)
        want.append((k.keypoints.copy(), k.descriptors.copy(), k.image_ids.copy()))
    table.close()
    for batch in (1, 4):
        got = _build(gpu_pkg, dm, batch=batch, resample="lanczos")
        assert got[1] == ref[1] == images.rows                                  # the image table does not depend on the resampling
        assert _levels_equal(got[2], want), batch
        assert _levels_equal(got[2][:1], ref[2][:1])                            # level 0 is a copy under both modes
        for lod in (1, 2):                                                      # ... and the switch does something above it
            assert len(got[2][lod][0]) > 100
            assert not (np.array_equal(got[2][lod][0], ref[2][lod][0]) and np.array_equal(got[2][lod][1], ref[2][lod][1])), lod
    # the host dataset's keyword goes through its lazily created device mosaic to the same rows
    assert _levels_equal(_build(gpu_pkg, host, resample="lanczos")[2], want)
    dm.close()


# ---- resources and errors -------------------------------------------------------------------------------------------------------------
def test_create_destroy_does_not_grow_device_memory(gpu_pkg):
    import torch
    ge = gpu_pkg.geotiff_extractor
    bands = _uniform(2048, 2048)                                                # 48 MiB per handle

    def cycle():
        dm = ge.DeviceMosaic(bands)
        dm.datasets_min_max()
        dm.window((0, 0), (1024, 1024), (512, 512), "lanczos")
        dm.close()

    cycle()                                                                     # the thread's workspace reaches its size
    torch.cuda.synchronize()
    assert gpu_pkg.lib().apds_release_cached_memory() == 0
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(20):
        cycle()
    assert gpu_pkg.lib().apds_release_cached_memory() == 0
    free1 = torch.cuda.mem_get_info()[0]
    print("free before / after 20 create-destroy cycles:", free0, free1)
    assert free0 - free1 < bands.nbytes, (free0, free1)                         # a leak of one handle per cycle would be 20 x this


def test_errors(gpu_pkg):
    ge, fe = gpu_pkg.geotiff_extractor, gpu_pkg.feature_extraction
    dm = ge.DeviceMosaic(_uniform(256, 512))
    E = gpu_pkg.ApdsError

    def code(fn):
        with pytest.raises(E) as e:
            fn()
        return e.value.code

    for mode in ("nearest", "lanczos"):
        assert code(lambda: dm.window((400, 0), (128, 128), (64, 64), mode)) == -211          # window outside the raster
        assert code(lambda: dm.window((0, 200), (128, 128), (64, 64), mode)) == -211
        assert code(lambda: dm.window((-1, 0), (128, 128), (64, 64), mode)) == -211
        assert code(lambda: dm.window((0, 0), (512, 256), (7, 7), mode)) == -5                # ratio 73 > 64
        assert code(lambda: dm.window((0, 0), (0, 128), (64, 64), mode)) == -215              # empty window
        assert code(lambda: dm.window((0, 0), (128, 128), (64, 0), mode)) == -215             # empty output
        assert code(lambda: fe.mosaic_tile_keypoint_descriptor_extraction(dm, (400, 0), (128, 128), (64, 64), mode)) == -211
        assert code(lambda: fe.mosaic_tiles_keypoint_descriptor_extraction(dm, [(0, 0), (400, 0)], (128, 128), (64, 64), mode)) == -211
    assert code(lambda: dm.window((0, 0), (128, 128), (64, 64), "cubic")) == -5
    out = np.zeros((3, 64, 64), np.float32)
    L = gpu_pkg.lib()
    assert L.apds_mosaic_window(dm.handle, 0, 0, 128, 128, 64, 64, 2, out.ctypes.data) == -5  # unknown resample
    assert L.apds_mosaic_window(None, 0, 0, 128, 128, 64, 64, 1, out.ctypes.data) == -5
    assert L.apds_mosaic_window(dm.handle, 0, 0, 128, 128, 64, 64, 1, None) == -5
    assert L.apds_mosaic_window(dm.handle, 0, 0, 512, 256, 8, 4, 1, out.ctypes.data) == 0     # ratio 64 exactly is served
    xy = np.zeros((4097, 2), np.int32)
    kps, desc, nb = C.c_void_p(), C.c_void_p(), C.c_int(0)
    counts = (C.c_int * 4097)()
    assert L.apds_mosaic_tile_extract_batch(dm.handle, xy.ctypes.data, 4097, 128, 128, 64, 64, 1, None, 0, C.byref(kps), C.byref(desc), counts, C.byref(nb)) == -5
    assert L.apds_mosaic_tile_extract_batch(dm.handle, xy.ctypes.data, 0, 128, 128, 64, 64, 1, None, 0, C.byref(kps), C.byref(desc), counts, C.byref(nb)) == -5
    dm.close()
    with pytest.raises(E):
        dm.window((0, 0), (128, 128), (64, 64))                                               # closed handle


def test_two_threads_share_one_handle(gpu_pkg):
    ge, fe = gpu_pkg.geotiff_extractor, gpu_pkg.feature_extraction
    dm = ge.DeviceMosaic(_mosaic(gpu_pkg, 2048))
    origins = [(0, 0), (1024, 0), (0, 1024), (1024, 1024), (512, 512), (300, 700), (1000, 24), (5, 999)]
    want = [fe.mosaic_tile_keypoint_descriptor_extraction(dm, o, (1024, 1024), (512, 512), "lanczos") for o in origins]
    got, errors = {}, []

    def work(idx):
        try:
            for _ in range(2):
                for i in idx:
                    got[i] = fe.mosaic_tile_keypoint_descriptor_extraction(dm, origins[i], (1024, 1024), (512, 512), "lanczos")
        except Exception as e:   # noqa: BLE001
            errors.append(e)
        finally:
            gpu_pkg.lib().apds_thread_release()

    threads = [threading.Thread(target=work, args=(range(k, len(origins), 2),)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, w in enumerate(want):
        assert _same(got[i], w), origins[i]
    dm.close()
