"""GPU: the keypoint table filled, geolocated and handed to the pipeline without leaving the device.

 * apds_db_insert_dev / apds_db_insert_batch_dev store exactly the rows apds_db_insert_image stores (coordinate lift, bytes 61-63 zeroed
   whatever the producer left there, image ids, order), at the borders of the 16-rows-per-block mapping and where the f32 offset rounds;
   a batch that does not fit, or a count above the capacity, changes nothing;
 * the preprocessor's device_insert build (apds_mosaic_tiles_to_db) gives the table and the image rows of the two-step batch build;
 * apds_db_world_coordinates equals apds_get_world_coordinates on float64(x), float64(y) bit for bit (and the oracle), counts the rows that
   miss the elevation raster, and takes the raster from the device as well;
 * apds_db_table goes stale and fresh with inserts; a pipeline over the table equals one over its downloaded and re-uploaded columns."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DGT = [9.0, 1e-4, 0, 57.0, 0, -1e-4]
EGT = [8.99, 3e-4, 0, 57.01, 0, -3e-4]


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def _download(pkg, addr, shape, dtype):
    out = np.zeros(shape, dtype)
    if out.nbytes:
        pkg._lib.check(pkg.lib().apds_dev_download(pkg._lib.ptr(out), addr, out.nbytes, None))
    return out


def _whole_table(pkg, table, with_xyz=False):
    """(rows64 [n, 64] u8, keypoints [n], xyz [n, 3] or None) of apds_db_table, downloaded"""
    rows64, kps, xyz, n = table.device_table()
    assert n == len(table)
    r = _download(pkg, rows64, (n, 64), np.uint8)
    k = _download(pkg, kps, n, pkg._lib.KEYPOINT_DTYPE)
    return (r, k, _download(pkg, xyz, (n, 3), np.float64) if xyz else None) if with_xyz else (r, k)


def _same_rows(a, b):
    return np.array_equal(a.ids, b.ids) and np.array_equal(a.keypoints, b.keypoints) and np.array_equal(a.descriptors, b.descriptors) and \
        np.array_equal(a.image_ids, b.image_ids)


def _same_tables(pkg, ta, tb, image_ids, lods):
    ra, ka = _whole_table(pkg, ta)
    rb, kb = _whole_table(pkg, tb)
    assert len(ta) == len(tb) and np.array_equal(ra, rb) and np.array_equal(ka, kb)
    assert not ra[:, 61:].any()
    for i in image_ids:
        assert _same_rows(ta.read_keypoints_from_image_id(i), tb.read_keypoints_from_image_id(i)), i
    for lod in lods:
        assert _same_rows(ta.read_keypoints_from_lod(lod), tb.read_keypoints_from_lod(lod)), lod


def _random_rows(pkg, n, seed):
    """n keypoints (with -0.0, a denormal response and equal responses among them) and n 64-byte rows whose bytes 61-63 are NOT zero"""
    rng = np.random.default_rng(seed)
    k = np.zeros(n, pkg._lib.KEYPOINT_DTYPE)
    k["x"], k["y"] = rng.uniform(0, 512, n).astype(np.float32), rng.uniform(0, 512, n).astype(np.float32)
    k["size"], k["angle"] = rng.uniform(4, 40, n).astype(np.float32), rng.uniform(0, 360, n).astype(np.float32)
    k["response"] = rng.uniform(1e-4, 1e-1, n).astype(np.float32)
    k["octave"], k["class_id"] = rng.integers(0, 4, n), rng.integers(-1, 3, n)
    if n >= 1:
        k["x"][0], k["angle"][0] = -0.0, -0.0
        k["response"][0] = np.float32(1e-41)                 # denormal
    if n >= 4:
        k["response"][2] = k["response"][3] = k["response"][1]
        k["response"][n - 1] = -0.0
    d = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    d[:, 61:] = rng.integers(1, 256, (n, 3), dtype=np.uint8)
    return k, d


def _to_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


class _Extracted:
    def __init__(self, keypoints, descriptors):
        self.keypoints, self.descriptors = keypoints, descriptors


# ---- 1. insert_dev = insert_image ------------------------------------------------------------------------------------------------------
LIFTS = [(0, 1, 2, (512, 512)), (3, 3, 1, (512, 384))]


@pytest.mark.parametrize("n,lod,column,row,tile", [(n, *lift) for n in (0, 1, 15, 16, 17, 257) for lift in LIFTS] +
                         [(17, 0, 40001, 50003, (513, 511))])     # column * tile_w = 20 520 513 > 2^24 and odd: the f32 offset rounds
def test_insert_dev_equals_insert_image(gpu_pkg, n, lod, column, row, tile):
    fd = gpu_pkg.feature_database
    k, d = _random_rows(gpu_pkg, n, 100 + n)
    k0, d0 = _random_rows(gpu_pkg, 3, 5)                      # both tables start with three rows: the new rows do not begin at a block border
    dev_t, host_t = fd.KeypointTable(300), fd.KeypointTable(300)
    try:
        for t in (dev_t, host_t):
            t.create_keypoints(_Extracted(k0, d0[:, :61].copy()), 1, 1, 2, 0, (64, 64))
        dk, dd = _to_device(k), _to_device(d)
        dev_t.create_keypoints_device(dk.data_ptr(), dd.data_ptr(), n, 9, lod, column, row, tile)
        host_t.create_keypoints(_Extracted(k, d[:, :61].copy()), 9, lod, column, row, tile)
        assert len(dev_t) == len(host_t) == 3 + n
        _same_tables(gpu_pkg, dev_t, host_t, (1, 9), (1, lod))
        # ... and both are what main.rs:299-300 says: v * 2^lod + (u64 product) as f32, one f32 operation each; the rest copied
        rows64, kps = _whole_table(gpu_pkg, dev_t)
        want = k.copy()
        want["x"] = k["x"] * np.float32(2.0 ** lod) + np.float32(column * tile[0] * 2 ** lod)
        want["y"] = k["y"] * np.float32(2.0 ** lod) + np.float32(row * tile[1] * 2 ** lod)
        assert kps[3:].tobytes() == want.tobytes()            # bytes: -0.0 stays -0.0, the denormal stays
        assert np.array_equal(rows64[3:, :61], d[:, :61])
        if column > 40000:
            assert float(np.float32(column * tile[0])) != column * tile[0]
    finally:
        dev_t.close()
        host_t.close()


# ---- 2. batch = sequence ---------------------------------------------------------------------------------------------------------------
def test_insert_batch_dev_equals_a_sequence_of_inserts(gpu_pkg):
    fd, L = gpu_pkg.feature_database, gpu_pkg.lib()
    cap, counts, first, lod, tile = 33, [0, 5, 0, 33, 1], 7, 1, (512, 512)
    cr = np.array([[0, 0], [1, 0], [2, 3], [3, 1], [0, 2]], np.uint32)
    k, d = _random_rows(gpu_pkg, cap * len(counts), 77)
    dk, dd = _to_device(k), _to_device(d)
    dev_t, host_t = fd.KeypointTable(60), fd.KeypointTable(60)

    def insert(cnts, capacity=cap):
        c = (C.c_int32 * len(cnts))(*cnts)
        return L.apds_db_insert_batch_dev(dev_t._h, dk.data_ptr(), dd.data_ptr(), len(cnts), capacity, c, first, lod, gpu_pkg._lib.ptr(cr), tile[0], tile[1], None)

    try:
        assert insert(counts) == 0
        for i, c in enumerate(counts):
            host_t.create_keypoints(_Extracted(k[i * cap:i * cap + c], d[i * cap:i * cap + c, :61].copy()), first + i, lod, int(cr[i, 0]), int(cr[i, 1]), tile)
        assert len(dev_t) == len(host_t) == sum(counts) == 39
        _same_tables(gpu_pkg, dev_t, host_t, range(first, first + len(counts)), (lod,))
        for i, c in enumerate(counts):
            assert len(dev_t.read_keypoints_from_image_id(first + i)) == c
        before = _whole_table(gpu_pkg, dev_t)
        # 21 rows are left: 22 do not fit, and nothing of them is written
        assert insert([0, 5, 0, 16, 1]) == gpu_pkg._lib.ERR_NOMEM
        assert insert([0, 0, 0, 0, cap + 1]) == gpu_pkg._lib.ERR_BAD_ARG
        assert insert([0, 5, 0, cap + 1, 1]) == gpu_pkg._lib.ERR_BAD_ARG
        assert insert([0, -1, 0, 3, 1]) == gpu_pkg._lib.ERR_BAD_ARG
        assert L.apds_db_rows(dev_t._h) == 39
        after = _whole_table(gpu_pkg, dev_t)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        _same_tables(gpu_pkg, dev_t, host_t, range(first, first + len(counts)), (lod,))
        assert insert([0, 5, 0, 15, 1]) == 0 and len(dev_t) == 60          # exactly full
    finally:
        dev_t.close()
        host_t.close()


# ---- 3. fused build = two-step build ---------------------------------------------------------------------------------------------------
def _mosaic(pkg, size):
    """tests/test_preprocessor_gpu.py's synthetic three-band mosaic, with a NaN hole that spans all three bands"""
    t = pkg.synth.make_tile(size, size, frame_index=11, channels=3).astype(np.float32)
    bands = np.stack([t[:, :, 2] * 3.0 + 10.0, t[:, :, 1] * 2.0 - 5.0, t[:, :, 0] * 1.5])
    bands[0, 5:9, 7:12] = np.nan
    bands[:, 300:420, 600:760] = np.nan
    return bands


@pytest.fixture(scope="module")
def builds(gpu_pkg):
    """{mask_nodata: (fused table, its images, its result), (two-step table, ...)} over one resident mosaic; read-only for the tests"""
    ge, pp, fd = gpu_pkg.geotiff_extractor, gpu_pkg.preprocessor, gpu_pkg.feature_database
    dm = ge.DeviceMosaic(_mosaic(gpu_pkg, 1024))
    out = {}
    for mask in (False, "support"):
        runs = []
        for device_insert in (True, False):
            table, images = fd.KeypointTable(100000), pp.ImageTable()
            res = pp.process_lod_from_mosaic(table, images, dm, 2, batch=4, mask_nodata=mask, device_insert=device_insert)
            runs.append((table, images, res))
        out[mask] = runs
    yield out
    for runs in out.values():
        for table, _, _ in runs:
            table.close()
    dm.close()


@pytest.mark.parametrize("mask", [False, "support"])
def test_fused_build_equals_the_two_step_build(gpu_pkg, builds, mask):
    (ft, fi, fr), (tt, ti, tr) = builds[mask]
    assert [len(level) for level in fr] == [4, 1]
    assert fr == tr and fi.rows == ti.rows
    assert len(ft) == sum(n for level in fr for _, n in level) > 100
    _same_tables(gpu_pkg, ft, tt, [r["id"] for r in fi.rows], (0, 1))
    assert ft.read_keypoints_from_lod(0).keypoints["x"].max() > 512          # the lift happened
    if mask:
        assert len(ft) < len(builds[False][0][0])                           # the hole's edges left no rows


# ---- 4. world points -------------------------------------------------------------------------------------------------------------------
def _elevation(pkg, ew=400, eh=400, with_raster=True):
    t = pkg.feature_database.ElevationTable()
    t.create_geotransform("dataset", DGT)
    if with_raster:
        t.create_geotransform("elevation", EGT)
        yy, xx = np.mgrid[0:eh, 0:ew]
        t.add_elevation_data(80 + 60 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + np.random.default_rng(4).uniform(0, 3, (eh, ew)))
    return t


def _host_world(pkg, xy, el):
    """apds_get_world_coordinates as it is: (status, xyz); a miss is APDS_ERR_OUT_OF_RANGE with those points NaN"""
    out = np.zeros((len(xy), 3), np.float64)
    dgt = el.transforms["dataset"]
    if el.elevation is None:
        rc = pkg.lib().apds_get_world_coordinates(pkg._lib.ptr(xy), len(xy), pkg._lib.ptr(dgt), None, None, 0, 0, pkg._lib.ptr(out))
    else:
        rc = pkg.lib().apds_get_world_coordinates(pkg._lib.ptr(xy), len(xy), pkg._lib.ptr(dgt), pkg._lib.ptr(el.transforms["elevation"]), pkg._lib.ptr(el.elevation),
                                                  el.elevation.shape[1], el.elevation.shape[0], pkg._lib.ptr(out))
    return rc, out


def test_world_coordinates_of_the_table_rows(gpu_pkg, oracle_mod, builds):
    import torch
    table = builds[False][0][0]
    n = len(table)
    _, kps = _whole_table(gpu_pkg, table)
    xy = np.ascontiguousarray(np.stack([kps["x"].astype(np.float64), kps["y"].astype(np.float64)], 1))
    assert xy.max() > 512 and n > 100                       # lifted coordinates of all five tiles
    # a raster that covers the mosaic
    el = _elevation(gpu_pkg)
    assert table.world_coordinates(el) == 0
    got = _whole_table(gpu_pkg, table, with_xyz=True)[2]
    rc, want = _host_world(gpu_pkg, xy, el)
    assert rc == 0 and got.tobytes() == want.tobytes() and np.isfinite(got).all()
    rc, ora = oracle_mod.world_coordinates(xy[:200], DGT, EGT, el.elevation)
    assert rc == 0 and np.array_equal(got[:200], ora)
    # the same raster passed as a device pointer
    dev_el = torch.from_numpy(el.elevation).to("cuda:0")
    torch.cuda.synchronize()
    assert table.world_coordinates(el, elevation_dev_ptr=dev_el.data_ptr()) == 0
    assert _whole_table(gpu_pkg, table, with_xyz=True)[2].tobytes() == want.tobytes()
    # no elevation data: height 0
    bare = _elevation(gpu_pkg, with_raster=False)
    assert table.world_coordinates(bare) == 0
    got = _whole_table(gpu_pkg, table, with_xyz=True)[2]
    rc, want0 = _host_world(gpu_pkg, xy, bare)
    assert rc == 0 and got.tobytes() == want0.tobytes() and got.tobytes() != want.tobytes()
    assert np.array_equal(got[:200], oracle_mod.world_coordinates(xy[:200], DGT)[1])
    # rasters that cover a part of the mosaic only: the left half (the reference's row id, round(y) * ew + round(x), wraps a column past
    # the raster's edge into the next row, so only ids past the last row miss) and the upper half (whose lower rows do miss)
    for ew, eh in ((200, 400), (400, 200)):
        part = _elevation(gpu_pkg, ew, eh)
        rc, wantp = _host_world(gpu_pkg, xy, part)
        miss = np.isnan(wantp).any(1)
        assert rc == (gpu_pkg._lib.ERR_OUT_OF_RANGE if miss.any() else 0)
        assert table.world_coordinates(part) == int(miss.sum())
        got = _whole_table(gpu_pkg, table, with_xyz=True)[2]
        assert np.array_equal(np.isnan(got), np.isnan(wantp)) and np.array_equal(np.isnan(got).all(1), miss)
        assert got[~miss].tobytes() == wantp[~miss].tobytes()
    assert 0 < miss.sum() < n
    # a singular elevation geotransform
    part.create_geotransform("elevation", [0, 0, 0, 0, 0, 0])
    with pytest.raises(gpu_pkg.ApdsError) as e:
        table.world_coordinates(part)
    assert e.value.code == gpu_pkg._lib.ERR_BAD_ARG


# ---- 5. staleness ----------------------------------------------------------------------------------------------------------------------
def test_the_table_view_follows_inserts(gpu_pkg):
    fd = gpu_pkg.feature_database
    k, d = _random_rows(gpu_pkg, 40, 9)
    el = _elevation(gpu_pkg)
    table = fd.KeypointTable(64)
    try:
        assert table.device_table()[2:] == (None, 0)                         # never computed
        table.create_keypoints(_Extracted(k[:39], d[:39, :61].copy()), 1, 0, 0, 0, (512, 512))
        rows64, kps, xyz, n = table.device_table()
        assert n == 39 and xyz is None and rows64 and kps
        assert table.world_coordinates(el) == 0
        rows64, kps, xyz, n = table.device_table()
        assert n == 39 and xyz
        first = _whole_table(gpu_pkg, table, with_xyz=True)
        table.create_keypoints(_Extracted(k[39:], d[39:, :61].copy()), 2, 1, 1, 0, (512, 512))
        rows64b, kpsb, xyzb, nb = table.device_table()
        assert nb == 40 and xyzb is None and (rows64b, kpsb) == (rows64, kps)
        r, kk = _whole_table(gpu_pkg, table)
        assert np.array_equal(r[:39], first[0]) and np.array_equal(kk[:39], first[1])
        want = k[39:].copy()
        want["x"] = want["x"] * np.float32(2) + np.float32(1024)
        want["y"] = want["y"] * np.float32(2)
        assert kk[39:].tobytes() == want.tobytes() and np.array_equal(r[39, :61], d[39, :61])
        assert table.world_coordinates(el) == 0
        again = _whole_table(gpu_pkg, table, with_xyz=True)
        assert again[2] is not None and again[2][:39].tobytes() == first[2].tobytes() and np.isfinite(again[2][39]).all()
    finally:
        table.close()


# ---- 6. the table as the pipeline's database -------------------------------------------------------------------------------------------
def test_a_pipeline_over_the_table_equals_one_over_its_downloaded_columns(gpu_pkg):
    import torch
    from importlib import import_module
    pl = import_module(gpu_pkg.__name__ + ".pipeline")
    fd, synth, L, check = gpu_pkg.feature_database, gpu_pkg.synth, gpu_pkg.lib(), gpu_pkg._lib.check
    T, ndb, dev = 512, 40000, torch.device("cuda:0")        # the smallest frames (and their DB size) of tests/test_streamed_pipeline_gpu.py
    frames_np = [synth.make_tile(T, T, frame_index=40 + i) for i in range(3)]
    cap = gpu_pkg.feature_extraction.MAX_POINTS
    kps = torch.empty((cap, 7), dtype=torch.float32, device=dev)
    desc = torch.empty((cap, 64), dtype=torch.uint8, device=dev)
    table = fd.KeypointTable(ndb)
    streamed = by_hand = None
    try:
        with torch.cuda.stream(torch.cuda.Stream(dev)):      # extraction and insert on one stream
            for i, f in enumerate(frames_np):                 # the DB: every frame rolled by (19, 23), straight from the extraction's buffers
                rolled = torch.from_numpy(np.roll(f, (19, 23), axis=(0, 1)).copy()).to(dev)
                n = C.c_int(0)
                check(L.apds_dev_akaze_extract(rolled.data_ptr(), T, T, 4, rolled.stride(0), cap, kps.data_ptr(), desc.data_ptr(), cap, C.byref(n),
                                               pl.torch_stream()))
                table.create_keypoints_device(kps.data_ptr(), desc.data_ptr(), n.value, i + 1, 0, 0, 0, (T, T), stream=pl.torch_stream())
            torch.cuda.synchronize()
        P = len(table)
        assert 100 < P < ndb
        pad = np.zeros(ndb - P, gpu_pkg._lib.KEYPOINT_DTYPE)   # ... then random rows, as that test pads its DB
        table.create_keypoints(_Extracted(pad, synth.make_descriptor_db(ndb - P)), 4, 0, 0, 0, (T, T))
        assert table.world_coordinates(_elevation(gpu_pkg)) == 0
        K = np.array([[4000.0, 0, T / 2], [0, 4000.0, T / 2], [0, 0, 1]])
        rows64, kk, xyz = _whole_table(gpu_pkg, table, with_xyz=True)
        origin = xyz.mean(0)
        blank = torch.zeros((T, T, 4), dtype=torch.uint8, device=dev)
        blank[..., 3] = 255
        frames = [torch.from_numpy(frames_np[1]).to(dev), blank]
        torch.cuda.synchronize()

        pose = pl.PoseStage.from_table(table, K, origin=origin)
        assert pose.db_xyz_dev.data_ptr() == table.device_table()[2] and np.array_equal(pose.db_xyz, xyz)
        streamed = pl.StreamedFramePipeline.from_table(table, pose=pose)
        assert streamed.matcher.rows.data_ptr() == table.device_table()[0] and streamed.db_kp.data_ptr() == table.device_table()[1]
        got, _ = streamed.run(frames, 2, filter_strength=0.3)
        streamed.close()

        db = torch.from_numpy(rows64).to(dev)
        db_xy = torch.from_numpy(np.ascontiguousarray(np.stack([kk["x"], kk["y"]], 1))).to(dev)
        torch.cuda.synchronize()
        by_hand = pl.StreamedFramePipeline(db, db_xy, pose=pl.PoseStage(xyz, K, origin=origin))
        want, _ = by_hand.run(frames, 2, filter_strength=0.3)
        by_hand.close()

        for i, (a, b) in enumerate(zip(got, want)):
            assert (a["n_keypoints"], a["n_matches"], a["n_inliers"], a["status"]) == (b["n_keypoints"], b["n_matches"], b["n_inliers"], b["status"]), (i, a, b)
            assert (a["H"] is None) == (b["H"] is None) and (a["H"] is None or np.array_equal(a["H"], b["H"])), i
            pa, pb = a["pose"], b["pose"]
            assert (pa["status"], pa["found"], pa["n_correspondences"], pa["n_inliers"]) == (pb["status"], pb["found"], pb["n_correspondences"], pb["n_inliers"]), i
            assert np.array_equal(pa["rvec"], pb["rvec"]) and np.array_equal(pa["tvec"], pb["tvec"]), i
        assert got[0]["n_matches"] > 0 and got[0]["H"] is not None and got[0]["pose"]["n_correspondences"] == got[0]["n_matches"]
        assert abs(got[0]["H"][0, 2] - 23) < 0.5 and abs(got[0]["H"][1, 2] - 19) < 0.5      # the planted translation: trainIdx is the table row
        assert got[1]["n_keypoints"] == 0 and got[1]["n_matches"] == 0 and got[1]["H"] is None
    finally:
        for p in (streamed, by_hand):
            if p is not None:
                p.close()
        table.close()
