"""GPU: a float keypoint table and a byte table built from the same four 256 x 256 tiles (synth.make_tile through a resident mosaic and the
band merger), each four ways: apds_db_insert_image(_float) from host arrays, apds_db_insert_dev tile by tile, apds_db_insert_batch_dev with
the four tiles, and apds_mosaic_tiles_to_db from the mosaic.

 * every non-descriptor column of the float table (the 28-byte keypoint with the lifted coordinates, image id, level of detail, id) equals
   the byte table's bit for bit, in every build;
 * the float table's descriptor column is the rows apds_dev_akaze_extract_float_batch wrote for those tiles, bit for bit, all 256 bytes;
 * the typed calls refuse a table of the other kind and a full table refuses rows, both without changing the table;
 * apds_db_read_keypoint_from_id_float: the first id, the last id, a deleted id."""
import ctypes as C

import numpy as np
import pytest

import db_float_cases as cases
from db_float_cases import Ex, Snapshot, bits

pytestmark = pytest.mark.gpu

T = 256
CELLS = [(0, 0), (1, 0), (0, 1), (1, 1)]      # (column, row) of the four tiles, images 1 .. 4
LOD = 1                                       # a lift that does something: x * 2 + column * 256 * 2


class Tiles:
    pass


@pytest.fixture(scope="module")
def tiles(gpu_pkg):
    """the mosaic, its four tiles as the BGRA images the library extracts from, and both extractions of them left on the device"""
    import torch
    pkg, L = gpu_pkg, gpu_pkg.lib()
    ge = pkg.geotiff_extractor
    t = pkg.synth.make_tile(2 * T, 2 * T, frame_index=11, channels=3, blobs_per_mpx=20000).astype(np.float32)
    out = Tiles()
    out.dm = ge.DeviceMosaic(np.stack([t[:, :, 2] * 3.0 + 10.0, t[:, :, 1] * 2.0 - 5.0, t[:, :, 0] * 1.5]))
    mm = out.dm.datasets_min_max()
    imgs = []
    for j, i in CELLS:
        win = out.dm.window((j * T, i * T), (T, T), (T, T))
        imgs.append(ge.band_merger([win[b].ravel() for b in range(3)], mm, bgra=True).reshape(T, T, 4))
    out.imgs = torch.from_numpy(np.stack(imgs)).to("cuda:0")
    cap = out.cap = 4096
    out.kps_f = torch.zeros((4, cap, 7), dtype=torch.float32, device="cuda:0")
    out.kps_b = torch.zeros((4, cap, 7), dtype=torch.float32, device="cuda:0")
    out.desc_f = torch.zeros((4, cap, 64), dtype=torch.float32, device="cuda:0")
    out.desc_b = torch.zeros((4, cap, 64), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    cf, cb = (C.c_int * 4)(), (C.c_int * 4)()
    pkg._lib.check(L.apds_dev_akaze_extract_float_batch(out.imgs.data_ptr(), 4, T * T * 4, T, T, 4, T * 4, None, 0, 0, 0, 0, out.kps_f.data_ptr(),
                                                        out.desc_f.data_ptr(), cap, cf, None))
    pkg._lib.check(L.apds_stream_synchronize(None))
    pkg._lib.check(L.apds_dev_akaze_extract_batch(out.imgs.data_ptr(), 4, T * T * 4, T, T, 4, T * 4, 0, out.kps_b.data_ptr(), out.desc_b.data_ptr(), cap, cb, None))
    pkg._lib.check(L.apds_stream_synchronize(None))
    out.counts = list(cf)
    assert out.counts == list(cb) and min(out.counts) >= 20
    out.h_kps = out.kps_f.cpu().numpy().view(np.uint8).reshape(4, cap, 28).copy().view(pkg._lib.KEYPOINT_DTYPE).reshape(4, cap)
    assert out.h_kps.tobytes() == out.kps_b.cpu().numpy().tobytes()            # the float extraction's keypoints are the M-LDB call's
    out.h_desc_f, out.h_desc_b = out.desc_f.cpu().numpy(), out.desc_b.cpu().numpy()
    out.total = sum(out.counts)
    # what every build must hold, by row
    out.want_desc = np.concatenate([out.h_desc_f[i, :c] for i, c in enumerate(out.counts)])
    out.want_desc_b = np.concatenate([out.h_desc_b[i, :c, :61] for i, c in enumerate(out.counts)])
    out.want_img = np.concatenate([np.full(c, 1 + i, np.int32) for i, c in enumerate(out.counts)])
    yield out
    out.dm.close()


def build(pkg, tiles, way, table):
    L, is_float = pkg.lib(), table.is_float
    kps, desc = (tiles.kps_f, tiles.desc_f) if is_float else (tiles.kps_b, tiles.desc_b)
    row_bytes = 256 if is_float else 64
    if way == "host":
        for i, (j, r) in enumerate(CELLS):
            c = tiles.counts[i]
            d = tiles.h_desc_f[i, :c] if is_float else tiles.h_desc_b[i, :c, :61].copy()
            table.create_keypoints(Ex(tiles.h_kps[i, :c], d), 1 + i, LOD, j, r, (T, T))
    elif way == "dev":
        for i, (j, r) in enumerate(CELLS):
            table.create_keypoints_device(kps.data_ptr() + i * tiles.cap * 28, desc.data_ptr() + i * tiles.cap * row_bytes, tiles.counts[i], 1 + i, LOD, j, r, (T, T))
    elif way == "batch":
        cr = np.array(CELLS, np.uint32)
        cnt = (C.c_int32 * 4)(*tiles.counts)
        pkg._lib.check(L.apds_db_insert_batch_dev(table._h, kps.data_ptr(), desc.data_ptr(), 4, tiles.cap, cnt, 1, LOD, pkg._lib.ptr(cr), T, T, None))
    else:
        got = pkg.feature_extraction.mosaic_tiles_to_database(tiles.dm, table, [(j * T, i * T) for j, i in CELLS], (T, T), (T, T), CELLS, 1, LOD, "nearest")
        assert got == tiles.counts


@pytest.mark.parametrize("way", ["host", "dev", "batch", "mosaic"])
def test_float_table_equals_byte_table_and_the_float_extraction(gpu_pkg, tiles, way):
    pkg, fd = gpu_pkg, gpu_pkg.feature_database
    tf, tb = fd.KeypointTable(tiles.total, descriptor="kaze"), fd.KeypointTable(tiles.total)
    try:
        build(pkg, tiles, way, tf)
        build(pkg, tiles, way, tb)
        assert len(tf) == len(tb) == tiles.total
        sf, sb = Snapshot(pkg, tf, [1, 2, 3, 4], [LOD]), Snapshot(pkg, tb, [1, 2, 3, 4], [LOD])
        for name, a in sf.columns().items():
            assert a.tobytes() == sb.columns()[name].tobytes(), (way, name)
        assert np.array_equal(sf.ids, np.arange(1, tiles.total + 1)) and np.array_equal(sf.image_id, tiles.want_img) and (sf.lod == LOD).all()
        # the lift itself, on the first tile that has a non-zero offset (column 1): v * 2^lod + (column * tile * 2^lod) as f32
        a, c = tiles.counts[0], tiles.counts[1]
        src = tiles.h_kps[1, :c]
        assert np.array_equal(sf.kps["x"][a:a + c], src["x"] * np.float32(2) + np.float32(1 * T * 2)) and np.array_equal(sf.kps["y"][a:a + c], src["y"] * np.float32(2))
        assert np.array_equal(sf.desc, bits(tiles.want_desc).reshape(tiles.total, 256)), way
        assert np.array_equal(sb.desc[:, :61], tiles.want_desc_b) and not sb.desc[:, 61:].any(), way
    finally:
        tf.close()
        tb.close()


def test_wrong_kind_and_full_table_change_nothing(gpu_pkg, tiles):
    pkg, fd, L = gpu_pkg, gpu_pkg.feature_database, gpu_pkg.lib()
    ptr, BAD, NOMEM = pkg._lib.ptr, pkg._lib.ERR_BAD_ARG, pkg._lib.ERR_NOMEM
    c0 = tiles.counts[0]
    tf, tb = fd.KeypointTable(c0 + 5, descriptor="kaze"), fd.KeypointTable(c0 + 5)
    try:
        build_one = lambda t, d: t.create_keypoints(Ex(tiles.h_kps[0, :c0], d), 1, 0)      # noqa: E731
        build_one(tf, tiles.h_desc_f[0, :c0])
        build_one(tb, tiles.h_desc_b[0, :c0, :61].copy())
        before = Snapshot(pkg, tf, [1], [0]), Snapshot(pkg, tb, [1], [0])
        kp = np.ascontiguousarray(tiles.h_kps[0, :3])
        d8, df = np.zeros((3, 61), np.uint8), np.zeros((3, 64), np.float32)
        ids, img = np.zeros(c0, np.int32), np.zeros(c0, np.int32)
        out_kp, out8, outf = np.zeros(c0, pkg._lib.KEYPOINT_DTYPE), np.zeros((c0, 61), np.uint8), np.zeros((c0, 64), np.float32)
        n = C.c_int(0)
        # byte-typed calls on the float table
        assert L.apds_db_insert_image(tf._h, ptr(kp), ptr(d8), 3, 2, 0, 0, 0, 0, 0) == BAD
        pkg._lib.check(L.apds_db_select(tf._h, 0, 1, 0.0, 0.0, 0.0, 0.0, C.byref(n)))
        assert n.value == c0
        assert L.apds_db_view_download(tf._h, ptr(out_kp), ptr(out8), ptr(ids), ptr(img)) == BAD
        assert L.apds_db_read_keypoint_from_id(tf._h, 1, ptr(out_kp), ptr(out8), None, None) == BAD
        # float-typed calls on the byte table
        assert L.apds_db_insert_image_float(tb._h, ptr(kp), ptr(df), 3, 2, 0, 0, 0, 0, 0) == BAD
        pkg._lib.check(L.apds_db_select(tb._h, 0, 1, 0.0, 0.0, 0.0, 0.0, C.byref(n)))
        assert L.apds_db_view_download_float(tb._h, ptr(out_kp), ptr(outf), ptr(ids), ptr(img)) == BAD
        assert L.apds_db_read_keypoint_from_id_float(tb._h, 1, ptr(out_kp), ptr(outf), None, None) == BAD
        with pytest.raises(pkg.ApdsError) as e:                 # the Python front, before any conversion of the array
            tf.create_keypoints(Ex(kp, d8), 2, 0)
        assert e.value.code == BAD
        assert len(tf) == len(tb) == c0
        # a full table: six rows do not fit into five, from the host and from the device; five do
        six = np.ascontiguousarray(tiles.h_kps[1, :6])
        assert L.apds_db_insert_image_float(tf._h, ptr(six), ptr(np.ascontiguousarray(tiles.h_desc_f[1, :6])), 6, 2, 0, 0, 0, 0, 0) == NOMEM
        assert L.apds_db_insert_dev(tf._h, tiles.kps_f.data_ptr(), tiles.desc_f.data_ptr(), 6, 2, 0, 0, 0, 0, 0, None) == NOMEM
        cnt, cr = (C.c_int32 * 2)(3, 3), np.zeros((2, 2), np.uint32)
        assert L.apds_db_insert_batch_dev(tf._h, tiles.kps_f.data_ptr(), tiles.desc_f.data_ptr(), 2, tiles.cap, cnt, 2, 0, ptr(cr), 0, 0, None) == NOMEM
        assert len(tf) == c0
        after = Snapshot(pkg, tf, [1], [0]), Snapshot(pkg, tb, [1], [0])
        for a, b in zip(before, after):
            assert a.desc.tobytes() == b.desc.tobytes()
            for name, col in a.columns().items():
                assert col.tobytes() == b.columns()[name].tobytes(), name
        assert L.apds_db_insert_dev(tf._h, tiles.kps_f.data_ptr(), tiles.desc_f.data_ptr(), 5, 2, 0, 0, 0, 0, 0, None) == 0 and len(tf) == c0 + 5
    finally:
        tf.close()
        tb.close()


def test_read_keypoint_from_id_float(gpu_pkg, tiles):
    pkg, fd = gpu_pkg, gpu_pkg.feature_database
    tf = fd.KeypointTable(tiles.total, descriptor="kaze")
    try:
        build(pkg, tiles, "batch", tf)
        snap = Snapshot(pkg, tf, [1, 2, 3, 4], [LOD])
        for id_ in (1, tiles.total):
            got = tf.read_keypoint_from_id(id_)
            assert got.descriptors.dtype == np.float32 and np.array_equal(bits(got.descriptors[0]), bits(tiles.want_desc[id_ - 1]))
            assert got.keypoints.tobytes() == snap.kps[id_ - 1:id_].tobytes() and got.image_ids[0] == tiles.want_img[id_ - 1]
        victim = tiles.counts[0] + 1                         # the first row of the second tile
        assert tf.delete_keypoint(victim) == 1 and len(tf) == tiles.total - 1
        with pytest.raises(pkg.ApdsError) as e:
            tf.read_keypoint_from_id(victim)
        assert e.value.code == pkg._lib.ERR_OUT_OF_RANGE
        got = tf.read_keypoint_from_id(victim + 1)           # its neighbour moved down one row and kept every bit
        assert np.array_equal(bits(got.descriptors[0]), bits(tiles.want_desc[victim])) and got.keypoints.tobytes() == snap.kps[victim:victim + 1].tobytes()
        last = tf.read_keypoint_from_id(tiles.total)
        assert np.array_equal(bits(last.descriptors[0]), bits(tiles.want_desc[-1]))
        for id_ in (0, -3, tiles.total + 1):
            with pytest.raises(pkg.ApdsError) as e:
                tf.read_keypoint_from_id(id_)
            assert e.value.code == pkg._lib.ERR_OUT_OF_RANGE
    finally:
        tf.close()
