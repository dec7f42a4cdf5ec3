"""GPU: rows leave the keypoint table by id, by image, by level of detail and by region; the survivors close up on the device.

The reference of every check is numpy on host copies (boolean indexing of the columns); it shares no text with the kernels. A table is
read through the apds_db_table pointers and apds_db_ids, so insertion order is what is compared; image id and level of detail, which no
pointer exposes, are rebuilt from the row ids of one select per value. Every comparison is on bytes.

 * structural borders of the TB = 1024 compaction: sizes around one and several workgroups, eight delete patterns each;
 * the chunk border (2^20 rows per gather / scatter pair) and more than 1024 workgroups through the one-workgroup offsets kernel;
 * the id rule: ids are never reused, keep their row's identity, and continue from the highest id ever given;
 * the delete predicates equal the select predicates, and selects on the survivors equal selects on a fresh table of the same rows."""
import ctypes as C

import numpy as np
import pytest

from db_table_snapshot import Snapshot, assert_same as _assert_same, download as _download

pytestmark = pytest.mark.gpu

TB = 1024
CHUNK = 1 << 20
DGT = [9.0, 1e-4, 0, 57.0, 0, -1e-4]
TILE = (64, 64)


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def _device_rows(n, seed):
    """n keypoints (28 bytes each, as [n, 7] f32 with two int32 columns) and n 64-byte rows with garbage in bytes 61-63, made on the device.
    x, y are multiples of 0.25 in [0, 64): rows that sit exactly on an integer bound exist in numbers."""
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(seed)
    kp = torch.empty((n, 7), dtype=torch.float32, device=dev)
    kp[:, 0:2] = torch.randint(0, 256, (n, 2), generator=g, device=dev).to(torch.float32) * 0.25
    kp[:, 2] = torch.rand(n, generator=g, device=dev) * 36 + 4
    kp[:, 3] = torch.rand(n, generator=g, device=dev) * 360
    kp[:, 4] = torch.rand(n, generator=g, device=dev) * 0.1
    kp[:, 5:7] = torch.randint(0, 4, (n, 2), generator=g, device=dev, dtype=torch.int32).view(torch.float32)
    desc = torch.randint(0, 256, (n, 64), generator=g, device=dev, dtype=torch.uint8)
    desc[:, 61:] |= 1
    torch.cuda.synchronize()
    return kp, desc


def _segments(n, parts=4, first_image_id=10):
    """[(start, end, image id, level of detail, tile column)]: `parts` runs of rows, levels of detail 0 and 1 in turn"""
    cuts = [n * i // parts for i in range(parts + 1)]
    return [(cuts[i], cuts[i + 1], first_image_id + i, i % 2, i) for i in range(parts)]


def _insert(pkg, table, kp, desc, start, count, image_id, lod, column):
    counts = (C.c_int32 * 1)(count)
    cr = (C.c_uint32 * 2)(column, 1)
    pkg._lib.check(pkg.lib().apds_db_insert_batch_dev(table._h, kp.data_ptr() + start * 28, desc.data_ptr() + start * 64, 1, count, counts, image_id, lod, cr,
                                                      TILE[0], TILE[1], None))


def _fill(pkg, table, kp, desc, segments, keep=None):
    """the segments' rows through apds_db_insert_batch_dev; keep (bool per source row): only those, from a compacted device copy"""
    import torch
    for start, end, image_id, lod, column in segments:
        if keep is None:
            _insert(pkg, table, kp, desc, start, end - start, image_id, lod, column)
        else:
            idx = torch.from_numpy(np.flatnonzero(keep[start:end]) + start).to(kp.device)
            k, d = kp.index_select(0, idx).contiguous(), desc.index_select(0, idx).contiguous()
            torch.cuda.synchronize()
            _insert(pkg, table, k, d, 0, len(idx), image_id, lod, column)


def _elevation(pkg):
    et = pkg.feature_database.ElevationTable()
    et.create_geotransform("dataset", DGT)
    return et


def _delete_ids(pkg, table, ids):
    a = np.ascontiguousarray(ids, np.int32)
    n = C.c_int64(-1)
    pkg._lib.check(pkg.lib().apds_db_delete_ids(table._h, pkg._lib.ptr(a), len(a), C.byref(n)))
    return n.value


@pytest.fixture(scope="module")
def source(gpu_pkg):
    """the device rows every small test inserts a prefix of; never written after this"""
    return _device_rows(3 * TB + 7 + 16, 2024)


def _table(pkg, source, n, spare=16):
    kp, desc = source
    table = pkg.feature_database.KeypointTable(n + spare)
    segs = _segments(n)
    _fill(pkg, table, kp, desc, segs)
    assert len(table) == n and table.world_coordinates(_elevation(pkg)) == 0
    return table, segs


# ---- 1. structural borders at TB = 1024 -------------------------------------------------------------------------------------------------
SIZES = [1, 2, TB - 1, TB, TB + 1, 3 * TB + 7]
PATTERNS = {
    "nothing": lambda n: np.zeros(n, bool),
    "everything": lambda n: np.ones(n, bool),
    "first": lambda n: np.arange(n) == 0,
    "last": lambda n: np.arange(n) == n - 1,
    "every_other": lambda n: np.arange(n) % 2 == 0,
    "straddle": lambda n: (np.arange(n) >= 1000) & (np.arange(n) <= 1100),
    "block_firsts": lambda n: np.arange(n) % TB == 0,
    "all_but_last": lambda n: np.arange(n) != n - 1,
}


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("n", SIZES)
def test_delete_at_the_workgroup_borders(gpu_pkg, source, n, pattern):
    pkg = gpu_pkg
    table, segs = _table(pkg, source, n)
    try:
        imgs, lods = [s[2] for s in segs], (0, 1)
        before = Snapshot(pkg, table, imgs, lods)
        assert np.array_equal(before.ids, np.arange(1, n + 1)) and before.xyz is not None and np.isfinite(before.xyz).all()
        for start, end, image_id, lod, _ in segs:
            assert (before.image_id[start:end] == image_id).all() and (before.lod[start:end] == lod).all()
        victims = PATTERNS[pattern](n)
        pointers = table.device_table()[:3]
        ids_ptr = C.c_void_p()
        pkg._lib.check(pkg.lib().apds_db_ids(table._h, C.byref(ids_ptr)))
        unknown = [0, -7, n + 1, 2 ** 31 - 1]
        got = _delete_ids(pkg, table, np.concatenate([before.ids[victims], unknown]).astype(np.int32))
        assert got == int(victims.sum())
        assert len(table) == n - got
        want = before.keep(~victims)
        if not victims.any():
            again = C.c_void_p()
            pkg._lib.check(pkg.lib().apds_db_ids(table._h, C.byref(again)))
            assert table.device_table()[:3] == pointers and again.value == ids_ptr.value
        if len(table):
            _assert_same(Snapshot(pkg, table, imgs, lods), want, pattern)
        else:
            assert pkg.lib().apds_db_rows(table._h) == 0 and table.device_table()[3] == 0
            assert len(table.read_keypoints_from_lod(0)) == 0
        # a following insert works, and its ids go on from the highest id ever given
        kp, desc = source
        _insert(pkg, table, kp, desc, 3 * TB + 7, 5, 77, 1, 3)
        after = Snapshot(pkg, table, imgs + [77], lods)
        assert after.n == want.n + 5
        assert np.array_equal(after.ids, np.concatenate([want.ids, np.arange(n + 1, n + 6)]))
        assert after.desc[:want.n].tobytes() == want.desc.tobytes() and after.kps[:want.n].tobytes() == want.kps.tobytes()
        assert (after.image_id[want.n:] == 77).all() and (after.lod[want.n:] == 1).all()
        assert np.array_equal(after.desc[want.n:, :61], _download(pkg, desc.data_ptr() + (3 * TB + 7) * 64, (5, 64), np.uint8)[:, :61])
        assert not after.desc[:, 61:].any() and after.xyz is None          # the new rows have no world points yet
    finally:
        table.close()


# ---- 2. the chunk border, and more than 1024 workgroups in the offsets kernel -----------------------------------------------------------
def test_delete_across_the_chunk_borders(gpu_pkg):
    """2 * chunk + 3 rows. Delete A: survivors and victims on both sides of both chunk borders, every other row at the borders, a third of the
    rows elsewhere. Rows are inserted again until the table spans three chunks once more; delete B removes one whole chunk (and the rows
    around it keep theirs). Delete C is a level of detail, by predicate."""
    pkg = gpu_pkg
    n = 2 * CHUNK + 3
    kp, desc = _device_rows(n, 7)
    table = pkg.feature_database.KeypointTable(n + 4096)
    try:
        segs = _segments(n, parts=20)                      # every image below the select's row limit
        imgs = [s[2] for s in segs]
        _fill(pkg, table, kp, desc, segs)
        assert len(table) == n and n > 1024 * TB and table.world_coordinates(_elevation(pkg)) == 0
        before = Snapshot(pkg, table, imgs)
        lod = np.concatenate([np.full(e - s, l, np.int32) for s, e, _, l, _ in segs])
        rng = np.random.default_rng(11)
        victims = rng.random(n) < 1 / 3
        victims[:5] = [False, False, False, True, False]   # the first victim is in block 0: the chunks are [0, 2^20), [2^20, 2^21), the rest
        for border in (CHUNK, 2 * CHUNK):
            victims[border - 4:border + 3] = [True, False, True, False, False, True, False]
        victims[n - 1] = False
        assert _delete_ids(pkg, table, before.ids[victims]) == int(victims.sum())
        want = before.keep(~victims)
        lod = lod[~victims]
        _assert_same(Snapshot(pkg, table, imgs), want, "A")

        # eight more tiles from the same device rows, one batch call: the table spans three chunks again
        per = (n + 4096 - want.n) // 8
        counts = (C.c_int32 * 8)(*([per] * 8))
        cr = np.zeros((8, 2), np.uint32)
        pkg._lib.check(pkg.lib().apds_db_insert_batch_dev(table._h, kp.data_ptr(), desc.data_ptr(), 8, per, counts, 100, 1, pkg._lib.ptr(cr), TILE[0], TILE[1], None))
        imgs += list(range(100, 108))
        assert len(table) == want.n + 8 * per > 2 * CHUNK + TB and table.world_coordinates(_elevation(pkg)) == 0
        before = Snapshot(pkg, table, imgs)
        assert before.kps[:want.n].tobytes() == want.kps.tobytes() and before.xyz[:want.n].tobytes() == want.xyz.tobytes()
        assert np.array_equal(before.ids, np.concatenate([want.ids, np.arange(n + 1, n + 1 + 8 * per)]))
        lod = np.concatenate([lod, np.ones(8 * per, np.int32)])
        victims = np.zeros(before.n, bool)
        victims[7] = True                                  # block 0 again
        victims[CHUNK:2 * CHUNK] = True                    # the whole second chunk
        victims[2 * CHUNK + 1] = True
        assert _delete_ids(pkg, table, before.ids[victims][::-1]) == CHUNK + 2
        want = before.keep(~victims)
        lod = lod[~victims]
        _assert_same(Snapshot(pkg, table, imgs), want, "B")

        assert table.delete_keypoints_from_lod(1) == int((lod == 1).sum()) > 0
        want = want.keep(lod == 0)
        got = Snapshot(pkg, table)
        want.image_id = None
        _assert_same(got, want, "C")
    finally:
        table.close()


# ---- 3. the id rule ---------------------------------------------------------------------------------------------------------------------
def test_ids_are_serial_and_never_reused(gpu_pkg, source):
    pkg, L = gpu_pkg, gpu_pkg.lib()
    n = 2000
    table, segs = _table(pkg, source, n, spare=40)
    try:
        # no delete yet: the ids of a selection are row + 1, as they always were
        sel = table.read_keypoints_from_lod(0)
        rows = _download(pkg, table.view_device_pointers()[2], len(sel), np.int32)
        assert len(sel) == 1000 and np.array_equal(sel.ids, rows + 1)
        before = Snapshot(pkg, table, [s[2] for s in segs], (0, 1))
        # an unsorted list with duplicates and unknown ids deletes exactly the known ones; the last row (the highest id) goes too
        listed = np.array([n, 17, 1500, 17, 0, -3, n + 50, 1024, 1025, 3, n, 1500, 2 ** 31 - 1], np.int32)
        known = np.unique(listed[(listed >= 1) & (listed <= n)])
        assert _delete_ids(pkg, table, listed) == len(known) == 6
        victims = np.isin(before.ids, known)
        want = before.keep(~victims)
        _assert_same(Snapshot(pkg, table, [s[2] for s in segs], (0, 1)), want, "ids")
        assert _delete_ids(pkg, table, listed) == 0 and len(table) == n - 6          # the same list again: nothing is left to delete
        assert table.delete_keypoint(5) == 1 and table.delete_keypoint(5) == 0       # the reference's delete_keypoint, Ok(()) both times
        want = want.keep(want.ids != 5)
        # read_keypoint_from_id: every survivor at the borders of the search, and a spread of the others
        probe = np.unique(np.concatenate([[0, 1, 2, want.n - 2, want.n - 1], np.arange(0, want.n, 37), np.flatnonzero(np.diff(want.ids) > 1)]))
        for r in probe:
            kp = np.zeros(1, pkg._lib.KEYPOINT_DTYPE)
            d = np.full(61, 0xAA, np.uint8)
            img, row = C.c_int(-1), C.c_int64(-1)
            assert L.apds_db_read_keypoint_from_id(table._h, int(want.ids[r]), pkg._lib.ptr(kp), pkg._lib.ptr(d), C.byref(img), C.byref(row)) == 0
            assert row.value == r and img.value == want.image_id[r]
            assert kp.tobytes() == want.kps[r:r + 1].tobytes() and np.array_equal(d, want.desc[r, :61])
        one = table.read_keypoint_from_id(int(want.ids[40]))
        assert one.keypoints.tobytes() == want.kps[40:41].tobytes() and one.image_ids[0] == want.image_id[40]
        for gone in (5, 17, n, 0, -1, n + 1, 2 ** 31 - 1):                            # deleted, zero, never given
            assert L.apds_db_read_keypoint_from_id(table._h, gone, None, None, None, None) == pkg._lib.ERR_OUT_OF_RANGE, gone
        with pytest.raises(pkg.ApdsError) as e:
            table.read_keypoint_from_id(17)
        assert e.value.code == pkg._lib.ERR_OUT_OF_RANGE
        # rows inserted now go on from the highest id ever given (n, whose row is gone), and ids still ascend
        kp, desc = source
        _insert(pkg, table, kp, desc, 100, 30, 50, 0, 0)
        ids = table.ids()
        assert np.array_equal(ids, np.concatenate([want.ids, np.arange(n + 1, n + 31)])) and (np.diff(ids) > 0).all()
        sel = table.read_keypoints_from_image_id(50)
        assert np.array_equal(np.sort(sel.ids), np.arange(n + 1, n + 31))             # a selection's ids are the stable ones
        rows = _download(pkg, table.view_device_pointers()[2], len(sel), np.int32)
        assert np.array_equal(sel.ids, ids[rows])
        assert table.delete_keypoints(np.arange(n + 1, n + 31)) == 30
        _insert(pkg, table, kp, desc, 0, 2, 51, 0, 0)
        assert np.array_equal(table.ids(), np.concatenate([want.ids, [n + 31, n + 32]]))
    finally:
        table.close()


# ---- 4. the delete predicates are the select predicates ----------------------------------------------------------------------------------
# segment 0 is image 10, level 0, tile column 0, tile row 1 of 64 x 64 tiles: x = k.x, y = k.y + 64. The box has fractional bounds:
# floor(5.3) = 5 <= x <= ceil(40.6) = 41, floor(70.5) = 70 <= y <= ceil(100.2) = 101.
BOX = (5.3, 70.5, 40.6, 100.2)
PLANTED = [(5.0, 80.0), (41.0, 80.0), (20.0, 70.0), (20.0, 101.0), (5.0, 70.0), (41.0, 101.0),         # exactly on floor(start) / ceil(end): inside
           (4.75, 80.0), (41.25, 80.0), (20.0, 69.75), (20.0, 101.25), (5.25, 70.25)]                  # just outside (four), just inside
N_PRED = 3 * TB + 7


@pytest.fixture(scope="module")
def predicate_rows(gpu_pkg):
    import torch
    kp, desc = _device_rows(N_PRED, 99)
    for i, (x, y) in enumerate(PLANTED):
        kp[3 + 2 * i, 0], kp[3 + 2 * i, 1] = x, y - 64.0
    torch.cuda.synchronize()
    return kp, desc


def _numpy_predicate(snap, mode, value, box):
    if mode == 0:
        return snap.image_id == value
    if mode == 1:
        return snap.lod == value
    x0, y0, x1, y1 = np.floor(np.float32(box[0])), np.floor(np.float32(box[1])), np.ceil(np.float32(box[2])), np.ceil(np.float32(box[3]))
    x, y = snap.kps["x"], snap.kps["y"]
    return (snap.lod == value) & (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)


def _selection(pkg, table, view, mode, value, box):
    """what apds_db_select and apds_db_view_select leave on the device for one selection, rows as rows"""
    m = C.c_int(0)
    pkg._lib.check(pkg.lib().apds_db_select(table._h, mode, value, *[float(b) for b in box], C.byref(m)))
    r64, kps, rows, img, n = table.view_device_pointers()
    out = [_download(pkg, r64, (n, 64), np.uint8), _download(pkg, kps, n, pkg._lib.KEYPOINT_DTYPE), _download(pkg, rows, n, np.int32),
           _download(pkg, img, n, np.int32)]
    sel = (lambda: view.read_keypoints_from_image_id(value, with_xyz=True)) if mode == 0 else \
        (lambda: view.read_keypoints_from_lod(value, with_xyz=True)) if mode == 1 else \
        (lambda: view.read_keypoints_from_coordinates(box[0], box[1], box[2], box[3], value, with_xyz=True))
    nv = sel()
    import torch
    torch.cuda.synchronize()
    r64, kps, rows, img, xyz, n2 = view.device_pointers()
    assert nv == n2 == n
    out += [_download(pkg, r64, (n, 64), np.uint8), _download(pkg, kps, n, pkg._lib.KEYPOINT_DTYPE), _download(pkg, rows, n, np.int32),
            _download(pkg, img, n, np.int32), _download(pkg, xyz, (n, 3), np.float64)]
    return out


CASES = [(0, 11, (0, 0, 0, 0)), (0, 999, (0, 0, 0, 0)), (1, 1, (0, 0, 0, 0)), (1, 0, (0, 0, 0, 0)), (2, 0, BOX), (2, 1, (200.2, 64.0, 300.9, 190.5)),
         (2, 0, (0.0, 64.0, 63.75, 127.75))]


@pytest.mark.parametrize("mode,value,box", CASES)
def test_delete_where_equals_the_select_predicate(gpu_pkg, predicate_rows, mode, value, box):
    pkg = gpu_pkg
    kp, desc = predicate_rows
    segs = _segments(N_PRED)
    imgs, lods = [s[2] for s in segs], (0, 1)
    table, fresh = pkg.feature_database.KeypointTable(N_PRED), pkg.feature_database.KeypointTable(N_PRED)
    views = []
    try:
        _fill(pkg, table, kp, desc, segs)
        assert table.world_coordinates(_elevation(pkg)) == 0
        before = Snapshot(pkg, table, imgs, lods)
        victims = _numpy_predicate(before, mode, value, box)
        if (mode, value, box) == (2, 0, BOX):
            planted = victims[3:3 + 2 * len(PLANTED):2]
            assert planted.tolist() == [True] * 6 + [False] * 4 + [True]
            assert before.kps["x"][3] == 5.0 and before.kps["y"][3 + 6] == 101.0           # rows exactly on floor(start) and on ceil(end)
        n_del = C.c_int64(-1)
        pkg._lib.check(pkg.lib().apds_db_delete_where(table._h, mode, value, *[float(b) for b in box], C.byref(n_del)))
        assert n_del.value == int(victims.sum()) and (value == 999) == (n_del.value == 0)
        want = before.keep(~victims)
        _assert_same(Snapshot(pkg, table, imgs, lods), want, "where")
        # the survivors, selected: equal to the same selects on a fresh table built from the surviving rows
        _fill(pkg, fresh, kp, desc, segs, keep=~victims)
        assert len(fresh) == want.n and fresh.world_coordinates(_elevation(pkg)) == 0
        views = [table.view(), fresh.view()]
        for smode, svalue, sbox in CASES + [(0, 10, (0, 0, 0, 0)), (0, 13, (0, 0, 0, 0))]:
            a = _selection(pkg, table, views[0], smode, svalue, sbox)
            b = _selection(pkg, fresh, views[1], smode, svalue, sbox)
            for i, (u, v) in enumerate(zip(a, b)):
                assert u.shape == v.shape and u.tobytes() == v.tobytes(), (smode, svalue, sbox, i)
            if (smode, svalue, sbox) == (mode, value, box):
                assert len(a[0]) == 0                                                      # what was deleted is not selected any more
    finally:
        for v in views:
            v.close()
        table.close()
        fresh.close()


def test_the_python_front_deletes_by_image_level_and_region(gpu_pkg, predicate_rows):
    pkg = gpu_pkg
    kp, desc = predicate_rows
    segs = _segments(N_PRED)
    table = pkg.feature_database.KeypointTable(N_PRED)
    try:
        _fill(pkg, table, kp, desc, segs)
        before = Snapshot(pkg, table, [s[2] for s in segs], (0, 1))
        region = _numpy_predicate(before, 2, 0, BOX)
        assert table.delete_keypoints_from_coordinates(*BOX, 0) == int(region.sum()) > 0
        assert table.delete_keypoints_from_image_id(12) == int(((before.image_id == 12) & ~region).sum())
        assert table.delete_keypoints_from_lod(1) == int(((before.lod == 1) & (before.image_id != 12)).sum())
        left = ~region & (before.image_id != 12) & (before.lod != 1)
        assert np.array_equal(table.ids(), before.ids[left]) and len(table) == int(left.sum()) > 0
        _assert_same(Snapshot(pkg, table), _without_columns(before.keep(left)), "front")
    finally:
        table.close()


def _without_columns(snap):
    snap.image_id = snap.lod = None
    return snap
