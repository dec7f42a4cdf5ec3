"""Host copies of a keypoint table for the delete tests: what apds_db_table and apds_db_ids point at, downloaded by row, with the two
columns no pointer exposes (image id, level of detail) rebuilt from the row ids of one select per value."""
import ctypes as C

import numpy as np


def download(pkg, addr, shape, dtype):
    out = np.zeros(shape, dtype)
    if out.nbytes:
        pkg._lib.check(pkg.lib().apds_dev_download(pkg._lib.ptr(out), addr, out.nbytes, None))
    return out


class Snapshot:
    """host copy of a table: descriptor rows, keypoints, world points and ids by row, through apds_db_table and apds_db_ids"""

    def __init__(self, pkg, table, image_ids=None, lods=None):
        rows64, kps, xyz, n = table.device_table()
        assert n == len(table)
        self.n = n
        self.desc = download(pkg, rows64, (n, 64), np.uint8)
        self.kps = download(pkg, kps, n, pkg._lib.KEYPOINT_DTYPE)
        self.xyz = download(pkg, xyz, (n, 3), np.float64) if xyz else None
        self.ids = table.ids()
        self.image_id = self._column(pkg, table, 0, image_ids, True) if image_ids is not None else None
        self.lod = self._column(pkg, table, 1, lods, False) if lods is not None else None

    def _column(self, pkg, table, mode, values, check_image_ids):
        """the column a select of `mode` reads, rebuilt from the row ids of one select per value (each below the 262143-row limit)"""
        col = np.full(self.n, -1, np.int32)
        for v in values:
            m = C.c_int(0)
            pkg._lib.check(pkg.lib().apds_db_select(table._h, mode, int(v), 0.0, 0.0, 0.0, 0.0, C.byref(m)))
            assert m.value < 262143
            _, _, rows, img, m2 = table.view_device_pointers()
            assert m2 == m.value
            r = download(pkg, rows, m2, np.int32)
            assert (col[r] == -1).all()
            col[r] = v
            if check_image_ids:
                assert (download(pkg, img, m2, np.int32) == v).all()
        return col

    def keep(self, mask):
        out = object.__new__(Snapshot)
        out.n = int(mask.sum())
        for name in ("desc", "kps", "xyz", "ids", "image_id", "lod"):
            a = getattr(self, name)
            setattr(out, name, None if a is None else a[mask])
        return out


def assert_same(got, want, what=""):
    assert got.n == want.n, (what, got.n, want.n)
    for name in ("desc", "kps", "xyz", "ids", "image_id", "lod"):
        a, b = getattr(got, name), getattr(want, name)
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name)
    assert not got.desc[:, 61:].any(), what
