"""Host-side mirror of the keypoint part of the reference crate `feature_database`
(/root/reference/feature_database/src/keypointdb.rs, models.rs) on a GPU-resident table instead of Postgres.
The table is what fills the descriptor database the matcher scans; a selection is directly usable as a train set."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import DMATCH_DTYPE, KEYPOINT_DTYPE, check, lib, ptr

OPENCV_KEYPOINT_LIMIT = 2 ** 18 - 1     # keypointdb.rs:12


class KeypointRows:
    """What `Vec<models::Keypoint>` holds (models.rs:27-41), column-wise."""

    def __init__(self, ids, keypoints, descriptors, image_ids):
        self.ids, self.keypoints, self.descriptors, self.image_ids = ids, keypoints, descriptors, image_ids

    def __len__(self):
        return len(self.ids)


class KeypointTable:
    """descriptor: "mldb" (a byte table: 61-byte M-LDB descriptors in 64-byte rows) or "kaze" (a float table: M-SURF rows of 64 floats, the
    L2 matcher's input). Every method serves both kinds; descriptors go in and come out as uint8 [n, 61] or float32 [n, 64]."""

    def __init__(self, capacity, descriptor="mldb"):
        if descriptor not in _lib.AKAZE_DESCRIPTORS:
            raise _lib.ApdsError(_lib.ERR_BAD_ARG, f"unknown descriptor {descriptor!r}: 'mldb' or 'kaze'")
        self.descriptor = descriptor
        self.is_float = descriptor == "kaze"
        self._h = C.c_void_p()
        check((lib().apds_db_create_float if self.is_float else lib().apds_db_create)(C.byref(self._h), int(capacity)))

    def _empty_descriptors(self, n):
        return np.zeros((n, _lib.DESC_FLOAT_DIM), np.float32) if self.is_float else np.zeros((n, 61), np.uint8)

    def close(self):
        if self._h:
            lib().apds_db_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(lib().apds_db_rows(self._h))

    def create_keypoints(self, extracted, image_id, level_of_detail=0, column=0, row=0, tile_size=(0, 0)):
        """preprocessor/src/main.rs:296-324: insert every keypoint of one tile (`keypoints.to_db_type(image_id)` with x, y
        lifted to level-of-detail-0 pixels) — one INSERT ... VALUES in the reference (keypointdb.rs:100-109)."""
        kp = np.ascontiguousarray(extracted.keypoints, KEYPOINT_DTYPE)
        d = extracted.descriptors
        if self.is_float != (np.asarray(d).dtype == np.float32):     # (the library's own check, made before the array is converted)
            raise _lib.ApdsError(_lib.ERR_BAD_ARG, "a float table takes float32 descriptors (a 'kaze' extraction), a byte table uint8 ones")
        d = np.ascontiguousarray(d, np.float32 if self.is_float else np.uint8)
        insert = lib().apds_db_insert_image_float if self.is_float else lib().apds_db_insert_image
        check(insert(self._h, ptr(kp), ptr(d), len(kp), int(image_id), int(level_of_detail), int(column), int(row), int(tile_size[0]), int(tile_size[1])))

    def create_keypoints_device(self, kps_ptr, desc64_ptr, n, image_id, level_of_detail=0, column=0, row=0, tile_size=(0, 0), stream=None):
        """create_keypoints for rows that are already on the device: kps_ptr / desc64_ptr are what apds_dev_akaze_extract wrote (28-byte
        keypoints, 64-byte descriptor rows; on a float table what apds_dev_akaze_extract_float wrote: rows of 64 floats), `stream` the
        stream it was issued on (None: the calling thread's own). Same stored rows."""
        check(lib().apds_db_insert_dev(self._h, kps_ptr, desc64_ptr, int(n), int(image_id), int(level_of_detail), int(column), int(row),
                                       int(tile_size[0]), int(tile_size[1]), stream))

    def world_coordinates(self, elevation_table, elevation_dev_ptr=None):
        """The world point (ElevationTable.get_world_coordinates_batch's arithmetic on float64(x), float64(y)) of every row, into the
        table's own xyz column on the device. Returns n_missing: the rows whose elevation lookup missed the raster (three NaNs each; no
        exception). elevation_dev_ptr: the elevation raster (float64, the shape of elevation_table.elevation) already on the device."""
        dgt = elevation_table.transforms["dataset"]
        el = elevation_table.elevation
        egt = elevation_table.transforms.get("elevation") if el is not None else None
        miss = C.c_int64(0)
        if egt is None:
            check(lib().apds_db_world_coordinates(self._h, ptr(dgt), None, None, 0, 0, 0, C.byref(miss)))
        elif elevation_dev_ptr is not None:
            check(lib().apds_db_world_coordinates(self._h, ptr(dgt), ptr(egt), elevation_dev_ptr, el.shape[1], el.shape[0], 1, C.byref(miss)))
        else:
            check(lib().apds_db_world_coordinates(self._h, ptr(dgt), ptr(egt), ptr(el), el.shape[1], el.shape[0], 0, C.byref(miss)))
        return miss.value

    def device_table(self):
        """(rows64, kps, xyz, n): device pointers of the WHOLE table in the layout a pipeline takes (descriptor rows, 28-byte keypoints,
        world points; all indexed by table row: ids()[row] is its id, row + 1 until the first delete). xyz is None unless
        world_coordinates() has run since the last insert; a delete keeps it current. The pointers hold until the next insert, delete or
        close()."""
        r, k, x, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64(0)
        check(lib().apds_db_table(self._h, C.byref(r), C.byref(k), C.byref(x), C.byref(n)))
        return r.value, k.value, x.value, n.value

    def _select(self, mode, value, box=(0, 0, 0, 0)):
        n = C.c_int(0)
        check(lib().apds_db_select(self._h, mode, int(value), float(box[0]), float(box[1]), float(box[2]), float(box[3]), C.byref(n)))
        m = n.value
        kp = np.zeros(m, KEYPOINT_DTYPE)
        d = self._empty_descriptors(m)
        ids = np.zeros(m, np.int32)
        img = np.zeros(m, np.int32)
        if m:
            download = lib().apds_db_view_download_float if self.is_float else lib().apds_db_view_download
            check(download(self._h, ptr(kp), ptr(d), ptr(ids), ptr(img)))
        return KeypointRows(ids, kp, d, img)

    def read_keypoints_from_image_id(self, image_id):
        """keypointdb.rs:38-48"""
        return self._select(0, image_id)

    def read_keypoints_from_lod(self, level_of_detail):
        """keypointdb.rs:50-65"""
        return self._select(1, level_of_detail)

    def read_keypoints_from_coordinates(self, x_start, y_start, x_end, y_end, level_of_detail):
        """keypointdb.rs:67-90"""
        return self._select(2, level_of_detail, (x_start, y_start, x_end, y_end))

    def read_keypoint_from_id(self, id):
        """keypointdb.rs:28-36 -> KeypointRows of one row (ids, keypoints, descriptors, image_ids of length 1). Raises
        ApdsError(ERR_OUT_OF_RANGE) where the reference returns Err(NotFound): an id that was deleted or never given."""
        kp = np.zeros(1, KEYPOINT_DTYPE)
        d = self._empty_descriptors(1)
        img = C.c_int(0)
        read = lib().apds_db_read_keypoint_from_id_float if self.is_float else lib().apds_db_read_keypoint_from_id
        check(read(self._h, int(id), ptr(kp), ptr(d), C.byref(img), None))
        return KeypointRows(np.array([id], np.int32), kp, d, np.array([img.value], np.int32))

    def ids(self):
        """The id of every row, by row (int32): row + 1 until the first delete, the reference's SERIAL values ever after."""
        out = np.zeros(len(self), np.int32)
        if len(out):
            p = C.c_void_p()
            check(lib().apds_db_ids(self._h, C.byref(p)))
            check(lib().apds_dev_download(ptr(out), p, out.nbytes, None))
        return out

    def _delete_where(self, mode, value, box=(0, 0, 0, 0)):
        n = C.c_int64(0)
        check(lib().apds_db_delete_where(self._h, mode, int(value), float(box[0]), float(box[1]), float(box[2]), float(box[3]), C.byref(n)))
        return n.value

    def delete_keypoints(self, ids):
        """keypointdb.rs:92-97 for a list of ids at once -> the number of rows deleted. Unknown ids delete nothing (the reference's
        Ok(())), duplicates count once. The surviving rows close up on the device in insertion order and keep their ids; device pointers,
        the last selection and earlier row ids are void after a delete that removed a row."""
        a = np.ascontiguousarray(ids, np.int32).reshape(-1)
        n = C.c_int64(0)
        check(lib().apds_db_delete_ids(self._h, ptr(a), len(a), C.byref(n)))
        return n.value

    def delete_keypoint(self, id):
        """keypointdb.rs:92-97"""
        return self.delete_keypoints([id])

    def delete_keypoints_from_image_id(self, image_id):
        """Every row read_keypoints_from_image_id qualifies (no 262143 limit) -> the number of rows deleted."""
        return self._delete_where(0, image_id)

    def delete_keypoints_from_lod(self, level_of_detail):
        """Every row read_keypoints_from_lod qualifies."""
        return self._delete_where(1, level_of_detail)

    def delete_keypoints_from_coordinates(self, x_start, y_start, x_end, y_end, level_of_detail):
        """Every row read_keypoints_from_coordinates qualifies (floor(start) <= v <= ceil(end))."""
        return self._delete_where(2, level_of_detail, (x_start, y_start, x_end, y_end))

    def view_device_pointers(self):
        """(rows64, keypoints, row_ids, image_ids, n): device pointers of the last selection (a ready train set)."""
        r, k, i, g, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(0)
        check(lib().apds_db_view(self._h, C.byref(r), C.byref(k), C.byref(i), C.byref(g), C.byref(n)))
        return r.value, k.value, i.value, g.value, n.value

    def view(self, capacity=None):
        """A TableView of this table: a selection object of its own (buffers and scratch allocated here), for reads that repeat per
        frame on a stream of the caller's. capacity None: min(262143, the table's capacity) rows."""
        return TableView(self, capacity)

    def knn_match_view(self, query_desc, k=2):
        """BFMatcher.knnMatch of host query descriptors against the last selection, which stays resident on the device. A float table:
        NORM_L2 on float32 [n, 64] queries, k 1 or 2, distances float32."""
        if self.is_float:
            q = np.ascontiguousarray(query_desc, np.float32).reshape(-1, _lib.DESC_FLOAT_DIM)
            idx = np.zeros((q.shape[0], k), np.int32)
            dist = np.zeros((q.shape[0], k), np.float32)
            check(lib().apds_db_l2_knn_match(self._h, ptr(q), q.shape[0], int(k), ptr(idx), ptr(dist)))
            return idx, dist
        q = np.ascontiguousarray(query_desc, np.uint8)
        idx = np.zeros((q.shape[0], k), np.int32)
        dist = np.zeros((q.shape[0], k), np.int32)
        check(lib().apds_db_knn_match(self._h, ptr(q), q.shape[0], q.shape[1], int(k), ptr(idx), ptr(dist)))
        return idx, dist


class TableView:
    """keypointdb.rs:50-90 as a per-frame read: the selection of KeypointTable.read_keypoints_from_* (same rows, same order: response
    descending, ties by table row, at most `capacity` rows), left on the device, on the caller's stream, with one host synchronisation.
    Any number of views of one table select concurrently from different threads on different streams; none touches the table's own
    last selection. The table must outlive the view and receive no inserts while a select is in flight."""

    def __init__(self, table, capacity=None):
        self._table = table     # keeps the table alive
        self._h = C.c_void_p()
        check(lib().apds_db_view_create(table._h, int(capacity) if capacity else 0, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().apds_db_view_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _select(self, mode, value, box, with_xyz, stream):
        n = C.c_int(0)
        check(lib().apds_db_view_select(self._h, mode, int(value), float(box[0]), float(box[1]), float(box[2]), float(box[3]), 1 if with_xyz else 0,
                                        stream, C.byref(n)))
        return n.value

    def read_keypoints_from_image_id(self, image_id, with_xyz=False, stream=None):
        """keypointdb.rs:38-48 -> the number of rows now in the view"""
        return self._select(0, image_id, (0, 0, 0, 0), with_xyz, stream)

    def read_keypoints_from_lod(self, level_of_detail, with_xyz=False, stream=None):
        """keypointdb.rs:50-65"""
        return self._select(1, level_of_detail, (0, 0, 0, 0), with_xyz, stream)

    def read_keypoints_from_coordinates(self, x_start, y_start, x_end, y_end, level_of_detail, with_xyz=False, stream=None):
        """keypointdb.rs:67-90"""
        return self._select(2, level_of_detail, (x_start, y_start, x_end, y_end), with_xyz, stream)

    def device_pointers(self):
        """(rows64, keypoints, row_ids, image_ids, xyz, n): device pointers of the last selection; xyz is None unless it ran with_xyz.
        Complete once the stream the selection ran on has finished."""
        r, k, i, g, x, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(0)
        check(lib().apds_db_view_pointers(self._h, C.byref(r), C.byref(k), C.byref(i), C.byref(g), C.byref(x), C.byref(n)))
        return r.value, k.value, i.value, g.value, x.value, n.value

    def l2_train(self):
        """A float table's view: the handle of the L2 train set over the last selection (apds_db_view_l2_train), as a c_void_p for
        apds_dev_l2_train_top2 / apds_l2_train_info. Borrowed: it lives as long as the view and follows every select; never destroy it."""
        h = C.c_void_p()
        check(lib().apds_db_view_l2_train(self._h, C.byref(h)))
        return h


class ElevationTable:
    """The `geotransform` and `elevation` tables of feature_database/src/elevationdb.rs (create_geotransform :20-45,
    add_elevation_data :196-232, get_world_coordinates :64-104) held in memory; the conversion runs on the GPU."""

    def __init__(self):
        self.transforms = {}
        self.elevation = None

    def create_geotransform(self, dataset_name, transform):
        """elevationdb.rs:20-45 — `transform`: GDAL's six coefficients."""
        t = np.ascontiguousarray(transform, np.float64)
        if t.shape != (6,):
            raise ValueError("a geotransform has six coefficients")
        self.transforms[dataset_name] = t

    def add_elevation_data(self, raster):
        """elevationdb.rs:196-232 — heights row by row (ids are 1-based row-major positions)."""
        self.elevation = np.ascontiguousarray(raster, np.float64)
        if self.elevation.ndim != 2:
            raise ValueError("elevation raster: H x W")

    def get_world_coordinates_batch(self, xy):
        """elevationdb.rs:64-104 for n pixel positions at once -> n x 3 ECEF metres. Raises ApdsError(ERR_OUT_OF_RANGE) where the
        reference returns Err (a lookup outside the elevation table)."""
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        out = np.zeros((len(xy), 3), np.float64)
        dgt = self.transforms["dataset"]
        egt = self.transforms.get("elevation") if self.elevation is not None else None
        if egt is None:
            check(lib().apds_get_world_coordinates(ptr(xy), len(xy), ptr(dgt), None, None, 0, 0, ptr(out)))
        else:
            check(lib().apds_get_world_coordinates(ptr(xy), len(xy), ptr(dgt), ptr(egt), ptr(self.elevation), self.elevation.shape[1],
                                                   self.elevation.shape[0], ptr(out)))
        return out

    def get_world_coordinates(self, x, y):
        """elevationdb.rs:64 — one point, (x, y, z) as the reference returns it."""
        return tuple(self.get_world_coordinates_batch([[x, y]])[0])
