"""CPU: the float keypoint table's entries (include/apds.h: apds_db_create_float and its twins) are exported and bound, and each rejects
null arguments with APDS_ERR_BAD_ARG before any device work (no GPU here: a call that reached the device would report -216 instead)."""
import ctypes as C

import numpy as np

NEW = ["apds_db_create_float", "apds_db_info", "apds_db_insert_image_float", "apds_db_view_download_float", "apds_db_read_keypoint_from_id_float",
       "apds_db_view_l2_train", "apds_db_l2_knn_match"]


def test_new_symbols_are_exported_and_bound(pkg):
    L = pkg.lib()
    for name in NEW:
        assert name in pkg._lib.SYMBOLS, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name


def test_null_arguments_are_rejected_before_device_work(pkg):
    L, BAD = pkg.lib(), pkg._lib.ERR_BAD_ARG
    ptr = pkg._lib.ptr
    h, n, m = C.c_void_p(), C.c_int(0), C.c_int(0)
    kp = np.zeros(4, pkg._lib.KEYPOINT_DTYPE)
    d = np.zeros((4, 64), np.float32)
    idx, dist = np.zeros((4, 2), np.int32), np.zeros((4, 2), np.float32)
    assert L.apds_db_create_float(None, 16) == BAD
    assert L.apds_db_create_float(C.byref(h), 0) == BAD and not h.value
    assert L.apds_db_create_float(C.byref(h), 2 ** 31) == BAD and not h.value
    assert L.apds_db_info(None, C.byref(n), C.byref(m)) == BAD
    assert L.apds_db_insert_image_float(None, ptr(kp), ptr(d), 4, 1, 0, 0, 0, 0, 0) == BAD
    assert L.apds_db_view_download_float(None, ptr(kp), ptr(d), None, None) == BAD
    assert L.apds_db_read_keypoint_from_id_float(None, 1, ptr(kp), ptr(d), None, None) == BAD
    assert L.apds_db_view_l2_train(None, C.byref(h)) == BAD and not h.value
    assert L.apds_db_l2_knn_match(None, ptr(d), 4, 2, ptr(idx), ptr(dist)) == BAD
    # null outputs and inputs beside a non-null handle: every one of these checks comes before the handle is read (a dummy address is enough)
    dummy = C.cast(C.create_string_buffer(4096), C.c_void_p)
    assert L.apds_db_view_l2_train(dummy, None) == BAD
    assert L.apds_db_l2_knn_match(dummy, ptr(d), 4, 2, None, ptr(dist)) == BAD
    assert L.apds_db_l2_knn_match(dummy, ptr(d), 4, 2, ptr(idx), None) == BAD
    assert L.apds_db_l2_knn_match(dummy, None, 4, 2, ptr(idx), ptr(dist)) == BAD
    assert L.apds_db_l2_knn_match(dummy, ptr(d), -1, 2, ptr(idx), ptr(dist)) == BAD
    assert L.apds_db_create_float(None, 0) == BAD
    assert b"null" in L.apds_last_error().lower() or b"bad" in L.apds_last_error().lower()


def test_python_front_rejects_an_unknown_descriptor(pkg):
    import pytest
    with pytest.raises(pkg.ApdsError) as e:
        pkg.feature_database.KeypointTable(16, descriptor="sift")
    assert e.value.code == pkg._lib.ERR_BAD_ARG
