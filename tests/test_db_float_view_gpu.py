"""GPU: selections and views of a FLOAT keypoint table (apds_db_create_float; csrc/keypoint_select.hip) and the L2 train side a float view's
gather writes beside the rows (apds_db_view_l2_train).

Rows are inserted with apds_db_insert_image_float from numpy. The expected selection is db_float_cases.Model: the predicate of
keypointdb.rs:50-90, response descending (-0.0 == +0.0), row ascending, the limit. A byte table with the same keypoints goes through the same
selections: rows, keypoints, row ids and image ids of the two kinds must agree bit for bit, and with the model.

Sizes: tables of 0, 1, 1023, 1024, 1025 and 2049 rows (TB = 1024 rows per ranking block); selections of 0, 1, 2, 3, 4, 5 (a 256-thread
block of the gather serves four float rows, one wave each), 127, 128, 129 (SC_TM = 128 train rows per tile of the screen) and 1025 rows; a
view of capacity 5 cut inside a run of tied responses. Queries: 1, 383, 384, 385 unit rows (a block of the screen holds 384).

The train side is held to three things, all bit for bit: apds_dev_l2_train_top2 on the view's handle in both modes equals apds_dev_l2_topk
with the exact kernel over the view's rows; it equals a handle apds_l2_train_create makes over the same rows; and in screen mode the
candidates per query equal that fresh handle's - the count depends on the largest norm, so a norm left over from an earlier selection
would show there (level of detail 0 holds rows of norm 3, level 1 rows of norm 0.5, selected in that order on one view)."""
import ctypes as C
import threading

import numpy as np
import pytest

import db_float_cases as cases
from db_float_cases import LIMIT, Model, bits, select

pytestmark = pytest.mark.gpu

NQS = [1, 383, 384, 385]
SEL_COUNTS = {10: 0, 11: 1, 12: 2, 13: 3, 14: 4, 15: 5, 16: 127, 17: 128, 18: 129, 19: 1025}     # image id -> rows of that image


@pytest.fixture(scope="module")
def dev(gpu_pkg):
    return cases.Dev(gpu_pkg)


@pytest.fixture(scope="module")
def queries(dev):
    return dev.up(cases.unit_rows(max(NQS), 0xF10A7))


def model_of(pkg, img, lod, seed, norms=None):
    n = len(img)
    desc = cases.unit_rows(n, seed + 1)
    if norms is not None:
        desc = np.ascontiguousarray(desc * np.asarray(norms, np.float32)[:, None])
    return Model(cases.keypoints(pkg, n, seed), np.asarray(img), np.asarray(lod), desc, cases.byte_rows(n, seed + 2))


@pytest.fixture(scope="module")
def big(gpu_pkg):
    """2049 rows: the images of SEL_COUNTS with their rows scattered over the table, the rest image 1; level of detail = row parity"""
    n = 2049
    img = np.ones(n, np.int64)
    pos = np.random.default_rng(7).permutation(n)
    at = 0
    for image_id, m in SEL_COUNTS.items():
        img[pos[at:at + m]] = image_id
        at += m
    lod = np.arange(n) % 2
    norms = np.where(lod == 0, 3.0, 0.5)
    model = model_of(gpu_pkg, img, lod, 100, norms)
    tf, tb = cases.make_tables(gpu_pkg, model)
    yield model, tf, tb
    tf.close()
    tb.close()


def check_train_side(dev, view, n, queries, nqs=NQS):
    """the view's train handle against the exact kernel over the view's rows and against a fresh handle over the same rows"""
    rows = dev.view_rows(view)
    assert rows.shape[0] == n
    ts = dev.pl.L2TrainSet.of_view(view)
    assert ts.info() == (n, 64, n >= 2)
    fresh = dev.pl.L2TrainSet(rows)
    try:
        want_all = dev.topk(queries, rows)
        for nq in nqs:
            q, want = queries[:nq], want_all[:nq]
            for mode in ("screen", "exact"):
                got, used, cpq = dev.top2(ts, q, mode)
                ref, ref_used, ref_cpq = dev.top2(fresh, q, mode)
                assert used == ref_used == ("screen" if mode == "screen" and n >= 2 else "exact"), (n, nq, mode, used, ref_used)
                assert np.array_equal(got, want), (n, nq, mode, np.flatnonzero((got != want).any(1))[:8])
                assert np.array_equal(ref, want), (n, nq, mode)
                if used == "screen":
                    assert cpq == ref_cpq, (n, nq, cpq, ref_cpq)
    finally:
        fresh.close()
        ts.close()


# ---- the kind of a table ---------------------------------------------------------------------------------------------------------------
def test_info_reports_the_kind(gpu_pkg):
    pkg, L = gpu_pkg, gpu_pkg.lib()
    for descriptor, want in (("kaze", (pkg._lib.AKAZE_DESCRIPTOR_KAZE, 256)), ("mldb", (pkg._lib.AKAZE_DESCRIPTOR_MLDB, 64))):
        t = pkg.feature_database.KeypointTable(8, descriptor=descriptor)
        try:
            d, b = C.c_int(0), C.c_int(0)
            pkg._lib.check(L.apds_db_info(t._h, C.byref(d), C.byref(b)))
            assert (d.value, b.value) == want
        finally:
            t.close()


# ---- table sizes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 2049])
def test_table_sizes(gpu_pkg, dev, queries, n):
    """the rows of level 0 (runs of seven rows, alternating) out of n rows, then every row of image 1 (all of them), then none"""
    pkg = gpu_pkg
    model = model_of(pkg, np.ones(n, np.int64), (np.arange(n) // 7) % 2, 200 + n)
    tf, tb = cases.make_tables(pkg, model)
    vf, vb = tf.view(), tb.view()
    try:
        for mode, value in ((1, 0), (0, 1), (1, 5)):
            want = model.select(mode, value)
            nf, nb = select(vf, mode, value, stream=dev.handle()), select(vb, mode, value, stream=dev.handle())
            cases.check_views(pkg, model, vf, vb, nf, nb, want, dev.handle())
            check_train_side(dev, vf, nf, queries, [385])
            old = tf.read_keypoints_from_lod(value) if mode == 1 else tf.read_keypoints_from_image_id(value)      # the table's own view
            assert np.array_equal(old.ids, model.ids[want]) and np.array_equal(bits(old.keypoints), bits(model.kp[want]))
            assert old.descriptors.dtype == np.float32 and np.array_equal(bits(old.descriptors), bits(model.desc_f[want]))
            assert np.array_equal(old.image_ids, model.img[want])
    finally:
        vf.close()
        vb.close()
        tf.close()
        tb.close()


# ---- selection sizes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image_id", sorted(SEL_COUNTS))
def test_selection_sizes(big, dev, queries, image_id):
    model, tf, tb = big
    want = model.select(0, image_id)
    assert len(want) == SEL_COUNTS[image_id]
    vf, vb = tf.view(), tb.view()
    try:
        nf, nb = select(vf, 0, image_id, stream=dev.handle()), select(vb, 0, image_id, stream=dev.handle())
        cases.check_views(dev.pkg, model, vf, vb, nf, nb, want, dev.handle())
        check_train_side(dev, vf, nf, queries)
    finally:
        vf.close()
        vb.close()


def test_bounding_box_selection(big, dev, queries):
    model, tf, tb = big
    box = (10.3, 20.7, 250.2, 300.1)
    want = model.select(2, 0, box)
    assert 100 < len(want) < int((model.lod == 0).sum())
    vf, vb = tf.view(), tb.view()
    try:
        nf = select(vf, 2, 0, box, stream=dev.handle())
        nb = select(vb, 2, 0, box, stream=dev.handle())
        cases.check_views(dev.pkg, model, vf, vb, nf, nb, want, dev.handle())
        check_train_side(dev, vf, nf, queries, [385])
    finally:
        vf.close()
        vb.close()


def test_capacity_five_cut_inside_ties(gpu_pkg, dev, queries):
    """40 rows, responses 1.0 x 3 then 0.5 x 30 then lower: a view of 5 rows takes the three and the two LOWEST ROWS of the tied run"""
    pkg = gpu_pkg
    model = model_of(pkg, np.ones(40, np.int64), np.zeros(40, np.int64), 300)
    resp = np.concatenate([np.full(3, 1.0), np.full(30, 0.5), np.arange(7) / 64]).astype(np.float32)
    perm = np.random.default_rng(301).permutation(40)
    model.kp["response"] = model.src_kp["response"] = resp[perm]
    tf, tb = cases.make_tables(pkg, model)
    vf, vb = tf.view(5), tb.view(5)
    try:
        want = model.select(1, 0, limit=5)
        tied = np.sort(np.flatnonzero(model.kp["response"] == 0.5))
        assert len(want) == 5 and np.array_equal(want[3:], tied[:2])
        nf, nb = select(vf, 1, 0, stream=dev.handle()), select(vb, 1, 0, stream=dev.handle())
        cases.check_views(pkg, model, vf, vb, nf, nb, want, dev.handle())
        check_train_side(dev, vf, nf, queries, [1, 385])
    finally:
        vf.close()
        vb.close()
        tf.close()
        tb.close()


# ---- the largest norm follows the selection --------------------------------------------------------------------------------------------
def test_largest_norm_is_not_left_over(big, dev, queries):
    """level 0 (norm 3), then level 1 (norm 0.5), then one row, then level 1 again on ONE view: the screen's candidate counts are a fresh handle's"""
    model, tf, _ = big
    vf = tf.view()
    try:
        for mode, value in ((1, 0), (1, 1), (0, 11), (1, 1), (0, 10), (1, 0)):
            want = model.select(mode, value)
            n = select(vf, mode, value, stream=dev.handle())
            assert n == len(want)
            check_train_side(dev, vf, n, queries, [384])
    finally:
        vf.close()


# ---- knn on the table's current view ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image_id", [10, 11, 12, 19])
def test_db_l2_knn_match_equals_l2_knn_match(gpu_pkg, big, image_id):
    pkg = gpu_pkg
    model, tf, tb = big
    rows = tf.read_keypoints_from_image_id(image_id)
    q = cases.unit_rows(37, 400 + image_id)
    L, ptr = pkg.lib(), pkg._lib.ptr
    for k in (1, 2):
        idx, dist = tf.knn_match_view(q, k)
        widx, wdist = np.zeros((37, k), np.int32), np.zeros((37, k), np.float32)
        t = np.ascontiguousarray(rows.descriptors, np.float32)
        pkg._lib.check(L.apds_l2_knn_match(ptr(q), 37, ptr(t), len(t), 64, k, ptr(widx), ptr(wdist)))
        assert np.array_equal(idx, widx) and np.array_equal(bits(dist), bits(wdist)), (image_id, k)
    # the byte-typed matcher on a float table, the float-typed one on a byte table
    idx, d32 = np.zeros((37, 2), np.int32), np.zeros((37, 2), np.int32)
    q8 = np.zeros((37, 61), np.uint8)
    assert L.apds_db_knn_match(tf._h, ptr(q8), 37, 61, 2, ptr(idx), ptr(d32)) == pkg._lib.ERR_BAD_ARG
    assert L.apds_db_l2_knn_match(tb._h, ptr(q), 37, 2, ptr(idx), ptr(d32)) == pkg._lib.ERR_BAD_ARG
    h = C.c_void_p()
    assert L.apds_db_shard(tf._h, 0, 1, pkg._lib.TRANSPORT_LOOPBACK, None, None, C.byref(h)) == pkg._lib.ERR_BAD_ARG and not h.value
    vb = tb.view(8)
    try:
        assert L.apds_db_view_l2_train(vb._h, C.byref(h)) == pkg._lib.ERR_BAD_ARG and not h.value
    finally:
        vb.close()


# ---- independence and memory -----------------------------------------------------------------------------------------------------------
def test_two_views_two_threads_two_streams(big, dev, queries):
    model, tf, _ = big
    pkg, L = dev.pkg, dev.L
    jobs = [(1, 0), (0, 19)]
    views = [tf.view() for _ in jobs]
    streams = []
    for _ in jobs:
        s = C.c_void_p()
        pkg._lib.check(L.apds_stream_create(0, None, 0, C.byref(s)))
        streams.append(s)
    q = queries[:385]
    got, errors = [None, None], []

    def work(i):
        try:
            keys = dev.torch.empty((385, 2), dtype=dev.torch.int64, device="cuda:0")
            h = views[i].l2_train()
            for _ in range(5):
                n = select(views[i], jobs[i][0], jobs[i][1], stream=streams[i])
                used = C.c_int(-1)
                pkg._lib.check(L.apds_dev_l2_train_top2(h, q.data_ptr(), 385, cases.SCREEN, keys.data_ptr(), streams[i], C.byref(used), None))
                pkg._lib.check(L.apds_stream_synchronize(streams[i]))
                got[i] = (n, cases.download_view(pkg, views[i], 256, streams[i]), keys.cpu().numpy(), used.value)
        except Exception as e:   # noqa: BLE001
            errors.append(e)
        finally:
            L.apds_thread_release()

    try:
        threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        for i, (mode, value) in enumerate(jobs):       # the single-threaded results: the model, and the exact kernel over the view's rows
            want = model.select(mode, value)
            n, (rows, kp, d, img), keys, used = got[i]
            assert n == len(want) and np.array_equal(rows, want) and np.array_equal(bits(kp), bits(model.kp[want]))
            assert np.array_equal(d, bits(model.desc_f[want]).reshape(n, 256)) and np.array_equal(img, model.img[want])
            assert used == cases.SCREEN and np.array_equal(keys, dev.topk(q, dev.up(model.desc_f[want])))
    finally:
        for v in views:
            v.close()
        for s in streams:
            L.apds_stream_destroy(s)


def test_fifty_selects_grow_nothing(big, dev):
    model, tf, _ = big
    torch, pkg = dev.torch, dev.pkg
    vf = tf.view()
    try:
        jobs = [(1, 0), (0, 19), (0, 10), (0, 11), (1, 1)]
        for mode, value in jobs:
            select(vf, mode, value, stream=dev.handle())
        torch.cuda.synchronize()
        ws, free, live = pkg._lib.workspace_info(), torch.cuda.mem_get_info()[0], dev.L.apds_live_contexts()
        for i in range(50):
            mode, value = jobs[i % len(jobs)]
            assert select(vf, mode, value, stream=dev.handle()) == len(model.select(mode, value))
        torch.cuda.synchronize()
        assert pkg._lib.workspace_info() == ws and torch.cuda.mem_get_info()[0] == free and dev.L.apds_live_contexts() == live
    finally:
        vf.close()
