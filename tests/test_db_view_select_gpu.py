"""GPU: apds_db_view_select (csrc/keypoint_select.hip, the view objects) - the read of keypointdb.rs:50-90 on a view object, on the caller's
stream. Every result is compared bit for bit with a numpy reference written from the definition (a predicate, a stable sort on
(-response with -0.0 -> +0.0, row), a cut); wherever the limits are equal, apds_db_select + apds_db_view_download - the other front of
the same selection engine - is held to the same numpy reference. Tables are built with apds_db_insert_image from synthetic rows; nothing is extracted.

The borders: 0, 1, 2 qualifying rows; capacity - 1, capacity, capacity + 1 (the radix cut starts at capacity + 1); the LDS sort block
SORT_B = 2048 keys: B - 1, B, B + 1, 2B + 1 (one block, two blocks, a global merge step); a capacity that is no power of two; the cut inside
a run of equal responses (row order decides; with the rows inside one 256-row block that is the LAST radix byte), and inside responses that
differ in their low mantissa bits only; -0.0 / +0.0 / infinities / denormals; the floor / ceil edges of the bounding box."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SORT_B = 2048          # csrc/keypoint_select.hip
CAP = 3000             # a view capacity that is no power of two
LIMIT = 2 ** 18 - 1    # keypointdb.rs:12


class _Ex:
    def __init__(self, kp, d):
        self.keypoints, self.descriptors = kp, d


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _keypoints(pkg, n, seed):
    rng = np.random.default_rng(seed)
    kp = np.zeros(n, pkg._lib.KEYPOINT_DTYPE)
    kp["x"], kp["y"] = rng.integers(0, 400, n), rng.integers(0, 400, n)
    kp["size"], kp["angle"] = rng.random(n, np.float32) * 9, rng.random(n, np.float32) * 360
    kp["response"] = np.round(rng.random(n, np.float32) * 64) / 64          # 65 levels: ties everywhere
    kp["octave"], kp["class_id"] = rng.integers(0, 4, n), rng.integers(0, 3, n)
    return kp


def reference(resp, mask, limit):
    """table rows of the selection: the predicate, ORDER BY response DESC (-0.0 == +0.0), ties by row, LIMIT"""
    rows = np.flatnonzero(mask)
    r = resp[rows].astype(np.float64)
    r[r == 0] = 0.0
    return rows[np.lexsort((rows, -r))][:limit]


class Table:
    """a table and the host copy of what it stores (coordinates lifted by 2^lod; tile column and row 0)"""

    def __init__(self, pkg, inserts, seed):
        self.pkg = pkg
        n = sum(len(kp) for _, _, kp in inserts)
        self.d = np.random.default_rng(seed).integers(0, 256, (n, 61), dtype=np.uint8)
        self.t = pkg.feature_database.KeypointTable(n)
        kps, imgs, lods, at = [], [], [], 0
        for image_id, lod, kp in inserts:
            self.t.create_keypoints(_Ex(kp, self.d[at:at + len(kp)]), image_id, lod)
            k = kp.copy()
            k["x"], k["y"] = kp["x"] * np.float32(2 ** lod), kp["y"] * np.float32(2 ** lod)
            kps.append(k); imgs.append(np.full(len(kp), image_id, np.int32)); lods.append(np.full(len(kp), lod, np.int32))
            at += len(kp)
        self.kp, self.img, self.lod = np.concatenate(kps), np.concatenate(imgs), np.concatenate(lods)

    def mask(self, mode, value, box=None):
        if mode == 0:
            return self.img == value
        m = self.lod == value
        if mode == 2:
            x0, y0, x1, y1 = np.floor(np.float32(box[0])), np.floor(np.float32(box[1])), np.ceil(np.float32(box[2])), np.ceil(np.float32(box[3]))
            m &= (self.kp["x"] >= x0) & (self.kp["x"] <= x1) & (self.kp["y"] >= y0) & (self.kp["y"] <= y1)
        return m


def download(pkg, view, stream=None):
    """(row ids, keypoints, 64-byte descriptor rows, image ids, xyz or None) of the view's last selection, ordered on `stream`"""
    r, k, i, g, x, n = view.device_pointers()
    out = [np.zeros(n, np.int32), np.zeros(n, pkg._lib.KEYPOINT_DTYPE), np.zeros((n, 64), np.uint8), np.zeros(n, np.int32),
           np.zeros((n, 3), np.float64) if x else None]
    for a, addr in zip(out, (i, k, r, g, x)):
        if a is not None:
            pkg._lib.check(pkg.lib().apds_dev_download(pkg._lib.ptr(a), addr, a.nbytes, stream))
    return out


def select(view, mode, value, box=None, **kw):
    if mode == 0:
        return view.read_keypoints_from_image_id(value, **kw)
    if mode == 1:
        return view.read_keypoints_from_lod(value, **kw)
    return view.read_keypoints_from_coordinates(box[0], box[1], box[2], box[3], value, **kw)


def check_view(tb, view, n, want, stream=None):
    rows, kp, d64, img, _ = download(tb.pkg, view, stream)
    assert n == len(want) == len(rows)
    assert np.array_equal(rows, want)
    assert np.array_equal(_bits(kp), _bits(tb.kp[want])) and np.array_equal(img, tb.img[want])
    assert np.array_equal(d64[:, :61], tb.d[want]) and not d64[:, 61:].any()


def check_old_path(tb, mode, value, box, want):
    """apds_db_select + apds_db_view_download on the same arguments (its limit is 262143: equal whenever nothing is cut)"""
    t = tb.t
    old = t.read_keypoints_from_image_id(value) if mode == 0 else t.read_keypoints_from_lod(value) if mode == 1 else \
        t.read_keypoints_from_coordinates(box[0], box[1], box[2], box[3], value)
    assert np.array_equal(old.ids - 1, want) and np.array_equal(_bits(old.keypoints), _bits(tb.kp[want]))
    assert np.array_equal(old.descriptors, tb.d[want]) and np.array_equal(old.image_ids, tb.img[want])


# ---- modes and the edges of the bounding box -------------------------------------------------------------------------------------------
BOX = (10.3, 20.7, 50.2, 60.1)      # floor -> 10, 20; ceil -> 51, 61


@pytest.fixture(scope="module")
def geo(gpu_pkg):
    a, b = _keypoints(gpu_pkg, 1800, 1), _keypoints(gpu_pkg, 1700, 2)
    for kp in (a, b):
        kp["x"], kp["y"] = kp["x"] / 4, kp["y"] / 4            # quarters of a pixel in [0, 100)
    edge = _keypoints(gpu_pkg, 16, 3)
    f = np.float32
    lo, hi = f(-np.inf), f(np.inf)
    edge["x"][:8] = [10, np.nextafter(f(10), lo), 51, np.nextafter(f(51), hi), 10, 51, 30, 30]
    edge["y"][:8] = [20, 40, 61, 40, np.nextafter(f(20), lo), np.nextafter(f(61), hi), 20, 61]
    edge["x"][8:], edge["y"][8:] = 30, 40
    tb = Table(gpu_pkg, [(1, 0, a), (2, 1, b), (3, 0, edge), (4, 1, _keypoints(gpu_pkg, 500, 4))], 10)
    yield tb
    tb.t.close()


@pytest.mark.parametrize("mode,value,box", [(0, 1, None), (0, 3, None), (0, 99, None), (1, 0, None), (1, 1, None), (1, 7, None), (2, 0, BOX),
                                            (2, 1, BOX), (2, 0, (10.0, 20.0, 51.0, 61.0)), (2, 0, (30.5, 40.5, 30.5, 40.5))])
def test_modes_against_reference_and_parent_path(geo, mode, value, box):
    want = reference(geo.kp["response"], geo.mask(mode, value, box), LIMIT)
    view = geo.t.view()
    try:
        check_view(geo, view, select(view, mode, value, box), want)
    finally:
        view.close()
    check_old_path(geo, mode, value, box, want)


def test_box_edges_are_inclusive_after_floor_and_ceil(geo):
    """the rows on floor(x_start), ceil(x_end), floor(y_start), ceil(y_end) are in, the rows one ulp outside are out"""
    base = int(np.flatnonzero(geo.img == 3)[0])
    got = set(reference(geo.kp["response"], geo.mask(2, 0, BOX), LIMIT).tolist())
    inside = {base + i for i in (0, 2, 6, 7)} | {base + i for i in range(8, 16)}
    outside = {base + i for i in (1, 3, 4, 5)}
    assert inside <= got and not (outside & got)


# ---- borders of the count --------------------------------------------------------------------------------------------------------------
COUNTS = {11: 1, 12: 2, 13: SORT_B - 1, 14: SORT_B, 15: SORT_B + 1, 16: 2 * SORT_B + 1, 17: CAP - 1, 18: CAP, 19: CAP + 1}
SPECIALS = np.array([-0.0, 0.0, np.inf, -np.inf, 1.4e-45, -1.4e-45, 1e-40, -1e-40, 1.17549435e-38, 1.0, -1.0, 3.4028235e38, -3.4028235e38, 0.0, -0.0, 0.5],
                    np.float32)


@pytest.fixture(scope="module")
def borders(gpu_pkg):
    inserts = []
    equal = _keypoints(gpu_pkg, 200, 20)            # rows 0 .. 199: one 256-row block, one response - the cut is decided by the last radix byte
    equal["response"] = 0.5
    inserts.append((1, 0, equal))
    low = _keypoints(gpu_pkg, 300, 21)              # responses that differ in the low mantissa bits only, in adjacent rows
    low["response"] = (np.uint32(0x3F000000) + np.random.default_rng(22).integers(0, 64, 300).astype(np.uint32)).view(np.float32)
    inserts.append((2, 0, low))
    spec = _keypoints(gpu_pkg, 64, 23)
    spec["response"] = np.random.default_rng(24).permutation(np.tile(SPECIALS, 4))
    inserts.append((3, 0, spec))
    run = _keypoints(gpu_pkg, 100, 25)              # 40 rows above, a run of 30 equal responses, 30 rows below - shuffled
    run["response"] = np.random.default_rng(26).permutation(np.concatenate([1 + np.arange(40) / 64, np.full(30, 0.25), np.arange(30) / 256]).astype(np.float32))
    inserts.append((4, 0, run))
    for image_id, m in COUNTS.items():
        inserts.append((image_id, 1, _keypoints(gpu_pkg, m, 100 + image_id)))
    tb = Table(gpu_pkg, inserts, 30)
    yield tb
    tb.t.close()


@pytest.mark.parametrize("image_id", [10] + sorted(COUNTS))
def test_count_borders(borders, image_id):
    """m = 0, 1, 2, B - 1, B, B + 1, 2B + 1, capacity - 1, capacity, capacity + 1 rows of one image into a view of CAP rows"""
    tb = borders
    mask = tb.mask(0, image_id)
    assert mask.sum() == COUNTS.get(image_id, 0)
    cap = CAP if mask.sum() <= CAP + 1 else 5000           # (2B + 1 rows: a larger capacity, still no power of two, nothing cut)
    want = reference(tb.kp["response"], mask, cap)
    view = tb.t.view(cap)
    try:
        check_view(tb, view, select(view, 0, image_id), want)
    finally:
        view.close()
    if mask.sum() <= cap:
        check_old_path(tb, 0, image_id, None, want)


@pytest.mark.parametrize("image_id,cap", [(1, 100), (1, 1), (1, 199), (2, 150), (2, 7), (3, 10), (3, 33), (3, 63), (4, 55), (4, 41), (4, 70)])
def test_cut_inside_ties_and_special_responses(borders, image_id, cap):
    """all responses equal; low-mantissa neighbours; -0.0 / +0.0 / inf / denormals; a run of equal responses across the cut"""
    tb = borders
    want = reference(tb.kp["response"], tb.mask(0, image_id), cap)
    assert len(want) == cap
    view = tb.t.view(cap)
    try:
        check_view(tb, view, select(view, 0, image_id), want)
    finally:
        view.close()


def test_special_responses_uncut_equal_parent_path(borders):
    tb = borders
    want = reference(tb.kp["response"], tb.mask(0, 3), LIMIT)
    z = tb.kp["response"][want]
    zeros = np.flatnonzero(z == 0)
    assert np.all(np.diff(want[zeros]) > 0) and np.signbit(z[zeros]).any() and not np.signbit(z[zeros]).all()     # -0.0 and +0.0 tie: row order
    view = tb.t.view()
    try:
        check_view(tb, view, select(view, 0, 3), want)
    finally:
        view.close()
    check_old_path(tb, 0, 3, None, want)


def test_level_of_detail_over_all_count_images_with_a_cut(borders):
    """mode 1 over every image of level 1 (~17 000 rows) into CAP rows: the cut, then a sort of more than one block"""
    tb = borders
    want = reference(tb.kp["response"], tb.mask(1, 1), CAP)
    view = tb.t.view(CAP)
    try:
        check_view(tb, view, select(view, 1, 1), want)
    finally:
        view.close()


# ---- the cut against the parent path ---------------------------------------------------------------------------------------------------
def test_full_limit_cut_equals_parent_path(gpu_pkg):
    """262143 + 300 rows of one level of detail, ties across the cut: the only size at which apds_db_select cuts"""
    m = LIMIT + 300
    kp = _keypoints(gpu_pkg, m, 40)
    kp["response"] = np.round(np.random.default_rng(41).random(m, np.float32) * 1000) / 1000
    tb = Table(gpu_pkg, [(1, 1, kp)], 42)
    try:
        want = reference(tb.kp["response"], tb.mask(1, 1), LIMIT)
        asc = np.sort(tb.kp["response"])
        assert len(want) == LIMIT and tb.kp["response"][want[-1]] == asc[300] == asc[299]      # the cut falls in a run of ties
        view = tb.t.view()
        try:
            check_view(tb, view, select(view, 1, 1), want)
        finally:
            view.close()
        check_old_path(tb, 1, 1, None, want)
    finally:
        tb.t.close()


# ---- independence ----------------------------------------------------------------------------------------------------------------------
def test_two_views_two_threads_two_streams(borders):
    tb, pkg = borders, borders.pkg
    L = pkg.lib()
    jobs = [(1, 1, CAP), (0, 16, 5000)]                   # (mode, value, capacity): a cut select and a two-block sort
    views = [tb.t.view(cap) for _, _, cap in jobs]
    streams = []
    for _ in jobs:
        s = C.c_void_p()
        pkg._lib.check(L.apds_stream_create(0, None, 0, C.byref(s)))
        streams.append(s)
    got, errors = [None, None], []

    def work(i):
        try:
            for _ in range(5):
                n = select(views[i], jobs[i][0], jobs[i][1], stream=streams[i])
                got[i] = (n, download(pkg, views[i], streams[i]))
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
        for i, (mode, value, cap) in enumerate(jobs):
            want = reference(tb.kp["response"], tb.mask(mode, value), cap)
            n, (rows, kp, d64, img, _) = got[i]
            assert n == len(want) and np.array_equal(rows, want) and np.array_equal(_bits(kp), _bits(tb.kp[want]))
            assert np.array_equal(d64[:, :61], tb.d[want]) and np.array_equal(img, tb.img[want])
    finally:
        for v in views:
            v.close()
        for s in streams:
            L.apds_stream_destroy(s)


def test_table_current_view_is_untouched(borders):
    tb, pkg = borders, borders.pkg
    before = tb.t.read_keypoints_from_image_id(13)
    view = tb.t.view(CAP)
    try:
        assert select(view, 1, 1) == CAP and select(view, 0, 99) == 0
    finally:
        view.close()
    m = len(before)
    kp, d, ids, img = np.zeros(m, pkg._lib.KEYPOINT_DTYPE), np.zeros((m, 61), np.uint8), np.zeros(m, np.int32), np.zeros(m, np.int32)
    pkg._lib.check(pkg.lib().apds_db_view_download(tb.t._h, pkg._lib.ptr(kp), pkg._lib.ptr(d), pkg._lib.ptr(ids), pkg._lib.ptr(img)))
    assert m == SORT_B - 1 and tb.t.view_device_pointers()[4] == m
    assert np.array_equal(ids, before.ids) and np.array_equal(_bits(kp), _bits(before.keypoints)) and np.array_equal(d, before.descriptors)
    assert np.array_equal(img, before.image_ids)


def test_view_object_is_untouched_by_a_table_select(borders):
    """the reverse: apds_db_select runs the same kernels from the same thread, on the workspace and the table's own current view"""
    tb, pkg = borders, borders.pkg
    view = tb.t.view(5000)
    try:
        want16 = reference(tb.kp["response"], tb.mask(0, 16), 5000)
        n = select(view, 0, 16)
        assert n == 2 * SORT_B + 1
        check_view(tb, view, n, want16)
        first = download(pkg, view)
        check_old_path(tb, 0, 13, None, reference(tb.kp["response"], tb.mask(0, 13), LIMIT))
        assert tb.t.view_device_pointers()[4] == SORT_B - 1
        again = download(pkg, view)
        for a, b in zip(first[:4], again[:4]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert view.device_pointers()[5] == n
    finally:
        view.close()


def test_interleaved_table_and_view_selects(borders):
    """twenty selects of one thread, the two fronts alternating with different arguments: each one against the numpy reference"""
    tb = borders
    args = [(0, 16, None), (1, 1, None), (0, 13, None), (2, 1, (10.3, 20.7, 250.2, 300.1)), (0, 3, None), (1, 0, None), (0, 99, None),
            (2, 0, (0.0, 0.0, 120.5, 399.0)), (0, 19, None), (0, 14, None)]
    view = tb.t.view(CAP)
    try:
        for i in range(20):
            mode, value, box = args[(3 * i + i // 2) % len(args)]
            mask = tb.mask(mode, value, box)
            if i % 2 == 0:
                check_old_path(tb, mode, value, box, reference(tb.kp["response"], mask, LIMIT))
            else:
                check_view(tb, view, select(view, mode, value, box), reference(tb.kp["response"], mask, CAP))
    finally:
        view.close()


def test_repeated_table_selects_allocate_nothing(borders):
    """apds_db_select's scratch is the thread's workspace, sized by the table's rows: after the largest selection nothing more is taken"""
    import torch
    tb, pkg = borders, borders.pkg
    L, n = pkg.lib(), C.c_int(0)
    jobs = [(1, 1, len(reference(tb.kp["response"], tb.mask(1, 1), LIMIT))), (0, 16, 2 * SORT_B + 1), (0, 99, 0), (1, 0, int(tb.mask(1, 0).sum()))]
    assert jobs[0][2] == max(j[2] for j in jobs)
    pkg._lib.check(L.apds_db_select(tb.t._h, jobs[0][0], jobs[0][1], 0.0, 0.0, 0.0, 0.0, C.byref(n)))
    assert n.value == jobs[0][2]
    torch.cuda.synchronize()
    live, free = L.apds_live_contexts(), torch.cuda.mem_get_info()[0]
    for i in range(50):
        mode, value, want = jobs[i % len(jobs)]
        pkg._lib.check(L.apds_db_select(tb.t._h, mode, value, 0.0, 0.0, 0.0, 0.0, C.byref(n)))
        assert n.value == want
    torch.cuda.synchronize()
    assert L.apds_live_contexts() == live and torch.cuda.mem_get_info()[0] == free
    check_old_path(tb, 1, 1, None, reference(tb.kp["response"], tb.mask(1, 1), LIMIT))


def test_repeated_selects_allocate_nothing(borders):
    import torch
    tb, L = borders, borders.pkg.lib()
    view = tb.t.view(CAP)
    try:
        assert select(view, 1, 1) == CAP
        torch.cuda.synchronize()
        live, free = L.apds_live_contexts(), torch.cuda.mem_get_info()[0]
        for _ in range(50):
            assert select(view, 1, 1) == CAP
        torch.cuda.synchronize()
        assert L.apds_live_contexts() == live and torch.cuda.mem_get_info()[0] == free
        check_view(tb, view, CAP, reference(tb.kp["response"], tb.mask(1, 1), CAP))
    finally:
        view.close()


# ---- with_xyz --------------------------------------------------------------------------------------------------------------------------
def test_with_xyz_gathers_the_table_column(gpu_pkg):
    pkg = gpu_pkg
    tb = Table(pkg, [(1, 0, _keypoints(pkg, 700, 50)), (2, 0, _keypoints(pkg, 900, 51))], 52)
    view = tb.t.view(500)
    try:
        with pytest.raises(pkg.ApdsError) as e:            # never computed
            select(view, 0, 2, with_xyz=True)
        assert e.value.code == pkg._lib.ERR_BAD_ARG
        et = pkg.feature_database.ElevationTable()
        et.create_geotransform("dataset", [12.0, 1e-4, 0.0, 55.0, 0.0, -1e-4])
        assert tb.t.world_coordinates(et) == 0
        _, _, xyz_addr, n_all = tb.t.device_table()
        column = np.zeros((n_all, 3), np.float64)
        pkg._lib.check(pkg.lib().apds_dev_download(pkg._lib.ptr(column), xyz_addr, column.nbytes, None))
        assert np.isfinite(column).all() and len(np.unique(column, axis=0)) > 100
        want = reference(tb.kp["response"], tb.mask(0, 2), 500)
        n = select(view, 0, 2, with_xyz=True)
        rows, _, _, _, xyz = download(pkg, view)
        assert n == 500 and np.array_equal(rows, want)
        assert np.array_equal(xyz.view(np.uint64), column[want].view(np.uint64))
        assert select(view, 0, 2) == 500 and view.device_pointers()[4] is None       # not asked for: no xyz pointer
    finally:
        view.close()
        tb.t.close()
    # stale after an insert (a table with room for one more image)
    t = pkg.feature_database.KeypointTable(64)
    try:
        kp, d = _keypoints(pkg, 20, 53), np.zeros((20, 61), np.uint8)
        t.create_keypoints(_Ex(kp, d), 1, 0)
        t.world_coordinates(et)
        v = t.view()
        try:
            assert v.read_keypoints_from_image_id(1, with_xyz=True) == 20
            t.create_keypoints(_Ex(kp, d), 2, 0)
            with pytest.raises(pkg.ApdsError) as e:
                v.read_keypoints_from_image_id(1, with_xyz=True)
            assert e.value.code == pkg._lib.ERR_BAD_ARG
            assert v.read_keypoints_from_image_id(2) == 20
        finally:
            v.close()
    finally:
        t.close()
