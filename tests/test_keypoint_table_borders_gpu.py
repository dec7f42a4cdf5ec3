"""GPU: apds_db_select (csrc/keypoint_select.hip) at its borders - selects on a table of more than 1024 scan blocks, the LIMIT cut inside groups of equal
responses, the sort network around a power of two, ORDER BY response DESC over zeros, subnormals, negative responses and +inf, the
bounding box on, and one ulp beside, its inclusive edges, the insert's zero padding and capacity, and the view after an empty select.
Exact equality with the numpy restatements of filter_border_cases.py (test_filter_border_inputs_cpu.py shows that the inputs sit where they
claim). NaN responses are out of scope: SQL's ORDER BY puts them first, a float comparison puts them nowhere, and the extractor never
produces one."""
import numpy as np
import pytest

import filter_border_cases as bc

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1


class _Ex:
    def __init__(self, kp, d):
        self.keypoints, self.descriptors = kp, d


@pytest.fixture(scope="module")
def descriptors():
    return bc.random_descriptors(bc.LIMIT_CUT_M, 0xDE5C)


def _bits(kp):
    return np.ascontiguousarray(kp).view(np.uint32)       # bitwise: NaN coordinates and the sign of a zero count


def _check(rows, want, kp, d, img):
    assert len(rows) == len(want)
    assert np.array_equal(rows.ids - 1, want)
    assert np.array_equal(_bits(rows.keypoints), _bits(kp[want])) and np.array_equal(rows.descriptors, d[want]) and np.array_equal(rows.image_ids, img[want])


# ---- more than 1024 scan blocks -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(gpu_pkg):
    img, lod = bc.big_table_columns()
    kp, d = bc.fake_keypoints(bc.BIG_ROWS, 77), bc.random_descriptors(bc.BIG_ROWS, 78)
    t = gpu_pkg.feature_database.KeypointTable(bc.BIG_ROWS)
    try:
        for a, b in bc.runs(img, lod):
            t.create_keypoints(_Ex(kp[a:b], d[a:b]), int(img[a]), int(lod[a]))
        assert len(t) == bc.BIG_ROWS
        want = kp.copy()
        one = lod == 1
        want[one] = bc.rescale(kp[one], 1)
        yield t, want, d, img, lod
    finally:
        t.close()


@pytest.mark.parametrize("image_id", [bc.BIG_IMG_BLOCK0, bc.BIG_IMG_BLOCK1024, bc.BIG_IMG_LAST, bc.BIG_IMG_SPARSE])
def test_big_table_select_by_image_id(big, image_id):
    """a single row in block 0, in block 1024, the very last row, a Bernoulli 1e-3 subset: block offsets beyond the scan's first trip"""
    t, kp, d, img, lod = big
    mask = img == image_id
    _check(t.read_keypoints_from_image_id(image_id), bc.select_reference(kp, mask), kp, d, img)
    assert mask.sum() == 1 or image_id == bc.BIG_IMG_SPARSE


def test_big_table_select_sparse_level_of_detail(big):
    t, kp, d, img, lod = big
    _check(t.read_keypoints_from_lod(1), bc.select_reference(kp, lod == 1), kp, d, img)


def test_big_table_select_over_a_million_keys(big):
    """everything at level of detail 0: m > 1024^2 > LIMIT, so the radix select and the second compaction run over more than 1024 blocks"""
    t, kp, d, img, lod = big
    rows = t.read_keypoints_from_lod(0)
    assert len(rows) == bc.APDS_MAX_POINTS
    _check(rows, bc.select_reference(kp, lod == 0), kp, d, img)


# ---- LIMIT cut ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.LIMIT_CUT_CASES)
def test_limit_cut(gpu_pkg, descriptors, name):
    resp = bc.limit_cut_responses(name)
    m = len(resp)
    kp = bc.fake_keypoints(m, 90)
    kp["response"] = resp
    d = descriptors[:m]
    t = gpu_pkg.feature_database.KeypointTable(m)
    try:
        t.create_keypoints(_Ex(kp, d), 1, 0)
        rows = t.read_keypoints_from_lod(0)
        assert len(rows) == bc.APDS_MAX_POINTS
        _check(rows, bc.select_reference(kp, np.ones(m, bool)), kp, d, np.ones(m, np.int32))
    finally:
        t.close()


# ---- small tables ---------------------------------------------------------------------------------------------------------------------
def _table(gpu_pkg, inserts, d):
    """inserts: [(image id, level of detail, column, row, keypoints)] -> table, rescaled keypoints, image ids, levels of detail"""
    t = gpu_pkg.feature_database.KeypointTable(sum(len(i[4]) for i in inserts))
    kps, imgs, lods, at = [], [], [], 0
    for image_id, lod, col, row, kp in inserts:
        t.create_keypoints(_Ex(kp, d[at:at + len(kp)]), image_id, lod, col, row, bc.TILE)
        kps.append(bc.rescale(kp, lod, col, row)); imgs.append(np.full(len(kp), image_id, np.int32)); lods.append(np.full(len(kp), lod, np.int32))
        at += len(kp)
    return t, np.concatenate(kps), np.concatenate(imgs), np.concatenate(lods)


def test_sort_sizes(gpu_pkg, descriptors):
    """m around a power of two, with ties: the all-ones keys that pad the bitonic network never reach the view"""
    inserts = []
    for image_id, m in enumerate(bc.SORT_M, start=1):
        kp = bc.fake_keypoints(m, 300 + m)
        kp["response"] = bc.sort_size_responses(m)
        inserts.append((image_id, 0, 0, 0, kp))
    t, kp, img, lod = _table(gpu_pkg, inserts, descriptors)
    try:
        for image_id, m in enumerate(bc.SORT_M, start=1):
            rows = t.read_keypoints_from_image_id(image_id)
            assert len(rows) == m and rows.ids.min() >= 1 and rows.ids.max() <= len(kp)
            _check(rows, bc.select_reference(kp, img == image_id), kp, descriptors, img)
    finally:
        t.close()


def test_response_order(gpu_pkg, descriptors):
    """+inf, large, 1.0, the smallest normal, subnormals, +0.0 and -0.0 (which tie), negative responses: ORDER BY response DESC"""
    kp = bc.fake_keypoints(50, 17)
    kp["response"] = bc.response_order_values()
    t, kp, img, lod = _table(gpu_pkg, [(1, 0, 0, 0, kp[:20]), (2, 0, 0, 0, kp[20:])], descriptors)
    try:
        for rows, mask in ((t.read_keypoints_from_lod(0), lod == 0), (t.read_keypoints_from_image_id(2), img == 2)):
            want = bc.select_reference(kp, mask)
            _check(rows, want, kp, descriptors, img)
    finally:
        t.close()


@pytest.fixture(scope="module")
def box_table(gpu_pkg, descriptors):
    t, kp, img, lod = _table(gpu_pkg, bc.box_table(), descriptors)
    try:
        yield t, kp, img, lod
    finally:
        t.close()


_BOXES = bc.EDGE_BOXES + bc.INVERTED_BOXES


@pytest.mark.parametrize("name,box_lod,box", _BOXES, ids=[b[0] for b in _BOXES])
def test_bounding_box(box_table, descriptors, name, box_lod, box):
    """floor(x_start) <= x <= ceil(x_end), both ends inclusive, on coordinates that went through the insert rescale (level of detail 0, 1, 3,
    8 with a non-zero column and row, and 30)"""
    t, kp, img, lod = box_table
    mask = bc.box_mask(kp, lod, box_lod, box)
    assert mask.any() == (name in [b[0] for b in bc.EDGE_BOXES])
    _check(t.read_keypoints_from_coordinates(*box, box_lod), bc.select_reference(kp, mask), kp, descriptors, img)


def test_insert_rescale_at_every_level_of_detail(box_table, descriptors):
    t, kp, img, lod = box_table
    for v in sorted(set(lod.tolist())):
        _check(t.read_keypoints_from_lod(v), bc.select_reference(kp, lod == v), kp, descriptors, img)


# ---- insert ---------------------------------------------------------------------------------------------------------------------------
def test_insert_pads_bytes_61_to_63_with_zeros(gpu_pkg, descriptors):
    """64-byte queries that end in three 0xFF bytes: every distance is the popcount over 61 bytes plus 24"""
    n, nq = 300, 40
    kp, d = bc.fake_keypoints(n, 23), descriptors[1000:1000 + n]
    t, kp, img, lod = _table(gpu_pkg, [(1, 0, 0, 0, kp)], d)
    try:
        rows = t.read_keypoints_from_lod(0)
        assert np.array_equal(rows.descriptors, d[rows.ids - 1])
        q = np.full((nq, 64), 0xFF, np.uint8)
        q[:, :61] = descriptors[5000:5000 + nq]
        q[:10, :61] = rows.descriptors[:10]                                   # some queries are table rows: 0 + 24
        dist = np.unpackbits(q[:, None, :61] ^ rows.descriptors[None, :, :], axis=2).sum(axis=2).astype(np.int32) + 24
        want_idx = np.argsort(dist, axis=1, kind="stable")[:, :2].astype(np.int32)
        idx, got = t.knn_match_view(q, 2)
        assert np.array_equal(got, np.take_along_axis(dist, want_idx, axis=1)) and np.array_equal(idx, want_idx)
        assert (got[:10, 0] == 24).all()
    finally:
        t.close()


def test_full_table_refuses_one_more_row(gpu_pkg, descriptors):
    cap = 1000
    kp = bc.fake_keypoints(cap + 1, 29)
    d = descriptors[:cap + 1]
    t = gpu_pkg.feature_database.KeypointTable(cap)
    try:
        t.create_keypoints(_Ex(kp[:0], d[:0]), 1)                             # zero rows into an empty table
        assert len(t) == 0 and len(t.read_keypoints_from_lod(0)) == 0
        for a, b in ((0, 400), (400, 999), (999, 1000)):
            t.create_keypoints(_Ex(kp[a:b], d[a:b]), 1)
        assert len(t) == cap
        with pytest.raises(gpu_pkg._lib.ApdsError) as e:
            t.create_keypoints(_Ex(kp[cap:], d[cap:]), 1)
        assert e.value.code == gpu_pkg._lib.ERR_NOMEM and len(t) == cap
        t.create_keypoints(_Ex(kp[:0], d[:0]), 2)                             # zero rows fit a full table
        assert len(t) == cap and len(t.read_keypoints_from_image_id(2)) == 0
        _check(t.read_keypoints_from_image_id(1), bc.select_reference(kp[:cap], np.ones(cap, bool)), kp, d, np.ones(cap, np.int32))
    finally:
        t.close()


# ---- view state -----------------------------------------------------------------------------------------------------------------------
def test_empty_select_after_a_non_empty_one(gpu_pkg, descriptors):
    kp = bc.fake_keypoints(500, 31)
    t, kp, img, lod = _table(gpu_pkg, [(1, 0, 0, 0, kp)], descriptors)
    try:
        assert len(t.read_keypoints_from_lod(0)) == 500 and t.view_device_pointers()[4] == 500
        rows = t.read_keypoints_from_image_id(99)
        assert len(rows) == 0 and t.view_device_pointers()[4] == 0
        idx, dist = t.knn_match_view(descriptors[:70], 2)
        assert (idx == -1).all() and (dist == INT_MAX).all() and idx.shape == (70, 2)
    finally:
        t.close()
