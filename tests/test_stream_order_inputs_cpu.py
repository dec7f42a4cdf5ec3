"""CPU: the inputs of test_stream_order_gpu.py (stream_order_cases.py). For every case the real and the decoy input have different expected
outputs - so an entry that reads the decoy is told from one that reads the real input - and the decoys meet the entries' input rules:
indices in range, key lists ascending, shapes and types equal to the real input's. The numpy references used on the GPU are pinned to
the oracle here."""
import numpy as np
import pytest

import filter_border_cases as bc
import stream_order_cases as sc


def _same_layout(real, decoy):
    assert len(real) == len(decoy)
    for r, d in zip(real, decoy):
        assert r.shape == d.shape and r.dtype == d.dtype


def test_the_threshold_is_the_codes(pkg):
    import os
    src = open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "hamming_mfma.hip")).read()
    assert "nt >= 65536" in src and sc.HM_SAMPLE_THRESHOLD == 65536
    assert sc.TOPK_NT[0] < sc.HM_SAMPLE_THRESHOLD < sc.TOPK_NT[1] and sc.PAIR_X[1] >= sc.HM_SAMPLE_THRESHOLD > sc.PAIR_Y[1]
    assert sc.mfma_backend(1) == sc.mfma_backend(2) == 2 and sc.mfma_backend(3) == 3


@pytest.mark.parametrize("nt", sc.TOPK_NT)
def test_topk_decoy_has_other_neighbours(pkg, oracle_mod, nt):
    real, decoy = sc.topk_inputs(pkg.synth, nt)
    _same_layout(real, decoy)
    for k in sc.TOPK_K:
        a, b = bc.keys_from_knn(*oracle_mod.knn_hamming(*real, k)), bc.keys_from_knn(*oracle_mod.knn_hamming(*decoy, k))
        assert a.shape == (sc.TOPK_NQ, k) and (a[:, 0] != b[:, 0]).mean() > 0.9
        # the real queries against the decoy train rows (one of the two inputs read early) differ too
        c = bc.keys_from_knn(*oracle_mod.knn_hamming(real[0], decoy[1], k))
        assert (a[:, 0] != c[:, 0]).mean() > 0.9


def test_pack_and_merge_and_sat():
    r, d = sc.pack_inputs()
    _same_layout((r,), (d,))
    assert sc.PACK_BYTES < 64 <= sc.PACK_STRIDE and not np.array_equal(sc.pack_reference(r), sc.pack_reference(d)) and not sc.pack_reference(r)[:, sc.PACK_BYTES:].any()
    r, d = sc.merge_inputs()
    _same_layout((r,), (d,))
    for keys in (r, d):                           # the merge's input rule: every list ascending, real keys distinct
        real = keys[keys != bc.EMPTY_KEY]
        assert (np.diff(keys.astype(object), axis=2) >= 0).all() and len(np.unique(real)) == len(real) and (keys == bc.EMPTY_KEY).any()
    assert (sc.merge_reference(r) != sc.merge_reference(d)).any(axis=1).mean() > 0.9
    r, d = sc.sat_inputs()
    _same_layout((r,), (d,))
    assert sc.sat_reference(r)[-1, -1] == (r == 0).sum() != (d == 0).sum() and sc.SAT_COLS % 64 and sc.SAT_ROWS % 4
    assert (sc.sat_reference(r) != sc.sat_reference(d)).mean() > 0.5


def test_filter_keys(pkg, oracle_mod):
    (q, t), (dq, dt) = sc.filter_descriptors(pkg.synth)
    _same_layout((q, t), (dq, dt))
    k2, dk2 = (bc.keys_from_knn(*oracle_mod.knn_hamming(a, b, 2)) for a, b in ((q, t), (dq, dt)))
    want, dwant = bc.ratio_reference(k2, 2, sc.FILTER_FS), bc.ratio_reference(dk2, 2, sc.FILTER_FS)
    assert np.array_equal(want, oracle_mod.get_knn_matches(q, t, 2, float(sc.FILTER_FS)))
    assert 0 < len(want) < sc.FILTER_NQ and not np.array_equal(want, dwant)
    tb, dtb = (bc.keys_from_knn(*oracle_mod.knn_hamming(b, a, 1)).ravel() for a, b in ((q, t), (dq, dt)))
    for keys in (tb, dtb):                        # the cross-check's input rule: every named query exists
        assert int((keys[keys != bc.EMPTY_KEY] & np.uint64(0xFFFFFFFF)).max()) < sc.FILTER_NQ
    cw, dcw = bc.cross_check_reference(tb, sc.FILTER_NQ), bc.cross_check_reference(dtb, sc.FILTER_NQ)
    assert np.array_equal(cw, oracle_mod.get_bruteforce_matches(q, t)) and len(cw) and not np.array_equal(cw, dcw)
    assert not np.array_equal(cw, oracle_mod.get_bruteforce_matches(q, dt)) and not np.array_equal(cw, oracle_mod.get_bruteforce_matches(dq, t))


@pytest.mark.parametrize("dim", sc.L2_DIMS)
def test_l2_decoy_has_other_neighbours(dim):
    r, d = sc.l2_inputs(dim)
    _same_layout(r, d)
    a, b, c = sc.l2_nearest(*r), sc.l2_nearest(*d), sc.l2_nearest(r[0], d[1])
    assert (a != b).mean() > 0.9 and (a != c).mean() > 0.9 and sc.L2_NQ % 64 and sc.L2_NT % 128


def test_band_inputs(oracle_mod):
    r, d = sc.band_inputs()
    _same_layout(r, d)
    a, b = oracle_mod.band_merger(*r, sc.BAND_MINMAX), oracle_mod.band_merger(*d, sc.BAND_MINMAX)
    assert (np.asarray(a).reshape(-1, 4) != np.asarray(b).reshape(-1, 4)).any(axis=1).mean() > 0.9


def test_point_inputs_are_in_range():
    r, d = sc.point_inputs()
    _same_layout(r, d)
    for kp1, kp2, m, xyz in (r, d):
        assert 0 <= m["query_idx"].min() and m["query_idx"].max() < len(kp1) and 0 <= m["train_idx"].min() and m["train_idx"].max() < len(kp2) == len(xyz)
        assert np.array_equal(np.float64(np.float32(xyz)), xyz)
    for f, pick in ((sc.points_reference, lambda s: s[:3]), (sc.correspondences_reference, lambda s: (s[0], s[3], s[2]))):
        a, b = f(*pick(r)), f(*pick(d))
        assert all((x != y).any(axis=1).mean() > 0.9 for x, y in zip(a, b))
        # one input of the three read early: the answer differs as well
        for i in range(3):
            mixed = list(pick(r))
            mixed[i] = pick(d)[i]
            assert any(not np.array_equal(x, y) for x, y in zip(a, f(*mixed)))


def test_homography_inputs(pkg, oracle_mod):
    r, d = sc.homography_inputs(pkg.synth)
    _same_layout(r, d)
    for method in sc.HOMOGRAPHY_METHODS:
        ok_r, Hr, mr = oracle_mod.find_homography(*r, method, 3.0)
        ok_d, Hd, md = oracle_mod.find_homography(*d, method, 3.0)
        assert ok_r and ok_d and not np.array_equal(Hr, Hd)
        if method:
            assert not np.array_equal(mr, md) and 4 < mr.sum() < sc.HOMOGRAPHY_N


def test_akaze_inputs(pkg, oracle_mod):
    r, d = sc.akaze_single_inputs(pkg.synth)
    _same_layout((r,), (d,))
    a, b = oracle_mod.akaze(r), oracle_mod.akaze(d)
    assert 10 <= len(a.keypoints) < sc.AKAZE_CAP and 10 <= len(b.keypoints) < sc.AKAZE_CAP and not np.array_equal(a.descriptors, b.descriptors)
    r, d = sc.akaze_batch_inputs(pkg.synth)
    _same_layout((r,), (d,))
    assert r.shape == sc.AKAZE_BATCH and all(not np.array_equal(r[i], d[i]) for i in range(sc.AKAZE_BATCH[0]))
    for i in range(sc.AKAZE_BATCH[0]):
        a, b = oracle_mod.akaze(r[i]), oracle_mod.akaze(d[i])
        assert 10 <= len(a.keypoints) < sc.AKAZE_CAP and 10 <= len(b.keypoints) and not np.array_equal(a.descriptors, b.descriptors)


def test_insert_inputs():
    r, d = sc.insert_inputs()
    _same_layout(r, d)
    assert sc.INSERT_N <= sc.INSERT_TABLE_ROWS and sc.INSERT_N % 16 and not r[1][:, 61:].any() and not d[1][:, 61:].any()
    assert (r[1] != d[1]).any(axis=1).all() and (r[0]["x"] != d[0]["x"]).mean() > 0.9
    r, d = sc.insert_batch_inputs()
    _same_layout(r, d)
    assert len(sc.INSERT_BATCH_COUNTS) == sc.INSERT_BATCH_TILES and len(sc.INSERT_BATCH_COLUMNS_ROWS) == 2 * sc.INSERT_BATCH_TILES
    assert all(0 < c <= sc.INSERT_BATCH_CAP for c in sc.INSERT_BATCH_COUNTS) and sum(sc.INSERT_BATCH_COUNTS) <= sc.INSERT_TABLE_ROWS
    assert min(sc.INSERT_BATCH_COUNTS) < sc.INSERT_BATCH_CAP            # rows behind a tile's count exist, and the reference skips them
    a, b = sc.insert_batch_rows(r[1]), sc.insert_batch_rows(d[1])
    assert len(a) == sum(sc.INSERT_BATCH_COUNTS) and (a != b).any(axis=1).all()
    assert np.array_equal(a[sc.INSERT_BATCH_COUNTS[0]], r[1][sc.INSERT_BATCH_CAP])


def test_view_selections_differ():
    t = sc.view_table()
    assert sum(len(x[2]) for x in t) <= sc.VIEW_TABLE_ROWS and [x[:2] + (len(x[2]),) for x in t] == list(sc.VIEW_IMAGES)
    (rows, img), (drows, dimg) = sc.view_reference(sc.VIEW_REAL), sc.view_reference(sc.VIEW_DECOY)
    assert len(rows) == 700 + 333 and len(drows) == 500 and not set(rows.tolist()) & set(drows.tolist())
    assert set(img.tolist()) == {1, 3} and set(dimg.tolist()) == {2}
    resp = np.concatenate([x[2]["response"] for x in t])
    assert (np.diff(resp[rows]) <= 0).all() and len(np.unique(resp[rows])) < len(rows)      # equal responses: the row decides
    ties = np.diff(resp[rows]) == 0
    assert (np.diff(rows)[ties] > 0).all() and not np.array_equal(rows, np.sort(rows))
