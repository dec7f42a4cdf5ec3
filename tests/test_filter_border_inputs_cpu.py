"""CPU: the references and inputs of test_match_filter_borders_gpu.py and test_keypoint_table_borders_gpu.py. The numpy references of
filter_border_cases.py are pinned to the oracle on real descriptor sets, and every input is shown to sit on the border it names: the GPU
files then only have to compare. Where a wrong reading of the contract is named (`<=`, an f64 product, an exclusive box edge, ties cut in
another order) it is the reference that is changed here, to show that the inputs tell the two apart."""
import numpy as np
import pytest

import filter_border_cases as bc


def test_restated_record_layouts(pkg):
    assert bc.DMATCH_DTYPE == pkg._lib.DMATCH_DTYPE and bc.KEYPOINT_DTYPE == pkg._lib.KEYPOINT_DTYPE
    assert bc.APDS_MAX_POINTS == pkg.feature_database.OPENCV_KEYPOINT_LIMIT


@pytest.fixture(scope="module")
def descriptor_sets(pkg):
    db = pkg.synth.make_descriptor_db(2000, seed=61)
    q, _ = pkg.synth.make_queries(db, 300, seed=62)
    q[7] = q[3]                                   # equal queries: the lower query index wins a train row
    db[100:110] = db[90:100]                      # equal train rows: the lower train index wins a query
    return q, db


@pytest.mark.parametrize("fs", [0.0, 0.3, 0.8, 1.0, 1.5])
def test_ratio_reference_equals_the_oracle(oracle_mod, descriptor_sets, fs):
    q, db = descriptor_sets
    for K in (2, 3):
        keys = bc.keys_from_knn(*oracle_mod.knn_hamming(q, db, K))
        want = oracle_mod.get_knn_matches(q, db, K, fs)
        assert np.array_equal(bc.ratio_reference(keys, K, fs), want)
    assert (fs == 0.0) == (len(want) == 0) and (fs > 1.0) == (len(want) == len(q))


def test_ratio_reference_on_missing_neighbours(oracle_mod, descriptor_sets):
    q, db = descriptor_sets
    keys = bc.keys_from_knn(*oracle_mod.knn_hamming(q, db[:1], 2))       # one train row: no second neighbour anywhere
    assert (keys[:, 1] == bc.EMPTY_KEY).all() and (keys[:, 0] != bc.EMPTY_KEY).all()
    assert len(bc.ratio_reference(keys, 2, 1.5)) == 0


def test_cross_check_reference_equals_the_oracle(oracle_mod, descriptor_sets):
    q, db = descriptor_sets
    for qq, tt in ((q, db), (db, q), (q[:1], db), (q, db[:1])):
        keys = bc.keys_from_knn(*oracle_mod.knn_hamming(tt, qq, 1)).ravel()
        want = oracle_mod.get_bruteforce_matches(qq, tt)
        assert np.array_equal(bc.cross_check_reference(keys, len(qq)), want) and len(want)
    assert len(oracle_mod.get_bruteforce_matches(db, q)) < len(db)          # queries nobody names


def _flagged(keys, fs, **kw):
    f = np.zeros(len(keys), bool)
    f[bc.ratio_reference(keys, 2, fs, **kw)["query_idx"]] = True
    return f


def test_ratio_grid_tells_the_wrong_readings_apart():
    keys = bc.ratio_grid_keys()
    assert keys.shape == (513 * 513, 2) and int(keys[-1, 0] >> np.uint64(32)) == 512 == int(keys[512, 1] >> np.uint64(32))
    fs = dict(zip(bc.RATIO_FS_IDS, bc.RATIO_FS))
    assert len(fs) == len(bc.RATIO_FS) == 14
    right = {k: _flagged(keys, v) for k, v in fs.items()}
    for k, floor in bc.RATIO_WIDE_FLOOR.items():
        assert int((_flagged(keys, fs[k], wide=True) != right[k]).sum()) >= floor, k
    for k in bc.RATIO_LEQ_IDS:
        assert int((_flagged(keys, fs[k], strict=False) != right[k]).sum()) >= bc.RATIO_LEQ_FLOOR, k
    for k in bc.RATIO_LEQ_ONE_IDS:
        assert int((_flagged(keys, fs[k], strict=False) != right[k]).sum()) >= 1, k
    # what the special values mean: nothing passes at 0, at -1 and at NaN; at +inf every d1 > 0 passes (0 * inf is NaN);
    # a subnormal fs passes exactly d0 = 0 against d1 > 0 - unless the product is flushed to zero
    assert not right["0"].any() and not right["-1"].any() and not right["nan"].any()
    assert int(right["inf"].sum()) == 513 * 512 and int(right["subnormal"].sum()) == 512
    assert 0 < float(fs["subnormal"]) < np.finfo(np.float32).tiny
    assert int(right["above1"].sum()) > int(right["1"].sum()) == int(right["below1"].sum())


def test_ratio_structure_rows():
    for nq in bc.RATIO_STRUCTURE_NQ:
        for K in bc.RATIO_STRUCTURE_K:
            keys = bc.ratio_structure_keys(nq, K)
            want = bc.ratio_reference(keys, K, bc.RATIO_STRUCTURE_FS)
            # any two neighbouring columns from 2 on would pass, also in the rows that fail or miss a neighbour
            for c in range(2, K - 1, 2):
                assert len(bc.ratio_reference(keys[:, c:c + 2], 2, bc.RATIO_STRUCTURE_FS)) == nq
            if nq >= 63:
                e0, e1 = keys[:, 0] == bc.EMPTY_KEY, keys[:, 1] == bc.EMPTY_KEY
                assert (e0 & ~e1).any() and (~e0 & e1).any() and (e0 & e1).any() and 0 < len(want) < (~e0 & ~e1).sum()
                assert {0, bc.TRAIN_MAX} == set(want["train_idx"].tolist())
    assert len(bc.ratio_reference(bc.ratio_structure_keys(1, 5), 5, bc.RATIO_STRUCTURE_FS)) == 1


def test_flag_patterns_reach_the_carry_loop():
    assert bc.CARRY_N == 1024 * 1024 and bc.COMPACTION_NQ[-1] == 2 * 1024 ** 2 + 1025
    for n in bc.COMPACTION_NQ[-2:]:
        last_block = (n - 1) // bc.SCAN_BLOCK
        assert last_block >= bc.SCAN_TRIP
        for name in bc.CARRY_PATTERNS:
            f = bc.flag_pattern(name, n)
            assert f[bc.SCAN_TRIP * bc.SCAN_BLOCK:(bc.SCAN_TRIP + 1) * bc.SCAN_BLOCK].any() and f[last_block * bc.SCAN_BLOCK:].any(), (name, n)
    n = bc.COMPACTION_NQ[-1]
    assert bc.flag_pattern("last", n)[((n - 1) // bc.SCAN_BLOCK) * bc.SCAN_BLOCK:].any()
    assert not bc.flag_pattern("carry_blocks", n)[:bc.CARRY_N].any() and not bc.flag_pattern("carry_blocks", bc.CARRY_N).any()
    assert set(bc.CARRY_PATTERNS) | {"none", "first", "last"} == set(bc.FLAG_PATTERNS) and len(bc.FLAG_PATTERNS) == 9
    for name in bc.FLAG_PATTERNS:                 # the keys carry the pattern: the reference's matches are the flagged queries
        f = bc.flag_pattern(name, 1025)
        assert np.array_equal(bc.ratio_reference(bc.compaction_keys(f), 2, 1.0)["query_idx"], np.nonzero(f)[0])


def test_carry_removed_misplaces_the_match_beyond_the_first_trip():
    # `carry += incl` removed: block 1024's offset restarts at 0. Restated on the block counts of the all-set pattern at 1024^2 + 1.
    counts = np.add.reduceat(bc.flag_pattern("all", bc.CARRY_N + 1).astype(np.int64), np.arange(0, bc.CARRY_N + 1, bc.SCAN_BLOCK))
    right = np.cumsum(counts) - counts
    wrong = np.concatenate([np.cumsum(counts[:bc.SCAN_TRIP]) - counts[:bc.SCAN_TRIP], np.cumsum(counts[bc.SCAN_TRIP:]) - counts[bc.SCAN_TRIP:]])
    assert len(counts) == bc.SCAN_TRIP + 1 and right[-1] == bc.CARRY_N and wrong[-1] == 0


def test_cross_check_cases_are_valid_and_contended():
    cases = bc.cross_check_cases()
    for name, (tb, nq) in cases.items():
        real = tb[tb != bc.EMPTY_KEY]
        assert not len(real) or int((real & np.uint64(0xFFFFFFFF)).max()) < nq, name
    w = bc.cross_check_reference(*cases["all_name_query0_equal_distance"])
    assert w.tolist() == [(0, 0, 0, 40.0)]
    w = bc.cross_check_reference(*cases["all_name_query0_last_is_nearer"])
    assert w.tolist() == [(0, 99_999, 0, 39.0)]
    w = bc.cross_check_reference(*cases["empty_rows_interleaved"])
    assert w.tolist() == [(0, 1, 0, 40.0)]
    tb, nq = cases["more_train_than_queries_contended"]
    w = bc.cross_check_reference(tb, nq)
    assert len(tb) > nq and len(w) == nq - 1 and 64 not in w["query_idx"] and (tb == bc.EMPTY_KEY).any()
    tb, nq = cases["fewer_train_than_queries"]
    assert len(tb) < nq and 0 < len(bc.cross_check_reference(tb, nq)) < len(tb)
    tb, nq = cases["carry_loop_sparse_hits"]
    w = bc.cross_check_reference(tb, nq)
    assert nq == bc.CARRY_N + 1 and w["query_idx"][-1] == bc.CARRY_N and w["query_idx"][0] == 0 and len(w) < len(tb)


def _rows(resp):
    kp = np.zeros(len(resp), bc.KEYPOINT_DTYPE)
    kp["response"] = resp
    return kp


def test_limit_cut_tables_cut_where_they_claim():
    L = bc.APDS_MAX_POINTS
    for name in bc.LIMIT_CUT_CASES:
        kp = _rows(bc.limit_cut_responses(name))
        m = len(kp)
        all_rows = np.ones(m, bool)
        keep = bc.select_reference(kp, all_rows)
        assert len(keep) == min(m, L)
        if name == "exactly_limit":
            assert m == L
            continue
        assert m > L
        cut = kp["response"][keep[-1]]
        at_cut = int((kp["response"] == cut).sum())
        if name == "limit_plus_one":
            assert m == L + 1 and sorted(set(range(m)) - set(keep.tolist())) == [1000]
            continue
        # more rows at the cut response than the view can take of them: the row decides, and another tie order keeps other rows
        kept_at_cut = int((kp["response"][keep] == cut).sum())
        assert at_cut > kept_at_cut > 0, name
        assert set(bc.select_reference(kp, all_rows, by_row=False).tolist()) != set(keep.tolist()), name
        if name == "all_equal":
            assert np.array_equal(keep, np.arange(L))
        if name == "two_groups":
            assert cut == 1.0 and int((kp["response"] == 2.0).sum()) == 100_000
        if name == "low_mantissa_byte":
            bits = kp["response"].view(np.uint32)
            assert len(np.unique(bits)) == 256 and len(np.unique(bits >> 8)) == 1
    # `keys[i] <= kth` read as `<`: the kth key itself leaves, one row short
    for name in ("limit_plus_one", "all_equal"):
        kp = _rows(bc.limit_cut_responses(name))
        assert len(bc.select_reference(kp, np.ones(len(kp), bool))[:-1]) == L - 1


def test_sort_and_response_order_inputs():
    for m in bc.SORT_M:
        r = bc.sort_size_responses(m)
        assert len(r) == m and (m < 3 or len(np.unique(r)) < m)
    assert {m & (m - 1) == 0 for m in bc.SORT_M} == {True, False}
    r = bc.response_order_values()
    kp = _rows(r)
    order = bc.select_reference(kp, np.ones(len(r), bool))
    s = r[order]
    assert not np.isnan(r).any() and len(r) == 50
    assert s[0] == np.inf and s[-1] == np.float32(-3.0e38) and (s[1:] <= s[:-1]).all()
    zeros = order[s == 0.0]
    assert len(zeros) == 10 and (np.diff(zeros) > 0).all() and len(set(np.signbit(r[zeros]).tolist())) == 2   # both zeros, tied, by row
    assert (r < 0).sum() == 15 and ((r > 0) & (r < np.finfo(np.float32).tiny)).sum() == 5
    # the order of the key `~bits << 32 | row` alone: negative responses come first, so this set tells it from ORDER BY response DESC
    naive = np.lexsort((np.arange(len(r)), (~r.view(np.uint32)).astype(np.uint64)))
    assert r[naive[0]] < 0 and not np.array_equal(naive, order)


def _box_table_columns():
    kps, lods, imgs = [], [], []
    for image_id, lod, col, row, kp in bc.box_table():
        kps.append(bc.rescale(kp, lod, col, row))
        lods.append(np.full(len(kp), lod))
        imgs.append(np.full(len(kp), image_id))
    return np.concatenate(kps), np.concatenate(lods), np.concatenate(imgs)


def test_box_rows_sit_on_and_beside_the_edges():
    kp, lod, img = _box_table_columns()
    assert sorted(v[0] for v in bc.BOX_IMAGES.values()) == [0, 1, 3, 8, 30] and max(v[0] for v in bc.BOX_IMAGES.values() if v[1] and v[2]) == 8
    for name, blod, box in bc.EDGE_BOXES:
        mask = bc.box_mask(kp, lod, blod, box)
        x0, y0, x1, y1 = bc.box_bounds(box)
        assert x0 <= x1 and y0 <= y1
        on_edge = 0
        for x, y, inside in bc.box_edge_targets(box):
            rows = np.nonzero((kp["x"] == x) & (kp["y"] == y) & (lod == blod))[0]      # the rescale lands exactly on the target
            assert len(rows) >= 1 and mask[rows].all() == inside and mask[rows].any() == inside, (name, x, y)
            on_edge += inside and (x in (x0, x1) or y in (y0, y1))
        assert on_edge >= 6
        assert (bc.box_mask(kp, lod, blod, box, strict=True) != mask).any(), name           # `<=` read as `<` loses the on-edge rows
        inside_elsewhere = bc.box_mask(kp, np.full(len(kp), blod), blod, box) & (lod != blod)
        if name in ("integer_ends", "lod3"):
            assert inside_elsewhere.any(), name                                              # a row inside the box at another level of detail
    assert np.floor(np.float32(-0.5)) == -1 and bc.box_mask(kp, lod, 0, bc.EDGE_BOXES[0][2])[(kp["x"] == -0.5) & (kp["y"] == -0.5)].all()
    assert (kp["x"] < 0).any() and np.isnan(kp["x"]).sum() == 1 and np.isnan(kp["y"]).sum() == 1
    nan_rows = np.isnan(kp["x"]) | np.isnan(kp["y"])
    for name, blod, box in bc.EDGE_BOXES + bc.INVERTED_BOXES:
        assert not bc.box_mask(kp, lod, blod, box)[nan_rows].any()
    for name, blod, box in bc.INVERTED_BOXES:
        x0, y0, x1, y1 = bc.box_bounds(box)
        assert (x0 > x1 or y0 > y1) and not bc.box_mask(kp, lod, blod, box).any()
        assert bc.box_mask(kp, lod, blod, (min(box[0], box[2]), min(box[1], box[3]), max(box[0], box[2]), max(box[1], box[3]))).any()
    assert kp["x"][lod == 30].max() > 2.0 ** 31


def test_big_table_layout():
    img, lod = bc.big_table_columns()
    blk = lambda r: r // bc.SCAN_BLOCK                                              # noqa: E731
    assert len(img) == bc.BIG_ROWS == 1024 ** 2 + 1025 and blk(bc.BIG_ROWS - 1) == bc.SCAN_TRIP + 1
    assert np.nonzero(img == bc.BIG_IMG_BLOCK0)[0].tolist() == [bc.BIG_ROW_BLOCK0] and blk(bc.BIG_ROW_BLOCK0) == 0
    assert np.nonzero(img == bc.BIG_IMG_BLOCK1024)[0].tolist() == [bc.BIG_ROW_BLOCK1024] and blk(bc.BIG_ROW_BLOCK1024) == bc.SCAN_TRIP
    assert np.nonzero(img == bc.BIG_IMG_LAST)[0].tolist() == [bc.BIG_ROWS - 1]
    sparse = np.nonzero(img == bc.BIG_IMG_SPARSE)[0]
    assert 800 < len(sparse) < 1300 and blk(sparse[0]) == 0 and blk(sparse[-1]) >= bc.SCAN_TRIP
    assert set(np.unique(lod).tolist()) == {0, 1} and int((lod == 0).sum()) > bc.CARRY_N > bc.APDS_MAX_POINTS
    assert blk(np.nonzero(lod == 1)[0][-1]) >= bc.SCAN_TRIP
    r = bc.runs(img, lod)
    assert r[0][0] == 0 and r[-1][1] == bc.BIG_ROWS and all(a[1] == b[0] for a, b in zip(r, r[1:])) and len(r) < 5000
