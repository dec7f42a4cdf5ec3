"""Inputs and numpy references of the filter and keypoint-table border tests: shared by test_match_filter_borders_gpu.py,
test_keypoint_table_borders_gpu.py (HIP against the references) and test_filter_border_inputs_cpu.py (the references against the oracle,
and: does every input sit on the border it names?). Not a test module; it needs neither a GPU nor the oracle.

Every size below is derived from a named constant of the source file beside it; the constants are restated here so that a change of one
of them in the source shows up against this table in review."""
import numpy as np

# ---- csrc/match_filter.hip ------------------------------------------------------------------------------------------------------------
SCAN_BLOCK = 1024                          # flags per block of scan_block_counts_kernel / emit_ratio_matches_kernel
WAVE = 64                                  # the ballots of block_exclusive_pos
SCAN_TRIP = 1024                           # block counts per trip of scan_offsets_kernel's loop
CARRY_N = SCAN_BLOCK * SCAN_TRIP           # 1 048 576: flags beyond this one are placed through `carry`
# ---- csrc/keypoint_select.hip ---------------------------------------------------------------------------------------------------------
TB = 1024                                  # keypoint_table.h: rows / keys per block of the select kernels
# ---- include/apds.h -------------------------------------------------------------------------------------------------------------------
APDS_MAX_POINTS = 2 ** 18 - 1              # LIMIT of every select (keypointdb.rs:12)
# ---- csrc/topk_keys.h -----------------------------------------------------------------------------------------------------------------
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)

# restated from cubesat-apds_amd/_lib.py (test_filter_border_inputs_cpu.py compares them)
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
DMATCH_DTYPE = np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("img_idx", "<i4"), ("distance", "<f4")])

_HI = np.uint64(0xFFFFFFFF00000000)
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def make_keys(dist, idx):
    """distance << 32 | index, as csrc/topk_keys.h packs them"""
    return (np.asarray(dist, np.uint64) << _32) | np.asarray(idx, np.uint64)


def keys_from_knn(idx, dist):
    """The keys a scan leaves for an (idx, dist) answer of knn_hamming: all ones where there is no row (idx -1)."""
    idx, dist = np.asarray(idx, np.int64), np.asarray(dist, np.int64)
    return np.where(idx < 0, EMPTY_KEY, make_keys(np.where(idx < 0, 0, dist), np.where(idx < 0, 0, idx)))


def _matches(query, key):
    out = np.zeros(len(query), DMATCH_DTYPE)
    out["query_idx"] = query
    out["train_idx"] = (key & _LO).astype(np.uint32).view(np.int32)
    out["distance"] = (key >> _32).astype(np.uint32).astype(np.float32)
    return out


# ---- references -----------------------------------------------------------------------------------------------------------------------
def ratio_reference(keys, K, fs, strict=True, wide=False):
    """feature_extraction/src/lib.rs:108 on [nq][K] keys: `d0 < d1 * filter_strength`, one IEEE f32 product and one f32 comparison; false
    where one of the two nearest is missing. strict=False (`<=`) and wide=True (an f64 product) are the two wrong readings the grid
    has to tell from the right one; no test compares a device result with them."""
    k = np.asarray(keys, np.uint64).reshape(-1, K)
    k0, k1 = k[:, 0], k[:, 1]
    d0, d1 = (k0 >> _32).astype(np.uint32).astype(np.float32), (k1 >> _32).astype(np.uint32).astype(np.float32)
    with np.errstate(all="ignore"):
        rhs = d1.astype(np.float64) * np.float64(np.float32(fs)) if wide else d1 * np.float32(fs)
        assert rhs.dtype == (np.float64 if wide else np.float32)
        keep = (d0 < rhs) if strict else (d0 <= rhs)
    keep &= (k0 != EMPTY_KEY) & (k1 != EMPTY_KEY)
    q = np.nonzero(keep)[0]
    return _matches(q, k0[q])


def cross_check_reference(train_best, nq):
    """feature_extraction/src/lib.rs:116-126 on the nearest query of every train row: per query the smallest (distance, train index) among
    the train rows that name it; queries nobody names are absent."""
    tb = np.asarray(train_best, np.uint64).ravel()
    rows = np.nonzero(tb != EMPTY_KEY)[0]
    q = (tb[rows] & _LO).astype(np.int64)
    assert not len(q) or (q.max() < nq and len(rows) < 2 ** 32)
    best = np.full(nq, EMPTY_KEY)
    np.minimum.at(best, q, (tb[rows] & _HI) | rows.astype(np.uint64))
    hit = np.nonzero(best != EMPTY_KEY)[0]
    return _matches(hit, best[hit])


def select_reference(rows, mask, limit=APDS_MAX_POINTS, by_row=True):
    """keypointdb.rs:38-90: the table rows (keypoint records) of `mask`, ORDER BY response DESC LIMIT limit, equal responses (-0.0 equals
    +0.0) by row. Float comparisons only (NaN responses are out of scope). by_row=False orders equal responses by row descending instead:
    the CPU file uses it to show that a case has ties the row has to settle, nothing compares a device result with it."""
    ids = np.nonzero(mask)[0]
    r = np.asarray(rows["response"], np.float32)[ids].astype(np.float64)
    assert not np.isnan(r).any()
    order = np.lexsort((ids if by_row else -ids, -r))[:limit]
    return ids[order]


# ---- ratio test -----------------------------------------------------------------------------------------------------------------------
RATIO_GRID_D = 513                         # every Hamming distance of a 64-byte row, 0..512, on both axes
_f = np.float32
RATIO_FS = (_f(0.0), _f(0.1), _f(0.3), _f(0.6), _f(0.7), _f(0.8), _f(1.0), np.nextafter(_f(1), _f(0)), np.nextafter(_f(1), _f(2)), _f(1.5), _f(-1.0),
            _f(np.inf), _f(np.nan), _f(1e-40))
RATIO_FS_IDS = ("0", "0.1f", "0.3f", "0.6f", "0.7f", "0.8f", "1", "below1", "above1", "1.5", "-1", "inf", "nan", "subnormal")
# cells of the grid where an f64 product decides otherwise than the f32 one (counted with numpy; the CPU file asserts them as a floor)
RATIO_WIDE_FLOOR = {"0.3f": 33, "0.8f": 102, "0.1f": 51, "0.6f": 63}
RATIO_LEQ_FLOOR = 34                       # and where `<=` does, at every fs in RATIO_LEQ_IDS (one cell at least in RATIO_LEQ_ONE_IDS)
RATIO_LEQ_IDS = ("0", "0.1f", "0.3f", "0.6f", "0.7f", "0.8f", "1", "1.5")
RATIO_LEQ_ONE_IDS = ("below1", "above1", "-1", "subnormal")


def ratio_grid_keys():
    """[513 * 513][2]: (d0 << 32 | d0, d1 << 32 | d1) for every pair of distances"""
    d0, d1 = np.divmod(np.arange(RATIO_GRID_D * RATIO_GRID_D, dtype=np.uint64), np.uint64(RATIO_GRID_D))
    return np.stack([make_keys(d0, d0), make_keys(d1, d1)], axis=1)


RATIO_STRUCTURE_NQ = (1, WAVE - 1, WAVE, WAVE + 1)
RATIO_STRUCTURE_K = (2, 5, 16)
TRAIN_MAX = 2 ** 31 - 1


def ratio_structure_keys(nq, K):
    """Rows that pass (d0 = 3, d1 = 9 at fs 0.5), rows that fail, rows whose first, second or both keys are missing, train indices 0 and
    2^31 - 1; the columns from 2 on hold pairs that would pass and that nobody may read (distances 1 and 9, index 0x7000000 + column)."""
    i = np.arange(nq, dtype=np.uint64)
    keys = np.empty((nq, K), np.uint64)
    kind = (i * np.uint64(7) + np.uint64(3)) % np.uint64(6)                       # nq = 1: kind 3
    keys[:, 0] = make_keys(np.where(kind == 1, 5, 3), np.where(i % np.uint64(2) == 0, TRAIN_MAX, 0))
    keys[:, 1] = make_keys(9, np.where(i % np.uint64(2) == 0, 0, TRAIN_MAX))
    keys[kind == 2, 0] = EMPTY_KEY
    keys[kind == 4, 1] = EMPTY_KEY
    keys[kind == 5, :2] = EMPTY_KEY
    for c in range(2, K):
        keys[:, c] = make_keys(9 if c % 2 else 1, 0x7000000 + c)
    return keys


RATIO_STRUCTURE_FS = _f(0.5)

# ---- ordered compaction ---------------------------------------------------------------------------------------------------------------
COMPACTION_NQ = (1, WAVE, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, CARRY_N - 1, CARRY_N, CARRY_N + 1, 2 * CARRY_N + SCAN_BLOCK + 1)
FLAG_PATTERNS = ("all", "none", "first", "last", "block_first", "wave_last", "alternating", "bernoulli", "carry_blocks")
# the patterns that by their own definition set a flag in block 1024 and in the last block once there are more than 1025 blocks
CARRY_PATTERNS = ("all", "block_first", "wave_last", "alternating", "bernoulli", "carry_blocks")


def flag_pattern(name, n):
    i = np.arange(n)
    if name == "all":
        return np.ones(n, bool)
    if name == "none":
        return np.zeros(n, bool)
    if name == "first":
        return i == 0
    if name == "last":
        return i == n - 1
    if name == "block_first":
        return i % SCAN_BLOCK == 0
    if name == "wave_last":                # the last lane of every wave that holds a flag: lane 63, or the lane of flag n - 1
        return (i % WAVE == WAVE - 1) | (i == n - 1)
    if name == "alternating":
        return i % 2 == 0
    if name == "bernoulli":
        f = np.random.default_rng(0xB0 + n % 251).random(n) < 0.5
        f[n - 1] = True                    # (the last block may hold one flag only)
        return f
    if name == "carry_blocks":
        return i >= CARRY_N
    raise KeyError(name)


def compaction_keys(flags):
    """[n][2] keys whose ratio flag at fs = 1 is `flags`: d0 = 0 < d1 = 1 where wanted, d0 = d1 = 1 elsewhere; the train index is a
    hash of the query, so a record in the wrong place shows."""
    flags = np.asarray(flags, bool)
    i = np.arange(len(flags), dtype=np.uint64)
    t = (i * np.uint64(2654435761)) & np.uint64(TRAIN_MAX)
    return np.stack([make_keys(np.where(flags, 0, 1), t), make_keys(1, t ^ np.uint64(1))], axis=1)


# ---- cross-check ----------------------------------------------------------------------------------------------------------------------
def cross_check_cases():
    """name -> (train_best keys, nq). Every query index is below nq."""
    rng = np.random.default_rng(0xCC)
    n = 100_000
    out = {}
    same = make_keys(np.full(n, 40), np.zeros(n))
    out["all_name_query0_equal_distance"] = (same, 3)
    one = same.copy()
    one[n - 1] = make_keys(39, 0)
    out["all_name_query0_last_is_nearer"] = (one, 3)
    holes = same.copy()
    holes[::2] = EMPTY_KEY                                                    # row 0 is missing: row 1 wins
    out["empty_rows_interleaved"] = (holes, 3)
    out["all_rows_empty"] = (np.full(1000, EMPTY_KEY), 70)
    out["one_train_one_query"] = (make_keys([7], [0]), 1)
    out["one_train_row_empty"] = (np.array([EMPTY_KEY]), 1)
    nq = 5000
    out["fewer_train_than_queries"] = (make_keys(rng.integers(0, 4, 700), rng.integers(0, nq, 700)), nq)
    tb = make_keys(rng.integers(0, 3, 60_000), rng.integers(0, 130, 60_000))    # heavy contention at few distances: ties on every query
    tb[rng.random(60_000) < 0.1] = EMPTY_KEY
    tb[(tb & _LO) == np.uint64(64)] = EMPTY_KEY                                 # query 64 is named by nobody
    out["more_train_than_queries_contended"] = (tb, 130)
    nq = CARRY_N + 1
    q = np.concatenate([rng.integers(0, nq, 3000), [0, SCAN_BLOCK - 1, CARRY_N - 1, CARRY_N, CARRY_N, 5, 5]])
    out["carry_loop_sparse_hits"] = (make_keys(rng.integers(0, 512, len(q)), q), nq)
    return out


# ---- keypoint table -------------------------------------------------------------------------------------------------------------------
def fake_keypoints(n, seed):
    """as _fake of test_keypoint_table_gpu.py: positive responses with ties"""
    rng = np.random.default_rng(seed)
    kp = np.zeros(n, KEYPOINT_DTYPE)
    kp["x"], kp["y"] = rng.random(n).astype(np.float32) * 512, rng.random(n).astype(np.float32) * 512
    kp["size"], kp["angle"] = 4.8, rng.random(n).astype(np.float32) * 360
    kp["response"] = (rng.random(n) * 0.05 + 0.001).astype(np.float32)
    kp["response"][:: max(n // 50, 1)] = np.float32(0.0123)
    kp["octave"], kp["class_id"] = rng.integers(0, 4, n), rng.integers(0, 16, n)
    return kp


def random_descriptors(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 61), dtype=np.uint8)


TILE = (512, 512)


def rescale(kp, lod, col=0, row=0, tile=TILE):
    """preprocessor/src/main.rs:299-300 in f32: x * 2^lod + (column * tile_w * 2^lod) as f32"""
    out = kp.copy()
    with np.errstate(invalid="ignore"):
        out["x"] = kp["x"] * np.float32(2.0 ** lod) + np.float32(col * tile[0] * 2 ** lod)
        out["y"] = kp["y"] * np.float32(2.0 ** lod) + np.float32(row * tile[1] * 2 ** lod)
    return out


def runs(*columns):
    """[(start, stop)] of the stretches on which all columns are constant: one insert each"""
    change = np.zeros(len(columns[0]), bool)
    change[0] = True
    for c in columns:
        change[1:] |= c[1:] != c[:-1]
    starts = np.nonzero(change)[0]
    return list(zip(starts.tolist(), starts[1:].tolist() + [len(columns[0])]))


BIG_ROWS = CARRY_N + SCAN_BLOCK + 1        # 1025 full scan blocks and one flag in block 1025
BIG_IMG_DEFAULT, BIG_IMG_BLOCK0, BIG_IMG_BLOCK1024, BIG_IMG_LAST, BIG_IMG_SPARSE = 1, 2, 3, 4, 5
BIG_ROW_BLOCK0, BIG_ROW_BLOCK1024 = 700, CARRY_N + 300


def big_table_columns():
    """(image id, level of detail) of every row of the table with more than 1024 scan blocks. Level of detail 1 is a Bernoulli 5e-4 subset,
    so level 0 alone keeps more than 1024 * 1024 rows: its select runs the carry loop on the table's flags and again on its > 1M keys."""
    rng = np.random.default_rng(0xB16)
    img = np.full(BIG_ROWS, BIG_IMG_DEFAULT, np.int32)
    img[rng.random(BIG_ROWS) < 1e-3] = BIG_IMG_SPARSE
    img[CARRY_N + 700] = BIG_IMG_SPARSE                                          # the subsets reach block 1024 whatever the draw
    img[BIG_ROW_BLOCK0], img[BIG_ROW_BLOCK1024], img[BIG_ROWS - 1] = BIG_IMG_BLOCK0, BIG_IMG_BLOCK1024, BIG_IMG_LAST
    lod = (rng.random(BIG_ROWS) < 5e-4).astype(np.int32)
    lod[CARRY_N + 900] = 1
    lod[[BIG_ROW_BLOCK0, BIG_ROW_BLOCK1024, BIG_ROWS - 1]] = 0
    return img, lod


LIMIT_CUT_CASES = ("exactly_limit", "limit_plus_one", "all_equal", "two_groups", "low_mantissa_byte")
LIMIT_CUT_M = 300_000


def limit_cut_responses(name):
    rng = np.random.default_rng(0x11C)
    if name == "exactly_limit":
        return fake_keypoints(APDS_MAX_POINTS, 41)["response"]
    if name == "limit_plus_one":
        r = fake_keypoints(APDS_MAX_POINTS + 1, 42)["response"]
        r[1000] = np.float32(1e-5)                                              # the one row that leaves, not at either end
        return r
    if name == "all_equal":
        return np.full(LIMIT_CUT_M, 0.0123, np.float32)
    if name == "two_groups":                                                    # 100 000 strong rows scattered among 200 000 weak ones
        r = np.full(LIMIT_CUT_M, 1.0, np.float32)
        r[rng.permutation(LIMIT_CUT_M)[:100_000]] = 2.0
        return r
    if name == "low_mantissa_byte":                                             # 256 values, ~1172 rows each: the cut falls inside one of them
        return (np.uint32(0x3F800000) | rng.integers(0, 256, LIMIT_CUT_M).astype(np.uint32)).view(np.float32)
    raise KeyError(name)


SORT_M = (1, 2, 3, 255, 256, 257)          # around a power of two: the bitonic network pads with all-ones keys up to the next one


def sort_size_responses(m):
    return (np.random.default_rng(m).integers(1, 1 + max(m // 3, 1), m) / 64.0).astype(np.float32)   # every value about three times


RESPONSE_VALUES = np.array([np.inf, 3.0e38, 1.0, np.finfo(np.float32).tiny, 1e-40, 0.0, -0.0, -1e-40, -2.5, -3.0e38], np.float32)


def response_order_values():
    """each value of RESPONSE_VALUES five times, shuffled"""
    return np.random.default_rng(0x0DE).permutation(np.repeat(RESPONSE_VALUES, 5))


# bounding boxes: image id -> (level of detail, column, row) of TILE-sized tiles
BOX_IMAGES = {1: (0, 0, 0), 2: (3, 2, 1), 3: (8, 1, 3), 4: (30, 0, 0), 5: (1, 0, 0)}
# (name, level of detail, (x_start, y_start, x_end, y_end)); floor(start) <= ceil(end) on both axes
EDGE_BOXES = (("fractional_negative", 0, (-0.5, -2.25, 100.25, 50.75)),
              ("integer_ends", 0, (10.0, 20.0, 30.0, 40.0)),
              ("start_above_end_rounds_open", 0, (10.7, 20.0, 10.2, 40.0)),        # floor 10 <= ceil 11
              ("lod3", 3, (8200.5, 4100.25, 8300.5, 4200.75)),
              ("lod8", 8, (131100.5, 393300.5, 131200.0, 393400.0)),
              ("lod30", 30, (2.0 ** 30, 2.0 ** 30, 2.0 ** 31, 2.0 ** 31)))
INVERTED_BOXES = (("inverted_integer", 0, (30.0, 20.0, 10.0, 40.0)), ("inverted_fractional", 0, (12.5, 20.0, 10.5, 40.0)),
                  ("inverted_y", 0, (10.0, 40.5, 30.0, 20.5)))
OTHER_LOD_ROWS = {5: [(10.0, 15.0)], 1: [(8250.0, 4150.0)]}                       # inside integer_ends at lod 1, inside lod3 at lod 0


def box_bounds(box):
    """floor(x_start), floor(y_start), ceil(x_end), ceil(y_end) of the f32 arguments"""
    b = np.asarray(box, np.float32)
    return np.floor(b[0]), np.floor(b[1]), np.ceil(b[2]), np.ceil(b[3])


def box_edge_targets(box):
    """(x, y, inside) in table coordinates: the centre, and per edge one row on it (inside: both ends are inclusive) and one an ulp beyond"""
    x0, y0, x1, y1 = box_bounds(box)
    xm, ym = np.float32((np.float64(x0) + x1) / 2), np.float32((np.float64(y0) + y1) / 2)
    lo, hi = np.float32(-np.inf), np.float32(np.inf)
    return [(xm, ym, True),
            (x0, ym, True), (np.nextafter(x0, lo), ym, False), (x1, ym, True), (np.nextafter(x1, hi), ym, False),
            (xm, y0, True), (xm, np.nextafter(y0, lo), False), (xm, y1, True), (xm, np.nextafter(y1, hi), False),
            (x0, y0, True), (x1, y1, True)]


def box_table():
    """[(image id, level of detail, column, row, keypoints)] in insert order: per image 200 random rows, the edge rows of its boxes
    (as the tile coordinates that the rescale lifts onto them), at level 0 a row with a NaN x, one with a NaN y and one at (-0.5, -0.5),
    and the rows of OTHER_LOD_ROWS."""
    out = []
    for image_id, (lod, col, row) in BOX_IMAGES.items():
        scale, xoff, yoff = 2.0 ** lod, col * TILE[0] * 2.0 ** lod, row * TILE[1] * 2.0 ** lod
        pts = [((np.float64(x) - xoff) / scale, (np.float64(y) - yoff) / scale) for _, blod, box in EDGE_BOXES if blod == lod
               for x, y, _ in box_edge_targets(box)]
        pts += OTHER_LOD_ROWS.get(image_id, [])
        if lod == 0:
            pts += [(np.nan, 30.0), (20.0, np.nan), (-0.5, -0.5)]
        kp = fake_keypoints(200 + len(pts), 500 + image_id)
        if pts:
            kp["x"][200:], kp["y"][200:] = np.array(pts, np.float64).T.astype(np.float32)
        out.append((image_id, lod, col, row, kp))
    return out


def box_mask(kp, lod, box_lod, box, strict=False):
    """the predicate of keypointdb.rs:67-90 on rescaled rows. strict=True is the wrong reading that drops the rows on an edge."""
    x0, y0, x1, y1 = box_bounds(box)
    x, y = kp["x"], kp["y"]
    with np.errstate(invalid="ignore"):
        if strict:
            return (lod == box_lod) & (x > x0) & (x < x1) & (y > y0) & (y < y1)
        return (lod == box_lod) & (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
