"""Inputs of test_stream_order_gpu.py (checked on the CPU by test_stream_order_inputs_cpu.py): per device entry a REAL input set and a DECOY of
the same shapes and types whose correct output differs. The GPU tests put the decoy into the buffers first and bring the real input in on
the caller's stream, behind a delay (or overwrite the real input with the decoy right after the call): an entry that does part of its work
off that stream answers from the decoy. Decoys are valid inputs - indices in range, key lists ascending - so a misordered run gives a
defined wrong answer and never an access out of range.

Restated from the code: hm_sample_rows (csrc/hamming_mfma.hip) starts the threshold launch at 65 536 train rows."""
import numpy as np

import filter_border_cases as bc

HM_SAMPLE_THRESHOLD = 65536                 # csrc/hamming_mfma.hip: hm_sample_rows, "none below 65 536 rows"
TOPK_NT = (3001, HM_SAMPLE_THRESHOLD + 777)  # below / above it; neither a multiple of a tile
TOPK_NQ = 300                               # no multiple of a wave or of a tile
TOPK_K = (1, 2, 3)
BACKEND_VECTOR, BACKEND_MFMA2, BACKEND_MFMA8 = 1, 2, 3   # apds_dev_hamming_topk_backend


def mfma_backend(k):
    return BACKEND_MFMA2 if k <= 2 else BACKEND_MFMA8


def pad64(rows):
    return np.ascontiguousarray(np.pad(rows, ((0, 0), (0, 64 - rows.shape[1]))))


def descriptor_pair(synth, nt, nq, seed):
    """(queries [nq, 61], train [nt, 61]) - queries planted near train rows, as synth makes them"""
    db = synth.make_descriptor_db(nt, seed=seed)
    q, _ = synth.make_queries(db, nq, seed=seed + 1)
    return np.ascontiguousarray(q), np.ascontiguousarray(db)


def topk_inputs(synth, nt):
    """real and decoy (q, t) of one train size"""
    return descriptor_pair(synth, nt, TOPK_NQ, 700 + nt % 97), descriptor_pair(synth, nt, TOPK_NQ, 900 + nt % 97)


# ---- apds_dev_pack_descriptors ------------------------------------------------------------------------------------------------------
PACK_N, PACK_BYTES, PACK_STRIDE = 1001, 61, 80


def pack_inputs():
    rng = np.random.default_rng(11)
    return tuple(rng.integers(0, 256, (PACK_N, PACK_STRIDE), dtype=np.uint8) for _ in range(2))


def pack_reference(src):
    out = np.zeros((len(src), 64), np.uint8)
    out[:, :PACK_BYTES] = src[:, :PACK_BYTES]
    return out


# ---- apds_dev_merge_topk ------------------------------------------------------------------------------------------------------------
MERGE_PARTS, MERGE_NQ, MERGE_K = 5, 300, 2


def merge_inputs():
    """[parts][nq][k] key lists, ascending, distinct, some short"""
    out = []
    for seed in (21, 22):
        rng = np.random.default_rng(seed)
        keys = rng.permutation(MERGE_PARTS * MERGE_NQ * MERGE_K).astype(np.uint64).reshape(MERGE_PARTS, MERGE_NQ, MERGE_K) * np.uint64(977) + np.uint64(1 << 32)
        keys[rng.random(keys.shape) < 0.2] = bc.EMPTY_KEY
        keys.sort(axis=2)
        out.append(keys)
    return tuple(out)


def merge_reference(keys):
    parts, nq, k = keys.shape
    return np.sort(keys.transpose(1, 0, 2).reshape(nq, parts * k), axis=1)[:, :k]


# ---- filters: keys of a real top-2 / top-1 answer -----------------------------------------------------------------------------------
FILTER_NQ, FILTER_NT, FILTER_FS = 700, 1500, np.float32(0.8)


def filter_descriptors(synth):
    return descriptor_pair(synth, FILTER_NT, FILTER_NQ, 31), descriptor_pair(synth, FILTER_NT, FILTER_NQ, 41)


# ---- apds_dev_l2_topk ---------------------------------------------------------------------------------------------------------------
L2_NQ, L2_NT, L2_DIMS = 300, 2100, (128, 64)


def l2_inputs(dim):
    out = []
    for seed in (51, 52):
        rng = np.random.default_rng(seed + dim)
        t = rng.standard_normal((L2_NT, dim)).astype(np.float32)
        q = (t[rng.integers(0, L2_NT, L2_NQ)] + 0.05 * rng.standard_normal((L2_NQ, dim))).astype(np.float32)
        out.append((q, t))
    return tuple(out)


def l2_nearest(q, t):
    """index of the nearest train row in float64 (the planted source row, far from every other)"""
    d = (q.astype(np.float64) ** 2).sum(1)[:, None] + (t.astype(np.float64) ** 2).sum(1)[None, :] - 2 * q.astype(np.float64) @ t.astype(np.float64).T
    return d.argmin(1)


# ---- apds_dev_band_merger -----------------------------------------------------------------------------------------------------------
BAND_N = 100003
BAND_MINMAX = np.array([0.0, 1.0, 0.1, 0.9, -0.1, 1.1], np.float64)


def band_inputs():
    out = []
    for seed in (61, 62):
        rng = np.random.default_rng(seed)
        bands = [rng.uniform(-0.2, 1.3, BAND_N).astype(np.float32) for _ in range(3)]
        bands[0][::17] = np.nan
        out.append(tuple(bands))
    return tuple(out)


# ---- apds_dev_mask_zero_sat ---------------------------------------------------------------------------------------------------------
SAT_ROWS, SAT_COLS = 131, 259


def sat_inputs():
    return tuple((np.random.default_rng(seed).random((SAT_ROWS, SAT_COLS)) < 0.7).astype(np.uint8) * 255 for seed in (71, 72))


def sat_reference(mask):
    out = np.zeros((mask.shape[0] + 1, mask.shape[1] + 1), np.uint32)
    out[1:, 1:] = np.cumsum(np.cumsum(mask == 0, axis=0), axis=1)
    return out


# ---- apds_dev_points_from_matches / apds_dev_pnp_correspondences --------------------------------------------------------------------
POINTS_N1, POINTS_N2, POINTS_NM = 900, 1300, 777
PNP_ORIGIN = np.array([1000.0, -2000.0, 30.0], np.float64)


def point_inputs():
    """(kp1, kp2, matches, xyz) twice: keypoint records, matches with every index in range, world points of the train rows"""
    out = []
    for seed in (81, 82):
        rng = np.random.default_rng(seed)
        kp1, kp2 = np.zeros(POINTS_N1, bc.KEYPOINT_DTYPE), np.zeros(POINTS_N2, bc.KEYPOINT_DTYPE)
        for kp in (kp1, kp2):
            kp["x"], kp["y"] = rng.uniform(0, 4096, len(kp)).astype(np.float32), rng.uniform(0, 4096, len(kp)).astype(np.float32)
        m = np.zeros(POINTS_NM, bc.DMATCH_DTYPE)
        m["query_idx"], m["train_idx"] = rng.integers(0, POINTS_N1, POINTS_NM), rng.integers(0, POINTS_N2, POINTS_NM)
        xyz = np.float64(np.float32(rng.uniform(-5000, 5000, (POINTS_N2, 3))))
        out.append((kp1, kp2, m, xyz))
    return tuple(out)


def points_reference(kp1, kp2, m):
    q, t = m["query_idx"], m["train_idx"]
    return np.stack([kp1["x"][q], kp1["y"][q]], 1), np.stack([kp2["x"][t], kp2["y"][t]], 1)


def correspondences_reference(kp1, xyz, m):
    q, t = m["query_idx"], m["train_idx"]
    return np.stack([kp1["x"][q], kp1["y"][q]], 1), np.float32(xyz[t] - PNP_ORIGIN)


# ---- apds_dev_find_homography -------------------------------------------------------------------------------------------------------
HOMOGRAPHY_N = 1200
HOMOGRAPHY_METHODS = (0, 8)                 # least squares over all pairs; RANSAC (include/apds.h APDS_HOMOGRAPHY_RANSAC)


def homography_inputs(synth):
    """(src, dst) twice, of two different homographies"""
    out = []
    for seed in (91, 92):
        src, dst, _, _ = synth.make_ransac_set(HOMOGRAPHY_N, seed=seed)
        out.append((np.ascontiguousarray(src, np.float32), np.ascontiguousarray(dst, np.float32)))
    return tuple(out)


# ---- apds_dev_akaze_extract(_batch) -------------------------------------------------------------------------------------------------
AKAZE_SINGLE = (256, 256, 4)                # rows, cols, channels
AKAZE_BATCH = (3, 200, 240, 1)              # images, rows, cols, channels
AKAZE_CAP = 8192


def akaze_single_inputs(synth):
    r, c, ch = AKAZE_SINGLE
    return tuple(np.ascontiguousarray(synth.make_tile(r, c, frame_index=f, channels=ch)) for f in (3, 17))


def akaze_batch_inputs(synth):
    b, r, c, ch = AKAZE_BATCH
    return tuple(np.ascontiguousarray(np.stack([synth.make_tile(r, c, frame_index=f0 + i, channels=ch).reshape(r, c, ch) for i in range(b)])) for f0 in (30, 50))


# ---- two streams, one thread --------------------------------------------------------------------------------------------------------
PAIR_X = (2048, HM_SAMPLE_THRESHOLD)         # the long call: queries, train rows
PAIR_Y = (256, 2048)                        # the four short calls that start with it
PAIR_STREAMS = 4
PAIR_L2_DIM = 128

# ---- the keypoint table: device insert (apds_db_insert_dev / apds_db_insert_batch_dev) ------------------------------------------------
INSERT_TABLE_ROWS = 2048                    # capacity of the fresh table every run inserts into
INSERT_N = 777
INSERT_ARGS = (5, 1, 3, 2, 640, 352)        # image id, level of detail, tile column, tile row, tile width, tile height
INSERT_BATCH_TILES, INSERT_BATCH_CAP, INSERT_BATCH_COUNTS = 2, 400, (399, 123)   # rows of capacity per tile, rows used
INSERT_BATCH_COLUMNS_ROWS = np.array([0, 0, 1, 0], np.uint32)                     # (column, row) per tile


def _table_rows(rng, n):
    """n keypoint records and n 64-byte descriptor rows (61 bytes + zero padding); responses quantised, so that many are equal"""
    kp = np.zeros(n, bc.KEYPOINT_DTYPE)
    kp["x"], kp["y"] = rng.uniform(0, 640, n).astype(np.float32), rng.uniform(0, 352, n).astype(np.float32)
    kp["size"], kp["angle"] = np.float32(4.8), rng.uniform(0, 360, n).astype(np.float32)
    kp["response"] = (rng.integers(1, 200, n) / np.float32(1000)).astype(np.float32)
    kp["octave"], kp["class_id"] = rng.integers(0, 3, n), rng.integers(0, 4, n)
    desc = np.zeros((n, 64), np.uint8)
    desc[:, :61] = rng.integers(0, 256, (n, 61), dtype=np.uint8)
    return kp, desc


def insert_inputs():
    return tuple(_table_rows(np.random.default_rng(seed), INSERT_N) for seed in (101, 102))


def insert_batch_inputs():
    """(keypoints, rows) of INSERT_BATCH_TILES tiles, INSERT_BATCH_CAP rows apart; the rows past a tile's count hold data nobody may read"""
    return tuple(_table_rows(np.random.default_rng(seed), INSERT_BATCH_TILES * INSERT_BATCH_CAP) for seed in (103, 104))


def insert_batch_rows(desc):
    """the descriptor column after the batch insert: every tile's first count rows, in tile order"""
    return np.concatenate([desc[i * INSERT_BATCH_CAP: i * INSERT_BATCH_CAP + c] for i, c in enumerate(INSERT_BATCH_COUNTS)])


# ---- apds_db_view_select ----------------------------------------------------------------------------------------------------------------
# One table of three images at two levels of detail. The entry's device input is the table itself, which must not change while a select is
# in flight; what a select can get wrong in time shows in the VIEW's buffers: they hold the decoy selection (the other level of detail)
# when the real one is queued behind the delay.
VIEW_TABLE_ROWS = 2048
VIEW_IMAGES = ((1, 0, 700), (2, 1, 500), (3, 0, 333))   # image id, level of detail, rows
VIEW_TILE = (640, 352)
VIEW_REAL, VIEW_DECOY = (1, 0), (1, 1)      # (mode, value): all rows of level of detail 0 / of level of detail 1


def view_table():
    """[(image id, lod, keypoints, 61-byte descriptors)] in insertion order"""
    rng = np.random.default_rng(111)
    out = []
    for image_id, lod, n in VIEW_IMAGES:
        kp, desc = _table_rows(rng, n)
        out.append((image_id, lod, kp, np.ascontiguousarray(desc[:, :61])))
    return out


def view_reference(selection):
    """(table rows of the selection in view order, their image ids): response descending, equal responses by row (bc.select_reference)"""
    t = view_table()
    kp = np.concatenate([x[2] for x in t])
    lod = np.concatenate([np.full(len(x[2]), x[1]) for x in t])
    img = np.concatenate([np.full(len(x[2]), x[0]) for x in t]).astype(np.int32)
    assert selection[0] == 1
    rows = bc.select_reference(kp, lod == selection[1])
    return np.asarray(rows, np.int32), img[rows]
