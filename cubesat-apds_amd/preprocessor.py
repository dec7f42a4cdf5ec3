"""Host-side mirror of the reference's tile scheduler (/root/reference/preprocessor/src/main.rs:175-327): every
level of detail of a mosaic is cut into tiles of one fixed pixel size, each tile goes through to_rgb -> raster_to_mat -> AKAZE,
and its keypoints are stored with their coordinates lifted back to level-0 pixels. The reference writes to Postgres through a
rayon pool; here the rows go to the GPU-resident KeypointTable (feature_database.py) and an in-memory image table."""
from . import _lib, feature_extraction, homographier
from .geotiff_extractor import DeviceMosaic


class ImageTable:
    """feature_database `ref_image` rows (models.rs InsertImage: level_of_detail, x_start, x_end, y_start, y_end); ids are 1-based
    serials as Postgres assigns them (imagedb.rs create_image returns the new id)."""

    def __init__(self):
        self.rows = []

    def create_image(self, level_of_detail, x_start, x_end, y_start, y_end):
        self.rows.append(dict(id=len(self.rows) + 1, level_of_detail=int(level_of_detail), x_start=int(x_start), x_end=int(x_end),
                              y_start=int(y_start), y_end=int(y_end)))
        return self.rows[-1]["id"]


def tile_grid(image_resolution, amount_lod, lod):
    """main.rs:212-216 — (tile_size, columns, rows) of level `lod` out of `amount_lod` levels (integer arithmetic as in the reference)."""
    tile_size = (image_resolution[0] // 2 ** (amount_lod - 1), image_resolution[1] // 2 ** (amount_lod - 1))
    columns = image_resolution[0] // (tile_size[0] * 2 ** lod)
    rows = image_resolution[1] // (tile_size[1] * 2 ** lod)
    return tile_size, columns, rows


def extract_tile(dataset, tile_size, column, row, lod, fused=True, resample="nearest", mask_nodata=False):
    """main.rs:258-277 — the part of one tile that does not touch the database: read, convert, extract. Thread-safe (the C ABI
    gives every calling thread its own stream and workspace, as the reference's rayon workers each own their OpenCV objects).
    resample: how a level > 0 window becomes a tile ("nearest", or "lanczos" as the reference reads it, mod.rs:339). A DeviceMosaic
    dataset is read, resampled and extracted on the device in one call.
    mask_nodata: the tile's alpha, which band_merger sets to 0 where all three bands are NaN (mod.rs:346-378) and the reference never reads
    again, is the extraction's mask (detectAndCompute's `mask`, empty at lib.rs:75-79): the edges of a nodata area leave no rows.
    "support" beside True / False: the mask reaches over the descriptor's support (mask_support 15), so no stored descriptor has sampled
    nodata; True consults the keypoint's own pixel alone."""
    span = (tile_size[0] * 2 ** lod, tile_size[1] * 2 ** lod)
    if isinstance(dataset, DeviceMosaic):
        return feature_extraction.mosaic_tile_keypoint_descriptor_extraction(dataset, (column * span[0], row * span[1]), span, tile_size, resample,
                                                                             mask_nodata=mask_nodata)
    extra = {} if resample == "nearest" else {"resample": resample}
    if fused:
        # the same three steps inside the library: the band windows go to the GPU once and the 8-bit image never comes back
        win = dataset.window((column * span[0], row * span[1]), span, tile_size, **extra)
        return feature_extraction.tile_keypoint_descriptor_extraction(win[0], win[1], win[2], dataset.datasets_min_max(), None, mask_nodata)
    tile = dataset.to_rgb((column * span[0], row * span[1]), span, tile_size, **extra)            # main.rs:258-272
    tile_mat = homographier.raster_to_mat(tile, tile_size[0], tile_size[1])                       # main.rs:274
    if mask_nodata:
        support = _lib.MASK_SUPPORT_DESCRIPTOR if feature_extraction._mask_mode(mask_nodata) == _lib.TILE_MASK_ALPHA_SUPPORT else 0
        return feature_extraction.akaze_keypoint_descriptor_extraction(tile_mat.mat, tile_mat.mat[..., 3], None, support)
    return feature_extraction.akaze_keypoint_descriptor_extraction_def(tile_mat.mat, None)        # main.rs:277


def create_tile_image(images, tile_size, column, row, lod):
    """main.rs:280-293 — the image row of one tile. Returns its id."""
    span = (tile_size[0] * 2 ** lod, tile_size[1] * 2 ** lod)
    return images.create_image(lod, column * span[0], column * span[0] + span[0] - 1, row * span[1], row * span[1] + span[1] - 1)


def store_tile(table, images, keypoints, tile_size, column, row, lod):
    """main.rs:280-324 — the image row and its keypoints. Returns (image_id, n_keypoints)."""
    image_id = create_tile_image(images, tile_size, column, row, lod)                              # main.rs:280-293
    # main.rs:296-324: x = x * 2^lod + column * tile_w * 2^lod (same for y), one multi-row INSERT
    table.create_keypoints(keypoints, image_id, lod, column, row, tile_size)
    return image_id, len(keypoints.keypoints)


def feature_extraction_to_database(table, images, dataset, tile_size, column, row, lod, fused=True, resample="nearest", mask_nodata=False):
    """main.rs:248-327 — one tile: read, convert, extract, insert the image row and its keypoints. Returns (image_id, n_keypoints)."""
    return store_tile(table, images, extract_tile(dataset, tile_size, column, row, lod, fused, resample, mask_nodata), tile_size, column, row, lod)


def downscale_from_lod(table, images, dataset, amount_lod, lod, workers=1, fused=True, batch=1, resample="nearest", mask_nodata=False, device_insert=False):
    """main.rs:197-246 — every tile of one level. The reference spawns the tiles on a rayon pool (main.rs:233-243) and image ids
    follow whatever order the inserts reach Postgres in; here the rows are stored in row-major tile order, so ids and table contents
    depend neither on `workers` nor on `batch`. Small tiles are launch-latency-bound on the GPU, so either `batch` tiles go through
    ONE library call (apds_tile_extract_batch: every kernel's grid covers all of them; the preferred form, one host thread) or
    `workers` threads extract tiles concurrently on their own streams. With a DeviceMosaic dataset the batch call is
    apds_mosaic_tile_extract_batch: one resampling launch per pass for the whole group, no band window crosses PCIe.
    mask_nodata (see extract_tile) reaches all three forms.
    device_insert: every group of max(batch, 1) tiles of a DeviceMosaic goes through ONE call that extracts them and appends their rows to
    the table on the device (apds_mosaic_tiles_to_db): no keypoint crosses PCIe, one synchronise per group instead of one per tile. Image
    rows, the returned list and the table are those of the `batch` form."""
    if device_insert and not isinstance(dataset, DeviceMosaic):
        raise ValueError("device_insert=True needs a DeviceMosaic dataset: the rows go from the extraction to the table on the device")
    tile_size, columns, rows = tile_grid(dataset.raster_size(), amount_lod, lod)
    cells = [(j, i) for i in range(rows) for j in range(columns)]
    extra = {} if resample == "nearest" else {"resample": resample}
    if device_insert:
        span = (tile_size[0] * 2 ** lod, tile_size[1] * 2 ** lod)
        step = max(int(batch), 1)
        out = []
        for k in range(0, len(cells), step):
            group = cells[k:k + step]
            ids = [create_tile_image(images, tile_size, j, i, lod) for j, i in group]
            if ids != list(range(ids[0], ids[0] + len(ids))):
                raise ValueError("device_insert=True needs an image table that hands out consecutive ids")
            counts = feature_extraction.mosaic_tiles_to_database(dataset, table, [(j * span[0], i * span[1]) for j, i in group], span, tile_size, group,
                                                                 ids[0], lod, resample, mask_nodata=mask_nodata)
            out += list(zip(ids, counts))
        return out
    if batch > 1:
        span = (tile_size[0] * 2 ** lod, tile_size[1] * 2 ** lod)
        out = []
        for k in range(0, len(cells), batch):
            group = cells[k:k + batch]
            if isinstance(dataset, DeviceMosaic):
                extracted = feature_extraction.mosaic_tiles_keypoint_descriptor_extraction(dataset, [(j * span[0], i * span[1]) for j, i in group], span,
                                                                                           tile_size, resample, mask_nodata=mask_nodata)
            else:
                wins = [dataset.window((j * span[0], i * span[1]), span, tile_size, **extra) for j, i in group]
                extracted = feature_extraction.tiles_keypoint_descriptor_extraction(wins, dataset.datasets_min_max(), None, mask_nodata)
            for (j, i), kp in zip(group, extracted):
                out.append(store_tile(table, images, kp, tile_size, j, i, lod))
        return out
    if workers <= 1:
        return [feature_extraction_to_database(table, images, dataset, tile_size, j, i, lod, fused, resample, mask_nodata) for j, i in cells]
    from concurrent.futures import ThreadPoolExecutor, wait
    import threading
    from ._lib import lib

    def work(cell):
        return extract_tile(dataset, tile_size, cell[0], cell[1], lod, fused, resample, mask_nodata)

    # every pool thread gives its stream + device workspace back before the pool goes away: the barrier makes each of the
    # `workers` threads take exactly one release task
    barrier = threading.Barrier(workers)

    def release():
        # generous, but finite: if one of the `workers` release tasks never reaches the barrier (a pool thread that could not start, an
        # exception in front of the wait) the others must not block the pool's shutdown for ever; the thread's context is released either way
        try:
            barrier.wait(timeout=120.0)
        except threading.BrokenBarrierError:
            pass
        finally:
            lib().apds_thread_release()

    out, pending = [], []
    with ThreadPoolExecutor(max_workers=workers) as pool:
        try:
            # bounded look-ahead: at most 2 x workers extracted tiles wait for their turn to be stored
            for cell in cells:
                pending.append((cell, pool.submit(work, cell)))
                if len(pending) >= 2 * workers:
                    (j, i), fut = pending.pop(0)
                    out.append(store_tile(table, images, fut.result(), tile_size, j, i, lod))
            while pending:
                (j, i), fut = pending.pop(0)
                out.append(store_tile(table, images, fut.result(), tile_size, j, i, lod))
        finally:
            # on an error above tiles may still be running: drain them first (cancel what has not started), so that every pool thread
            # is free to take its release task and the barrier cannot be left waiting; a failing release never replaces the
            # exception that brought us here
            for _, fut in pending:
                fut.cancel()
            wait([fut for _, fut in pending])
            for f in [pool.submit(release) for _ in range(workers)]:
                try:
                    f.result()
                except Exception:   # noqa: BLE001
                    pass
    return out


def replace_tiles(table, images, dataset, amount_lod, lod, cells, batch=1, resample="nearest", mask_nodata=False):
    """The tiles `cells` = [(column, row), ...] of level `lod` again, from a DeviceMosaic that now holds their new imagery: the rows of each
    tile's image leave the table (KeypointTable.delete_keypoints_from_image_id) and the tile goes through the device_insert path of
    downscale_from_lod once more, under the image id it already has. The tiles' new rows follow every row that stayed, in the order of
    `cells`, with new keypoint ids; nothing else in the table changes. Returns [(image_id, n_deleted, n_inserted), ...]."""
    if not isinstance(dataset, DeviceMosaic):
        raise ValueError("replace_tiles needs a DeviceMosaic dataset: the rows go from the extraction to the table on the device")
    tile_size, _, _ = tile_grid(dataset.raster_size(), amount_lod, lod)
    span = (tile_size[0] * 2 ** lod, tile_size[1] * 2 ** lod)
    by_place = {(r["level_of_detail"], r["x_start"], r["y_start"]): r["id"] for r in images.rows}
    cells = [(int(j), int(i)) for j, i in cells]
    try:
        ids = [by_place[(int(lod), j * span[0], i * span[1])] for j, i in cells]
    except KeyError:
        raise ValueError("replace_tiles: a tile that has no image row cannot be replaced") from None
    deleted = [table.delete_keypoints_from_image_id(image_id) for image_id in ids]
    inserted, k, step = [], 0, max(int(batch), 1)
    while k < len(cells):          # one call per run of consecutive image ids, `batch` tiles at the most
        e = k + 1
        while e < len(cells) and e - k < step and ids[e] == ids[e - 1] + 1:
            e += 1
        inserted += feature_extraction.mosaic_tiles_to_database(dataset, table, [(j * span[0], i * span[1]) for j, i in cells[k:e]], span, tile_size,
                                                                cells[k:e], ids[k], lod, resample, mask_nodata=mask_nodata)
        k = e
    return list(zip(ids, deleted, inserted))


def process_lod_from_mosaic(table, images, dataset, lod, workers=1, fused=True, batch=1, resample="nearest", mask_nodata=False, device_insert=False,
                            descriptor=None):
    """main.rs:175-194 — all levels 0 .. lod-1.
    descriptor: None (the table's own kind), "mldb" or "kaze": it must be the kind of `table` (KeypointTable(.., descriptor=..)). A float
    ("kaze") table is built through device_insert only: apds_mosaic_tiles_to_db extracts rows of the table's kind, and the keypoint columns
    are the ones a byte table gets from the same tiles."""
    kind = getattr(table, "descriptor", "mldb")
    if descriptor is not None and descriptor != kind:
        raise ValueError(f"descriptor={descriptor!r} but the table holds {kind!r} rows: make it with KeypointTable(capacity, descriptor={descriptor!r})")
    if kind == "kaze" and not device_insert:
        raise ValueError('a float ("kaze") table is built with device_insert=True')
    if device_insert and not isinstance(dataset, DeviceMosaic):
        raise ValueError("device_insert=True needs a DeviceMosaic dataset: the rows go from the extraction to the table on the device")
    return [downscale_from_lod(table, images, dataset, lod, i, workers, fused, batch, resample, mask_nodata, device_insert) for i in range(lod)]
