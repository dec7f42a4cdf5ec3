"""CPU: the bookkeeping of the preprocessor's device_insert path (apds_mosaic_tiles_to_db per group of tiles) without a device: it refuses a
host dataset before any device work, and on a stub DeviceMosaic whose library calls are replaced by recorders it walks the same tile grid,
creates the same ImageTable rows and returns the same (image_id, n) lists as the batch path it stands beside."""
import numpy as np
import pytest


def test_device_insert_needs_a_device_mosaic(pkg, monkeypatch):
    ge, pp, fe = pkg.geotiff_extractor, pkg.preprocessor, pkg.feature_extraction

    def no_device_work(*a, **k):
        raise AssertionError("device work before the dataset was checked")

    for name in ("mosaic_tiles_to_database", "mosaic_tiles_keypoint_descriptor_extraction", "tiles_keypoint_descriptor_extraction",
                 "tile_keypoint_descriptor_extraction"):
        monkeypatch.setattr(fe, name, no_device_work)
    ds = ge.MosaicedDataset(np.zeros((3, 64, 64), np.float32))
    images = pp.ImageTable()
    with pytest.raises(ValueError):
        pp.process_lod_from_mosaic(object(), images, ds, 2, batch=4, device_insert=True)
    with pytest.raises(ValueError):
        pp.downscale_from_lod(object(), images, ds, 2, 0, batch=4, device_insert=True)
    assert images.rows == []


def _count(column, row, lod):
    return 100 + 7 * column + 13 * row + 1000 * lod


@pytest.mark.parametrize("size,levels,batch", [((1024, 1024), 2, 4), ((2048, 1024), 3, 3), ((1024, 1024), 1, 1), ((2048, 2048), 3, 0)])
def test_bookkeeping_equals_the_batch_path(pkg, monkeypatch, size, levels, batch):
    ge, pp, fe = pkg.geotiff_extractor, pkg.preprocessor, pkg.feature_extraction

    class Stub(ge.DeviceMosaic):
        def __init__(self):      # no handle: every library call is replaced below
            pass

        def raster_size(self):
            return size

        def close(self):
            pass

    class Table:
        def __init__(self):
            self.inserts = []

        def create_keypoints(self, extracted, image_id, level_of_detail=0, column=0, row=0, tile_size=(0, 0)):
            self.inserts.append((int(image_id), int(level_of_detail), int(column), int(row), tuple(tile_size), len(extracted.keypoints)))

    calls = {"old": [], "new": []}

    def old_extract(mosaic, windows, window_size, tile, resample="nearest", min_max=None, max_points=None, mask_nodata=False):
        calls["old"].append((list(windows), tuple(window_size), tuple(tile), resample, mask_nodata))
        lod = int(np.log2(window_size[0] // tile[0]))
        return [fe.ExtractedKeyPoint(np.zeros(_count(x // window_size[0], y // window_size[1], lod), pkg._lib.KEYPOINT_DTYPE), None) for x, y in windows]

    def new_store(mosaic, table, windows, window_size, tile, columns_rows, first_image_id, level_of_detail, resample="nearest", min_max=None, max_points=None,
                  mask_nodata=False):
        calls["new"].append((list(windows), tuple(window_size), tuple(tile), resample, mask_nodata))
        counts = [_count(j, i, level_of_detail) for j, i in columns_rows]
        for k, ((j, i), n) in enumerate(zip(columns_rows, counts)):
            table.inserts.append((first_image_id + k, int(level_of_detail), int(j), int(i), tuple(tile), n))
        return counts

    monkeypatch.setattr(fe, "mosaic_tiles_keypoint_descriptor_extraction", old_extract)
    monkeypatch.setattr(fe, "mosaic_tiles_to_database", new_store)
    ds = Stub()
    t_old, i_old, t_new, i_new = Table(), pp.ImageTable(), Table(), pp.ImageTable()
    # the batch path needs batch > 1 to take its grouped form; groups of max(batch, 1) tiles give the same rows whatever the group size
    out_old = pp.process_lod_from_mosaic(t_old, i_old, ds, levels, batch=max(batch, 2), resample="lanczos", mask_nodata="support")
    out_new = pp.process_lod_from_mosaic(t_new, i_new, ds, levels, batch=batch, resample="lanczos", mask_nodata="support", device_insert=True)
    assert out_new == out_old and i_new.rows == i_old.rows and t_new.inserts == t_old.inserts
    assert len(i_new.rows) == sum(c * r for _, c, r in (pp.tile_grid(size, levels, lod) for lod in range(levels)))
    # the groups: max(batch, 1) cells each, in row-major tile order, every level on its own
    step = max(batch, 1)
    want_groups = []
    for lod in range(levels):
        tile, columns, rows = pp.tile_grid(size, levels, lod)
        span = (tile[0] * 2 ** lod, tile[1] * 2 ** lod)
        cells = [(j * span[0], i * span[1]) for i in range(rows) for j in range(columns)]
        want_groups += [(cells[k:k + step], span, tile, "lanczos", "support") for k in range(0, len(cells), step)]
    assert calls["new"] == want_groups
