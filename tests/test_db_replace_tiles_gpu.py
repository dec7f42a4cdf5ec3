"""GPU: "replace these tiles" = delete the tiles' rows, extract and insert the tiles again, all on the device.

 * preprocessor.replace_tiles on a table of four 256 x 256 tiles A, B, C, D leaves the table a fresh build in the order A, C, D, B
   holds - every column, the descriptors, the world points - with the old ids of A, C and D followed by new ones for B;
 * the streamed pipeline (whole table and per-frame view) and the pose stage on a table after a delete return what they return on a
   fresh table that holds the same rows: trainIdx is the row in both."""
from importlib import import_module

import numpy as np
import pytest

from db_table_snapshot import Snapshot, assert_same

pytestmark = pytest.mark.gpu

T = 256
DGT = [9.0, 1e-4, 0, 57.0, 0, -1e-4]
KMAT = np.array([[900.0, 0, 128], [0, 900.0, 128], [0, 0, 1]])
POSE = dict(method=1, iter_count=100, reproj_thres=8.0, confidence=0.99)


def _elevation(pkg):
    et = pkg.feature_database.ElevationTable()
    et.create_geotransform("dataset", DGT)
    return et


@pytest.fixture(scope="module")
def mosaic(gpu_pkg):
    """a three-band 512 x 512 mosaic: four tiles of 256 x 256 at level 0 of two levels"""
    t = gpu_pkg.synth.make_tile(2 * T, 2 * T, frame_index=11, channels=3, blobs_per_mpx=20000).astype(np.float32)
    dm = gpu_pkg.geotiff_extractor.DeviceMosaic(np.stack([t[:, :, 2] * 3.0 + 10.0, t[:, :, 1] * 2.0 - 5.0, t[:, :, 0] * 1.5]))
    yield dm
    dm.close()


def test_replace_equals_rebuild(gpu_pkg, mosaic):
    pkg = gpu_pkg
    pp, fd, fe = pkg.preprocessor, pkg.feature_database, pkg.feature_extraction
    table, fresh, images = fd.KeypointTable(20000), fd.KeypointTable(20000), pp.ImageTable()
    try:
        built = pp.downscale_from_lod(table, images, mosaic, 2, 0, batch=4, device_insert=True)          # A, B, C, D = images 1 .. 4
        assert [i for i, _ in built] == [1, 2, 3, 4] and min(n for _, n in built) >= 20
        counts = dict(built)
        total = len(table)
        before = Snapshot(pkg, table, [1, 2, 3, 4], (0,))
        assert np.array_equal(before.ids, np.arange(1, total + 1))

        done = pp.replace_tiles(table, images, mosaic, 2, 0, [(1, 0)])                                  # B is the tile at column 1, row 0
        assert done == [(2, counts[2], counts[2])] and len(images.rows) == 4 and len(table) == total
        assert table.world_coordinates(_elevation(pkg)) == 0
        got = Snapshot(pkg, table, [1, 2, 3, 4], (0,))

        cells = {1: (0, 0), 2: (1, 0), 3: (0, 1), 4: (1, 1)}
        for first, ids in ((1, [1]), (3, [3, 4]), (2, [2])):                                            # the order A, C, D, B
            group = [cells[i] for i in ids]
            fe.mosaic_tiles_to_database(mosaic, fresh, [(j * T, i * T) for j, i in group], (T, T), (T, T), group, first, 0, "nearest")
        assert fresh.world_coordinates(_elevation(pkg)) == 0
        want = Snapshot(pkg, fresh, [1, 2, 3, 4], (0,))
        stayed = before.image_id != 2
        want.ids = np.concatenate([before.ids[stayed], np.arange(total + 1, total + 1 + counts[2])]).astype(np.int32)
        assert_same(got, want, "replace")
        assert (got.image_id[-counts[2]:] == 2).all() and got.kps[:int(stayed.sum())].tobytes() == before.kps[stayed].tobytes()
    finally:
        table.close()
        fresh.close()


class _Ex:
    def __init__(self, kp, d):
        self.keypoints, self.descriptors = kp, d


def _same_result(got, want, i):
    for k in ("status", "n_keypoints", "n_matches", "n_inliers"):
        assert got[k] == want[k], (i, k, got, want)
    assert (got["H"] is None) == (want["H"] is None), (i, got, want)
    if want["H"] is not None:
        assert np.array_equal(got["H"].view(np.uint64), want["H"].view(np.uint64)), (i, got["H"], want["H"])
    if "pose" in want:
        a, b = got["pose"], want["pose"]
        for k in ("status", "found", "n_correspondences", "n_inliers"):
            assert a[k] == b[k], (i, k, a, b)
        assert np.array_equal(a["rvec"], b["rvec"]) and np.array_equal(a["tvec"], b["tvec"]), (i, a, b)


def test_pipelines_on_a_table_after_a_delete(gpu_pkg):
    """the frame's own keypoints (the tile rolled by (19, 23)) between two images of filler rows; the first filler image is deleted, so
    every row the frame matches has moved"""
    import torch
    pkg = gpu_pkg
    pl = import_module(pkg.__name__ + ".pipeline")
    fe, fd, synth = pkg.feature_extraction, pkg.feature_database, pkg.synth
    tile = synth.make_tile(T, T, frame_index=70, blobs_per_mpx=20000)
    frame = torch.from_numpy(tile).to("cuda:0")
    ex = fe.akaze_keypoint_descriptor_extraction_def(np.roll(tile, (19, 23), axis=(0, 1)).copy(), None)
    assert len(ex.keypoints) >= 50
    rng = np.random.default_rng(5)

    def filler(n):
        k = np.zeros(n, pkg._lib.KEYPOINT_DTYPE)
        k["x"], k["y"], k["response"] = rng.uniform(0, 255, n), rng.uniform(0, 255, n), rng.uniform(0, 0.01, n)
        return _Ex(k, synth.make_descriptor_db(n, seed=1000 + n))

    f1, f2 = filler(1500), filler(700)
    table, fresh = fd.KeypointTable(4000), fd.KeypointTable(4000)
    pipes = []
    try:
        table.create_keypoints(f1, 1, 0, 1, 0, (T, T))
        table.create_keypoints(ex, 2, 0, 0, 0, (T, T))
        table.create_keypoints(f2, 3, 0, 2, 0, (T, T))
        assert table.world_coordinates(_elevation(pkg)) == 0
        assert table.delete_keypoints_from_image_id(1) == 1500
        fresh.create_keypoints(ex, 2, 0, 0, 0, (T, T))
        fresh.create_keypoints(f2, 3, 0, 2, 0, (T, T))
        assert fresh.world_coordinates(_elevation(pkg)) == 0
        assert_same(_no_ids(Snapshot(pkg, table, [2, 3], (0,))), _no_ids(Snapshot(pkg, fresh, [2, 3], (0,))), "tables")

        def run(t, per_frame_view):
            pose = pl.PoseStage.from_table(t, KMAT, **POSE)
            p = pl.StreamedFramePipeline.from_table(t, per_frame_view=per_frame_view, max_points=8192, pose=pose)
            pipes.append(p)
            sel = [pl.StreamedFramePipeline.selection(2, 0, (0, 0, 255.5, 255.5)), pl.StreamedFramePipeline.selection(1, 0)] if per_frame_view else None
            out, _ = p.run([frame], 2, selections=sel)
            p.close()
            return out

        for per_frame_view in (False, True):
            got, want = run(table, per_frame_view), run(fresh, per_frame_view)
            for i, (g, w) in enumerate(zip(got, want)):
                _same_result(g, w, (per_frame_view, i))
            assert want[0]["n_matches"] >= 8 and want[0]["H"] is not None and want[0]["pose"]["n_correspondences"] == want[0]["n_matches"]
            assert abs(want[0]["H"][0, 2] - 23) < 0.5 and abs(want[0]["H"][1, 2] - 19) < 0.5      # the planted translation: trainIdx is the row
    finally:
        for p in pipes:
            p.close()
        table.close()
        fresh.close()


def _no_ids(snap):
    snap.ids = None
    return snap
