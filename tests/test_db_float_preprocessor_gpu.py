"""GPU: the Python fronts of the float table's DB build: preprocessor.process_lod_from_mosaic(.., descriptor="kaze", device_insert=True) and
preprocessor.replace_tiles on a float table, against the same calls on a byte table: image rows, row counts and every non-descriptor column
equal; the float rows are unit-length M-SURF rows; the two argument errors of the new parameter."""
import numpy as np
import pytest

from db_float_cases import Snapshot

pytestmark = pytest.mark.gpu

T = 256


@pytest.fixture(scope="module")
def mosaic(gpu_pkg):
    t = gpu_pkg.synth.make_tile(2 * T, 2 * T, frame_index=11, channels=3, blobs_per_mpx=20000).astype(np.float32)
    dm = gpu_pkg.geotiff_extractor.DeviceMosaic(np.stack([t[:, :, 2] * 3.0 + 10.0, t[:, :, 1] * 2.0 - 5.0, t[:, :, 0] * 1.5]))
    yield dm
    dm.close()


def same_columns(a, b, what):
    assert a.n == b.n, what
    for name, col in a.columns().items():
        assert col.tobytes() == b.columns()[name].tobytes(), (what, name)


def test_build_and_replace_on_a_float_table(gpu_pkg, mosaic):
    pkg = gpu_pkg
    pp, fd = pkg.preprocessor, pkg.feature_database
    tf, tb = fd.KeypointTable(20000, descriptor="kaze"), fd.KeypointTable(20000)
    imf, imb = pp.ImageTable(), pp.ImageTable()
    try:
        with pytest.raises(ValueError):            # the table is a float table
            pp.process_lod_from_mosaic(tf, imf, mosaic, 2, batch=4, device_insert=True, descriptor="mldb")
        with pytest.raises(ValueError):            # a float table is built on the device only
            pp.process_lod_from_mosaic(tf, imf, mosaic, 2, batch=4, descriptor="kaze")
        with pytest.raises(ValueError):
            pp.process_lod_from_mosaic(tb, imb, mosaic, 2, batch=4, device_insert=True, descriptor="kaze")
        assert len(tf) == 0 and len(tb) == 0 and not imf.rows and not imb.rows
        built_f = pp.process_lod_from_mosaic(tf, imf, mosaic, 2, batch=4, device_insert=True, descriptor="kaze")
        built_b = pp.process_lod_from_mosaic(tb, imb, mosaic, 2, batch=4, device_insert=True)
        assert built_f == built_b and imf.rows == imb.rows and len(tf) == len(tb) > 100
        images = [r["id"] for r in imf.rows]
        sf, sb = Snapshot(pkg, tf, images, (0, 1)), Snapshot(pkg, tb, images, (0, 1))
        same_columns(sf, sb, "build")
        rows = sf.desc.view(np.float32)
        assert rows.shape == (len(tf), 64) and np.allclose(np.linalg.norm(rows.astype(np.float64), axis=1), 1.0, atol=1e-4)
        # tile (1, 0) of level 0 again: its rows leave and come back behind every row that stayed, in both tables alike
        done_f = pp.replace_tiles(tf, imf, mosaic, 2, 0, [(1, 0)])
        done_b = pp.replace_tiles(tb, imb, mosaic, 2, 0, [(1, 0)])
        assert done_f == done_b and done_f[0][1] == done_f[0][2] > 20 and len(tf) == len(tb) == sf.n
        rf, rb = Snapshot(pkg, tf, images, (0, 1)), Snapshot(pkg, tb, images, (0, 1))
        same_columns(rf, rb, "replace")
        image_id, n = done_f[0][0], done_f[0][1]
        stayed = sf.image_id != image_id
        assert rf.desc[:int(stayed.sum())].tobytes() == sf.desc[stayed].tobytes()                    # the rows that stayed keep every bit
        assert rf.desc[-n:].tobytes() == sf.desc[~stayed].tobytes() and (rf.image_id[-n:] == image_id).all()   # the same imagery: the same rows again
        assert np.array_equal(rf.ids[-n:], np.arange(sf.n + 1, sf.n + 1 + n))
    finally:
        tf.close()
        tb.close()
