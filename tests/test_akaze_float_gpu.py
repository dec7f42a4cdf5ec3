"""GPU: AKAZE's float descriptor (DESCRIPTOR_KAZE, 64 x f32; csrc/akaze_describe_msurf.hip) against the float64 reference of
tests/msurf_reference.py within its measured tolerance TOL = 4 E32, and what the new calls promise bit for bit: the M-LDB call's keypoints,
the same rows through max_points, a batch, a mask and the device form; then extract -> L2 k-NN -> ratio test end to end on a shifted view.

Observed on the MI355X (max |GPU - f64 reference|, printed by the tests): see DESIGN.md section 2, "the float descriptor".
"""
import ctypes as C

import numpy as np
import pytest

import akaze_float_cases as fc
import msurf_reference as ref

pytestmark = pytest.mark.gpu


class _DeviceBuffers:
    """device allocations of one test, released at its end"""

    def __init__(self, pkg):
        self.pkg, self.L, self.held = pkg, pkg.lib(), []

    def alloc(self, nbytes):
        p = C.c_void_p()
        self.pkg._lib.check(self.L.apds_dev_alloc(max(int(nbytes), 256), C.byref(p)))
        self.held.append(p)
        return p

    def upload(self, host):
        host = np.ascontiguousarray(host)
        p = self.alloc(host.nbytes)
        if host.nbytes:
            self.pkg._lib.check(self.L.apds_dev_upload(p, host.ctypes.data, host.nbytes, None))
            self.pkg._lib.check(self.L.apds_stream_synchronize(None))
        return p

    def download(self, p, shape, dtype):
        out = np.zeros(shape, dtype)
        if out.nbytes:
            self.pkg._lib.check(self.L.apds_dev_download(out.ctypes.data, p, out.nbytes, None))
        return out

    def release(self):
        for p in self.held:
            self.L.apds_dev_release(p)
        self.held = []


@pytest.fixture
def dev(gpu_pkg):
    d = _DeviceBuffers(gpu_pkg)
    yield d
    d.release()


def _describe_on_device(dev, lx, ly, kps):
    """apds_dev_akaze_describe_float on one plane -> n x 64 float32 (the rows start as NaN: what the call leaves unwritten shows)"""
    h, w = lx.shape
    lxy = dev.upload(np.stack([lx, ly], axis=2).astype(np.float32))
    dk = dev.upload(kps)
    dd = dev.upload(np.full((max(len(kps), 1), 64), np.nan, np.float32))
    dev.pkg._lib.check(dev.L.apds_dev_akaze_describe_float(lxy, w, h, dk, len(kps), dd, None))
    return dev.download(dd, (len(kps), 64), np.float32)


@pytest.fixture(scope="module")
def hook_reference():
    """the float64 reference rows of every hook case, computed once"""
    return {name: ref.describe_plane(lx, ly, kps, np.float64) for name, (lx, ly, kps) in fc.hook_cases().items()}


def _worst(got, want):
    return float(np.abs(got.astype(np.float64) - want).max()) if len(want) else 0.0


# ---------------------------------------------------------------------------------------------------------------- the describe hook
def test_constant_planes_give_the_closed_form(dev):
    for name, (lx, ly, kps, angle) in fc.constant_cases().items():
        got = _describe_on_device(dev, lx, ly, kps)
        e = _worst(got, np.repeat(ref.constant_plane_row(angle)[None, :], len(kps), 0))
        print(f"{name}: max |gpu - closed form| = {e:.3e}")
        assert e <= ref.TOL, name


@pytest.mark.parametrize("group", ["random", "rint_ties", "count"])
def test_hook_matches_the_float64_reference(dev, hook_reference, group):
    names = [n for n in fc.random_cases() if n.startswith(group)]
    assert names
    cases = fc.hook_cases()
    for name in names:
        lx, ly, kps = cases[name]
        got = _describe_on_device(dev, lx, ly, kps)
        assert np.isfinite(got).all(), name                      # every row of every live wave was written
        e = _worst(got, hook_reference[name])
        print(f"{name}: n = {len(kps)}, max |gpu - f64| = {e:.3e} (TOL {ref.TOL:.3e})")
        assert e <= ref.TOL, name
        assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() <= 1e-5, name


def test_hook_writes_only_its_own_rows(dev):
    """n = 5 of a buffer of 8 rows: the three waves past the end of the second block write nothing"""
    lx, ly, kps = fc.random_cases()["count5_40x56"]
    h, w = lx.shape
    lxy = dev.upload(np.stack([lx, ly], axis=2))
    dk = dev.upload(kps)
    dd = dev.upload(np.full((8, 64), np.nan, np.float32))
    dev.pkg._lib.check(dev.L.apds_dev_akaze_describe_float(lxy, w, h, dk, 5, dd, None))
    rows = dev.download(dd, (8, 64), np.float32)
    assert np.isfinite(rows[:5]).all() and np.isnan(rows[5:]).all()


def test_no_keypoints_is_a_no_op(gpu_pkg):
    assert gpu_pkg.lib().apds_dev_akaze_describe_float(None, 40, 56, None, 0, None, None) == 0


def test_zero_planes_give_zero_rows(dev):
    lx, ly, kps = fc.zero_case()
    got = _describe_on_device(dev, lx, ly, kps)
    assert got.shape == (3, 64) and not np.isnan(got).any() and not got.any()


# ---------------------------------------------------------------------------------------------------------------- extraction
def _gpu_planes(pkg, img, kps):
    """level -> (Lx, Ly) read back with apds_akaze_debug_plane, for the levels that carry a keypoint"""
    shapes = fc.level_shapes(img.shape[0], img.shape[1])
    ch = 1 if img.ndim == 2 else img.shape[2]
    out = {}
    for lv in np.unique(kps["class_id"]):
        planes = []
        for which in (2, 3):
            p = np.zeros(shapes[int(lv)], np.float32)
            pkg._lib.check(pkg.lib().apds_akaze_debug_plane(pkg._lib.ptr(img), img.shape[0], img.shape[1], ch, img.strides[0], int(lv), which, pkg._lib.ptr(p)))
            planes.append(p)
        out[int(lv)] = tuple(planes)
    return out


def _by_place(kps):
    key = [(int(k["class_id"]), float(k["x"]), float(k["y"])) for k in kps]
    assert len(set(key)) == len(key)
    return {k: i for i, k in enumerate(key)}


@pytest.mark.parametrize("shape", fc.TILES)
def test_extraction_matches_the_reference_on_its_own_planes(gpu_pkg, shape):
    fe = gpu_pkg.feature_extraction
    tile = gpu_pkg.synth.make_tile(shape[0], shape[1], channels=shape[2])
    mldb = fe.akaze_keypoint_descriptor_extraction(tile)
    flt = fe.akaze_keypoint_descriptor_extraction(tile, descriptor="kaze")
    assert len(flt.keypoints) >= 4
    assert flt.keypoints.tobytes() == mldb.keypoints.tobytes()                      # field for field, bit for bit
    assert flt.descriptors.dtype == np.float32 and flt.descriptors.shape == (len(flt.keypoints), 64)
    want = ref.describe_levels(_gpu_planes(gpu_pkg, tile, flt.keypoints), flt.keypoints, np.float64)
    e = _worst(flt.descriptors, want)
    print(f"tile {shape}: n = {len(flt.keypoints)}, max |gpu - f64| = {e:.3e} (TOL {ref.TOL:.3e})")
    assert e <= ref.TOL
    assert np.abs(np.linalg.norm(flt.descriptors.astype(np.float64), axis=1) - 1).max() <= 1e-5


def test_max_points_below_the_count_keeps_the_rows(gpu_pkg):
    fe = gpu_pkg.feature_extraction
    tile = gpu_pkg.synth.make_tile(200, 333, channels=3)
    full = fe.akaze_keypoint_descriptor_extraction(tile, descriptor="kaze")
    keep = len(full.keypoints) // 2
    assert keep >= 4
    cut = fe.akaze_keypoint_descriptor_extraction(tile, max_points=keep, descriptor="kaze")
    assert len(cut.keypoints) == keep
    assert cut.keypoints.tobytes() == fe.akaze_keypoint_descriptor_extraction(tile, max_points=keep).keypoints.tobytes()
    place = _by_place(full.keypoints)
    rows = [place[k] for k in _by_place(cut.keypoints)]
    assert cut.keypoints.tobytes() == full.keypoints[rows].tobytes()
    assert cut.descriptors.tobytes() == full.descriptors[rows].tobytes()


def test_batch_equals_the_single_calls(gpu_pkg):
    fe = gpu_pkg.feature_extraction
    imgs = [gpu_pkg.synth.make_tile(200, 333, frame_index=0, channels=3), np.full((200, 333, 3), 128, np.uint8),
            gpu_pkg.synth.make_tile(200, 333, frame_index=1, channels=3)]
    batch = fe.akaze_keypoint_descriptor_extraction_batch(imgs, descriptor="kaze")
    assert [len(b.keypoints) for b in batch][1] == 0 and len(batch[0].keypoints) and len(batch[2].keypoints)
    for img, b in zip(imgs, batch):
        one = fe.akaze_keypoint_descriptor_extraction(img, descriptor="kaze")
        assert b.keypoints.tobytes() == one.keypoints.tobytes()
        assert b.descriptors.dtype == np.float32 and b.descriptors.shape == (len(one.keypoints), 64)
        assert b.descriptors.tobytes() == one.descriptors.tobytes()


def test_masked_call_keeps_the_survivors_rows(gpu_pkg):
    fe = gpu_pkg.feature_extraction
    tile = gpu_pkg.synth.make_tile(200, 333, channels=3)
    full = fe.akaze_keypoint_descriptor_extraction(tile, descriptor="kaze")
    mask = np.ones((200, 333), np.uint8)
    mask[:, :160] = 0
    for support in (0, 2):
        got = fe.akaze_keypoint_descriptor_extraction(tile, mask, None, support, descriptor="kaze")
        assert got.keypoints.tobytes() == fe.akaze_keypoint_descriptor_extraction(tile, mask, None, support).keypoints.tobytes()
        assert 0 < len(got.keypoints) < len(full.keypoints)
        place = _by_place(full.keypoints)
        rows = [place[k] for k in _by_place(got.keypoints)]
        assert rows == sorted(rows)
        assert got.descriptors.tobytes() == full.descriptors[rows].tobytes()


def test_device_form_equals_the_host_form(gpu_pkg, dev):
    fe, L = gpu_pkg.feature_extraction, gpu_pkg.lib()
    tile = gpu_pkg.synth.make_tile(256, 256, channels=4)
    host = fe.akaze_keypoint_descriptor_extraction(tile, descriptor="kaze")
    capacity = 2048
    dimg = dev.upload(tile)
    dk, dd = dev.alloc(capacity * 28), dev.alloc(capacity * 256)
    n = C.c_int(-1)
    gpu_pkg._lib.check(L.apds_dev_akaze_extract_float(dimg, 256, 256, 4, tile.strides[0], None, 0, 0, capacity, dk, dd, capacity, C.byref(n), None))
    gpu_pkg._lib.check(L.apds_stream_synchronize(None))
    assert n.value == len(host.keypoints) > 0
    assert dev.download(dk, n.value, gpu_pkg._lib.KEYPOINT_DTYPE).tobytes() == host.keypoints.tobytes()
    assert dev.download(dd, (n.value, 64), np.float32).tobytes() == host.descriptors.tobytes()
    # ... and the batch form of it, two copies of the image, the second one's rows `capacity` rows after the first's
    two = dev.upload(np.stack([tile, tile]))
    dk2, dd2 = dev.alloc(2 * capacity * 28), dev.alloc(2 * capacity * 256)
    counts = (C.c_int * 2)()
    gpu_pkg._lib.check(L.apds_dev_akaze_extract_float_batch(two, 2, tile.nbytes, 256, 256, 4, tile.strides[0], None, 0, 0, 0, capacity, dk2, dd2, capacity, counts,
                                                            None))
    gpu_pkg._lib.check(L.apds_stream_synchronize(None))
    assert list(counts) == [n.value, n.value]
    rows = dev.download(dd2, (2 * capacity, 64), np.float32)
    assert rows[:n.value].tobytes() == host.descriptors.tobytes() and rows[capacity:capacity + n.value].tobytes() == host.descriptors.tobytes()


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_shifted_views_match_as_the_reference_says(gpu_pkg):
    """extract -> L2 k-NN -> ratio test on the GPU against the same ratio test in NumPy on the float64 reference descriptors"""
    fe = gpu_pkg.feature_extraction
    a, b = fc.shifted_views()
    dx, dy = fc.SHIFT
    ea, eb = (fe.akaze_keypoint_descriptor_extraction(v, descriptor="kaze") for v in (a, b))
    ka, kb = ea.keypoints, eb.keypoints
    assert len(ka) > 200 and len(kb) > 200
    ra, rb = (ref.describe_levels(_gpu_planes(gpu_pkg, v, e.keypoints), e.keypoints, np.float64) for v, e in ((a, ea), (b, eb)))
    print(f"views: max |gpu - f64| = {max(_worst(ea.descriptors, ra), _worst(eb.descriptors, rb)):.3e} (TOL {ref.TOL:.3e})")
    got = fe.get_knn_matches_l2(ea.descriptors, eb.descriptors, 2, fc.RATIO)
    keep, train, ds, _ = ref.ratio_matches(ra, rb, fc.RATIO)
    m0, m1 = fc.ratio_margins(ds)
    near = (m0 < 8 * ref.TOL) | (m1 < 8 * ref.TOL)              # queries whose decision a TOL-sized error may turn
    print(f"{int(near.sum())} of {len(near)} queries within 8 TOL of a decision; {len(got)} matches, the reference has {len(keep)}")
    assert near.mean() <= 0.02
    want = {(int(q), int(t)) for q, t in zip(keep, train) if not near[q]}
    have = {(int(q), int(t)) for q, t in zip(got["query_idx"], got["train_idx"]) if not near[q]}
    assert have == want, sorted(have ^ want)
    # the surviving matches lie at the shift: content at (x, y) of a is at (x - dx, y - dy) of b
    pa, pb = np.stack([ka["x"], ka["y"]], 1).astype(np.float64), np.stack([kb["x"], kb["y"]], 1).astype(np.float64)

    def share_at_the_shift(qs, ts):
        qs, ts = np.asarray(qs, np.int64), np.asarray(ts, np.int64)
        off = np.linalg.norm(pa[qs] - pb[ts] - np.array([dx, dy], np.float64), axis=1)
        return float((off <= 0.5 * 2.0 ** ka["octave"][qs]).mean())

    ref_share = share_at_the_shift(keep, train)
    gpu_share = share_at_the_shift(got["query_idx"], got["train_idx"])
    print(f"matches at the shift: gpu {gpu_share:.3f}, reference {ref_share:.3f}")
    assert len(got) > 50 and gpu_share >= ref_share - 0.05
