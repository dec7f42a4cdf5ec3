"""GPU: the lens kernels (csrc/lens.hip) against the numpy reference of the documented evaluation order (tests/lens_reference.py).

 * apds_distort_points / apds_undistort_points equal the reference bit for bit (n on either side of a wave and of a block, three
   coefficient sets, 5 and 20 iterations); apds_dev_undistort_points at strides 8 and 28 equals the f64 reference of the widened f32
   inputs rounded once, and leaves the other 20 bytes of a keypoint alone; no distortion returns the input bits;
 * a round trip from the construction, not from either implementation: distort then undistort (20 iterations) is the identity to 1e-6 px;
 * apds_undistort_image equals the reference bit for bit (two sizes either side of the 256-wide block, 1 / 3 / 4 channels, with and
   without new_K); a constant image comes back constant where the footprint is inside and 0 where it is outside;
 * apds_pnp_solver_ransac_dist finds a known pose from distorted projections as well as the plain call does from reference-undistorted
   ones, the plain call on the distorted points does not, and with n_dist = 0 the two calls agree in every output bit."""
import ctypes as C

import numpy as np
import pytest

import lens_reference as lr

pytestmark = pytest.mark.gpu

K = lr.camera()
NS = [0, 1, 63, 64, 65, 257]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _points(n, seed):
    return np.random.default_rng(seed).uniform(0.0, 4095.0, (n, 2))


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_host_array_points_equal_the_reference_bit_for_bit(gpu_pkg, name):
    hg, dist = gpu_pkg.homographier, lr.SETS[name]
    for n in NS:
        p = _points(n, 100 + n)
        got = hg.distort_points(p, K, dist)
        assert got.shape == (n, 2) and np.array_equal(_bits(got), _bits(lr.distort_points_ref(p, K, dist))), (name, n, "distort")
        for iters in (5, 20):
            got = hg.undistort_points(p, K, dist, iters=iters)
            assert np.array_equal(_bits(got), _bits(lr.undistort_points_ref(p, K, dist, iters))), (name, n, iters)
    p = _points(65, 7)
    assert np.array_equal(_bits(hg.undistort_points(p, K, dist, iters=0)), _bits(lr.undistort_points_ref(p, K, dist, 5)))     # iters <= 0 means 5


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_device_points_in_place_at_strides_8_and_28(gpu_pkg, name):
    import torch
    from importlib import import_module
    pl = import_module(gpu_pkg.__name__ + ".pipeline")
    dist = lr.SETS[name]
    with torch.cuda.stream(torch.cuda.Stream("cuda:0")):
        for n in NS:
            rows = np.random.default_rng(200 + n).uniform(0.0, 4095.0, (n, 7)).astype(np.float32)
            rows[:, 5:7] = np.random.default_rng(300 + n).integers(-2 ** 31, 2 ** 31, (n, 2), dtype=np.int64).astype(np.int32).view(np.float32)   # octave, class_id: any bits
            for iters in (5, 20):
                want = lr.undistort_points_f32_ref(rows[:, 0:2], K, dist, iters)
                pts = torch.from_numpy(rows[:, 0:2].copy()).to("cuda:0")
                pl.dev_undistort_points(pts, K, dist, iters)
                torch.cuda.current_stream().synchronize()
                assert np.array_equal(_bits(pts.cpu().numpy()), _bits(want)), (name, n, iters, "stride 8")
                kps = torch.from_numpy(rows.copy()).to("cuda:0")
                assert n < 2 or kps.stride(0) * 4 == 28
                pl.dev_undistort_points(kps, K, dist, iters)
                torch.cuda.current_stream().synchronize()
                back = kps.cpu().numpy()
                assert np.array_equal(_bits(back[:, 0:2].copy()), _bits(want)), (name, n, iters, "stride 28")
                assert np.array_equal(_bits(back[:, 2:7].copy()), _bits(rows[:, 2:7].copy())), (name, n, "the other 20 bytes")


def test_no_distortion_returns_the_input_bits(gpu_pkg):
    import torch
    from importlib import import_module
    pl = import_module(gpu_pkg.__name__ + ".pipeline")
    hg = gpu_pkg.homographier
    p = _points(257, 9)
    f = np.random.default_rng(10).uniform(0.0, 4095.0, (257, 2)).astype(np.float32)
    with torch.cuda.stream(torch.cuda.Stream("cuda:0")):
        for dist in (None, np.zeros(5)):
            assert np.array_equal(_bits(hg.undistort_points(p, K, dist)), _bits(p)) and np.array_equal(_bits(hg.distort_points(p, K, dist)), _bits(p))
            t = torch.from_numpy(f.copy()).to("cuda:0")
            pl.dev_undistort_points(t, K, dist, 5)
            torch.cuda.current_stream().synchronize()
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(f))
    # the identity is the skip's doing, not the arithmetic's: (u - cx) / fx * fx + cx does not return every u
    u = p[:, 0]
    assert ((u - K[0, 2]) / K[0, 0] * K[0, 0] + K[0, 2] != u).any()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_round_trip_distort_then_undistort_is_the_identity(gpu_pkg, name):
    hg, dist = gpu_pkg.homographier, lr.SETS[name]
    g = np.linspace(0.0, 4095.0, 33)
    p = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    back = hg.undistort_points(hg.distort_points(p, K, dist), K, dist, iters=20)
    err = np.abs(back - p).max()
    print("set %s: undistort(distort(p)) - p, worst of the grid: %.3g px" % (name, err))
    assert err < 1e-6, (name, err)


def _small_camera(rows, cols):
    """a lens whose distortion is strong over a small image: f = half the diagonal, principal point off the pixel grid"""
    f = 0.5 * float(np.hypot(rows, cols))
    return np.array([[f, 0.0, (cols - 1) / 2 + 0.25], [0.0, f, (rows - 1) / 2 - 0.25], [0.0, 0.0, 1.0]])


@pytest.mark.parametrize("shape", [(37, 53), (5, 257)])
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_image_equals_the_reference_bit_for_bit(gpu_pkg, shape, channels):
    hg = gpu_pkg.homographier
    rows, cols = shape
    img = np.random.default_rng(rows * 1000 + cols + channels).integers(0, 256, (rows, cols, channels), dtype=np.uint8)
    Ks = _small_camera(rows, cols)
    wide = Ks.copy()
    wide[0, 0] *= 0.8
    wide[1, 1] *= 0.8
    for name in ("A", "C"):
        for new_K in (None, wide):
            got = hg.undistort_image(img, Ks, lr.SETS[name], new_K).mat
            want = lr.undistort_image_ref(img, Ks, lr.SETS[name], new_K)
            assert np.array_equal(got, want), (shape, channels, name, new_K is not None, int((got != want).sum()))
            # the cases do what they are for: with the wider view the footprint leaves the source on every side
            ins, _, _ = lr.footprint(*lr.undistort_map_ref(rows, cols, Ks, lr.SETS[name], new_K), rows, cols)
            if new_K is not None:
                out = ~ins.any(-1)
                assert out[0].any() and out[-1].any() and out[:, 0].any() and out[:, -1].any(), (shape, name)
    # no distortion and no new camera: the source itself
    assert np.array_equal(hg.undistort_image(img, Ks, np.zeros(5)).mat, img)
    assert np.array_equal(hg.undistort_image(img if channels > 1 else img[:, :, 0], Ks, None).mat, img if channels > 1 else img[:, :, 0])


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_constant_image_is_constant_inside_and_zero_outside(gpu_pkg, channels):
    hg = gpu_pkg.homographier
    rows, cols = 37, 53
    img = np.full((rows, cols, channels), 200, np.uint8)
    Ks = _small_camera(rows, cols)
    wide = Ks.copy()
    wide[0, 0] *= 0.8
    wide[1, 1] *= 0.8
    for name in ("A", "C"):
        got = hg.undistort_image(img, Ks, lr.SETS[name], wide).mat
        ins, _, _ = lr.footprint(*lr.undistort_map_ref(rows, cols, Ks, lr.SETS[name], wide), rows, cols)
        inside, outside = ins.all(-1), ~ins.any(-1)
        assert inside.any() and outside.any()
        assert (got[inside] == 200).all() and (got[outside] == 0).all(), name


# ---- PnP anchor ---------------------------------------------------------------------------------------------------------------------------
def _rot(rv):
    th = np.linalg.norm(rv)
    k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _solve(pkg, obj, img, dist, n_dist=None, plain=False):
    L, ptr = pkg.lib(), pkg._lib.ptr
    n = len(obj)
    obj, img = np.ascontiguousarray(obj, np.float64), np.ascontiguousarray(img, np.float64)
    rv, tv, inl = np.zeros(3), np.zeros(3), np.full(n, -1, np.int32)
    ni, found = C.c_int(-1), C.c_int(-1)
    if plain:
        rc = L.apds_pnp_solver_ransac(ptr(obj), ptr(img), n, ptr(K), 100, 8.0, 0.99, 1, ptr(rv), ptr(tv), ptr(inl), C.byref(ni), C.byref(found))
    else:
        d = None if dist is None else np.ascontiguousarray(dist, np.float64)
        rc = L.apds_pnp_solver_ransac_dist(ptr(obj), ptr(img), n, ptr(K), 100, 8.0, 0.99, 1, ptr(d) if d is not None else None,
                                           (len(d) if d is not None else 0) if n_dist is None else n_dist, ptr(rv), ptr(tv), ptr(inl), C.byref(ni), C.byref(found))
    return rc, found.value, rv, tv, inl[:max(ni.value, 0)].copy()


def _pose_error(rv, tv, rv_true, tv_true):
    R = _rot(rv) @ _rot(rv_true).T
    return float(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))), float(np.linalg.norm(tv - tv_true))


def test_pnp_dist_finds_the_pose_the_plain_call_misses(gpu_pkg):
    """200 non-coplanar points and a known pose, f = 3000 on 4096^2, projected with the reference's forward model and set A, no noise."""
    rng = np.random.default_rng(42)
    obj = np.stack([rng.uniform(-480, 480, 200), rng.uniform(-480, 480, 200), rng.uniform(-100, 100, 200)], 1)
    rv_true, tv_true = np.array([0.05, -0.04, 0.3]), np.array([15.0, -10.0, 1000.0])
    cam = obj @ _rot(rv_true).T + tv_true
    ideal = cam[:, :2] / cam[:, 2:3] * np.array([K[0, 0], K[1, 1]]) + np.array([K[0, 2], K[1, 2]])
    assert ideal.min() > 0 and ideal.max() < 4095 and np.ptp(ideal, 0).min() > 3000      # the points fill the frame, corners included
    img = lr.distort_points_ref(ideal, K, lr.SET_A)
    assert np.abs(img - ideal).max() > 50
    got = _solve(gpu_pkg, obj, img, lr.SET_A)
    base = _solve(gpu_pkg, obj, lr.undistort_points_ref(img, K, lr.SET_A, 5), None, plain=True)      # the bar: the reference path
    naive = _solve(gpu_pkg, obj, img, None, plain=True)
    assert got[0] == 0 and got[1] == 1 and base[0] == 0 and base[1] == 1, (got[:2], base[:2])
    e_got, e_base = _pose_error(got[2], got[3], rv_true, tv_true), _pose_error(base[2], base[3], rv_true, tv_true)
    print("rotation / translation error: _dist %.3g rad %.3g, plain on reference-undistorted points %.3g rad %.3g" % (e_got + e_base))
    assert e_got[0] <= 2 * e_base[0] + 1e-9 and e_got[1] <= 2 * e_base[1] + 1e-9, (e_got, e_base)
    # the plain call on the distorted points is worse than both: the coefficients reach the solve
    if naive[0] == 0 and naive[1] == 1:
        e_naive = _pose_error(naive[2], naive[3], rv_true, tv_true)
        print("plain on the distorted points: %.3g rad %.3g" % e_naive)
        assert e_naive[0] > max(e_got[0], e_base[0]) and e_naive[1] > max(e_got[1], e_base[1]), (e_naive, e_got, e_base)
    # with no distortion the _dist call IS the plain call
    for dist, nd in ((None, 0), (np.zeros(5), 5), (np.array(lr.SET_A), 0)):
        a, b = _solve(gpu_pkg, obj, img, dist, n_dist=nd), _solve(gpu_pkg, obj, img, None, plain=True)
        assert a[:2] == b[:2] and all(np.array_equal(_bits(x) if x.dtype == np.float64 else x, _bits(y) if y.dtype == np.float64 else y) for x, y in zip(a[2:], b[2:]))
