"""CPU: the lens entries' argument errors, found before any device work (no GPU here), and the numpy reference's own consistency.

 * n_dist outside {0, 4, 5, 8}: 12 and 14 (thin prism, tilt) are APDS_ERR_NOT_IMPLEMENTED, everything else APDS_ERR_BAD_ARG; a coefficient
   that is not finite and a focal length that is not finite and positive are APDS_ERR_BAD_ARG - for every lens entry, with valid
   buffers, on a machine without a device (a compute call there would be APDS_ERR_NO_DEVICE, tests/test_abi.py);
 * apds_pnp_solver_ransac_dist with fewer than four correspondences is APDS_ERR_ASSERT like the plain call;
 * no distortion needs no device: the input bits come back;
 * the reference: forward(inverse(p)) returns p within 1e-6 px at 20 iterations for the three coefficient sets on a 65 x 65 grid over
   4096^2 (f = 3000, c = 2047.5); at 5 iterations - OpenCV's count - the residual is what a five-step fixed-point iteration leaves at the
   corners of such a lens (printed).
(apds_pipeline_set_lens after a submit needs a pipeline, which needs a device: tests/test_pipeline_lens_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

import lens_reference as lr

BAD_ARG, NOT_IMPLEMENTED, ASSERT = -5, -213, -215
K = lr.camera()


def _calls(pkg, Kmat, dist, n_dist):
    """every lens entry on small valid buffers with this (K, dist, n_dist): [(name, status)]"""
    L, ptr = pkg.lib(), pkg._lib.ptr
    Kc = np.ascontiguousarray(Kmat, np.float64)
    d = None if dist is None else np.ascontiguousarray(dist, np.float64)
    pd = ptr(d) if d is not None else None
    xy, out = np.full((3, 2), 100.0), np.zeros((3, 2))
    img, dst = np.zeros((4, 5, 3), np.uint8), np.zeros((4, 5, 3), np.uint8)
    obj, ipt = np.random.default_rng(1).uniform(-1, 1, (8, 3)), np.full((8, 2), 50.0)
    rv, tv, inl = np.zeros(3), np.zeros(3), np.zeros(8, np.int32)
    ni, found = C.c_int(0), C.c_int(0)
    fake_dev = C.c_void_p(0x1000)      # never dereferenced: the argument errors come first
    return [
        ("distort_points", L.apds_distort_points(ptr(xy), 3, ptr(Kc), pd, n_dist, ptr(out))),
        ("undistort_points", L.apds_undistort_points(ptr(xy), 3, ptr(Kc), pd, n_dist, 5, ptr(out))),
        ("dev_undistort_points", L.apds_dev_undistort_points(fake_dev, 3, 8, ptr(Kc), pd, n_dist, 5, None)),
        ("undistort_image", L.apds_undistort_image(ptr(img), 4, 5, 3, ptr(Kc), pd, n_dist, None, ptr(dst))),
        ("dev_undistort_image", L.apds_dev_undistort_image(fake_dev, 4, 5, 3, ptr(Kc), pd, n_dist, None, C.c_void_p(0x2000), None)),
        ("pnp_solver_ransac_dist", L.apds_pnp_solver_ransac_dist(ptr(obj), ptr(ipt), 8, ptr(Kc), 100, 8.0, 0.99, 1, pd, n_dist, ptr(rv), ptr(tv), ptr(inl),
                                                                 C.byref(ni), C.byref(found))),
        ("pipeline_set_lens", L.apds_pipeline_set_lens(None, ptr(Kc), pd, n_dist, 5)),
    ]


@pytest.mark.parametrize("n_dist,want", [(3, BAD_ARG), (6, BAD_ARG), (12, NOT_IMPLEMENTED), (14, NOT_IMPLEMENTED), (-1, BAD_ARG)])
def test_coefficient_counts_that_are_not_served(pkg, n_dist, want):
    dist = np.full(16, 1e-3)
    for name, rc in _calls(pkg, K, dist, n_dist):
        assert rc == want, (name, n_dist, rc)
    assert pkg.lib().apds_last_error()


def test_non_finite_coefficient_and_bad_focal_length(pkg):
    for bad in (np.nan, np.inf, -np.inf):
        for n_dist in (4, 5, 8):
            dist = np.array(lr.SET_C)
            dist[n_dist - 1] = bad
            for name, rc in _calls(pkg, K, dist, n_dist):
                assert rc == BAD_ARG, (name, bad, n_dist, rc)
    for fx, fy in ((0.0, 3000.0), (3000.0, 0.0), (-3000.0, 3000.0), (np.nan, 3000.0), (3000.0, np.inf)):
        Kb = K.copy()
        Kb[0, 0], Kb[1, 1] = fx, fy
        for name, rc in _calls(pkg, Kb, np.array(lr.SET_A), 4):
            assert rc == BAD_ARG, (name, fx, fy, rc)
    # new_K is held to the same rule
    img, dst, Kb = np.zeros((4, 5), np.uint8), np.zeros((4, 5), np.uint8), K.copy()
    Kb[0, 0] = 0.0
    d = np.array(lr.SET_A)
    ptr = pkg._lib.ptr
    assert pkg.lib().apds_undistort_image(ptr(img), 4, 5, 1, ptr(K), ptr(d), 4, ptr(Kb), ptr(dst)) == BAD_ARG


def test_pnp_dist_with_fewer_than_four_correspondences(pkg):
    L, ptr = pkg.lib(), pkg._lib.ptr
    obj, ipt = np.zeros((3, 3)), np.zeros((3, 2))
    rv, tv, inl = np.zeros(3), np.zeros(3), np.zeros(3, np.int32)
    ni, found = C.c_int(-1), C.c_int(-1)
    d = np.array(lr.SET_A)
    for n in (0, 3):
        for dist, nd in ((ptr(d), 4), (None, 0)):
            rc = L.apds_pnp_solver_ransac_dist(ptr(obj), ptr(ipt), n, ptr(K), 100, 8.0, 0.99, 1, dist, nd, ptr(rv), ptr(tv), ptr(inl), C.byref(ni), C.byref(found))
            assert rc == ASSERT and found.value == 0, (n, nd, rc)
    # ... and the python front forwards a non-None dist_coeffs to that call
    hg = pkg.homographier
    with pytest.raises(hg.MatError) as e:
        hg.pnp_solver_ransac([hg.ImgObjCorrespondence((0, 0, 0), (0, 0))] * 3, hg.Cmat(K, np.float64), 100, 8.0, 0.99, dist_coeffs=np.ones(6))
    assert e.value.inner.code == BAD_ARG          # six coefficients: the lens check, which the plain call does not have


def test_no_distortion_returns_the_input_without_a_device(pkg):
    hg = pkg.homographier
    xy = np.random.default_rng(2).uniform(0, 4096, (65, 2))
    for dist in (None, [], np.zeros(4), np.zeros(5), np.zeros(8)):
        assert np.array_equal(hg.distort_points(xy, K, dist), xy)
        assert np.array_equal(hg.undistort_points(xy, K, dist, iters=20), xy)
    img = np.random.default_rng(3).integers(0, 256, (9, 11, 4), dtype=np.uint8)
    assert np.array_equal(hg.undistort_image(img, K, np.zeros(5)).mat, img)
    # n == 0 is fine with a lens that distorts
    assert hg.undistort_points(np.zeros((0, 2)), K, lr.SET_A).shape == (0, 2)
    assert hg.distort_points(np.zeros((0, 2)), K, lr.SET_C).shape == (0, 2)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_reference_forward_of_inverse_is_the_identity(name):
    dist = lr.SETS[name]
    g = np.linspace(0.0, 4095.0, 65)
    p = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    err20 = np.abs(lr.distort_points_ref(lr.undistort_points_ref(p, K, dist, 20), K, dist) - p).max()
    err5 = np.abs(lr.distort_points_ref(lr.undistort_points_ref(p, K, dist, 5), K, dist) - p).max()
    print("set %s: forward(inverse(p)) - p, worst of the grid: %.3g px at 20 iterations, %.3g px at 5" % (name, err20, err5))
    assert err20 < 1e-6, (name, err20)
    assert err5 < 1.0 and err20 < err5, (name, err5)      # five steps leave a visible residual at the corners; twenty remove it

