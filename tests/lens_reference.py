"""The lens model in numpy float64, operation for operation in the order csrc/lens_core.h documents. Not a test module.

numpy's float64 +, -, *, / are IEEE operations rounded to nearest even and are never fused, which is what the library's build
(-ffp-contract=off) gives every operation of lens_core.h: the kernels are held to these bits. The fixed-point sampling tail of the frame
undistort uses the exact integer weights of tests/ingest_reference.py (the warp's reference) with border value 0."""
import numpy as np

from ingest_reference import DYADIC_W

# the issue's three coefficient sets, OpenCV order (k1, k2, p1, p2[, k3[, k4, k5, k6]])
SET_A = (-0.12, 0.03, 1e-3, -5e-4)
SET_B = SET_A + (-0.01,)
SET_C = (0.2, -0.05, 1e-3, -5e-4, 0.01, 0.1, -0.02, 0.003)
SETS = {"A": SET_A, "B": SET_B, "C": SET_C}


def camera(f=3000.0, c=2047.5):
    return np.array([[f, 0.0, c], [0.0, f, c], [0.0, 0.0, 1.0]])


def _coeffs(dist):
    k = np.zeros(8, np.float64)
    d = np.asarray(dist, np.float64).ravel()
    assert d.size in (0, 4, 5, 8)
    k[:d.size] = d
    return k          # k1 k2 p1 p2 k3 k4 k5 k6


def _terms(k, x, y):
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(v) for v in k)
    one, two = np.float64(1.0), np.float64(2.0)
    xx = x * x
    yy = y * y
    r2 = xx + yy
    r4 = r2 * r2
    r6 = r4 * r2
    num = ((one + k1 * r2) + k2 * r4) + k3 * r6
    den = ((one + k4 * r2) + k5 * r4) + k6 * r6
    rc = num / den
    a1 = (two * x) * y
    a2 = r2 + two * xx
    a3 = r2 + two * yy
    dx = p1 * a1 + p2 * a2
    dy = p1 * a3 + p2 * a1
    return rc, dx, dy


def _forward_normalised(K, k, x, y):
    fx, cx, fy, cy = np.float64(K[0, 0]), np.float64(K[0, 2]), np.float64(K[1, 1]), np.float64(K[1, 2])
    rc, dx, dy = _terms(k, x, y)
    xd = x * rc + dx
    yd = y * rc + dy
    return fx * xd + cx, fy * yd + cy


def distort_points_ref(xy, K, dist):
    """ideal pixels [n, 2] -> distorted pixels [n, 2]"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    K = np.asarray(K, np.float64).reshape(3, 3)
    fx, cx, fy, cy = np.float64(K[0, 0]), np.float64(K[0, 2]), np.float64(K[1, 1]), np.float64(K[1, 2])
    with np.errstate(all="ignore"):
        u, v = _forward_normalised(K, _coeffs(dist), (xy[:, 0] - cx) / fx, (xy[:, 1] - cy) / fy)
    return np.stack([u, v], 1)


def undistort_points_ref(xy, K, dist, iters=5):
    """distorted pixels [n, 2] -> ideal pixels [n, 2]: exactly `iters` fixed-point steps"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    K = np.asarray(K, np.float64).reshape(3, 3)
    k = _coeffs(dist)
    fx, cx, fy, cy = np.float64(K[0, 0]), np.float64(K[0, 2]), np.float64(K[1, 1]), np.float64(K[1, 2])
    with np.errstate(all="ignore"):
        x0 = (xy[:, 0] - cx) / fx
        y0 = (xy[:, 1] - cy) / fy
        x, y = x0, y0
        for _ in range(int(iters)):
            rc, dx, dy = _terms(k, x, y)
            x, y = (x0 - dx) / rc, (y0 - dy) / rc
        return np.stack([fx * x + cx, fy * y + cy], 1)


def undistort_points_f32_ref(xy_f32, K, dist, iters=5):
    """the device call on f32 pairs: widened to f64, undistorted, rounded once to f32"""
    return undistort_points_ref(np.asarray(xy_f32, np.float32).astype(np.float64), K, dist, iters).astype(np.float32)


def _sat_int_rn(v):
    """round half to even, saturated to int32 (np.rint is IEEE roundTiesToEven)"""
    return np.clip(np.rint(v), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def undistort_map_ref(rows, cols, K, dist, new_K=None):
    """(X, Y) [rows, cols] int64: the source position of every destination pixel in 1/32 pixel"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    N = K if new_K is None else np.asarray(new_K, np.float64).reshape(3, 3)
    nfx, ncx, nfy, ncy = np.float64(N[0, 0]), np.float64(N[0, 2]), np.float64(N[1, 1]), np.float64(N[1, 2])
    u = np.arange(cols, dtype=np.float64)[None, :] + np.zeros((rows, 1))
    v = np.arange(rows, dtype=np.float64)[:, None] + np.zeros((1, cols))
    with np.errstate(all="ignore"):
        us, vs = _forward_normalised(K, _coeffs(dist), (u - ncx) / nfx, (v - ncy) / nfy)
        return _sat_int_rn(us * np.float64(32.0)), _sat_int_rn(vs * np.float64(32.0))


def footprint(X, Y, rows, cols):
    """(inside [rows, cols, 4] bool per tap in the order (0,0) (1,0) (0,1) (1,1) as (dx, dy), sx, sy)"""
    sx, sy = X >> 5, Y >> 5
    ins = []
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        ins.append((sx + dx >= 0) & (sx + dx < cols) & (sy + dy >= 0) & (sy + dy < rows))
    return np.stack(ins, -1), sx, sy


def undistort_image_ref(src, K, dist, new_K=None, border=0):
    """cv::undistort's shape with the warp's fixed-point tail: exact integers, (sum p w + 2^14) >> 15, taps outside the source = border"""
    a = np.asarray(src)
    assert a.dtype == np.uint8
    img = (a[:, :, None] if a.ndim == 2 else a).astype(np.int64)
    rows, cols = img.shape[:2]
    X, Y = undistort_map_ref(rows, cols, K, dist, new_K)
    ins, sx, sy = footprint(X, Y, rows, cols)
    w = DYADIC_W[Y & 31, X & 31]                                # [rows, cols, 4]
    acc = np.zeros((rows, cols, img.shape[2]), np.int64)
    for k, (dx, dy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        tap = img[np.clip(sy + dy, 0, rows - 1), np.clip(sx + dx, 0, cols - 1)]
        tap = np.where(ins[:, :, k, None], tap, border)
        acc += tap * w[:, :, k, None]
    out = (acc + (1 << 14)) >> 15
    assert out.min() >= 0 and out.max() <= 255
    out = out.astype(np.uint8)
    return out[:, :, 0] if a.ndim == 2 else out
