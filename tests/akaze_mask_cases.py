"""Shared by tests/test_akaze_mask_cpu.py and tests/test_akaze_mask_gpu.py: the expected result of a masked extraction, built from the
UNMASKED oracle result with numpy alone (no text in common with the kernels), and the one tile both files use.

The rule (OpenCV 4.8 AKAZE_Impl::detectAndCompute -> KeyPointsFilter::runByPixelsMask, recalled): detection runs
unmasked; a keypoint goes iff mask[(int)(pt.y + 0.5f)][(int)(pt.x + 0.5f)] == 0, f32 additions, truncating conversion; the survivors keep
their order; then, if more than max_points remain, the strongest responses stay (ties by detection order), strongest first."""
import numpy as np

H, W = 352, 640        # the smallest shape with four octaves (octave 3: 80 x 44, above the 80 / 40 stop); not square
FRAME = 22             # tried on the CPU with the oracle: the preconditions the tests assert hold for this frame

# Octave 3 of a 352-row image (44 rows) lies inside its own border (29 pixels and more on every side) and holds no keypoint, whatever the
# content. The smallest image that gives it room, with content of that scale: a 544 x 672 tile plus six wide Gaussian blobs
# (row, column, sigma, amplitude) around its centre. Tried on the CPU with the oracle: one keypoint in octave 3.
H3, W3 = 544, 672
WIDE_BLOBS = [(259, 433, 16, 93), (264, 323, 17, 55), (270, 284, 15, -59), (294, 320, 15, -79), (279, 365, 23, 68), (256, 239, 14, -69)]


def octave3_tile(pkg):
    img = pkg.synth.make_tile(H3, W3, frame_index=0, channels=1).astype(np.float64)
    yy, xx = np.mgrid[0:H3, 0:W3]
    for cy, cx, s, a in WIDE_BLOBS:
        img += a * np.exp(-0.5 * (((yy - cy) / s) ** 2 + ((xx - cx) / s) ** 2))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


class Extraction:
    """what _assert_same_extraction of tests/test_akaze_gpu.py compares: .keypoints (structured) and .descriptors"""

    def __init__(self, keypoints, descriptors):
        self.keypoints, self.descriptors = keypoints, descriptors


def rounded(keypoints):
    """(row, column) of the mask byte every keypoint is judged by"""
    half = np.float32(0.5)
    ys = (keypoints["y"].astype(np.float32) + half).astype(np.int32)
    xs = (keypoints["x"].astype(np.float32) + half).astype(np.int32)
    return ys, xs


def survivors(keypoints, mask):
    """boolean row selector"""
    ys, xs = rounded(keypoints)
    return np.asarray(mask)[ys, xs] != 0 if len(keypoints) else np.zeros(0, bool)


def masked(ref, mask, max_points=None):
    keep = survivors(ref.keypoints, mask)
    k, d = ref.keypoints[keep], ref.descriptors[keep]
    if max_points is not None and len(k) > max_points:
        order = np.argsort(-k["response"].astype(np.float64), kind="stable")[:max_points]
        k, d = k[order], d[order]
    return Extraction(k, d)


def assert_same(got, ref):
    """bit-exact on all seven keypoint fields and the descriptors"""
    gk, rk = got.keypoints, ref.keypoints
    assert len(gk) == len(rk), (len(gk), len(rk))
    for f in ("class_id", "octave", "x", "y", "size", "response", "angle"):
        assert np.array_equal(gk[f], rk[f]), f
    assert np.array_equal(got.descriptors, ref.descriptors)


def checkerboard(h=H, w=W):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx + yy) & 1).astype(np.uint8)


def left_half(h=H, w=W):
    m = np.zeros((h, w), np.uint8)
    m[:, : w // 2] = 1
    return m


def top_half(h=H, w=W):
    m = np.zeros((h, w), np.uint8)
    m[: h // 2] = 200
    return m
