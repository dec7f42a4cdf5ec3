"""The inputs of tests/test_akaze_float_cpu.py and tests/test_akaze_float_gpu.py, built in one place so that the tolerance of
tests/msurf_reference.py (E32: the f32 form of the reference against its f64 form) is measured over every one of them:

    python tests/akaze_float_cases.py        # no GPU: prints the figure case by case, then E32 and TOL

Hook cases (apds_dev_akaze_describe_float): synthetic planes of 40 x 56 and 33 x 33 - the smallest shapes at which the kernel can still go
wrong (a pattern of scale 1 reaches 12 * sqrt(2) = 17 pixels, so every corner keypoint clamps and at scale 5 most of the lattice does).
Image cases: three synth tiles and a scene with its shifted view; where there is no GPU their planes and keypoints are the oracle's.
"""
import os
import sys

import numpy as np

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

HOOK_SHAPES = ((40, 56), (33, 33))                  # (h, w)
CONSTANT_ANGLES = (0.0, 37.0, 180.0, 301.5)
HOOK_SCALES = (1, 2, 5)
HOOK_ANGLES = (0.0, 90.0, 359.9)
LIVE_LANE_COUNTS = (1, 3, 4, 5, 9)                  # keypoints per call: the live / not-live waves of a block of four
TILES = ((96, 640, 1), (200, 333, 3), (256, 256, 4))
SHIFT = (7, -5)                                     # the second view of the scene moved by (+7, -5) px
SCENE_VIEW = (256, 320)
RATIO = 0.7


def keypoints(rows):
    """rows of (x, y, size, angle, octave) in full-resolution units -> cv::KeyPoint array (class_id 0: the hook ignores it)"""
    k = np.zeros(len(rows), KEYPOINT_DTYPE)
    for n, (x, y, size, angle, octave) in enumerate(rows):
        k[n] = (x, y, size, angle, 1.0, octave, 0)
    return k


def _positions(h, w):
    """the plane's four corners and its centre (plane coordinates)"""
    return ((0.0, 0.0), (w - 1.0, 0.0), (0.0, h - 1.0), (w - 1.0, h - 1.0), (0.5 * w + 0.25, 0.5 * h - 0.375))


def _random_planes(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((h, w)).astype(np.float32), rng.standard_normal((h, w)).astype(np.float32)


def constant_cases():
    """name -> (lx, ly, kps, angle): Lx = 1, Ly = 0; keypoints at the centre, at a corner and with most of the pattern off the plane"""
    out = {}
    for h, w in HOOK_SHAPES:
        lx, ly = np.ones((h, w), np.float32), np.zeros((h, w), np.float32)
        for a in CONSTANT_ANGLES:
            rows = [(0.5 * w, 0.5 * h, 4.0, a, 0), (0.0, 0.0, 4.0, a, 0), (-3.0, h + 2.0, 6.0, a, 0), (4.0 * (w - 1), 4.0 * 2, 16.0, a, 2)]
            out[f"constant_{h}x{w}_{a}"] = (lx, ly, keypoints(rows), a)
    return out


def random_cases():
    """name -> (lx, ly, kps): seeded random planes; corners and centre at scales 1, 2, 5, octaves 0 and 2, angles 0, 90, 359.9; the ties of
    rint; 1, 3, 4, 5 and 9 keypoints per call"""
    out = {}
    for si, (h, w) in enumerate(HOOK_SHAPES):
        lx, ly = _random_planes(h, w, 1000 + si)
        for scale in HOOK_SCALES:
            rows = [(x, y, 2.0 * scale, a, 0) for (x, y) in _positions(h, w) for a in HOOK_ANGLES]
            rows += [(4.0 * x, 4.0 * y, 8.0 * scale, 37.0, 2) for (x, y) in _positions(h, w)]       # octave 2: ratio 4
            out[f"random_{h}x{w}_scale{scale}"] = (lx, ly, keypoints(rows))
        cx, cy = _positions(h, w)[4]
        # 0.5 * size / ratio = 2.5 -> 2, 3.5 -> 4 (ties to even), and 2.5 again at octave 2
        out[f"rint_ties_{h}x{w}"] = (lx, ly, keypoints([(cx, cy, 5.0, 123.4, 0), (cx, cy, 7.0, 123.4, 0), (4 * cx, 4 * cy, 20.0, 123.4, 2)]))
        rng = np.random.default_rng(2000 + si)
        nine = [(float(rng.uniform(0, w)), float(rng.uniform(0, h)), 4.0, float(rng.uniform(0, 360)), 0) for _ in range(9)]
        for n in LIVE_LANE_COUNTS:
            out[f"count{n}_{h}x{w}"] = (lx, ly, keypoints(nine[:n]))
    return out


def zero_case():
    h, w = HOOK_SHAPES[0]
    z = np.zeros((h, w), np.float32)
    return z, z.copy(), keypoints([(0.5 * w, 0.5 * h, 4.0, 10.0, 0), (0.0, 0.0, 10.0, 200.0, 0), (8.0, 8.0, 16.0, 45.0, 2)])


def hook_cases():
    """every hook case as name -> (lx, ly, kps)"""
    out = {name: c[:3] for name, c in constant_cases().items()}
    out.update(random_cases())
    out["zero_plane"] = zero_case()
    return out


def smooth_scene(h, w, seed, blobs=None):
    """The scene of tests/test_akaze_anchors.py: Gaussian blobs of random size, sign and place on mid-grey (float64)."""
    rng = np.random.default_rng(seed)
    n = blobs if blobs is not None else (h * w) // 50
    img = np.full((h, w), 128.0)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(n):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        s = rng.uniform(1.2, 6.0)
        a = rng.uniform(30, 100) * rng.choice([-1.0, 1.0])
        r = int(4 * s) + 1
        x0, x1, y0, y1 = max(0, int(cx) - r), min(w, int(cx) + r + 1), max(0, int(cy) - r), min(h, int(cy) + r + 1)
        img[y0:y1, x0:x1] += a * np.exp(-((xx[y0:y1, x0:x1] - cx) ** 2 + (yy[y0:y1, x0:x1] - cy) ** 2) / (2 * s * s))
    return img


SCENE_SEED = 23


def shifted_views():
    """(a, b): b is the view of the same scene moved by SHIFT = (+dx, +dy), so content at (x, y) of a appears at (x - dx, y - dy) of b"""
    h, w = SCENE_VIEW
    dx, dy = SHIFT
    scene = smooth_scene(h + 16, w + 20, seed=SCENE_SEED)
    u8 = lambda v: np.clip(np.rint(v), 0, 255).astype(np.uint8)      # noqa: E731
    y0, x0 = 8, 6
    return u8(scene[y0:y0 + h, x0:x0 + w]), u8(scene[y0 + dy:y0 + dy + h, x0 + dx:x0 + dx + w])


def image_cases(synth):
    """name -> u8 image: the three tiles and the two views"""
    out = {f"tile_{h}x{w}x{c}": synth.make_tile(h, w, channels=c) for h, w, c in TILES}
    out["view_a"], out["view_b"] = shifted_views()
    return out


def oracle_planes(res):
    """level -> (Lx, Ly) of the levels that carry a keypoint, from an oracle run with keep_planes=True"""
    return {int(lv): (res.plane(int(lv), 2), res.plane(int(lv), 3)) for lv in np.unique(res.keypoints["class_id"])}


def level_shapes(h, w):
    """(h, w) of AKAZE's 16 evolution levels: halved per octave until a side falls below 80 x 40"""
    out = []
    for _ in range(4):
        out += [(h, w)] * 4
        h, w = h >> 1, w >> 1
        if w < 80 or h < 40:
            break
    return out


def ratio_margins(ds, ratio=RATIO):
    """per query, the reference's margins |d0 - ratio d1| and |d1 - d2| (ds: sorted distances [nq, 3])"""
    return np.abs(ds[:, 0] - ratio * ds[:, 1]), np.abs(ds[:, 1] - ds[:, 2])


def measure_e32(log=print):
    """max |f32 form - f64 form| of the reference over every input of the two test modules (the image cases on the oracle's planes)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.dirname(os.path.abspath(__file__))):
        if p not in sys.path:
            sys.path.insert(0, p)
    import __graft_entry__ as graft
    import msurf_reference as ref
    import oracle
    oracle.build()
    worst = 0.0
    for name, (lx, ly, kps) in hook_cases().items():
        e = float(np.abs(ref.describe_plane(lx, ly, kps, np.float32).astype(np.float64) - ref.describe_plane(lx, ly, kps, np.float64)).max())
        log(f"{name:32s} n={len(kps):4d}  e32={e:.3e}")
        worst = max(worst, e)
    for name, img in image_cases(graft.load_package().synth).items():
        res = oracle.akaze(img, keep_planes=True)
        planes = oracle_planes(res)
        e = float(np.abs(ref.describe_levels(planes, res.keypoints, np.float32).astype(np.float64) - ref.describe_levels(planes, res.keypoints, np.float64)).max())
        log(f"{name:32s} n={len(res.keypoints):4d}  e32={e:.3e}")
        worst = max(worst, e)
    return worst


if __name__ == "__main__":
    e32 = measure_e32()
    print(f"E32 = {e32!r}\nTOL = 4 * E32 = {4 * e32!r}")
