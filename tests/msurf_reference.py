"""NumPy restatement of AKAZE's float descriptor (DESCRIPTOR_KAZE: M-SURF, 64 floats), written from the formulas of include/apds.h and
DESIGN.md section 2 ("the float descriptor"), not from the kernel (csrc/akaze_describe_msurf.hip): the reference of tests/test_akaze_float_*.py.

Per keypoint, on the (Lx, Ly) planes of its level:
    ratio = 2^octave, scale = rint(0.5f * size / ratio) in f32 (ties to even), xf = x / ratio, yf = y / ratio, angle = kp.angle * pi / 180,
    co, si = cos, sin of it;
    4 x 4 cells with origins i, j in {-12, -7, -2, 3} (i outer), ky = i + 5, kx = j + 5, the cell centre
        xs = xf + (-kx scale si + ky scale co),  ys = yf + (kx scale co + ky scale si);
    81 samples k = i .. i + 8 (outer), l = j .. j + 8 (inner):
        sample_y = yf + (l scale co + k scale si),  sample_x = xf + (-l scale si + k scale co),
        g1 = exp(-((xs - sample_x)^2 + (ys - sample_y)^2) / (2 (2.5 scale)^2)),
        x1 = floor(sample_x), y1 = floor(sample_y), x2 = x1 + 1, y2 = y1 + 1, all four clamped to the plane, fx = sample_x - x1, fy = sample_y - y1
        with the CLAMPED x1, y1; rx, ry the bilinear blends of Lx, Ly with weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy;
        rry = g1 (rx co + ry si), rrx = g1 (-rx si + ry co); dx += rrx, dy += rry, mdx += |rrx|, mdy += |rry|;
    the cell writes (dx, dy, mdx, mdy) g2 at 4 (4 ci + cj), g2 = exp(-((ci - 1.5)^2 + (cj - 1.5)^2) / (2 1.5^2));
    every entry times 1 / sqrt(sum of squares); a zero sum leaves 64 zeros (OpenCV: NaN).

dtype float64: all arithmetic in double on the f32 keypoint fields and planes, `scale` alone in f32 as specified. dtype float32: the same
formulas with every operation rounded to f32 (sums sequential, k-major and l-minor; the entries' squares in entry order).

E32 / TOL: the f32 form's largest absolute difference from the f64 form over EVERY input of tests/test_akaze_float_cpu.py and
tests/test_akaze_float_gpu.py (tests/akaze_float_cases.py builds them all: the hook cases, and the oracle's planes and keypoints for the
image cases; `python tests/akaze_float_cases.py` prints the figure case by case), and the tests' tolerance 4 * E32: the factor covers what
the kernel may do differently from the f32 form - contract multiply-adds, take g1 from a table, reduce the norm in another order - each of
the order of the f32 form's own rounding. Entries are at most 1 and unrelated descriptors are of order 1 apart, so a TOL above 1e-3 would
mean the f32 form is wrong. The GPU's own error never sets these.
"""
import numpy as np

E32 = 3.2227002154938678e-06      # measured (python tests/akaze_float_cases.py): the 33 x 33 random plane at scale 5, where most corners are clamped
TOL = 4 * E32                     # 1.2890800861975471e-05

CELL_ORIGINS = (-12, -7, -2, 3)


def _scale_f32(kp):
    """rint(0.5f * size / ratio), every operation in f32, ties to even - in both forms"""
    ratio = np.float32(2.0 ** int(kp["octave"]))
    return np.rint(np.float32(0.5) * np.float32(kp["size"]) / ratio)


def _seq_sum(a):
    """the sum of a 1-D array in index order, in the array's own precision"""
    return np.add.accumulate(a)[-1]


def describe_one(lx, ly, kp, dtype=np.float64):
    """One keypoint (a row of a cv::KeyPoint structured array) on the planes lx, ly (h x w float32) -> 64 values of `dtype`."""
    F = np.dtype(dtype).type
    h, w = lx.shape
    lx, ly = lx.astype(F), ly.astype(F)
    ratio = F(2.0 ** int(kp["octave"]))
    scale = F(_scale_f32(kp))
    xf, yf = F(kp["x"]) / ratio, F(kp["y"]) / ratio
    angle = F(kp["angle"]) * (F(np.pi) / F(180))
    co, si = np.cos(angle), np.sin(angle)
    assert co.dtype == F and scale.dtype == F
    desc = np.zeros(64, F)
    for ci, i in enumerate(CELL_ORIGINS):
        for cj, j in enumerate(CELL_ORIGINS):
            ky, kx = F(i + 5), F(j + 5)
            xs = xf + (-kx * scale * si + ky * scale * co)
            ys = yf + (kx * scale * co + ky * scale * si)
            k = np.arange(i, i + 9).astype(F)[:, None]          # outer
            l = np.arange(j, j + 9).astype(F)[None, :]          # inner
            sample_y = yf + (l * scale * co + k * scale * si)
            sample_x = xf + (-l * scale * si + k * scale * co)
            g1 = np.exp(-((xs - sample_x) * (xs - sample_x) + (ys - sample_y) * (ys - sample_y)) / (F(2) * (F(2.5) * scale) * (F(2.5) * scale)))
            x1, y1 = np.floor(sample_x).astype(np.int64), np.floor(sample_y).astype(np.int64)
            x2, y2 = x1 + 1, y1 + 1
            x1, x2 = np.clip(x1, 0, w - 1), np.clip(x2, 0, w - 1)
            y1, y2 = np.clip(y1, 0, h - 1), np.clip(y2, 0, h - 1)
            fx, fy = sample_x - x1.astype(F), sample_y - y1.astype(F)
            w11, w21, w12, w22 = (F(1) - fx) * (F(1) - fy), fx * (F(1) - fy), (F(1) - fx) * fy, fx * fy
            rx = w11 * lx[y1, x1] + w21 * lx[y1, x2] + w12 * lx[y2, x1] + w22 * lx[y2, x2]
            ry = w11 * ly[y1, x1] + w21 * ly[y1, x2] + w12 * ly[y2, x1] + w22 * ly[y2, x2]
            rry = g1 * (rx * co + ry * si)
            rrx = g1 * (-rx * si + ry * co)
            assert rrx.dtype == F and rrx.shape == (9, 9)
            g2 = np.exp(-((F(ci) - F(1.5)) * (F(ci) - F(1.5)) + (F(cj) - F(1.5)) * (F(cj) - F(1.5))) / (F(2) * F(1.5) * F(1.5)))
            sums = (_seq_sum(rrx.ravel()), _seq_sum(rry.ravel()), _seq_sum(np.abs(rrx).ravel()), _seq_sum(np.abs(rry).ravel()))
            for c in range(4):
                desc[(ci * 4 + cj) * 4 + c] = sums[c] * g2
    len_sq = _seq_sum(desc * desc)
    if len_sq == 0:
        return np.zeros(64, F)
    return desc * (F(1) / np.sqrt(len_sq))


def describe_plane(lx, ly, kps, dtype=np.float64):
    """All of `kps` on ONE plane (class_id ignored: what apds_dev_akaze_describe_float does) -> n x 64"""
    out = np.zeros((len(kps), 64), dtype)
    for n, kp in enumerate(kps):
        out[n] = describe_one(lx, ly, kp, dtype)
    return out


def describe_levels(planes, kps, dtype=np.float64):
    """Every keypoint on the planes of its level: planes[class_id] = (lx, ly) -> n x 64"""
    out = np.zeros((len(kps), 64), dtype)
    for n, kp in enumerate(kps):
        lx, ly = planes[int(kp["class_id"])]
        out[n] = describe_one(lx, ly, kp, dtype)
    return out


def constant_plane_row(angle_deg):
    """The normalised row on planes Lx = 1, Ly = 0, in closed form (float64): every sample has rx = 1, ry = 0 (the clamp keeps a constant
    constant), so every cell is (-si, co, |si|, |co|) S g2 with one common S > 0, and the row is g2(ci, cj) (-si, co, |si|, |co|) / sqrt(2 sum g2^2)
    (si^2 + co^2 twice per cell)."""
    a = np.float64(np.float32(angle_deg)) * (np.pi / 180)
    co, si = np.cos(a), np.sin(a)
    c = np.arange(4) - 1.5
    g2 = np.exp(-(c[:, None] ** 2 + c[None, :] ** 2) / (2 * 1.5 ** 2))
    row = g2[:, :, None] * np.array([-si, co, abs(si), abs(co)])[None, None, :]
    return row.reshape(64) / np.sqrt(2 * (g2 ** 2).sum())


def ratio_matches(q, t, ratio):
    """BFMatcher(NORM_L2).knnMatch(q -> t, 2) and the ratio test of lib.rs:107-111 in float64: (kept query indices, their train indices,
    d sorted ascending per query [nq, 3] for the margins, the order [nq, 3])."""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    d = np.stack([np.sqrt(((row[None, :] - t) ** 2).sum(1)) for row in q])
    order = np.argsort(d, axis=1, kind="stable")[:, :3]
    ds = np.take_along_axis(d, order, axis=1)
    keep = np.flatnonzero(ds[:, 0] < ds[:, 1] * ratio)
    return keep, order[keep, 0], ds, order
