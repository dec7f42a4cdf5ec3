"""Shared by tests/test_akaze_mask_support_cpu.py and tests/test_akaze_mask_support_gpu.py: the expected result of a masked extraction
with a mask SUPPORT, built from the UNMASKED oracle result with numpy alone (integers only; no text in common with the kernels), on top of
akaze_mask_cases.py, whose tiles, masks and cut it uses.

The rule (include/apds.h, apds_akaze_extract_masked_support). A keypoint of octave o has ratio = 2^o, scale = rint(0.5f * size / ratio)
in f32, half to even, and with an integer support >= 0 the radius R = support * scale * ratio full-resolution pixels. Its centre is the
pixel of the plain mask rule, cx = (int)(pt.x + 0.5f), cy = (int)(pt.y + 0.5f). It is removed iff at least one mask byte is zero in
[cx - R, cx + R] x [cy - R, cy + R] clipped to the image (outside the image nothing is masked). Survivors keep their order; the max_points
cut of akaze_mask_cases.masked comes after. Support 0 is akaze_mask_cases.survivors."""
import numpy as np

import akaze_mask_cases as mc

SUPPORT_DESCRIPTOR = 15      # APDS_MASK_SUPPORT_DESCRIPTOR

# Single zero pixels (row, column) of the 544 x 672 octave-3 tile at support 15, asserted on the oracle by the CPU test. The oracle's one
# octave-3 keypoint rounds to (255, 233) and has R = 15 * 2 * 8 = 240: its square is rows 15 .. 495, columns 0 .. 473.
PIXEL_CORNER = (0, 0)          # outside that square: 461 of 462 stay, the one removed is of octave 1
PIXEL_OCT3_EDGE = (495, 0)     # its last row: 461 stay, the one removed is the octave-3 keypoint
PIXEL_OCT3_PAST = (496, 0)     # one row further: all 462 stay


def zero_table(mask):
    """S[y][x] = the number of zero bytes in rows < y and columns < x: (rows + 1) x (cols + 1), int64"""
    m = np.asarray(mask)
    s = np.zeros((m.shape[0] + 1, m.shape[1] + 1), np.int64)
    s[1:, 1:] = np.cumsum(np.cumsum(m == 0, axis=0, dtype=np.int64), axis=1)
    return s


def scales(keypoints):
    ratio = np.exp2(keypoints["octave"].astype(np.float32)).astype(np.float32)
    return np.rint(np.float32(0.5) * keypoints["size"].astype(np.float32) / ratio).astype(np.int64)       # np.rint: half to even


def radii(keypoints, support):
    return int(support) * scales(keypoints) * (np.int64(1) << keypoints["octave"].astype(np.int64))


def square_zero_counts(keypoints, mask, support):
    """zero mask bytes in every keypoint's clipped square"""
    h, w = np.asarray(mask).shape
    if len(keypoints) == 0:
        return np.zeros(0, np.int64)
    s = zero_table(mask)
    cy, cx = mc.rounded(keypoints)
    r = radii(keypoints, support)
    y0, y1 = np.maximum(cy - r, 0), np.minimum(cy + r, h - 1) + 1
    x0, x1 = np.maximum(cx - r, 0), np.minimum(cx + r, w - 1) + 1
    return s[y1, x1] - s[y0, x1] - s[y1, x0] + s[y0, x0]


def survivors(keypoints, mask, support):
    """boolean row selector"""
    return square_zero_counts(keypoints, mask, support) == 0


def masked(ref, mask, support, max_points=None):
    keep = survivors(ref.keypoints, mask, support)
    kept = mc.Extraction(ref.keypoints[keep], ref.descriptors[keep])
    return mc.masked(kept, np.ones(np.asarray(mask).shape, np.uint8), max_points)       # the existing cut; an all-ones mask removes nothing


def hole(h=mc.H, w=mc.W):
    m = np.ones((h, w), np.uint8)
    m[150:200, 300:340] = 0
    return m


def single_pixel(row, col, h=mc.H, w=mc.W):
    m = np.full((h, w), 255, np.uint8)
    m[row, col] = 0
    return m
