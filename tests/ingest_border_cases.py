"""Inputs of the ingest border tests: shared by test_ingest_reference_cpu.py (the oracle against tests/ingest_reference.py) and
test_ingest_borders_gpu.py (the HIP kernels against the same references and the oracle). Data only; not a test module.

Launch shapes restated from csrc/ingest.hip so that a change there shows up against this table in review:
band_merger_kernel runs min(ceil(n / 256), 256 * 16) blocks of 256 threads with a grid-stride loop; the warp kernels run 256 threads along
x and one destination row per block; the world-point kernels run 256 threads (four waves of 64) per block."""
from fractions import Fraction

import numpy as np

import ingest_reference as ref

# ---- band merge ------------------------------------------------------------------------------------------------------------------------
BAND_BLOCK, BAND_GRID_CAP = 256, 256 * 16
BAND_LENGTHS = (1, 255, 256, 257, BAND_BLOCK * BAND_GRID_CAP + 3)      # the last: three elements into the loop's second trip
BAND_MINMAX = {
    "plain": (0.0, 1.0, 0.0017, 0.93, -1.0, 2.0),
    "degenerate": (0.5, 0.5, 1.0, 0.0, 0.0, 1.0),                      # red: min == max; green: min > max
}


def u8_boundary_values(mn, mx):
    """For each of the 255 rounding boundaries k + 0.5 of 255 f^(1/2.2): the f32 band values nearest to it from either side that the
    reference places outside its near-tie band, for a band normalised by (mn, mx): 510 values in pairs. With mn == mx nothing is valid
    and the values are mn itself."""
    mn, mx = np.float32(mn), np.float32(mx)
    if mn == mx:
        return np.full(510, mn, np.float32)
    k = np.arange(255)
    out = []
    for want, side in ((k, -1), (k + 1, 1)):
        # start at the edge of the band (where f is small the f32 grid is far finer than the band), then step until the reference agrees
        f = (((k + ref.LD(0.5) + side * ref.LD(ref.TIE_BAND)) / 255) ** (1 / ref.LD(ref.GAMMA_F32))).astype(np.float32)
        v = (mn + f * (mx - mn)).astype(np.float32)
        towards = np.float32(side) * np.sign(mx - mn)
        for _ in range(64):
            got, tie = ref.band_to_u8_ref(v, mn, mx)
            bad = (got != want) | tie
            if not bad.any():
                break
            # one step of the grid that v - mn lives on (a step of v alone may be lost in that subtraction)
            v[bad] = v[bad] + np.sign(towards) * np.maximum(np.spacing(np.abs(v[bad])), np.spacing(np.abs(mn)))
        assert not bad.any()
        out.append(v)
    return np.stack(out, 1).ravel()


_NAN_PIXELS = [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]     # which bands are NaN; all three first


def band_specials(minmax6):
    """[3, L] f32: per band the NaN patterns, then min and max themselves, one f32 step outside and inside each, -0.0, +-inf, then the
    band's u8 boundary values. Bands are rolled against each other so
    that no pixel has three equal bytes."""
    bands = []
    for c in range(3):
        mn, mx = np.float32(minmax6[2 * c]), np.float32(minmax6[2 * c + 1])
        edge = [mn, mx, np.nextafter(mn, np.float32(-np.inf)), np.nextafter(mn, np.float32(np.inf)), np.nextafter(mx, np.float32(-np.inf)),
                np.nextafter(mx, np.float32(np.inf)), np.float32(-0.0), np.float32(np.inf), np.float32(-np.inf)]
        body = np.concatenate([np.array(edge, np.float32), u8_boundary_values(mn, mx)])
        body = np.roll(body, 3 * c)
        mid = np.float32(0.5) * (mn + mx) + np.float32(0.125)
        head = np.array([np.nan if p[c] else mid for p in _NAN_PIXELS], np.float32)
        bands.append(np.concatenate([head, body]))
    return np.stack(bands)


def band_case(n, minmax_name):
    """(bands [3, n] f32, minmax6). Pixel n - 1 - i is special i for as long as the specials last, so the last pixels of every length are
    NaN patterns and edges; a longer array also begins with the specials and holds seeded values from a little outside [min, max] between."""
    mm = BAND_MINMAX[minmax_name]
    sp = band_specials(mm)
    L = sp.shape[1]
    if n <= L:
        return np.ascontiguousarray(sp[:, :n][:, ::-1]), mm
    rng = np.random.default_rng(n)
    out = np.empty((3, n), np.float32)
    for c in range(3):
        lo, hi = min(mm[2 * c], mm[2 * c + 1]), max(mm[2 * c], mm[2 * c + 1])
        span = (hi - lo) or 1.0
        out[c] = rng.uniform(lo - 0.1 * span, hi + 0.1 * span, n).astype(np.float32)
    out[:, :L] = sp
    out[:, n - L:] = sp[:, ::-1]
    return out, mm


BAND_CASES = [(n, name) for name in BAND_MINMAX for n in BAND_LENGTHS] + [(band_specials(BAND_MINMAX[name]).shape[1], name) for name in BAND_MINMAX]

# ---- perspective warp ------------------------------------------------------------------------------------------------------------------
WARP_BLOCK = 256
WARP_TYPES = [(np.uint8, 1), (np.uint8, 3), (np.uint8, 4), (np.float32, 1), (np.float32, 3), (np.float32, 4)]
WARP_SOURCES = [(7, 5), (1, 1), (1, 9), (9, 1)]                           # (width, height)
WARP_SHIFTS_1D = (0, 1, 31, 32, 33, -1, -31, -32, -33)                    # in 1/32 pixel
WARP_SHIFTS = [(tx, ty) for ty in WARP_SHIFTS_1D for tx in WARP_SHIFTS_1D]
WARP_SHIFT_OUTSIDE = (32 * 64, -32 * 64)                                  # the whole destination reads border
WARP_WIDTHS, WARP_HEIGHTS = (1, 255, 256, 257), (1, 2)
# for the wide destinations over the 7 x 5 source: the second and third put columns 256 / 254..256 (the second block) onto the source
WARP_WIDTH_SHIFTS = [(0, 0), (-(32 * 251) - 1, 31), (-(32 * 254) - 31, -33)]


def warp_source(dtype, channels, width, height):
    """seeded image; f32 elements are integers below 2^10, so every product with a 10-bit weight and every sum of four is exact in
    binary32 in any order"""
    rng = np.random.default_rng(1000 * width + 10 * height + channels)
    shape = (height, width) if channels == 1 else (height, width, channels)
    return rng.integers(0, 256, shape).astype(np.uint8) if dtype == np.uint8 else rng.integers(0, 1 << 10, shape).astype(np.float32)


def shift_matrix(tx32, ty32):
    """the forward map whose inverse is "destination (x, y) reads source (x + tx32 / 32, y + ty32 / 32)": exact in f64"""
    return np.array([[1, 0, -tx32 / 32], [0, 1, -ty32 / 32], [0, 0, 1]], np.float64)


def exact_inverse(m):
    """Gauss-Jordan in exact rationals -> 3 x 3 list of Fraction"""
    a = [[Fraction(float(v)) for v in row] + [Fraction(int(i == r)) for i in range(3)] for r, row in enumerate(np.asarray(m, np.float64))]
    for c in range(3):
        p = next(r for r in range(c, 3) if a[r][c] != 0)
        a[c], a[p] = a[p], a[c]
        a[c] = [v / a[c][c] for v in a[c]]
        for r in range(3):
            if r != c:
                a[r] = [v - a[r][c] * w for v, w in zip(a[r], a[c])]
    return [row[3:] for row in a]


def forward_of(minv):
    """the f64 forward matrix of a dyadic inverse map; raises if an entry is not exactly representable"""
    inv = exact_inverse(minv)
    out = np.array([[float(v) for v in row] for row in inv], np.float64)
    assert all(Fraction(float(out[r, c])) == inv[r][c] for r in range(3) for c in range(3))
    return out


WARP_BOUNDED_SRC = (40, 56)                                               # (width, height), value 3 x + y + 10 c
WARP_BOUNDED_DST = (48, 60)
# destination -> source, every entry dyadic, determinant a power of two (checked in test_ingest_reference_cpu.py), W > 0 on the destination
WARP_BOUNDED_MINV = [
    [[127 / 128, 1 / 8, -341 / 128], [-1 / 16, 1.0, 43 / 16], [131 / 65536, -3 / 4096, 65023 / 65536]],      # determinant 1
    [[1 / 2, 0.0, 17 / 4], [1 / 8, 1.0, -79 / 16], [-7 / 4096, 1 / 512, 7977 / 8192]],                          # determinant 1/2
    [[3 / 4, -1 / 4, 19 / 2], [1 / 2, 1 / 2, 1.0], [1 / 256, 1 / 256, 129 / 128]],                              # determinant 1/2
]


def warp_bounded_source(dtype, channels):
    y, x, c = np.mgrid[0:WARP_BOUNDED_SRC[1], 0:WARP_BOUNDED_SRC[0], 0:channels]
    img = (3 * x + y + 10 * c).astype(dtype)
    return img[:, :, 0] if channels == 1 else img


# W == 0 on destination column 4, W < 0 on columns 0-3: M's third row is (0.25, 0, -0.25), identity otherwise
WARP_WZERO_M = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.25, 0.0, -0.25]]
WARP_WZERO_MINV = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 0.0, -4.0]]
WARP_WZERO_COLUMN = 4
# both source coordinates beyond the int range for x > 0: (X0, Y0, W) = (x + 1, y + 1, 2^-40 x)
WARP_SATURATE_MINV = [[1.0, 0.0, 1.0], [0.0, 1.0, 1.0], [2.0 ** -40, 0.0, 0.0]]
WARP_STRUCT_SRC, WARP_STRUCT_DST = (7, 5), (12, 5)

# ---- world points ----------------------------------------------------------------------------------------------------------------------
WORLD_BLOCK, WAVE = 256, 64
ELEV_W, ELEV_H = 8, 6
_r, _c = np.mgrid[0:ELEV_H, 0:ELEV_W]
ELEV = (100.0 + 37.0 * _r + 3.5 * _c).astype(np.float64)                  # every height differs from its neighbours by metres
ELEV[2, 3] = -412.25
# power-of-two steps on a common origin: px = x / 4 and py = y / 4 exactly, in f64 and for the f32 columns of the keypoint table
DGT_POW2 = [9.0, 2.0 ** -12, 0.0, 57.0, 0.0, -(2.0 ** -12)]
EGT_POW2 = [9.0, 2.0 ** -10, 0.0, 57.0, 0.0, -(2.0 ** -10)]
POW2_SCALE = 4.0


def _edge_positions(n):
    return [-0.5, -0.5 + 2.0 ** -20, 0.5, 1.5, n - 0.5, n - 0.5 - 2.0 ** -20, float(n), -1.0]


WORLD_EDGE_PXPY = [(px, float(py)) for py in (0, 3, ELEV_H - 1) for px in _edge_positions(ELEV_W)] + \
                  [(float(px), py) for px in (0, 3, ELEV_W - 1) for py in _edge_positions(ELEV_H)]
WORLD_EDGE_XY = np.array([(POW2_SCALE * px, POW2_SCALE * py) for px, py in WORLD_EDGE_PXPY], np.float64)
WORLD_COLUMN_COUNTS = (1, 63, 64, 65, 257)                                # partial waves, a full wave, a second block


def world_edge_points(n):
    """the edge points, repeated in order up to n"""
    return np.ascontiguousarray(WORLD_EDGE_XY[np.arange(n) % len(WORLD_EDGE_XY)])


# the globe: (x, y) is (lon, lat) in degrees; the 8 x 6 raster covers it in 64-degree cells
DGT_GLOBE = [0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
EGT_GLOBE = [-256.0, 64.0, 0.0, 128.0, 0.0, -64.0]
WORLD_GLOBE_XY = np.array([(lon, lat) for lat in (90.0, -90.0, 89.999999, -89.999999, 0.0)
                           for lon in (0.0, 180.0, -180.0, 179.999999, -179.999999, 190.0, -190.0)], np.float64)
# rotated / sheared transforms: the general inverse
DGT_ROT = [-70.6, 2e-4, 1e-6, -33.3, -2e-6, -2e-4]
EGT_ROT = [-70.62, 0.03, 1e-4, -33.27, 2e-4, -0.04]
WORLD_ROT_XY = np.random.default_rng(12).uniform(0, 1000, (64, 2))

WORLD_CASES = {                                                           # name: (xy, dataset transform, elevation transform or None)
    "edges": (WORLD_EDGE_XY, DGT_POW2, EGT_POW2),
    "globe": (WORLD_GLOBE_XY, DGT_GLOBE, None),
    "globe_elevation": (WORLD_GLOBE_XY, DGT_GLOBE, EGT_GLOBE),
    "rotated": (WORLD_ROT_XY, DGT_ROT, None),
    "rotated_elevation": (WORLD_ROT_XY, DGT_ROT, EGT_ROT),
}
