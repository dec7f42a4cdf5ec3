"""Plain high-precision references of the three ingest operations (band merge, perspective warp, world points). Not a test module.

Written from the definitions of the operations (the reference crates' Rust, cv::warpPerspective's documented map, WGS 84), in numpy with
np.longdouble or exact integers; nothing here is taken from the HIP kernels or from oracle/, and oracle/ is not imported. Used by
test_ingest_reference_cpu.py (the oracle against these) and test_ingest_borders_gpu.py (the kernels against these)."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the references need an extended long double (x87 or wider)"

# ---- band merge: geotiff_extractor/src/image_extractor/mod.rs:346-378, 402-422 --------------------------------------------------------
GAMMA_F32 = np.float32(1.0) / np.float32(2.2)      # mod.rs:14, an f32 constant
TIE_BAND = 1e-4   # the product rounds g to f32 and g * 255 to f32: each at most 2^-24 * 255 = 1.5e-5 absolute; the band is 3x their sum


def band_to_u8_ref(v, mn, mx):
    """(u8 [n], near_tie [n]) of one band: f = (v - mn) / (mx - mn) in f32 (mod.rs:415 computes it in f32, so f32 is the specification);
    0 for NaN v and for f outside [0, 1] (NaN and +-inf included); else floor(255 f^(1/2.2) + 0.5), the power and the product in long
    double. near_tie marks the valid elements whose 255 f^(1/2.2) lies within TIE_BAND of a rounding tie."""
    v = np.asarray(v, np.float32)
    mn, mx = np.float32(mn), np.float32(mx)
    with np.errstate(all="ignore"):
        f = (v - mn) / (mx - mn)
        assert f.dtype == np.float32
        valid = ~np.isnan(v) & (f >= 0) & (f <= 1)      # comparisons with NaN are False
    g255 = LD(255) * np.where(valid, f, np.float32(0)).astype(LD) ** LD(GAMMA_F32)
    out = np.where(valid, np.floor(g255 + LD(0.5)), LD(0)).astype(np.uint8)
    near_tie = valid & (np.abs(g255 - np.floor(g255) - LD(0.5)) < LD(TIE_BAND))
    return out, near_tie


def band_merge_ref(red, green, blue, minmax6):
    """(rgba [n, 4] u8, near_tie [n, 4] bool): the three bands through band_to_u8_ref; alpha is 0 only where all three are NaN."""
    bands = [np.asarray(b, np.float32).ravel() for b in (red, green, blue)]
    out = np.zeros((len(bands[0]), 4), np.uint8)
    tie = np.zeros((len(bands[0]), 4), bool)
    for c, b in enumerate(bands):
        out[:, c], tie[:, c] = band_to_u8_ref(b, minmax6[2 * c], minmax6[2 * c + 1])
    out[:, 3] = np.where(np.isnan(bands[0]) & np.isnan(bands[1]) & np.isnan(bands[2]), 0, 255)
    return out, tie


# ---- perspective warp: homographier/src/homographier/mod.rs:271-300 (cv::warpPerspective, INTER_LINEAR, BORDER_CONSTANT 1) ------------
BORDER = 1


def _dyadic_weights():
    """[32, 32, 4] exact 15-bit weights of the fractions (i / 32 along x, j / 32 along y), taps in the order (0,0) (1,0) (0,1) (1,1) as
    (dx, dy). For a 1/32-step fraction the four products (1 - j/32)(1 - i/32) 2^15 ... are the integers 32 (32 - i)(32 - j) ...: they
    need no rounding and sum to 2^15 by themselves."""
    i = np.arange(32, dtype=np.int64)[None, :]
    j = np.arange(32, dtype=np.int64)[:, None]
    w = np.stack([32 * (32 - i) * (32 - j), 32 * i * (32 - j), 32 * (32 - i) * j, 32 * i * j], -1)
    assert (w.sum(-1) == 1 << 15).all()
    # A fixed-point implementation stores these in int16 and adjusts one tap when a rounded set does not sum to 2^15. Exact sets sum to
    # 2^15, so that step can act at one place only: i = j = 0, whose single weight 2^15 does not fit int16 and becomes 32767 with one
    # unit moved to another tap. Everywhere else every weight fits:
    big = w > 32767
    assert big.sum() == 1 and big[0, 0, 0]
    # ... and at i = j = 0 the moved unit cannot change a byte: (32767 p + q + 2^14) >> 15 == p for all bytes p, q
    p = np.arange(256, dtype=np.int64)[:, None]
    q = np.arange(256, dtype=np.int64)[None, :]
    assert (((32767 * p + q + (1 << 14)) >> 15) == p).all()
    return w


DYADIC_W = _dyadic_weights()


def _padded(src, pad, dtype):
    """src as [H + 2 pad, W + 2 pad, C] of dtype with the border value all round"""
    a = np.asarray(src)
    a = a[:, :, None] if a.ndim == 2 else a
    out = np.full((a.shape[0] + 2 * pad, a.shape[1] + 2 * pad, a.shape[2]), BORDER, dtype)
    out[pad:pad + a.shape[0], pad:pad + a.shape[1]] = a
    return out


def warp_ref_dyadic(src, tx32, ty32, dst_size):
    """The exact result of the map "destination (x, y) reads source (x + tx32 / 32, y + ty32 / 32)", integer tx32, ty32 of either sign,
    dst_size = (width, height). The 1/32 quantisation of the coordinates is exact for such a map. u8 sources: (sum p w + 2^14) >> 15 in
    exact integers; f32 sources: sum p w / 2^15 in long double; taps outside the source are the border value 1."""
    a = np.asarray(src)
    h, w = a.shape[:2]
    dw, dh = dst_size
    X = 32 * np.arange(dw, dtype=np.int64) + int(tx32)
    Y = 32 * np.arange(dh, dtype=np.int64) + int(ty32)
    sx, i = np.floor_divide(X, 32), np.mod(X, 32)          # floor and a fraction in [0, 32) for negative coordinates too
    sy, j = np.floor_divide(Y, 32), np.mod(Y, 32)
    # taps further out than one pixel are border whatever their distance: clamp them onto the padding
    cx = np.clip(sx, -2, w) + 2
    cy = np.clip(sy, -2, h) + 2
    is_u8 = a.dtype == np.uint8
    pad = _padded(a, 2, np.int64 if is_u8 else LD)
    wt = DYADIC_W[j[:, None], i[None, :]]                   # [dh, dw, 4]
    acc = 0
    for k, (dx, dy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        tap = pad[(cy + dy)[:, None], (cx + dx)[None, :]]   # [dh, dw, C]
        acc = acc + tap * (wt[:, :, k, None] if is_u8 else wt[:, :, k, None].astype(LD))
    out = ((acc + (1 << 14)) >> 15) if is_u8 else acc / LD(1 << 15)
    if is_u8:
        assert out.min() >= 0 and out.max() <= 255
        out = out.astype(np.uint8)
    return out[:, :, 0] if a.ndim == 2 else out


def warp_ref_bilinear(src, Minv, dst_size):
    """Continuous bilinear interpolation, in long double, of src (border value 1 outside) at (X0 / W, Y0 / W), where (X0, Y0, W) =
    Minv (x, y, 1) for every destination pixel; Minv maps destination to source and is used as given. dst_size = (width, height).

    Returns (ref [dh, dw, C], Lx, Ly, mag, w): Lx / Ly [dh, dw, C] are the largest absolute differences of horizontally / vertically
    adjacent samples (border included) over the 3 x 3 cells around the sample point: a bound on the interpolant's slope wherever a
    coordinate error of less than a pixel can take the sample point. mag = sum |v_k| w_k at the sample point. ref is NaN where W == 0."""
    a = np.asarray(src)
    h, w = a.shape[:2]
    dw, dh = dst_size
    m = np.asarray(Minv, np.float64).astype(LD).reshape(3, 3)
    x = np.arange(dw).astype(LD)[None, :]
    y = np.arange(dh).astype(LD)[:, None]
    X0 = m[0, 0] * x + m[0, 1] * y + m[0, 2]
    Y0 = m[1, 0] * x + m[1, 1] * y + m[1, 2]
    W = m[2, 0] * x + m[2, 1] * y + m[2, 2] + 0 * x
    with np.errstate(all="ignore"):
        u, v = X0 / W, Y0 / W
    undefined = W == 0
    # a point 3 pixels or more outside has border samples in all of its 3 x 3 cells, however far out it is
    u = np.where(undefined, LD(0), np.clip(u, -4, w + 3))
    v = np.where(undefined, LD(0), np.clip(v, -4, h + 3))
    x0, y0 = np.floor(u), np.floor(v)
    fx, fy = (u - x0)[:, :, None], (v - y0)[:, :, None]
    P = 7
    pad = _padded(a, P, LD)
    ix, iy = x0.astype(np.int64) + P, y0.astype(np.int64) + P

    def S(dx, dy):
        return pad[iy + dy, ix + dx]

    wts = ((1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy)
    taps = (S(0, 0), S(1, 0), S(0, 1), S(1, 1))
    ref = sum(t * k for t, k in zip(taps, wts))
    mag = sum(np.abs(t) * k for t, k in zip(taps, wts))
    Lx = np.zeros_like(ref)
    Ly = np.zeros_like(ref)
    for d in range(-1, 3):          # the 3 x 3 cells span samples -1 .. 2 on either axis
        for e in range(-1, 2):
            Lx = np.maximum(Lx, np.abs(S(e + 1, d) - S(e, d)))
            Ly = np.maximum(Ly, np.abs(S(d, e + 1) - S(d, e)))
    ref = np.where(undefined[:, :, None], LD(np.nan), ref)
    return ref, Lx, Ly, mag, W


# ---- world points: feature_database/src/elevationdb.rs:64-104, 240 -------------------------------------------------------------------
WGS84_A = LD(6378137)
WGS84_F = 1 / LD("298.257223563")
PI = 4 * np.arctan(LD(1))


def round_half_away(v):
    """f64::round: to the nearest integer, halves away from zero"""
    v = np.asarray(v, LD)
    t = np.trunc(v)
    return t + np.sign(v) * (np.abs(v - t) >= LD(0.5))


def world_ref(xy, dgt, egt=None, elev=None):
    """(xyz [n, 3] long double, miss [n] bool, px, py, h): mosaic pixel -> (lon, lat) through the dataset geotransform;
    height = elev[round(py), round(px)] through the inverse of the elevation geotransform (0 without one); geodetic -> geocentric on
    WGS 84. The reference looks the height up by the row id round(py) * ew + round(px), valid iff in [0, ew * eh): there is no check
    per axis, so a column past one edge reads the neighbouring row. A miss is three NaNs."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2).astype(LD)
    d = np.asarray(dgt, np.float64).astype(LD)
    lon = d[0] + xy[:, 0] * d[1] + xy[:, 1] * d[2]
    lat = d[3] + xy[:, 0] * d[4] + xy[:, 1] * d[5]
    n = len(xy)
    h = np.zeros(n, LD)
    miss = np.zeros(n, bool)
    px = py = None
    if egt is not None:
        e = np.asarray(egt, np.float64).astype(LD)
        el = np.asarray(elev, np.float64)
        eh, ew = el.shape
        # (lon, lat) = (e0, e3) + [[e1, e2], [e4, e5]] (px, py), solved by the 2 x 2 closed form
        det = e[1] * e[5] - e[2] * e[4]
        px = (e[5] * (lon - e[0]) - e[2] * (lat - e[3])) / det
        py = (e[1] * (lat - e[3]) - e[4] * (lon - e[0])) / det
        rid = [int(r) * ew + int(c) for r, c in zip(round_half_away(py), round_half_away(px))]     # exact Python integers
        miss = np.array([not 0 <= i < ew * eh for i in rid], bool)
        flat = el.ravel()
        h = np.array([LD(0) if m else LD(flat[i]) for i, m in zip(rid, miss)], LD)
    phi, lam = lat * PI / 180, lon * PI / 180
    e2 = WGS84_F * (2 - WGS84_F)
    N = WGS84_A / np.sqrt(1 - e2 * np.sin(phi) ** 2)
    xyz = np.stack([(N + h) * np.cos(phi) * np.cos(lam), (N + h) * np.cos(phi) * np.sin(lam), (N * (1 - e2) + h) * np.sin(phi)], 1)
    xyz[miss] = np.nan
    return xyz, miss, px, py, h


def world_bound(h):
    """metres: a dozen f64 roundings of a quantity of the size of the geocentric radius, and the angle's own rounding"""
    return 32 * LD(2) ** -52 * (WGS84_A + np.abs(np.asarray(h, LD)))


# ---- the comparison rules, one copy for the oracle (CPU) and the kernels (GPU) --------------------------------------------------------
def band_mismatches(got, want, near_tie, bgra=False):
    """indices [k, 2] of the bytes of got [n, 4] that differ from the reference outside its near-tie band (where the product's f32
    roundings may legitimately fall on the other side); bgra: got has red and blue swapped"""
    if bgra:
        want, near_tie = want[:, [2, 1, 0, 3]], near_tie[:, [2, 1, 0, 3]]
    return np.argwhere((np.asarray(got) != want) & ~near_tie)


def warp_bounded_ratio(got, src, Minv, dst_size):
    """max over the destination of |got - ref| / bound, bound = (Lx + Ly) / 64 [the coordinates are quantised to 1/32 pixel: at most
    1/64 per axis] + 4 * 255 * 2^-15 [four weights rounded to 15 bits] + 0.5 [u8 output rounding] or 4 * 2^-24 * sum |v_k| w_k [f32:
    binary32 products and sums]. Pixels with W == 0 have no reference and are left out."""
    ref, Lx, Ly, mag, _ = warp_ref_bilinear(src, Minv, dst_size)
    g = np.asarray(got)
    is_u8 = g.dtype == np.uint8
    g = (g[:, :, None] if g.ndim == 2 else g).astype(LD)
    bound = (Lx + Ly) / 64 + 4 * 255 * LD(2) ** -15 + (LD(0.5) if is_u8 else 4 * LD(2) ** -24 * mag)
    defined = ~np.isnan(ref)
    assert np.isfinite(g).all()
    return float((np.abs(g - ref)[defined] / bound[defined]).max())


def world_ratio(got, xy, dgt, egt=None, elev=None):
    """(max |got - ref| / world_bound over the points that hit, miss [n]): the misses must be three NaNs and nothing else may be"""
    want, miss, _, _, h = world_ref(xy, dgt, egt, elev)
    got = np.asarray(got, np.float64)
    assert np.array_equal(np.isnan(got).any(1), miss) and np.array_equal(np.isnan(got).all(1), miss) and np.isfinite(got[~miss]).all()
    if miss.all():
        return 0.0, miss
    return float((np.abs(got.astype(LD) - want)[~miss] / world_bound(h)[~miss, None]).max()), miss
