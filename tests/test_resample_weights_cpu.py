"""CPU: apds_resample_weights (host arithmetic, no device) against a float64 numpy restatement of the resampling rule of DESIGN.md
section 2, written here independently of the library:

    ratio = span / n_out, sw = min(1, 1 / ratio), radius = 3 / sw, centre c = (i + 0.5) ratio + offset,
    taps j in [floor(c - radius + 0.5), (int)(c + radius + 0.5)) clamped to the raster [0, n_src),
    w_j = L((j + 0.5 - c) sw) / sum, L(0) = 1, L(x) = sin(pi x) sin(pi x / 3) / (pi^2 x^2 / 3) for 0 < |x| < 3, else 0.

start / count must be equal; every weight within one f32 rounding of the double (|w32 - w64| <= 2^-24 |w64|); a row sums to 1 within
count * 2^-24 (each of the count weights is at most 1 in magnitude, so its rounding moves the sum by at most 2^-24)."""
import ctypes as C
import math

import numpy as np
import pytest

NEAREST, LANCZOS = 0, 1
U = 2.0 ** -24


def lanczos(x):
    if x == 0.0:
        return 1.0
    if not abs(x) < 3.0:
        return 0.0
    a = math.pi * x
    return math.sin(a) * math.sin(a / 3.0) / (a * a / 3.0)


def reference_tables(n_src, offset, span, n_out):
    """-> start[n_out], count[n_out], list of float64 weight arrays"""
    ratio = span / n_out
    sw = min(1.0, 1.0 / ratio)
    radius = 3.0 / sw
    start, count, weights = [], [], []
    for i in range(n_out):
        c = (i + 0.5) * ratio + offset
        a = max(int(math.floor(c - radius + 0.5)), 0)
        b = min(int(c + radius + 0.5), n_src)
        w = np.array([lanczos((j + 0.5 - c) * sw) for j in range(a, b)], np.float64)
        total = 0.0
        for v in w:
            total += v
        start.append(a)
        count.append(b - a)
        weights.append(w / total)
    return np.array(start), np.array(count), weights


def library_tables(pkg, n_src, offset, span, n_out, mode, max_taps):
    start, count = np.full(n_out, -7, np.int32), np.full(n_out, -7, np.int32)
    weights = np.full((n_out, max_taps), np.nan, np.float32)
    rc = pkg.lib().apds_resample_weights(n_src, float(offset), float(span), n_out, mode, max_taps, start.ctypes.data, count.ctypes.data, weights.ctypes.data)
    return rc, start, count, weights


# (n_src, offset, span, n_out): interior, both raster edges, windows smaller than the radius
CASES = [
    (4096, 1024, 512, 512),     # ratio 1
    (4096, 1024, 1024, 512),    # ratio 2, interior
    (4096, 0, 1024, 512),       # ratio 2, left edge
    (4096, 3072, 1024, 512),    # ratio 2, right edge
    (4096, 1024, 2048, 512),    # ratio 4
    (4096, 0, 4096, 512),       # ratio 8, the whole raster
    (4096, 512, 4096 - 512, 448),   # ratio 8 exactly, right edge
    (4096, 300, 1536, 512),     # ratio 3
    (4096, 301, 1280, 512),     # ratio 2.5, odd origin
    (4096, 2048, 256, 512),     # ratio 0.5 (magnification)
    (4096, 0, 256, 512),        # ratio 0.5 at the left edge
    (4096, 4096 - 256, 256, 512),   # ratio 0.5 at the right edge
    (10, 0, 10, 2),             # ratio 5: radius 15 > the raster
    (7, 2, 4, 2),               # ratio 2: radius 6 > the window, footprint cut on both sides
    (5, 0, 5, 5),               # ratio 1 on a raster narrower than the kernel
    (64, 0, 64, 1),             # ratio 64: the limit
]


@pytest.mark.parametrize("n_src,offset,span,n_out", CASES)
def test_lanczos_tables_match_the_float64_restatement(pkg, n_src, offset, span, n_out):
    rs, rc_, rw = reference_tables(n_src, offset, span, n_out)
    max_taps = int(rc_.max()) + 3
    rc, start, count, weights = library_tables(pkg, n_src, offset, span, n_out, LANCZOS, max_taps)
    assert rc == 0, pkg.lib().apds_last_error()
    assert np.array_equal(start, rs) and np.array_equal(count, rc_)
    assert (count >= 1).all() and (start >= 0).all() and (start + count <= n_src).all()
    for i in range(n_out):
        w32 = weights[i, :count[i]].astype(np.float64)
        assert (np.abs(w32 - rw[i]) <= U * np.abs(rw[i])).all(), (i, np.abs(w32 - rw[i]).max())
        assert abs(w32.sum() - 1.0) <= count[i] * U, (i, w32.sum())
        assert (weights[i, count[i]:] == 0).all()            # zero past count


def test_ratio_two_aligned_is_twelve_taps_at_quarter_offsets(pkg):
    rc, start, count, weights = library_tables(pkg, 4096, 1024, 1024, 512, LANCZOS, 12)
    assert rc == 0
    assert (count == 12).all()
    centres = (np.arange(512) + 0.5) * 2 + 1024
    assert np.array_equal(start, (centres - 6).astype(np.int64))
    x = (np.arange(12) - 6 + 0.5) * 0.5                       # (j + 0.5 - c) * sw: -2.75, -2.25, ..., 2.75
    assert np.array_equal(np.abs(x), np.abs([2.75, 2.25, 1.75, 1.25, 0.75, 0.25, 0.25, 0.75, 1.25, 1.75, 2.25, 2.75]))
    w = np.array([lanczos(v) for v in x])
    total = 0.0
    for v in w:                                                # summed in tap order, as the rule's normalisation is
        total += v
    w = w / total
    assert (np.abs(weights.astype(np.float64) - w[None]) <= U * np.abs(w)[None]).all()
    assert np.array_equal(weights[0], weights[511]) and np.array_equal(weights[0], weights[0][::-1])   # every interior output, and symmetric


@pytest.mark.parametrize("n_src,offset,span,n_out", [(4096, 1024, 1024, 512), (4096, 7, 1536, 512), (4096, 100, 1000, 333), (4096, 0, 256, 512), (64, 3, 33, 33)])
def test_nearest_tables_are_the_documented_indices(pkg, n_src, offset, span, n_out):
    rc, start, count, weights = library_tables(pkg, n_src, offset, span, n_out, NEAREST, 2)
    assert rc == 0
    want = offset + np.minimum(((np.arange(n_out) + 0.5) * (span / n_out)).astype(np.int64), span - 1)
    assert np.array_equal(start, want) and (count == 1).all()
    assert (weights[:, 0] == 1).all() and (weights[:, 1] == 0).all()


def test_argument_errors(pkg):
    L = pkg.lib()
    ok = np.zeros(16, np.int32), np.zeros(16, np.int32), np.zeros((16, 400), np.float32)

    def call(n_src, offset, span, n_out, mode, max_taps, start=ok[0], count=ok[1], weights=ok[2]):
        p = lambda a: None if a is None else a.ctypes.data       # noqa: E731
        return L.apds_resample_weights(n_src, float(offset), float(span), n_out, mode, max_taps, p(start), p(count), p(weights))

    assert call(4096, 0, 1024, 16, LANCZOS, 400) == 0
    assert call(4096, 0, 1024, 16, LANCZOS, 400, start=None) == -5
    assert call(4096, 0, 1024, 16, LANCZOS, 400, weights=None) == -5
    assert call(4096, 0, 1024, 16, 2, 400) == -5                 # unknown mode
    assert call(4096, 0, 1024, 16, -1, 400) == -5
    assert call(4096, 0, 1040, 16, LANCZOS, 400) == -5           # ratio 65 > 64
    assert call(4096, 0, 1024, 16, LANCZOS, 384) == 0            # ratio 64: radius 192, 384 taps here (385 is the header's ceiling)
    assert call(4096, 0, 1024, 16, LANCZOS, 383) == -5           # max_taps below the footprint
    assert call(4096, 0, 1024, 16, LANCZOS, 0) == -5
    assert call(4096, -1, 64, 16, LANCZOS, 400) == -211          # window outside the raster
    assert call(4096, 4090, 64, 16, LANCZOS, 400) == -211
    assert call(4096, 0, 0, 16, LANCZOS, 400) == -215            # empty window / output / raster
    assert call(4096, 0, 64, 0, LANCZOS, 400) == -215
    assert call(0, 0, 64, 16, LANCZOS, 400) == -215
    assert b"" != L.apds_last_error()
    assert C.sizeof(C.c_int32) == 4
