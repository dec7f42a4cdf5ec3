"""CPU: apds_overview_weights (host arithmetic, no device) - the table of one axis of one step of the overview cascade, n_src -> n_out -
against a float64 numpy restatement of the rule of DESIGN.md section 2, written here independently of the library:

    ratio = n_src / n_out, sw = min(1, 1 / ratio), radius = 2 / sw, centre c = (i + 0.5) ratio,
    taps j in [floor(c - radius + 0.5), (int)(c + radius + 0.5)) clamped to the raster [0, n_src),
    w_j = W((j + 0.5 - c) sw) / sum, W = Keys' cubic with a = -0.5:
    W(x) = 1.5|x|^3 - 2.5|x|^2 + 1 for |x| <= 1, -0.5|x|^3 + 2.5|x|^2 - 4|x| + 2 for 1 < |x| < 2, else 0.

start / count must be equal; every weight within one f32 rounding of the double (|w32 - w64| <= 2^-24 |w64|); a row sums to 1 within
count * 2^-24 (each of the count weights is at most 1 in magnitude, so its rounding moves the sum by at most 2^-24). The function returns
the widest footprint."""
import math

import numpy as np
import pytest

U = 2.0 ** -24


def cubic(x):
    a = abs(x)
    if a <= 1.0:
        return 1.5 * a * a * a - 2.5 * a * a + 1.0
    if a < 2.0:
        return -0.5 * a * a * a + 2.5 * a * a - 4.0 * a + 2.0
    return 0.0


def reference_tables(n_src, n_out):
    """-> start[n_out], count[n_out], list of float64 weight arrays"""
    ratio = n_src / n_out
    sw = min(1.0, 1.0 / ratio)
    radius = 2.0 / sw
    start, count, weights = [], [], []
    for i in range(n_out):
        c = (i + 0.5) * ratio
        a = max(int(math.floor(c - radius + 0.5)), 0)
        b = min(int(c + radius + 0.5), n_src)
        w = np.array([cubic((j + 0.5 - c) * sw) for j in range(a, b)], np.float64)
        total = 0.0
        for v in w:
            total += v
        start.append(a)
        count.append(b - a)
        weights.append(w / total)
    return np.array(start), np.array(count), weights


def library_tables(pkg, n_src, n_out, max_taps):
    start, count = np.full(n_out, -7, np.int32), np.full(n_out, -7, np.int32)
    weights = np.full((n_out, max_taps), np.nan, np.float32)
    rc = pkg.lib().apds_overview_weights(n_src, n_out, max_taps, start.ctypes.data, count.ctypes.data, weights.ctypes.data)
    return rc, start, count, weights


def test_ratio_two_is_eight_dyadic_taps(pkg):
    # W(+-0.25), W(+-0.75), W(+-1.25), W(+-1.75) = 222, 58, -18, -6 over 256: their sum is 2, every weight is exact in f32
    assert [cubic(x) * 256 for x in (0.25, 0.75, 1.25, 1.75)] == [222.0, 58.0, -18.0, -6.0]
    rc, start, count, weights = library_tables(pkg, 64, 32, 8)
    assert rc == 8, pkg.lib().apds_last_error()
    want = np.array([-3, -9, 29, 111, 111, 29, -9, -3], np.float32) / np.float32(256)
    for i in range(4, 28):
        assert start[i] == 2 * i - 3 and count[i] == 8
        assert np.array_equal(weights[i], want), i


@pytest.mark.parametrize("n_src", [1, 2, 3, 5, 64, 65, 127, 1025])
def test_tables_match_the_float64_restatement(pkg, n_src):
    n_out = (n_src + 1) // 2
    rs, rc_, rw = reference_tables(n_src, n_out)
    need = int(rc_.max())
    assert need <= 9
    assert pkg.lib().apds_overview_weights(n_src, n_out, 0, None, None, None) == need     # only the footprint
    max_taps = need + 2
    rc, start, count, weights = library_tables(pkg, n_src, n_out, max_taps)
    assert rc == need, pkg.lib().apds_last_error()
    assert np.array_equal(start, rs) and np.array_equal(count, rc_)
    assert (count >= 1).all() and (count <= 9).all() and (start >= 0).all() and (start + count <= n_src).all()
    assert start[0] == 0 and start[-1] + count[-1] == n_src                                # the edge rows are clamped at 0 and at n_src
    ratio = n_src / n_out
    assert math.floor(0.5 * ratio - 2 * ratio + 0.5) < 0 and int((n_out - 0.5) * ratio + 2 * ratio + 0.5) > n_src     # ... and were cut there
    for i in range(n_out):
        w32 = weights[i, :count[i]].astype(np.float64)
        assert (np.abs(w32 - rw[i]) <= U * np.abs(rw[i])).all(), (i, np.abs(w32 - rw[i]).max())
        assert abs(w32.sum() - 1.0) <= count[i] * U, (i, w32.sum())
        assert (weights[i, count[i]:] == 0).all()            # zero past count


def test_argument_errors(pkg):
    L = pkg.lib()
    ok = np.zeros(32, np.int32), np.zeros(32, np.int32), np.zeros((32, 12), np.float32)

    def call(n_src, n_out, max_taps, start=ok[0], count=ok[1], weights=ok[2]):
        p = lambda a: None if a is None else a.ctypes.data       # noqa: E731
        return L.apds_overview_weights(n_src, n_out, max_taps, p(start), p(count), p(weights))

    assert call(64, 32, 12) == 8
    assert call(64, 32, 8) == 8
    assert call(64, 32, 7) == -5                                 # max_taps below the footprint
    assert call(64, 32, 0) == -5
    assert call(65, 33, 7) == -5 and call(65, 33, 8) == 8        # an odd size: ratio 65 / 33
    assert call(64, 32, 12, start=None) == -5                    # null outputs
    assert call(64, 32, 12, count=None) == -5
    assert call(64, 32, 12, weights=None) == -5
    assert call(64, 32, 0, start=None, count=None) == -5         # the footprint query wants all three null
    assert call(32, 33, 12) == -5                                # n_out larger than n_src
    assert call(0, 1, 12) == -215 and call(64, 0, 12) == -215    # empty
    assert b"" != L.apds_last_error()
