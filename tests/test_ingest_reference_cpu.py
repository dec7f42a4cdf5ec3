"""CPU: the independent references of tests/ingest_reference.py against the reference project's known answers, and the oracle
(oracle/ingest_oracle.cpp, which the HIP kernels are held bit-equal to) against those references on the border inputs of
tests/ingest_border_cases.py. The oracle shares its text with the kernels; the references share nothing with either, so a misreading that
both copies carry fails here, without a GPU.

No bound below comes from the oracle's output: the near-tie band (1e-4) is three times the sum of the product's two f32 roundings of
255 f^(1/2.2); the warp bound is the coordinate quantisation times the local slope plus the output and weight roundings; the world-point
bound is 32 * 2^-52 * (6378137 + |h|) m, a dozen f64 roundings of a quantity of that size plus the angle's own rounding.
Largest observed fractions of each bound (the oracle, x86-64): near-tie share 1.3e-4 over the band-merge inputs and 2.0e-4 over a dense
sweep of [0, 1], of the allowed 1e-3, with no byte differing outside the band (on the sweep the oracle differs from the exact value
at 17 points, all inside it); warp, projective maps: u8 0.94, f32 0.97 (the slope
term is nearly attained where the coordinate lands half a 1/32 step off); warp, W < 0 columns: 0.50; world points: 0.034 (edges),
0.033 (globe, with and without elevation), 0.033 (rotated)."""
from fractions import Fraction

import numpy as np
import pytest

import ingest_border_cases as bc
import ingest_reference as ref


@pytest.fixture(scope="module")
def band_refs():
    """{case: (bands, minmax, reference rgba, near_tie)}, computed once"""
    out = {}
    for case in bc.BAND_CASES:
        bands, mm = bc.band_case(*case)
        out[case] = (bands, mm) + ref.band_merge_ref(*bands, mm)
    return out


@pytest.fixture(scope="module")
def sweep_ref():
    """(2 000 001 values of [0, 1], reference u8, near_tie)"""
    sweep = np.linspace(0, 1, 2_000_001, dtype=np.float32)
    return (sweep,) + ref.band_to_u8_ref(sweep, 0.0, 1.0)


# ---- the references themselves -------------------------------------------------------------------------------------------------------
def test_references_reproduce_the_known_answers():
    one = lambda v, mn, mx: int(ref.band_to_u8_ref([v], mn, mx)[0][0])
    assert one(0.2, 0.1, 0.3) == 186                                          # mod.rs:547-555
    assert one(np.nan, 0.1, 0.3) == 0 and ref.band_merge_ref([np.nan], [0.5], [np.nan], (0, 1) * 3)[0].tolist() == [[0, 186, 0, 255]]
    assert one(0.5, 0.0, 1.0) == round(float(np.float32(0.7297401)) * 255)    # gamma_correct_input, mod.rs:517-525
    rgba, _ = ref.band_merge_ref(*[[0.0, 0.5, 1.0]] * 3, (-1.0, 2.0) * 3)     # merging_bands, mod.rs:626-646
    assert rgba[0].tolist() == [155, 155, 155, 255]
    n = 4                                                                     # warp_image_empty, mod.rs:683-707
    img = np.array([[1, (i % n) + 1, (i // n) + 1, 1] for i in range(n * n)], np.uint8).reshape(n, n, 4)
    assert np.array_equal(ref.warp_ref_dyadic(img, 0, 0, (n, n)), img)
    assert np.array_equal(ref.warp_ref_bilinear(img, np.eye(3), (n, n))[0], img.astype(ref.LD))
    f = img.astype(np.float32)
    assert np.array_equal(ref.warp_ref_dyadic(f, 0, 0, (n, n)), f.astype(ref.LD))


def test_the_two_warp_references_agree_on_dyadic_shifts():
    """written apart (integer weights on a 1/32 grid; continuous long double interpolation), they describe one map"""
    for dtype in (np.uint8, np.float32):
        src = bc.warp_source(dtype, 3, 7, 5)
        for tx, ty in ((0, 0), (1, 31), (-33, 33), (-31, -1), (32, -32)):
            exact = ref.warp_ref_dyadic(src, tx, ty, (9, 7))
            cont = ref.warp_ref_bilinear(src, [[1, 0, tx / 32], [0, 1, ty / 32], [0, 0, 1]], (9, 7))[0]
            if dtype == np.uint8:
                assert np.array_equal(exact, np.floor(cont + ref.LD(0.5)).astype(np.uint8)), (tx, ty)   # no tie: 2^14 / 2^15 needs an odd sum
            else:
                assert np.abs(exact - cont).max() < 1e-12, (tx, ty)


def test_round_half_away_from_zero():
    v = np.array([-1.5, -0.5, -0.5 + 2.0 ** -20, -0.0, 0.5 - 2.0 ** -20, 0.5, 1.5, 2.5, 7.5 - 2.0 ** -20])
    assert ref.round_half_away(v).tolist() == [-2, -1, 0, 0, 0, 1, 2, 3, 7]


# ---- the inputs sit where their names say ----------------------------------------------------------------------------------------------
def _exact(x):
    return Fraction(float(x)) == x


def test_bounded_maps_invert_exactly():
    """A forward matrix is handed to the product, which inverts it by cofactors; the reference takes the inverse as given. Both see
    one map only if that inversion is exact in f64: every entry, every product of two entries, every 2 x 2 minor, every entry times a
    minor and the determinant are representable, and the determinant is a power of two (so the division is exact as well)."""
    for minv in bc.WARP_BOUNDED_MINV + [bc.WARP_WZERO_MINV, bc.WARP_SATURATE_MINV]:
        m = bc.forward_of(minv)
        f = [[Fraction(float(v)) for v in row] for row in m]
        back = bc.exact_inverse(m)
        assert all(back[r][c] == Fraction(float(minv[r][c])) for r in range(3) for c in range(3))
        flat = [v for row in f for v in row]
        assert all(_exact(a * b) for a in flat for b in flat)
        minors = [f[r0][c0] * f[r1][c1] - f[r0][c1] * f[r1][c0] for r0 in range(3) for r1 in range(r0 + 1, 3) for c0 in range(3)
                  for c1 in range(c0 + 1, 3)]
        assert all(_exact(v) for v in minors) and all(_exact(a * v) for a in flat for v in minors)
        exact_det = sum(f[0][c] * (f[1][(c + 1) % 3] * f[2][(c + 2) % 3] - f[1][(c + 2) % 3] * f[2][(c + 1) % 3]) for c in range(3))
        assert exact_det != 0 and _exact(exact_det)
        n, d = abs(exact_det.numerator), exact_det.denominator
        assert n & (n - 1) == 0 and d & (d - 1) == 0 and min(n, d) == 1, exact_det
    assert np.array_equal(bc.forward_of(bc.WARP_WZERO_MINV), np.array(bc.WARP_WZERO_M))
    for minv in bc.WARP_BOUNDED_MINV:                         # W > 0 all over the destination
        assert ref.warp_ref_bilinear(bc.warp_bounded_source(np.uint8, 1), minv, bc.WARP_BOUNDED_DST)[4].min() > 0.5


def test_world_inputs_sit_on_their_borders():
    _, miss, px, py, _ = ref.world_ref(bc.WORLD_EDGE_XY, bc.DGT_POW2, bc.EGT_POW2, bc.ELEV)
    want = np.array(bc.WORLD_EDGE_PXPY, np.float64)
    assert np.array_equal(px, want[:, 0].astype(ref.LD)) and np.array_equal(py, want[:, 1].astype(ref.LD))     # exactly, ties included
    assert np.array_equal(bc.WORLD_EDGE_XY.astype(np.float32).astype(np.float64), bc.WORLD_EDGE_XY)            # ... and as f32 columns
    # the row id wraps: a column one past either edge is a hit on the neighbouring row, except before the first and after the last element
    by = {p: bool(m) for p, m in zip(bc.WORLD_EDGE_PXPY, miss)}
    ew, eh = bc.ELEV_W, bc.ELEV_H
    assert by[(-0.5, 0.0)] and by[(-1.0, 0.0)] and not by[(-0.5 + 2.0 ** -20, 0.0)] and not by[(-0.5, 3.0)] and not by[(-1.0, 3.0)]
    assert not by[(float(ew), 0.0)] and not by[(ew - 0.5, 3.0)] and by[(ew - 0.5, eh - 1.0)] and not by[(ew - 0.5 - 2.0 ** -20, eh - 1.0)]
    assert by[(0.0, -0.5)] and not by[(0.0, -0.5 + 2.0 ** -20)] and by[(0.0, eh - 0.5)] and not by[(0.0, eh - 0.5 - 2.0 ** -20)]
    assert by[(ew - 1.0, -0.5)] and by[(3.0, float(eh))] and 0 < miss.sum() < len(miss)
    for n in bc.WORLD_COLUMN_COUNTS:
        assert len(bc.world_edge_points(n)) == n
    assert max(bc.WORLD_COLUMN_COUNTS) > bc.WORLD_BLOCK and {bc.WAVE - 1, bc.WAVE, bc.WAVE + 1} <= set(bc.WORLD_COLUMN_COUNTS)
    # the inexact transforms stay clear of the rounding boundary, so f64 and long double must round alike
    for name in ("globe_elevation", "rotated_elevation"):
        xy, dgt, egt = bc.WORLD_CASES[name]
        _, miss, px, py, _ = ref.world_ref(xy, dgt, egt, bc.ELEV)
        for p in (px, py):
            assert np.abs(np.abs(p - np.floor(p)) - 0.5).min() > 1e-6
        assert (not miss.any()) if name == "globe_elevation" else 0 < miss.sum() < len(miss)


# ---- the oracle against the references -------------------------------------------------------------------------------------------------
def test_near_tie_share_is_small(band_refs, sweep_ref):
    """from the reference alone: bytes the comparison below excuses are at most 1e-3 of all band-merge inputs"""
    ties = np.concatenate([t[:, :3].ravel() for _, _, _, t in band_refs.values()])
    print("near-tie share", ties.mean())
    assert ties.mean() <= 1e-3
    share = sweep_ref[2].mean()                                     # and over a dense sweep of [0, 1]
    print("near-tie share of the sweep", share)
    assert share <= 1e-3


def test_band_sweep_oracle_differs_inside_the_band_only(oracle_mod, sweep_ref):
    sweep, want, tie = sweep_ref
    got = oracle_mod.band_merger(sweep, sweep, sweep, np.array((0.0, 1.0) * 3))[:, 0]
    differs = got != want
    print("sweep: oracle differs from the exact value at", int(differs.sum()), "points, outside the band at", int((differs & ~tie).sum()))
    assert not (differs & ~tie).any() and len(np.unique(got)) == 256


@pytest.mark.parametrize("case", bc.BAND_CASES, ids=lambda c: f"{c[1]}-{c[0]}")
def test_band_merge_oracle_equals_reference(oracle_mod, band_refs, case):
    bands, mm, want, tie = band_refs[case]
    got = oracle_mod.band_merger(*bands, np.array(mm, np.float64))
    bad = ref.band_mismatches(got, want, tie)
    assert len(bad) == 0, (bad[:5], got[bad[:5, 0]], want[bad[:5, 0]])
    all_nan = np.isnan(bands).all(0)
    assert np.array_equal(got[:, 3], np.where(all_nan, 0, 255))
    if case[1] == "degenerate":
        assert not got[:, 0].any()                                  # min == max: every pixel 0, alpha untouched
        assert case[0] == 1 or (got[:, 1].any() and got[:, 2].any())   # min > max is a band like any other (n = 1: the all-NaN pixel)
    if case[0] >= 526:                                              # the boundary values did land on either side of every boundary
        assert len(np.unique(got[:, 2])) == 256


@pytest.mark.parametrize("dtype,channels", bc.WARP_TYPES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_warp_oracle_equals_exact_reference(oracle_mod, dtype, channels):
    for w, h in bc.WARP_SOURCES:
        src = bc.warp_source(dtype, channels, w, h)
        size = (w + 2, h + 2)
        for tx, ty in bc.WARP_SHIFTS + [bc.WARP_SHIFT_OUTSIDE]:
            got = oracle_mod.warp_perspective(src, bc.shift_matrix(tx, ty), size)
            want = ref.warp_ref_dyadic(src, tx, ty, size)
            assert got.dtype == dtype and np.array_equal(got.astype(ref.LD), want.astype(ref.LD)), (w, h, tx, ty)
            if (tx, ty) == bc.WARP_SHIFT_OUTSIDE:
                assert (got == 1).all()
    src = bc.warp_source(dtype, channels, 7, 5)
    for dw in bc.WARP_WIDTHS:
        for dh in bc.WARP_HEIGHTS:
            for tx, ty in bc.WARP_WIDTH_SHIFTS:
                got = oracle_mod.warp_perspective(src, bc.shift_matrix(tx, ty), (dw, dh))
                assert np.array_equal(got.astype(ref.LD), ref.warp_ref_dyadic(src, tx, ty, (dw, dh)).astype(ref.LD)), (dw, dh, tx, ty)


@pytest.mark.parametrize("dtype,channels", bc.WARP_TYPES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_warp_oracle_within_the_bilinear_bound(oracle_mod, dtype, channels):
    src = bc.warp_bounded_source(dtype, channels)
    for minv in bc.WARP_BOUNDED_MINV:
        got = oracle_mod.warp_perspective(src, bc.forward_of(minv), bc.WARP_BOUNDED_DST)
        ratio = ref.warp_bounded_ratio(got, src, minv, bc.WARP_BOUNDED_DST)
        print("warp bounded", dtype.__name__, channels, ratio)
        assert ratio <= 1.0


@pytest.mark.parametrize("dtype,channels", bc.WARP_TYPES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_warp_oracle_w_zero_and_saturation(oracle_mod, dtype, channels):
    src = bc.warp_source(dtype, channels, *bc.WARP_STRUCT_SRC)
    s3 = src.reshape(src.shape[0], src.shape[1], -1)
    got = oracle_mod.warp_perspective(src, np.array(bc.WARP_WZERO_M), bc.WARP_STRUCT_DST)
    g3 = got.reshape(got.shape[0], got.shape[1], -1)
    assert (g3[:, bc.WARP_WZERO_COLUMN] == s3[0, 0]).all()          # W == 0 reads source pixel (0, 0)
    ratio = ref.warp_bounded_ratio(got, src, bc.WARP_WZERO_MINV, bc.WARP_STRUCT_DST)      # W < 0 (columns 0-3) and W > 0 alike
    print("warp W<0", dtype.__name__, channels, ratio)
    assert ratio <= 1.0
    got = oracle_mod.warp_perspective(src, bc.forward_of(bc.WARP_SATURATE_MINV), bc.WARP_STRUCT_DST)
    g3 = got.reshape(got.shape[0], got.shape[1], -1)
    assert (g3[:, 1:] == 1).all() and (g3[:, 0] == s3[0, 0]).all()  # saturated coordinates: border; x == 0 has W == 0


@pytest.mark.parametrize("name", list(bc.WORLD_CASES))
def test_world_points_oracle_within_bound(oracle_mod, name):
    xy, dgt, egt = bc.WORLD_CASES[name]
    rc, got = oracle_mod.world_coordinates(xy, dgt, egt, bc.ELEV if egt is not None else None)
    ratio, miss = ref.world_ratio(got, xy, dgt, egt, bc.ELEV if egt is not None else None)
    print("world", name, ratio, int(miss.sum()))
    assert rc == (-211 if miss.any() else 0)
    assert ratio <= 1.0
