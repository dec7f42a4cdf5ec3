"""CPU, oracle only: do the inputs of akaze_tie_cases.py sit where they claim? Every case ties as much as its table says, every
max_points value named "inside a run" really cuts between two equal responses, the oracle's cut equals the rule "the first max_points
of a stable sort by descending response" restated in numpy, the oracle's result does not depend on its thread count, and the
suppression-depth helpers agree with the oracle's sequential suppression."""
import numpy as np
import pytest

import akaze_tie_cases as tc

FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")

# the colour variants' own figures (keypoints, distinct, longest run, octaves, class_ids), measured on the oracle like the grey table:
# the grey weights change the contrast, so counts move, but every symmetry survives (run lengths 50 / 4 / 12 / 36 / 17)
COLOUR_FIGURES = {"checker32_256": (280, 8, 50, (0, 1), 4), "mirror128": (28, 7, 4, (0, 1), 3), "periodic96x4": (85, 14, 12, (0, 1), 4),
                  "lattice48": (88, 3, 36, (0, 1), 3), "kron_binary8": (1544, 1314, 17, (0, 1), 7)}


@pytest.fixture(scope="module")
def inputs(pkg):
    return dict(tc.all_inputs(pkg.synth))


@pytest.fixture(scope="module")
def uncut(inputs, oracle_mod):
    oracle_mod.set_threads(8)
    return {name: oracle_mod.akaze(img) for name, img in inputs.items()}


def _expected(name):
    if name in tc.CASE:
        c = tc.CASE[name]
        return c.kp, c.distinct, c.longest, c.octaves, c.class_ids
    return COLOUR_FIGURES[name.rsplit("_", 1)[0]]


def test_names_and_shapes(inputs):
    assert list(inputs) == tc.ALL_NAMES
    for name, img in inputs.items():
        assert img.dtype == np.uint8 and max(img.shape[:2]) <= 512, name
        if name.endswith("_bgr") or name.endswith("_bgra"):
            ch = 3 if name.endswith("_bgr") else 4
            g = inputs[name.rsplit("_", 1)[0]]
            assert img.shape == g.shape + (ch,)
            # unequal channels, each a function of the pattern alone: 1, 3/4 and 1/2 of it, rounded
            assert np.array_equal(img[..., 0], g) and np.array_equal(img[..., 2], (g.astype(np.int32) + 1) // 2)
            assert np.abs(img[..., 1].astype(np.float64) - 0.75 * g).max() <= 0.5
            assert ch == 3 or (img[..., 3] == 255).all()


@pytest.mark.parametrize("name", tc.ALL_NAMES)
def test_tie_counts(uncut, name):
    k = uncut[name].keypoints
    kp, distinct, longest = tc.tie_figures(k["response"])
    octaves, class_ids = tuple(sorted(set(k["octave"].tolist()))), len(set(k["class_id"].tolist()))
    print(f"{name}: keypoints {kp} distinct {distinct} longest run {longest} octaves {octaves} class_ids {class_ids}")
    e_kp, e_distinct, e_longest, e_octaves, e_class = _expected(name)
    assert kp > 0
    assert 2 * distinct >= e_distinct and 2 * longest >= e_longest
    assert longest >= 2 and distinct < kp              # a tie case ties
    assert octaves == e_octaves and class_ids == e_class


@pytest.mark.parametrize("name", tc.ALL_NAMES)
def test_cuts_land_in_runs(uncut, name):
    resp = uncut[name].keypoints["response"]
    s = resp[tc.ranked(resp)]
    cuts = tc.tie_cuts(resp)
    print(name, cuts)
    assert sum(inside for _, inside in cuts) >= 2 and any(not inside for _, inside in cuts)
    for mp, inside in cuts:
        assert 1 <= mp <= len(s)
        if inside:
            assert s[mp - 1] == s[mp], (mp, s[mp - 1], s[mp])
        else:
            assert mp == len(s) or s[mp - 1] != s[mp], mp
    # the longest run is among them, cut before, inside and after
    a, b = max(tc.runs(resp), key=lambda r: (r[1] - r[0], -r[0]))
    assert b - a == tc.tie_figures(resp)[2]
    assert {a + 1, (a + b) // 2, b - 1, b} <= {mp for mp, _ in cuts}


@pytest.mark.parametrize("name", tc.ALL_NAMES)
def test_oracle_cut_is_the_first_rows_of_a_stable_descending_sort(inputs, uncut, oracle_mod, name):
    """independent of the oracle's own cut code: numpy's stable argsort of the UNCUT result (the sentence above rank_select_kernel)"""
    full = uncut[name]
    resp = full.keypoints["response"]
    for mp, _ in tc.tie_cuts(resp):
        got = oracle_mod.akaze(inputs[name], max_points=mp)
        rows = tc.cut_rows(resp, mp)
        assert len(got.keypoints) == len(rows) == min(mp, len(resp))
        for f in FIELDS:
            assert np.array_equal(got.keypoints[f], full.keypoints[f][rows]), (mp, f)
        assert np.array_equal(got.descriptors, full.descriptors[rows]), mp


@pytest.mark.parametrize("name", ["checker32_256", "kron_binary8"])
def test_oracle_is_the_same_at_1_and_8_threads(inputs, oracle_mod, name):
    """the sequential suppression (and everything else) must not depend on the oracle's threading: identical bytes"""
    res = []
    for threads in (1, 8):
        oracle_mod.set_threads(threads)
        r = oracle_mod.akaze(inputs[name], keep_planes=True)
        res.append((r.keypoints.tobytes(), r.descriptors.tobytes(), [r.plane(i, oracle_mod.PLANE_MASK1).tobytes() for i in range(len(r.levels))]))
    oracle_mod.set_threads(8)
    assert res[0] == res[1]


def test_a_shifted_checkerboard_still_ties(oracle_mod):
    """the ties come from the content, not from a frame that happens to be symmetric: one pixel of shift leaves long runs"""
    for cell, size in ((16, 256), (32, 256)):
        kp, distinct, longest = tc.tie_figures(oracle_mod.akaze(tc.checkerboard(size, size, cell, shift=1)).keypoints["response"])
        print(f"checkerboard {cell} px shifted by 1: keypoints {kp} distinct {distinct} longest run {longest}")
        assert kp > 0 and longest >= 50 and distinct <= 16


# --- suppression depth ---------------------------------------------------------------------------------------------------------------
def test_suppress_depth_on_hand_made_candidates():
    """the header's rule on planes small enough to do by hand. One level pair, sigma_size 2 on both, same octave: phase 0 D = 4."""
    m = np.zeros((12, 40), bool)
    m[5, [2, 6, 10, 14, 19, 23]] = True            # gaps 4, 4, 4, 5, 4: the chain breaks at the gap of 5
    assert tc.suppress_depth([m, m], [2, 2], [1, 1], phases=(0,)) == {(0, 1): 4}
    m2 = m.copy()
    m2[9, 27] = True                               # 4 rows below and 4 columns right of (5, 23), whose depth is 2: depth 3
    m2[10, 35] = True                              # out of everyone's reach
    assert tc.suppress_depth([m2, m2], [2, 2], [1, 1], phases=(0,)) == {(0, 1): 4}
    m3 = np.zeros((12, 40), bool)
    m3[5, 23] = m3[9, 27] = m3[9, 31] = True
    assert tc.suppress_depth([m3, m3], [2, 2], [1, 1], phases=(0,)) == {(0, 1): 3}
    # phase 1 (against the level above, radius = its sigma_size 2): D = (2 * 2 + 1) * 1 = 5, so the gap of 5 no longer breaks the chain
    assert tc.suppress_depth([m, m], [2, 2], [1, 1], phases=(1,)) == {(1, 0): 6}
    # a later candidate never holds an earlier one back: the same row reversed gives the same depth
    assert tc.suppress_depth([m[:, ::-1], m[:, ::-1]], [2, 2], [1, 1], phases=(0,)) == {(0, 1): 4}


def _depths(oracle_mod, img):
    m0, m1, ld, sigma, ratio = tc.oracle_planes(oracle_mod, img)
    header = tc.suppress_depth(m0, sigma, ratio)
    rounds, final = tc.suppress_rounds(m0, ld, sigma, ratio)
    # the model ends where the oracle's sequential loops end: it stands for the same order
    assert all(np.array_equal(f, m != 0) for f, m in zip(final, m1))
    return header, rounds


def test_suppression_depths_of_the_table(inputs, oracle_mod):
    """How deep are the tie cases? Printed for the next reader; the bounds say only what the helpers must agree on: the kernel's rule
    lets through every candidate the header's rule lets through, so it never needs more rounds."""
    for c in tc.CASES:
        header, rounds = _depths(oracle_mod, inputs[c.name])
        print(f"{c.name}: rounds under the header's rule {max(header.values())} at (phase, level) {max(header, key=header.get)}; "
              f"under the kernel's rule {max(rounds.values())}")
        assert header.keys() == rounds.keys()
        assert all(rounds[k] <= header[k] for k in header)


def test_deepest_suppression_inputs(oracle_mod):
    """What the search for an input that reaches suppress_tail_kernel's stamp retirement (round 253, i.e. 254 rounds in one pass) found.
    Under the header's rule a fine checkerboard on a 128 x 4096 image passes two stamp periods (507) on five passes. Under the rule
    the kernel implements (a candidate waits only for an earlier one whose search window holds its victim) every regular pattern
    tried needs ONE round - checkerboards of 3 .. 16 pixel cells, cosine and square gratings of pitch 2 .. 16 in either direction,
    Gaussian lattices of pitch 6 .. 16: aligned keypoints at a pitch above the search radius (at most 4) never share a victim, and a
    pitch of 4 or less either aliases with the derivative step of one of the two levels or does not survive the smoothing. Irregular
    dense content reaches 2 to 3 rounds per pass. So the `round % 253 == 0` branch stays uncovered: both images are kept as the
    deepest of their kind."""
    imgs = {k: f() for k, f in tc.DEEP_IMAGES.items()}
    assert all(i.shape == (128, 4096) and i.size < 1 << 20 for i in imgs.values())
    header, rounds = _depths(oracle_mod, imgs["checker5"])
    print("checker5 128 x 4096: header's rule", {k: v for k, v in header.items() if v}, "kernel's rule", {k: v for k, v in rounds.items() if v})
    deep = [k for k, v in header.items() if v >= 2 * tc.STAMP_PERIOD + 1]
    assert len(deep) == 5 and max(rounds.values()) == 1
    kp, distinct, longest = tc.tie_figures(oracle_mod.akaze(imgs["checker5"]).keypoints["response"])
    assert kp > 10000 and longest > 5000 and distinct == 2
    header, rounds = _depths(oracle_mod, imgs["blocks"])
    print("blocks 128 x 4096: header's rule", {k: v for k, v in header.items() if v}, "kernel's rule", {k: v for k, v in rounds.items() if v})
    assert max(header.values()) >= 30 and max(rounds.values()) >= 2
    assert sum(v >= 2 for v in rounds.values()) >= 6          # two rounds or more on six passes at least: the tail of the chains is real
