"""CPU: the inputs of test_estimator_borders_gpu.py against the oracle alone - does every case sit on the border it names? Runs on any
machine; the GPU file then only has to compare. The only numbers here are border values derived from the constants restated in
estimator_border_cases.py and the one-in-four cap on "nothing found"."""
import numpy as np
import pytest

import estimator_border_cases as bc


@pytest.fixture(scope="module")
def synth(pkg):
    return pkg.synth


def test_restated_batches_and_parts():
    # the table in estimator_border_cases.py: every tail the scoring cases are there for is present
    batches = {k: bc.ransac_batches(k) for k in bc.SCORE_TAIL_ITERS}
    assert batches == {1: [1], 7: [7], 8: [8], 9: [9], 17: [17], 513: [512, 1], 4102: [512, 3590], 4611: [512, 4096, 3]}
    all_b = [b for v in batches.values() for b in v]
    assert {b % bc.HT for b in all_b} >= {0, 1, 3, 6, 7} and {b % bc.COOP_PER_BLOCK for b in all_b} >= {0, 1, 3, 6, 7, 8, 9}
    assert len(batches[8]) == 1 and -(-batches[8][0] // bc.HT) == 1                      # a one-block grid
    assert [bc.score_parts(b) for b in (1, 256, 512, 3590, 4096)] == [64, 64, 32, 5, 4]
    for n in bc.SCORE_TAIL_N:
        for b in all_b:
            assert -(-n // bc.score_parts(b)) % bc.SCORE_THREADS != 0
    assert -(-bc.SCORE_TAIL_N[-1] // bc.score_parts(4096)) > 2 * bc.SCORE_THREADS       # three passes, the last for one point
    for k in bc.PNP_BORDER_ITERS:
        assert k <= bc.PNP_BATCH and k % bc.PNP_THREADS and k % bc.P3P_THREADS
    assert [k % bc.PNP_HT for k in bc.PNP_BORDER_ITERS] == [1, 2, 3]
    assert -(-bc.PNP_BORDER_N[-1] // bc.score_parts(bc.PNP_BORDER_ITERS[0], bc.PNP_HT)) == bc.SCORE_THREADS + 1
    assert bc.RHO_STRIDE_N > bc.RHO_GRID_POINTS and bc.RHO_STRIDE_N % bc.RHO_WORD == 1 and {n % bc.RHO_WORD for n in bc.RHO_N} >= {0, 1, 63}


@pytest.mark.parametrize("method,n,count,extent", bc.EXACT_INLIER_CASES)
def test_exact_inlier_sets_give_exactly_that_mask(oracle_mod, synth, method, n, count, extent):
    src, dst, flag = bc.exact_inlier_set(synth, method, n, count, extent)
    found, _, mo = oracle_mod.find_homography(src, dst, method, 3.0, 2000, 0.995)
    assert found and int(flag.sum()) == count and int(mo.sum()) == count and np.array_equal(mo.astype(bool), flag)


def test_mask_block_set_selects_the_leading_indices(oracle_mod, synth):
    src, dst, flag = bc.mask_block_set(synth)
    found, _, mo = oracle_mod.find_homography(src, dst, bc.RANSAC, 3.0, 2000, 0.995)
    assert found and int(mo.sum()) == bc.MASK_BLOCK_INLIERS > bc.HOST_REFIT_MAX
    assert mo[:bc.MASK_BLOCK_INLIERS].all() and not mo[bc.MASK_BLOCK_INLIERS:].any()
    assert bc.MASK_BLOCK_INLIERS < 2 * bc.RED_THREADS < 4 * bc.RED_THREADS < bc.MASK_BLOCK_N < bc.RED_STRIDE


def test_scoring_tail_sets_keep_their_budget(oracle_mod, synth):
    """RANSACUpdateNumIters, re-derived in numpy, leaves max_iters alone for the oracle's final (largest) consensus set, hence for every
    smaller one before it: the batches are ransac_batches(max_iters)."""
    for max_iters, n in bc.score_tail_cases():
        src, dst = bc.score_tail_set(synth, max_iters, n)
        found, _, mo = oracle_mod.find_homography(src, dst, bc.RANSAC, bc.SCORE_TAIL_THR, max_iters, bc.SCORE_TAIL_CONF)
        good = int(mo.sum())
        assert found and good >= 4, (max_iters, n)
        assert bc.update_num_iters(bc.SCORE_TAIL_CONF, (n - good) / n, 4, max_iters) == max_iters, (max_iters, n, good)


def test_scoring_tail_sets_end_on_their_last_hypothesis(oracle_mod, synth):
    # one hypothesis fewer gives another consensus set: the budget's last hypothesis (index B - 1 of a one-batch run) is the winner
    for max_iters in bc.LAST_WINS_ITERS:
        for n in bc.SCORE_TAIL_N:
            src, dst = bc.score_tail_set(synth, max_iters, n)
            _, _, mo = oracle_mod.find_homography(src, dst, bc.RANSAC, bc.SCORE_TAIL_THR, max_iters, bc.SCORE_TAIL_CONF)
            _, _, mb = oracle_mod.find_homography(src, dst, bc.RANSAC, bc.SCORE_TAIL_THR, max_iters - 1, bc.SCORE_TAIL_CONF)
            assert not np.array_equal(mo, mb) and mo.sum() > mb.sum(), (max_iters, n)


def test_lmeds_zero_median_set_has_a_model_of_zero_error(oracle_mod):
    src, dst = bc.lmeds_zero_median_set()
    niters = max(bc.update_num_iters(0.995, 0.45, 4, 2000), 3)
    zero = 0
    for idx in oracle_mod.ransac_samples(src, dst, niters):
        rc, H = oracle_mod.homography_4pt(src[idx], dst[idx])
        if rc <= 0:
            continue
        h = H.ravel().astype(np.float32)
        ww = np.float32(1) / (h[6] * src[:, 0] + h[7] * src[:, 1] + np.float32(1))
        dx = (h[0] * src[:, 0] + h[1] * src[:, 1] + h[2]) * ww - dst[:, 0]
        dy = (h[3] * src[:, 0] + h[4] * src[:, 1] + h[5]) * ww - dst[:, 1]
        err = dx * dx + dy * dy
        assert err.dtype == np.float32
        zero += int(np.sort(err)[len(err) // 2] == 0.0)
    assert zero > 0
    found, _, mo = oracle_mod.find_homography(src, dst, bc.LMEDS, 3.0, 2000, 0.995)
    assert found and mo.all()


def test_lmeds_ties_and_minority_sets(synth):
    src, dst = bc.lmeds_ties_set(synth)
    _, counts = np.unique(np.concatenate([src, dst], 1), axis=0, return_counts=True)
    assert len(src) == 1500 and sorted(set(counts)) == [7, 8]
    assert bc.lmeds_minority_set(synth)[0].shape == (1000, 2)
    flag = synth.make_ransac_set(1000, seed=0x3077, inlier_frac=0.3, noise=0.3, extent=1024.0)[3]
    assert 2 * int(flag.sum()) < len(flag)


def test_rho_on_threshold_set_has_inliers_at_exactly_the_threshold(oracle_mod):
    src, dst = bc.rho_on_threshold_set()
    found, H, mo = oracle_mod.find_homography(src, dst, bc.RHO, 3.0, 2000, 0.995)
    assert found and mo[2::3].any() and mo[0::3].all() and mo[1::3].all()


def test_rho_fuzz_mostly_finds_a_model(oracle_mod, synth):
    """Observed on the oracle: 5 of the 120 cases end with found = False (cap: 30)."""
    not_found = sum(1 for _, src, dst, thr, iters, conf in bc.rho_fuzz_cases(synth) if not oracle_mod.find_homography(src, dst, bc.RHO, thr, iters, conf)[0])
    assert 4 * not_found <= bc.RHO_FUZZ_CASES, not_found


def test_pnp_sweep_mostly_finds_a_pose(oracle_mod, pkg, synth):
    """Observed on the oracle: 45 of the 60 cases end with a pose; 11 end with none and 4 with SOLVEPNP_IPPE_SQUARE's npoints == 4
    assertion (-215), both counted as found = False: 15 (cap: 15)."""
    hg = pkg.homographier
    rcs = [oracle_mod.solve_pnp_ransac(obj, img, K, iters, thr, conf, method=int(getattr(hg.SolvePnPMethod, name)))[0]
           for _, name, obj, img, K, iters, thr, conf in bc.pnp_sweep_cases(synth)]
    assert len(rcs) == bc.PNP_SWEEP_CASES and 4 * sum(rc != 1 for rc in rcs) <= bc.PNP_SWEEP_CASES, rcs
    names = {name for _, name, *_ in bc.pnp_sweep_cases(synth)}
    assert names == set(bc.PNP_SWEEP_METHODS)
