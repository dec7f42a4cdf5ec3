"""GPU: the robust estimators (findHomography least squares / RANSAC / LMEDS / RHO, solvePnPRansac) at the structural borders of their
kernels - refit switch, reduction stride, scoring tails, radix-select sizes, bit-row tails - through the C ABI against the oracle.
Bar: test_homography_gpu.py::_check (found-or-not equal, mask equal, H bit-equal) and test_fuzz_gpu.py::test_pnp_random_sets' (inlier
indices, rvec, tvec equal). Every size is derived from a named constant in estimator_border_cases.py; no number here is a tolerance."""
import numpy as np
import pytest

import estimator_border_cases as bc
from test_homography_gpu import _check

pytestmark = pytest.mark.gpu


# ---- homography ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [bc.HOST_REFIT_MAX - 1, bc.HOST_REFIT_MAX, bc.HOST_REFIT_MAX + 1],
                         ids=["HOST_REFIT_MAX-1", "HOST_REFIT_MAX", "HOST_REFIT_MAX+1"])
def test_refit_switch_by_n(gpu_pkg, oracle_mod, n):
    src, dst, _, _ = gpu_pkg.synth.make_ransac_set(n, seed=0xF170 + n, inlier_frac=1.1, noise=0.3, extent=1024.0)
    found, _, mask = _check(gpu_pkg, oracle_mod, src, dst, 0, 3.0)
    assert found and mask.all()


@pytest.mark.parametrize("method,n,count,extent", bc.EXACT_INLIER_CASES,
                         ids=[f"{'RANSAC' if c[0] == bc.RANSAC else 'LMEDS'}-HOST_REFIT_MAX{'+1' if c[2] > bc.HOST_REFIT_MAX else ''}" for c in bc.EXACT_INLIER_CASES])
def test_refit_switch_by_inlier_count(gpu_pkg, oracle_mod, method, n, count, extent):
    src, dst, flag = bc.exact_inlier_set(gpu_pkg.synth, method, n, count, extent)
    _, _, mo = oracle_mod.find_homography(src, dst, method, 3.0, 2000, 0.995)
    assert int(mo.sum()) == count and np.array_equal(mo.astype(bool), flag)      # the case sits on its border
    found, _, _ = _check(gpu_pkg, oracle_mod, src, dst, method, 3.0)
    assert found


@pytest.mark.parametrize("method", [0, bc.RANSAC], ids=["least_squares", "RANSAC"])
@pytest.mark.parametrize("n", [bc.RED_STRIDE - 1, bc.RED_STRIDE, bc.RED_STRIDE + 1, 2 * bc.RED_STRIDE + 1],
                         ids=["RED_STRIDE-1", "RED_STRIDE", "RED_STRIDE+1", "2*RED_STRIDE+1"])
def test_reduction_stride(gpu_pkg, oracle_mod, n, method):
    src, dst, _, _ = gpu_pkg.synth.make_ransac_set(n, seed=0x57D0 + n, inlier_frac=1.1, noise=0.3, extent=4096.0)
    found, _, mask = _check(gpu_pkg, oracle_mod, src, dst, method, 3.0)
    assert found and int(mask.sum()) > bc.HOST_REFIT_MAX


def test_reduction_mask_confined_to_leading_blocks(gpu_pkg, oracle_mod):
    # see estimator_border_cases.py for why this is n = 1200 with the inliers in blocks 0 and 1, not the 20000 / one block first asked for
    src, dst, flag = bc.mask_block_set(gpu_pkg.synth)
    found, _, mask = _check(gpu_pkg, oracle_mod, src, dst, bc.RANSAC, 3.0)
    assert found and np.array_equal(mask.astype(bool), flag) and int(mask.sum()) == bc.MASK_BLOCK_INLIERS


@pytest.mark.parametrize("max_iters,n", bc.score_tail_cases(), ids=[f"iters{k}-n{n}" for k, n in bc.score_tail_cases()])
def test_scoring_tails(gpu_pkg, oracle_mod, max_iters, n):
    # B % HT, B % COOP_PER_BLOCK and per % SCORE_THREADS of every case: the table in estimator_border_cases.py
    src, dst = bc.score_tail_set(gpu_pkg.synth, max_iters, n)
    _check(gpu_pkg, oracle_mod, src, dst, bc.RANSAC, bc.SCORE_TAIL_THR, max_iters=max_iters, conf=bc.SCORE_TAIL_CONF)


@pytest.mark.parametrize("n", bc.LMEDS_N, ids=[f"n{n}" for n in bc.LMEDS_N])
def test_lmeds_select_sizes(gpu_pkg, oracle_mod, n):
    # KTH_THREADS - 1 .. 2 * KTH_THREADS + 1: the block's strided loads end in a partial pass; n = 5 is kth = 2, n = 6 kth = 3
    src, dst = bc.lmeds_set(gpu_pkg.synth, n)
    found, _, _ = _check(gpu_pkg, oracle_mod, src, dst, bc.LMEDS, 3.0)
    assert found


def test_lmeds_median_zero(gpu_pkg, oracle_mod):
    src, dst = bc.lmeds_zero_median_set()
    found, _, mask = _check(gpu_pkg, oracle_mod, src, dst, bc.LMEDS, 3.0)
    assert found and mask.all()


def test_lmeds_kth_inside_a_run_of_equal_errors(gpu_pkg, oracle_mod):
    src, dst = bc.lmeds_ties_set(gpu_pkg.synth)
    found, _, _ = _check(gpu_pkg, oracle_mod, src, dst, bc.LMEDS, 3.0)
    assert found


def test_lmeds_fewer_than_half_inliers(gpu_pkg, oracle_mod):
    src, dst = bc.lmeds_minority_set(gpu_pkg.synth)       # a meaningless model, but the oracle's meaningless model
    _check(gpu_pkg, oracle_mod, src, dst, bc.LMEDS, 3.0)


@pytest.mark.parametrize("n", bc.RHO_N, ids=[f"n{n}" for n in bc.RHO_N])
def test_rho_bit_row_tails(gpu_pkg, oracle_mod, n):
    # n % RHO_WORD = 63, 0, 1 around one word; RHO_BLOCK - 1, RHO_BLOCK, RHO_BLOCK + 1 and k * RHO_BLOCK + 1: the last block reaches past
    # the last word (the `(i >> 6) < words` guard)
    src, dst = bc.rho_set(gpu_pkg.synth, n)
    found, _, _ = _check(gpu_pkg, oracle_mod, src, dst, bc.RHO, 3.0)
    assert found


def test_rho_points_exactly_on_the_threshold(gpu_pkg, oracle_mod):
    src, dst = bc.rho_on_threshold_set()
    found, _, mask = _check(gpu_pkg, oracle_mod, src, dst, bc.RHO, 3.0)
    assert found and mask[2::3].any()        # pairs whose squared error is maxDsq itself are inliers


def test_rho_grid_stride(gpu_pkg, oracle_mod):
    # RHO_GRID_POINTS + RHO_WORD + 1 points: the grid is capped at RHO_GRID_CAP blocks and every block of the first RHO_WORD + 1 points'
    # column takes a second stride; the one large shape of this file (at most 100 models, most cut short by the SPRT)
    src, dst = bc.rho_set(gpu_pkg.synth, bc.RHO_STRIDE_N)
    found, _, _ = _check(gpu_pkg, oracle_mod, src, dst, bc.RHO, 3.0, max_iters=100)
    assert found


def test_rho_random_sets(gpu_pkg, oracle_mod):
    for case, src, dst, thr, iters, conf in bc.rho_fuzz_cases(gpu_pkg.synth):
        try:
            _check(gpu_pkg, oracle_mod, src, dst, bc.RHO, thr, max_iters=iters, conf=conf)
        except AssertionError as e:
            raise AssertionError(f"case {case} (n {len(src)}, thr {thr}, iters {iters}, conf {conf}): {e}") from e


# ---- PnP -------------------------------------------------------------------------------------------------------------------------------
def _check_pnp(pkg, oracle_mod, obj, img, K, iters, thr, conf, method):
    """(found-or-not or the error code) equal; if found: inlier indices, rvec and tvec equal"""
    hg = pkg.homographier
    corr = [hg.ImgObjCorrespondence(o, i) for o, i in zip(obj, img)]
    rc, r, t, idx = oracle_mod.solve_pnp_ransac(obj, img, K, iters, thr, conf, method=int(method))
    try:
        sol = hg.pnp_solver_ransac(corr, hg.Cmat(np.ascontiguousarray(K, np.float64), np.float64), iters, thr, conf, None, method)
    except hg.MatError as e:
        assert e.kind == "Opencv" and e.inner.code == rc, (e.kind, e.inner.code, rc)
        return rc
    assert rc in (0, 1) and (sol is not None) == (rc == 1), rc
    if sol is not None:
        assert np.array_equal(sol.inliers.mat.ravel(), idx), (len(sol.inliers.mat.ravel()), len(idx))
        assert np.array_equal(sol.rvec.mat.ravel(), r, equal_nan=True) and np.array_equal(sol.tvec.mat.ravel(), t, equal_nan=True)
    return rc


def test_pnp_random_sets_other_methods(gpu_pkg, oracle_mod):
    hg = gpu_pkg.homographier
    for case, name, obj, img, K, iters, thr, conf in bc.pnp_sweep_cases(gpu_pkg.synth):
        try:
            _check_pnp(gpu_pkg, oracle_mod, obj, img, K, iters, thr, conf, getattr(hg.SolvePnPMethod, name))
        except AssertionError as e:
            raise AssertionError(f"case {case} ({name}, n {len(obj)}, iters {iters}, thr {thr}, conf {conf}): {e}") from e


@pytest.mark.parametrize("name", bc.PNP_BORDER_METHODS)
@pytest.mark.parametrize("iters", bc.PNP_BORDER_ITERS, ids=["PNP_THREADS+1", "P3P_THREADS+2", "2*P3P_THREADS+3"])
def test_pnp_batch_and_point_tails(gpu_pkg, oracle_mod, name, iters):
    # iters % PNP_HT = 1, 2, 3 and no multiple of the hypothesis kernels' block; n around SCORE_THREADS and one past 64 parts' single pass
    hg = gpu_pkg.homographier
    for n in bc.PNP_BORDER_N:
        obj, img, K = bc.pnp_border_set(gpu_pkg.synth, n)
        try:
            _check_pnp(gpu_pkg, oracle_mod, obj, img, K, iters, 3.0, 0.99, getattr(hg.SolvePnPMethod, name))
        except AssertionError as e:
            raise AssertionError(f"n {n}: {e}") from e
