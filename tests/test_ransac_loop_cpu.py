"""CPU: the RANSAC controller of the product (csrc/ransac_loop.h: cv::RNG, RANSACUpdateNumIters, the subset draws of findHomography and
solvePnPRansac, the speculative loop both estimators run), compiled by g++ into a host-only test library (tests/cpp/ransac_loop_host.cpp).

Sample streams: the header's draws equal the oracle's, index by index and in number - findHomography's on a generic set, on a set whose
points lie on three lines (checkSubset rejects the draws whose last point makes three on a line, so the stream shifts) and on a
collinear set (the draw fails at iteration 0: no sample on either side); solvePnPRansac's for 5 and for 4 model points.

update_num_iters: equal to the restatement in estimator_border_cases.py on a grid that takes every branch.

The loop: `evaluate` reads scripted scores by global iteration and records every (B, first iteration) it is called with; the outcome
(found, maxGood, the winner's iteration, iterations replayed) equals a plain sequential loop written below, and the recorded batches
equal estimator_border_cases.ransac_batches while the budget is unchanged."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import estimator_border_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = 0.995


@pytest.fixture(scope="module")
def loop(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ransac_loop") / "libransac_loop_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "ransac_loop_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    lib.ransac_rng_stream.argtypes = [C.c_uint64, i, vp]
    lib.ransac_update_num_iters.argtypes = [d, d, i, i]
    lib.ransac_homography_samples.argtypes = [vp, vp, i, i, vp]
    lib.ransac_pnp_samples.argtypes = [i, i, i, vp]
    lib.ransac_scripted_loop.argtypes = [i, i, i, d, i, i, vp, vp, i, i, vp, vp, i]
    return lib


@pytest.fixture(scope="module")
def synth(pkg):
    return pkg.synth


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- sample streams -----------------------------------------------------------------------------------------------------------------------
def three_lines_set(n):
    """n pairs on the lines y = 0, 300, 700 under a similarity (which keeps lines and orientation): a draw whose last point shares its line
    with two of the first three is rejected (haveCollinearPoints looks at the triples of the last point)"""
    rng = np.random.default_rng(0x3117E5)
    src = np.stack([rng.permutation(4 * n)[:n], rng.choice([0, 300, 700], n)], 1).astype(np.float32)
    return src, (src @ np.array([[0.0, 2.0], [-2.0, 0.0]], np.float32) + np.array([40, -8], np.float32)).astype(np.float32)


def collinear_set(n):
    x = np.arange(n, dtype=np.float32)
    src = np.stack([x, 2 * x + 1], 1)
    return src, src + np.array([5, 5], np.float32)


def homography_samples(loop, src, dst, iters):
    idx = np.zeros((iters, 4), np.int32)
    return idx[:loop.ransac_homography_samples(ptr(src), ptr(dst), len(src), iters, ptr(idx))]


@pytest.mark.parametrize("kind", ["generic", "three_lines", "collinear"])
def test_homography_sample_stream_equals_the_oracle(loop, oracle_mod, synth, kind):
    iters = 300
    if kind == "generic":
        src, dst, _, _ = synth.make_ransac_set(200, seed=0x5A3C)
    else:
        src, dst = three_lines_set(60) if kind == "three_lines" else collinear_set(40)
    src, dst = np.ascontiguousarray(src), np.ascontiguousarray(dst)
    got, want = homography_samples(loop, src, dst, iters), oracle_mod.ransac_samples(src, dst, iters)
    assert len(got) == len(want) == (0 if kind == "collinear" else iters)
    assert np.array_equal(got, want)
    if kind == "three_lines":   # the subset check did reject draws: the unchecked draw of the same generator gives another stream
        plain = np.zeros((iters, 4), np.int32)
        loop.ransac_pnp_samples(len(src), iters, 4, ptr(plain))
        assert not np.array_equal(got, plain)
        assert all(int(np.sum(src[s[:3], 1] == src[s[3], 1])) <= 1 for s in got)


@pytest.mark.parametrize("model_points,n", [(5, 5), (5, 6), (5, 37), (5, 1000), (4, 5), (4, 37), (4, 1000)])
def test_pnp_sample_stream_equals_the_oracle(loop, oracle_mod, model_points, n):
    iters = 300
    got = np.zeros((iters, model_points), np.int32)
    loop.ransac_pnp_samples(n, iters, model_points, ptr(got))
    want = oracle_mod.pnp_ransac_samples(n, iters) if model_points == 5 else oracle_mod.pnp_ransac_samples4(n, iters)
    assert np.array_equal(got, want)


def test_rng_maps_a_zero_seed_as_cv_rng_does(loop):
    a, b, c = (np.zeros(8, np.uint32) for _ in range(3))
    loop.ransac_rng_stream(0, 8, ptr(a))
    loop.ransac_rng_stream(0xFFFFFFFF, 8, ptr(b))
    loop.ransac_rng_stream(1, 8, ptr(c))
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    state = 0xFFFFFFFF                      # cv::RNG::next, restated: state = (unsigned)state * 4164903690 + (state >> 32)
    for v in a:
        state = (state & 0xFFFFFFFF) * 4164903690 + (state >> 32)
        assert int(v) == state & 0xFFFFFFFF


# ---- update_num_iters ---------------------------------------------------------------------------------------------------------------------
def test_update_num_iters_equals_the_restatement_on_every_branch(loop):
    tiny = float(np.finfo(np.float64).tiny)
    branches = set()
    for p in (-0.5, 0.0, 0.5, 0.9, 0.99, CONF, 1.0 - 1e-12, 1.0, 1.5):
        for ep in (-1.0, 0.0, 1e-320, 1e-17, 1e-5, 0.1, 0.45, 0.5, 0.7, 0.9, 0.999, 1.0, 2.0):
            for mp in (4, 5):
                for max_iters in (1, 5, 100, 2000, 100000):
                    assert loop.ransac_update_num_iters(p, ep, mp, max_iters) == bc.update_num_iters(p, ep, mp, max_iters), (p, ep, mp, max_iters)
                    denom = 1.0 - (1.0 - min(max(ep, 0.0), 1.0)) ** mp
                    if denom < tiny:
                        branches.add("denom < DBL_MIN")
                    elif np.log(denom) >= 0:
                        branches.add("ep = 1")
                    elif -np.log(max(1.0 - min(max(p, 0.0), 1.0), tiny)) >= max_iters * -np.log(denom):
                        branches.add("budget kept")
                    else:
                        branches.add("budget shortened")
    assert branches == {"denom < DBL_MIN", "ep = 1", "budget kept", "budget shortened"}
    assert loop.ransac_update_num_iters(CONF, 0.0, 4, 2000) == 0 and loop.ransac_update_num_iters(CONF, 1.0, 4, 2000) == 2000
    assert loop.ransac_update_num_iters(1.0, 0.5, 4, 2000) == 2000 and loop.ransac_update_num_iters(CONF, 0.5, 4, 2000) == 82


# ---- the loop -----------------------------------------------------------------------------------------------------------------------------
def sequential(n, model_points, max_iters, good, valid, fail_at=-1):
    """RANSACPointSetRegistrator::run on scripted scores, one iteration at a time: (found, maxGood, winner, iterations run)"""
    niters, max_good, winner, it = max(max_iters, 1), 0, -1, 0
    while it < niters:
        if it == fail_at:               # getSubset failed: no model at iteration 0, the best so far later
            break
        if valid[it] and good[it] > max(max_good, model_points - 1):
            max_good, winner = int(good[it]), it
            niters = bc.update_num_iters(CONF, (n - good[it]) / n, model_points, niters)
        it += 1
    return winner >= 0, max_good, winner, it


def run(loop, n, model_points, max_iters, sizes, good, valid=None, fail_at=-1):
    """the product's loop on the same script: the same tuple, and the (B, first iteration) of every evaluate call"""
    good = np.ascontiguousarray(good, np.int32)
    valid = np.ones(len(good), np.uint8) if valid is None else np.ascontiguousarray(valid, np.uint8)
    out, batches = np.zeros(4, np.int32), np.zeros((32, 2), np.int32)
    calls = loop.ransac_scripted_loop(n, model_points, max_iters, CONF, sizes[0], sizes[1], ptr(good), ptr(valid), len(good), fail_at, ptr(out), ptr(batches), 32)
    assert calls >= 0, "the loop read outside the script, drew out of order or kept a model that is not the winner's"
    got = (bool(out[0]), int(out[1]), int(out[3]), int(out[2]))
    assert got == sequential(n, model_points, max_iters, good, valid, fail_at)
    return got, [(int(b), int(f)) for b, f in batches[:calls]]


def sizes_of(schedule, max_iters):
    return bc.ransac_batch_sizes(max_iters) if schedule == "homography" else (bc.pnp_batch_size(max_iters),) * 2


BUDGETS = [("homography", k) for k in (1, 7, 8, 9, 513, 4097 + 5, 512 + 4096 + 3)] + [("pnp", k) for k in (1, 4, 5, 2049)]


@pytest.mark.parametrize("schedule,max_iters", BUDGETS, ids=[f"{s}-{k}" for s, k in BUDGETS])
def test_budget_borders(loop, schedule, max_iters):
    n, mp, sizes = 1000, 4 if schedule == "homography" else 5, sizes_of(schedule, max_iters)
    # no sample ever wins: the budget stays, and the batches are the restated schedule's
    got, batches = run(loop, n, mp, max_iters, sizes, np.zeros(max_iters, np.int32))
    assert got == (False, 0, -1, max_iters)
    want = bc.ransac_batches(max_iters, None if schedule == "homography" else sizes)
    assert [b for b, _ in batches] == want and [f for _, f in batches] == [sum(want[:q]) for q in range(len(want))]
    if schedule == "pnp":
        assert want == {1: [1], 4: [4], 5: [5], 2049: [2048, 1]}[max_iters]
    # rising scores of up to a fifth of the points: budgets of a few thousand shorten a little, again and again
    rng = np.random.default_rng(max_iters)
    got, batches = run(loop, n, mp, max_iters, sizes, rng.integers(0, n // 5, max_iters), rng.random(max_iters) < 0.9)
    assert [f for _, f in batches] == [sum(b for b, _ in batches[:q]) for q in range(len(batches))]
    assert all(b <= sizes[0 if q == 0 else 1] for q, (b, _) in enumerate(batches)) and got[3] <= max_iters


def test_budget_collapses_inside_the_first_batch(loop):
    n, k = 1000, 2000
    good = np.zeros(k, np.int32)
    good[3], good[10], good[600] = 900, 999, 1000          # 900 of 1000 at confidence 0.995: five iterations in all
    assert bc.update_num_iters(CONF, 0.1, 4, k) == 5
    got, batches = run(loop, n, 4, k, bc.ransac_batch_sizes(k), good)
    assert got == (True, 900, 3, 5) and batches == [(512, 0)]   # samples 10 and 600 were speculated, and never win
    good[4] = 901                                            # the last iteration of the shortened budget still does
    assert run(loop, n, 4, k, bc.ransac_batch_sizes(k), good)[0][:3] == (True, 901, 4)


def test_budget_collapses_to_a_value_inside_the_second_batch(loop):
    n, k = 1000, 2000
    good = np.zeros(k, np.int32)
    good[100] = 295
    niters = bc.update_num_iters(CONF, (n - 295) / n, 4, k)
    assert 512 < niters < k
    good[niters - 1], good[niters] = 296, 999               # the last iteration inside the budget wins, the first outside is never drawn
    got, batches = run(loop, n, 4, k, bc.ransac_batch_sizes(k), good)
    assert got[:3] == (True, 296, niters - 1) and batches == [(512, 0), (niters - 512, 512)]


@pytest.mark.parametrize("model_points", [4, 5])
def test_a_count_of_model_points_minus_one_never_wins(loop, model_points):
    k = 100
    sizes = sizes_of("homography" if model_points == 4 else "pnp", k)
    assert run(loop, 1000, model_points, k, sizes, np.full(k, model_points - 1))[0] == (False, 0, -1, k)
    good = np.full(k, model_points - 1)
    good[57] = model_points
    assert run(loop, 1000, model_points, k, sizes, good)[0][:3] == (True, model_points, 57)


def test_a_tie_keeps_the_earlier_model(loop):
    good = np.zeros(50, np.int32)
    good[2], good[5], good[9] = 20, 20, 19
    assert run(loop, 1000, 4, 50, bc.ransac_batch_sizes(50), good)[0] == (True, 20, 2, 50)


def test_every_sample_invalid_gives_no_model(loop):
    k = 600
    got, batches = run(loop, 1000, 4, k, bc.ransac_batch_sizes(k), np.full(k, 900), np.zeros(k, np.uint8))
    assert got == (False, 0, -1, k) and batches == [(512, 0), (88, 512)]


def test_draw_failure(loop):
    k = 2000
    good = np.zeros(k, np.int32)
    good[2], good[4], good[5], good[550] = 10, 12, 900, 14
    sizes = bc.ransac_batch_sizes(k)
    assert run(loop, 1000, 4, k, sizes, good, fail_at=0) == ((False, 0, -1, 0), [])            # iteration 0: no model, nothing evaluated
    assert run(loop, 1000, 4, k, sizes, good, fail_at=5) == ((True, 12, 4, 5), [(5, 0)])       # later: the drawn samples are scored, the best stays
    good[5] = 0
    assert run(loop, 1000, 4, k, sizes, good, fail_at=512) == ((True, 12, 4, 512), [(512, 0)])   # the first draw of the second batch
    assert run(loop, 1000, 4, k, sizes, good, fail_at=600) == ((True, 14, 550, 600), [(512, 0), (88, 512)])
