"""CPU: the inputs, the bound and the acceptance check of test_l2_borders_gpu.py (l2_border_cases.py). Every case is shown to sit on the
border it names, computed from the restated launch geometry; the cap (planted queries decided at both ranks, filler pairs to 99 %) is
checked with the float64 reference alone; `accept` passes the oracle's independent f32 matcher on every case, keeps a numpy binary32
emulation of the kernel's formula within the bound, and rejects six named mistakes applied to that emulation's keys."""
import numpy as np
import pytest

import l2_border_cases as bc


def _reference_keys(case, k=2, index_base=0):
    """keys of the float64 reference itself (distance rounded to float32: well inside B)"""
    return bc.topk_keys(bc.d2_64(case["q"], case["t"]).astype(np.float32), k, index_base)


def _small_cases():
    yield "wave", bc.wave_case()
    yield "base", bc.base_case()
    yield "scale", bc.scale_case()
    for nt in bc.TILE_NT:
        yield f"tile-nt{nt}", bc.tile_case(129, nt)
    for nq in bc.TILE_NQ:
        yield f"tile-nq{nq}", bc.tile_case(nq, 128 * 3 + 1)
    for dim in bc.DIMS:
        yield f"dim{dim}", bc.dim_case(dim)


@pytest.fixture(scope="module")
def small_cases():
    return dict(_small_cases())


def test_restated_geometry():
    assert bc.L2_TM == bc.L2_TN == 128 and bc.SC_Q == 384 and bc.SC_TM == 128 and bc.SC_REGION == 73728
    assert bc.split_plan(128 * 17 - 1, 8200) == (17, 6, 3) and bc.split_plan(128 * 17, 8200) == (17, 6, 3) and bc.split_plan(128 * 17 + 1, 8200) == (18, 6, 3)
    assert bc.split_plan(385, 129) == (4, 4, 1) and bc.split_plan(257, 130) == (3, 3, 1) and bc.split_plan(385, 1) == (4, 4, 1)
    assert bc.split_plan(70_000, 384, bc.SC_TM, bc.SC_Q) == (547, 274, 2) and 2 * bc.SC_TM * 384 == 98304 > bc.SC_REGION
    assert [bc.screen_sample_rows(n) for n in bc.SCREEN_NT] == [2, 129, 8191, 8192, 8192, 11776]
    assert bc.screen_sample_rows(140_000, 16) == 8832          # a divisor of 16, as earlier documents state it


def test_tile_cases_sit_on_the_tile_borders(small_cases):
    for nt in bc.TILE_NT:
        case = small_cases[f"tile-nt{nt}"]
        tiles = bc.ceil_div(nt, bc.L2_TM)
        near = {p[1] for p in case["planted"]}
        for T in range(tiles):
            first, last = T * bc.L2_TM, min((T + 1) * bc.L2_TM, nt) - 1
            assert first in near and last in near, (nt, T)                       # both ends of every tile are somebody's nearest row ...
            if first != last:
                assert (first, last) in {(p[1], p[2]) for p in case["planted"]} and (last, first) in {(p[1], p[2]) for p in case["planted"]}
        assert len(case["planted"]) == sum(1 if a == b else 2 for a, b in bc.tile_pairs(nt))
        if nt % bc.L2_TM:
            assert nt - 1 in near and (nt - 1) % bc.L2_TM == nt % bc.L2_TM - 1  # ... the last row of a partial tile among them
    for nq in bc.TILE_NQ:
        case = small_cases[f"tile-nq{nq}"]
        assert len(case["planted"]) == min(nq, 7) and {0, nq - 1} <= set(case["planted_q"].tolist())
    for a, f, l in small_cases["wave"]["planted"]:
        assert abs(f - l) == 15 and min(f, l) % 16 == 0 and (min(f, l) % 128) // 16 in (0, 3, 7) and f // 128 == l // 128
    assert len(small_cases["wave"]["planted"]) == 12
    base = small_cases["base"]
    assert (base["planted"][0][1], base["planted"][0][2]) == (384, 127) and base["ties"][0][1:] == (130, 300)
    assert np.array_equal(base["t"][130], base["t"][300])


def test_split_cases_sit_on_the_split_borders():
    for nt in bc.SPLIT_NT:
        t_tiles, splits, tps = bc.split_plan(nt, bc.SPLIT_NQ)
        assert (splits, tps) == (6, 3) and bc.ceil_div(bc.SPLIT_NQ, bc.L2_TN) == 65
        last_rows = nt - (splits - 1) * tps * bc.L2_TM
        assert last_rows < tps * bc.L2_TM                                        # the last split is shorter
        case = bc.split_case(nt)
        a, near, second = case["planted"][0]
        assert near == (splits - 1) * tps * bc.L2_TM == 1920 and second == tps * bc.L2_TM - 1 == 383
        assert case["planted"][4][1] == nt - 1 and case["planted"][4][2] == 0
        q, lo, hi = case["ties"][0]
        assert lo // (tps * bc.L2_TM) == 1 and hi // (tps * bc.L2_TM) == 4 and np.array_equal(case["t"][lo], case["t"][hi])
        sel = bc.split_case_checked_queries(case)
        assert set(case["planted_q"].tolist()) <= set(sel.tolist()) and q in sel
        if nt == bc.SPLIT_NT[1]:
            sub = {**case, "q": case["q"]}
            keys = bc.topk_keys(bc.d2_64(case["q"][sel], case["t"]).astype(np.float32), 2)
            bc.accept_case(keys, sub, sel=sel)


def test_the_cap_holds_by_the_reference_alone(small_cases):
    for name, case in small_cases.items():
        for k in (1, 2):
            share = bc.accept_case(_reference_keys(case, k), case, k=k)
            assert share >= 0.99 or len(case["t"]) < 3 or name == "scale", (name, share)      # (scale: exact ties at the zero rows)
    case = small_cases["scale"]
    sp = case["special"]
    assert not case["q"][sp["zero_query"]].any() and not case["t"][list(sp["zero_rows"])].any()
    assert np.array_equal(case["q"][sp["equal"][0]], case["t"][sp["equal"][1]])
    n = np.linalg.norm(np.concatenate([case["q"], case["t"]]).astype(np.float64), axis=1)
    assert n[n > 0].min() < 0.02 and n.max() > 15


def test_accept_passes_the_oracle(oracle_mod, small_cases):
    oracle_mod.set_threads(8)
    for name, case in small_cases.items():
        for k in (1, 2):
            kk = min(k, len(case["t"]))
            idx, dist = oracle_mod.knn_l2(case["q"], case["t"], kk)
            # the oracle reports sqrt(f32 sum): square it in float64 and round once; its own error is (dim + 2) u d^2, far inside B
            f = (dist.astype(np.float64) ** 2).astype(np.float32)
            keys = np.full((len(case["q"]), k), bc.EMPTY_KEY, np.uint64)
            keys[:, :kk] = bc.make_keys(f, idx)
            bc.accept_case(keys, case, k=k)


@pytest.mark.parametrize("dim", bc.DIMS)
def test_emulation_stays_within_the_bound(dim):
    """The numpy binary32 emulation of the kernel's formula against d2_64 on 600 pairs per dim: raw rows with norms from 0.01 to 30 (equal
    and very different norms in a pair), near-duplicates at 1e-6 and 1e-3, exact duplicates and zero vectors.
    Largest error / B measured: 0.137 (dim 1, 3, 4: 0.116, 0.131, 0.137; dim 63, 64, 65: 0.070, 0.096, 0.081; dim 100, 127, 128: 0.070,
    0.061, 0.052). B is a worst-case bound and random roundings cancel, so the figures are far below the 1 that is asserted."""
    rng = np.random.default_rng(0x4C32BE00 + dim)
    n = 100
    unit = lambda: bc._unit(rng, n, dim) if dim > 1 else rng.choice([-1.0, 1.0], size=(n, 1))
    scale = lambda: np.exp(rng.uniform(np.log(0.01), np.log(30.0), size=(n, 1)))
    s = scale()
    a = unit() * s
    sets = [(a, unit() * s), (a, unit() * scale()), (a, a + 1e-6 * s * rng.normal(size=(n, dim))), (a, a + 1e-3 * s * rng.normal(size=(n, dim))), (a, a),
            (np.where(np.arange(n)[:, None] % 2, a, 0.0), np.where(np.arange(n)[:, None] % 3, unit() * s, 0.0))]
    q = np.concatenate([p[0] for p in sets]).astype(np.float32)
    t = np.concatenate([p[1] for p in sets]).astype(np.float32)
    F = bc.emulate_pairs(q, t).astype(np.float64)
    D = np.einsum("ij,ij->i", q.astype(np.float64) - t, q.astype(np.float64) - t)
    B = (dim + 16) * 2.0 ** -24 * ((q.astype(np.float64) ** 2).sum(1) + (t.astype(np.float64) ** 2).sum(1))
    ok = B > 0
    assert (F[~ok] == 0).all()                                  # zero against zero: exactly 0
    ratio = (np.abs(F - D)[ok] / B[ok]).max()
    print(f"dim {dim}: largest error / B = {ratio:.3f}")
    assert ratio < 1.0
    assert (F[4 * n:5 * n] <= B[4 * n:5 * n]).all()             # a row against itself


def test_emulated_kernel_passes_and_six_mistakes_do_not(small_cases):
    base, part = small_cases["base"], small_cases["tile-nt129"]
    for case in (base, part, small_cases["scale"], small_cases["dim65"]):
        F = bc.emulate_matrix(case["q"], case["t"])
        for ib in bc.INDEX_BASES:
            bc.accept_case(bc.topk_keys(F, 2, ib), case, index_base=ib)
    Fb, Fp = bc.emulate_matrix(base["q"], base["t"]), bc.emulate_matrix(part["q"], part["t"])

    def rejected(keys, case, ib=0):
        with pytest.raises(AssertionError):
            bc.accept_case(keys, case, index_base=ib)

    # 1: the last row of a partial tile dropped (row 128 of 129; row 384 of 385)
    for F, case in ((Fp, part), (Fb, base)):
        G = F.copy()
        G[:, -1] = np.inf
        rejected(bc.topk_keys(G, 2), case)
    # 2: a tile's first row dropped
    G = Fb.copy()
    G[:, 128] = np.inf
    rejected(bc.topk_keys(G, 2), base)
    # 3: ties resolved to the higher row
    rejected(bc.topk_keys(Fb, 2, higher_row_first=True), base)
    # 4: index_base added twice
    for ib in (1, 3_000_000_000):
        rejected(bc.topk_keys(Fb, 2, 2 * ib), base, ib)
    # 5: the second key taken from the split of the first (one tile per split here) instead of from all splits
    keys = bc.topk_keys(Fb, 2)
    for i in range(len(keys)):
        T = int(keys[i, 0] & bc.U32) // bc.L2_TM
        lo, hi = T * bc.L2_TM, min((T + 1) * bc.L2_TM, Fb.shape[1])
        keys[i] = bc.topk_keys(Fb[i:i + 1, lo:hi], 2, lo)[0]
    rejected(keys, base)
    # 6: distances off by 4B
    B = bc.bound(base["q"], base["t"])
    rejected(bc.topk_keys((Fb.astype(np.float64) + 4 * B).astype(np.float32), 2), base)
    rejected(bc.topk_keys(np.maximum(Fb.astype(np.float64) - 4 * B, 0).astype(np.float32), 2), base)


def test_equal_distance_cases_share_lanes():
    for group in (4, 8):
        case = bc.equal_case(group)
        rows = case["rows"]
        lane = rows[:, :group] // bc.L2_LANE_ROWS                                # (tile, wave, kc) of a row
        assert (lane[:, :4] == lane[:, :1]).all() and (rows[:, :group] % bc.L2_LANE_ROWS == np.arange(group) % 4).all()
        if group == 8:
            assert (lane[:, 4:] == lane[:, :1] + 1).all() and (rows[:, 0] % 16 // 4 < 3).all()        # the neighbouring lane of the same wave
        assert len(np.unique(rows)) == rows.size and rows.max() < bc.EQ_NT
        assert all(np.array_equal(case["t"][rows[i, group]], case["t"][rows[i, 1]]) for i in range(bc.EQ_NQ))
        # the emulation's prediction (not a condition on the hardware): the computed values of a query's planted rows collide
        F = np.stack([bc.emulate_pairs(case["q"], case["t"][rows[:, j]]) for j in range(group + 1)], 1)
        collide = np.array([np.unique(f, return_counts=True)[1].max() >= 3 for f in F])
        assert collide.mean() >= 0.25
        D = bc.d2_64(case["q"], case["t"])
        far = np.delete(D[0], rows[0]).min()
        assert D[np.arange(bc.EQ_NQ)[:, None], rows].max() < 1e-9 and far > 1.0


def test_screen_cases_sit_on_the_sample_border():
    for nt in bc.SCREEN_NT:
        case = bc.screen_case(100, nt)
        s = case["sample"]
        assert s == bc.screen_sample_rows(nt)
        if nt in (8193, 140_000):
            a, near, second = case["planted"][0]
            assert (near, second) == (s - 1, s) and case["planted"][1][1:] == (s, s - 1)     # nearest inside / second outside, and the reverse
        if nt == 140_000:
            assert (8831, 8832) in [p[1:] for p in case["planted"]]
            (a, r0, r1, copies), = case["outside_copies"]
            assert r1 < s and min(copies) >= s and all(np.array_equal(case["t"][c], case["t"][r1]) for c in copies)
        if nt <= 8193:
            bc.accept_case(_reference_keys(case), case)
    for nq in bc.SCREEN_NQ:
        case = bc.screen_case(nq, 300)
        assert {0, nq - 1} <= set(case["planted_q"].tolist())
        assert any((nq + d) % 48 == 0 for d in (-1, 0, 1))             # a wave's 48 queries; 384 = a block's


def test_adversarial_case_inverts_the_screen_order():
    case = bc.adversarial_case()
    q, t = case["q"], case["t"]
    for x in (q, t):
        m = (x.astype(np.float64) / float(bc.BESIDE_MIDPOINT)).astype(np.float32)
        assert np.array_equal(m.astype(np.float64) * float(bc.BESIDE_MIDPOINT), x.astype(np.float64))      # x = m (1 + 2^-9) exactly ...
        assert np.array_equal(bc.bf16_round(m), m) and np.array_equal(bc.bf16_round(x), m)                 # ... m is bf16, and x rounds to it
    D, S = bc.d2_64(q, t), bc.screen_values(q, t)
    ahead = []
    for qi, r0, r1, rivals in case["adv"]:
        order = np.argsort(D[qi], kind="stable")
        assert tuple(order[:2]) == (r0, r1) and D[qi, order[2]] - D[qi, r1] > 4 * bc.bound(q[[qi]], t).max()   # the true top-2, decided
        assert (D[qi, rivals] > D[qi, r1]).all() and (S[qi, rivals] < S[qi, r0]).all()                           # truly farther, screened nearer
        assert abs(float(q[qi].astype(np.float64) @ t[rivals[0]].astype(np.float64))) < 1e-9
        ahead.append(int((S[qi] < S[qi, r0]).sum()))
    assert min(ahead) >= 2 * bc.ADV_RIVALS
