"""CPU: the inputs, the bound and the acceptance check of test_l2_borders_gpu.py (l2_border_cases.py). Every case is shown to sit on the
border it names, computed from the restated launch geometry; the cap (planted queries decided at both ranks, filler pairs to 99 %) is
checked with the float64 reference alone; `accept` passes the oracle's independent f32 matcher on every case, keeps a numpy binary32
emulation of the kernel's formula within the bound, and rejects six named mistakes applied to that emulation's keys. The screen's cases
are shown at both row lengths it is built for (64 and 128), also for test_l2_train_borders_gpu.py; a numpy emulation of the screen
(bf16 screen values, sample threshold, exact re-rank) is accepted by them and rejected under three mistakes of a screen."""
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


@pytest.mark.parametrize("dim", bc.SC_DIMS)
def test_restated_geometry(dim):
    assert bc.L2_TM == bc.L2_TN == 128 and bc.SC_Q == 384 and bc.SC_TM == 128 and bc.SC_REGION == 73728
    assert bc.split_plan(128 * 17 - 1, 8200) == (17, 6, 3) and bc.split_plan(128 * 17, 8200) == (17, 6, 3) and bc.split_plan(128 * 17 + 1, 8200) == (18, 6, 3)
    assert bc.split_plan(385, 129) == (4, 4, 1) and bc.split_plan(257, 130) == (3, 3, 1) and bc.split_plan(385, 1) == (4, 4, 1)
    assert bc.split_plan(70_000, 384, bc.SC_TM, bc.SC_Q) == (547, 274, 2) and 2 * bc.SC_TM * 384 == 98304 > bc.SC_REGION
    # the staging of a tile: 128 rows x dim / 8 pieces of 16 bytes over 512 threads; piece p of a thread is row ROWS_PER_PASS p + tid / (dim / 8)
    groups = dim // 8
    pieces = bc.SC_TM * groups // 512
    assert bc.SC_ROWS_PER_PASS[dim] == 512 // groups == {128: 32, 64: 64}[dim] and pieces == dim // 32 == bc.SC_TM // bc.SC_ROWS_PER_PASS[dim]
    assert bc.SC_PITCH[dim] == {128: 272, 64: 160}[dim] and bc.SC_PITCH[dim] % 16 == 0 and bc.SC_PITCH[dim] >= 2 * dim + 16      # bf16 rows, padded
    assert 2 * bc.SC_TM * bc.SC_PITCH[dim] + 2 * bc.SC_TM * 4 <= 160 * 1024 // 2                                          # two buffers + norms
    nts = bc.SCREEN_NT_BY_DIM[dim]
    assert nts[:5] == [2, 129, 8191, 8192, 8193] and nts[5] == bc.SCREEN_NT_LARGE[dim] == {128: 140_000, 64: 100_000}[dim]
    assert [bc.screen_sample_rows(n) for n in nts] == [2, 129, 8191, 8192, 8192, {128: 11776, 64: 8448}[dim]]
    assert bc.screen_sample_rows(140_000, 16) == 8832 and bc.screen_sample_rows(100_000, 16) == 8192   # a divisor of 16, as earlier documents state it
    assert bc.screen_sample_rows(98_304) == 8192 and bc.screen_sample_rows(98_316) == 8320           # where nt / 12 first passes the floor


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


def _screen_cases(dim):
    """(name, case, the queries `accept_case` runs on or None for all) of the screen at one row length"""
    for nq in bc.SCREEN_NQ:
        yield f"screen-nq{nq}", bc.screen_case(nq, 300, dim), None
    for nt in bc.SCREEN_NT_BY_DIM[dim]:
        case = bc.screen_case(100, nt, dim)
        yield f"screen-nt{nt}", case, (None if nt <= 8193 else bc.screen_case_checked_queries(case))


@pytest.mark.parametrize("dim", bc.SC_DIMS)
def test_the_cap_holds_by_the_reference_alone(small_cases, dim):
    """dim 128: every case of the exact kernel (all at 128 but the dimension cases). dim 64: the screen's cases at 64 elements per row: every
    planted query decided at both ranks, the filler to 99 %, for every case of at most 8193 rows; at 100 000 rows the cap is asked of
    the planted and outside-copy queries, the filler's decided share is printed and not conditioned on (measured: 1.000)."""
    if dim == 64:
        for name, case, sel in _screen_cases(64):
            q = case["q"] if sel is None else case["q"][sel]
            share = bc.accept_case(bc.topk_keys(bc.d2_64(q, case["t"]).astype(np.float32), 2), case, sel=sel)
            assert share >= 0.99 or len(case["t"]) < 3 or sel is not None, (name, share)
            if sel is not None:
                rest = np.setdiff1d(np.arange(len(case["q"])), sel)
                d = bc.check(bc.topk_keys(bc.d2_64(case["q"][rest], case["t"]).astype(np.float32), 2), case["q"][rest], case["t"], 0, 2)
                print(f"dim 64, {name}: filler pairs decided {d.mean():.3f}")
            if len(case["t"]) == 300:
                bc.accept_case(_reference_keys(case, 1), case, k=1)
        return
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


@pytest.mark.parametrize("dim", bc.SC_DIMS)
def test_equal_distance_cases_share_lanes(dim):
    for group in (4, 8):
        case = bc.equal_case(group, dim)
        assert case["q"].shape == (bc.EQ_NQ, dim) and case["t"].shape == (bc.EQ_NT, dim)
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


@pytest.mark.parametrize("dim", bc.SC_DIMS)
def test_screen_cases_sit_on_the_sample_border(dim):
    large = bc.SCREEN_NT_LARGE[dim]
    for nt in bc.SCREEN_NT_BY_DIM[dim]:
        case = bc.screen_case(100, nt, dim)
        s = case["sample"]
        assert s == bc.screen_sample_rows(nt) and case["q"].shape == (100, dim) and case["t"].shape == (nt, dim)
        pairs = [p[1:] for p in case["planted"]]
        assert len(np.unique([p[0] for p in case["planted"]])) == len(case["planted"])        # a query of its own per planted neighbour pair
        assert len(np.unique([r for p in pairs[::2] for r in p])) == len(pairs)               # no row planted twice
        if nt in (8193, large):
            a, near, second = case["planted"][0]
            assert (near, second) == (s - 1, s) and case["planted"][1][1:] == (s, s - 1)     # nearest inside / second outside, and the reverse
        if nt == large:
            assert 8192 < s < nt and s == {128: 11776, 64: 8448}[dim]
            s16 = bc.screen_sample_rows(nt, 16)
            assert s16 == {128: 8832, 64: 8192}[dim] and (s16 - 1, s16) in pairs and (s16, s16 - 1) in pairs
            (a, r0, r1, copies), = case["outside_copies"]
            assert r1 < s and min(copies) >= s and all(np.array_equal(case["t"][c], case["t"][r1]) for c in copies)
            assert not set(copies) & {r for p in pairs for r in p}
        if dim == 64 and nt >= 129:
            # the rows of a thread's second staged piece: (63, 64) across ROWS_PER_PASS, (127, 128) across the tile's end, both orders
            rp = bc.SC_ROWS_PER_PASS[64]
            for f, l in ((rp - 1, rp), (bc.SC_TM - 1, bc.SC_TM)):
                assert (f, l) in pairs and (l, f) in pairs, (nt, f, l)
            assert any(rp <= r % bc.SC_TM for p in pairs for r in p)
            if nt > 129 and nt % bc.SC_TM >= 2:                                                # a pair inside the last, partial tile
                last0 = nt // bc.SC_TM * bc.SC_TM
                inside = [p for p in pairs if min(p) >= last0 and (s >= nt or min(p) > s)]
                assert inside and all(max(p) < nt for p in inside), (nt, pairs)
            if nt == 8191:
                assert (8064, 8064 + 63) in pairs                                              # the last row of the first piece, in a partial tile
        if nt <= 8193:
            bc.accept_case(_reference_keys(case), case)
    for nq in bc.SCREEN_NQ:
        case = bc.screen_case(nq, 300, dim)
        assert {0, nq - 1} <= set(case["planted_q"].tolist())
        assert any((nq + d) % 48 == 0 for d in (-1, 0, 1))             # a wave's 48 queries; 384 = a block's
        if dim == 64:
            pairs = [p[1:] for p in case["planted"]]
            assert {(63, 64), (64, 63), (127, 128), (128, 127), (256, 277), (277, 256), (298, 299), (0, 255)} <= set(pairs)
    if dim == 128:                                                     # the cases of the existing GPU tests are the default arguments
        for a, b in ((bc.screen_case(47, 300), bc.screen_case(47, 300, 128)), (bc.adversarial_case(), bc.adversarial_case(128)), (bc.equal_case(4), bc.equal_case(4, 128))):
            assert np.array_equal(a["q"], b["q"]) and np.array_equal(a["t"], b["t"])


@pytest.mark.parametrize("dim", bc.SC_DIMS)
def test_adversarial_case_inverts_the_screen_order(dim):
    """Measured share of the 2 eps margin that the true second neighbour uses: 0.067 at dim 128, 0.045 at dim 64."""
    case = bc.adversarial_case(dim)
    q, t = case["q"], case["t"]
    assert q.shape[1] == t.shape[1] == dim
    for x in (q, t):
        m = (x.astype(np.float64) / float(bc.BESIDE_MIDPOINT)).astype(np.float32)
        assert np.array_equal(m.astype(np.float64) * float(bc.BESIDE_MIDPOINT), x.astype(np.float64))      # x = m (1 + 2^-9) exactly ...
        assert np.array_equal(bc.bf16_round(m), m) and np.array_equal(bc.bf16_round(x), m)                 # ... m is bf16, and x rounds to it
    D, S = bc.d2_64(q, t), bc.screen_values(q, t)
    eps = bc.screen_eps(q, t)
    assert bc.screen_sample_rows(len(t)) == len(t)                                                         # the sample is the whole set here
    ahead, share = [], []
    for qi, r0, r1, rivals in case["adv"]:
        order = np.argsort(D[qi], kind="stable")
        assert tuple(order[:2]) == (r0, r1) and D[qi, order[2]] - D[qi, r1] > 4 * bc.bound(q[[qi]], t).max()   # the true top-2, decided
        assert (D[qi, rivals] > D[qi, r1]).all() and (S[qi, rivals] < S[qi, r0]).all()                           # truly farther, screened nearer
        assert abs(float(q[qi].astype(np.float64) @ t[rivals[0]].astype(np.float64))) < 1e-9
        ahead.append(int((S[qi] < S[qi, r0]).sum()))
        # what gives the case its power: the true second neighbour is a candidate only through the margin of screen_theta_kernel
        s2 = np.sort(S[qi])[1]
        assert s2 < S[qi, r1] < s2 + 2.0 * eps[qi], (qi, s2, S[qi, r1], eps[qi])
        share.append((S[qi, r1] - s2) / (2.0 * eps[qi]))
    assert min(ahead) >= 2 * bc.ADV_RIVALS
    print(f"dim {dim}: {min(ahead)} rows screen ahead of t0; the true second neighbour uses {min(share):.4f} .. {max(share):.4f} of the 2 eps margin")


def test_screen_emulation_passes_and_three_mistakes_do_not():
    """The checks of test_l2_train_borders_gpu.py on emulated keys: a correct screen in numpy is accepted at both lengths; without eps, with
    the whole set's second screen value as the threshold, or without rows 64..127 of every tile among the candidates it is rejected."""
    def judge(case, keys):
        if "adv" in case:
            _, rows = bc.split_keys(keys)
            for qi, r0, r1, rivals in case["adv"]:
                assert tuple(rows[qi]) == (r0, r1), (qi, rows[qi], r0, r1)
            bc.check(keys, case["q"], case["t"], 0, 2)
        else:
            bc.accept_case(keys, case)

    def rejected(case, F, **mistake):
        with pytest.raises(AssertionError):
            judge(case, bc.emulate_screen(case["q"], case["t"], exact=F, **mistake)[0])

    for dim in bc.SC_DIMS:
        adv, tile, border = bc.adversarial_case(dim), bc.screen_case(49, 300, dim), bc.screen_case(100, 8193, dim)
        F = {id(c): bc.emulate_matrix(c["q"], c["t"]) for c in (adv, tile, border)}
        for c in (adv, tile, border):
            keys, cpq = bc.emulate_screen(c["q"], c["t"], exact=F[id(c)])
            judge(c, keys)
            assert np.array_equal(keys, bc.topk_keys(F[id(c)], 2))                              # the screen loses nothing of the exact top-2
            print(f"dim {dim}, {len(c['q'])} x {len(c['t'])}: {cpq:.1f} candidates per query in the emulation")
        rejected(adv, F[id(adv)], eps_scale=0.0)
        rejected(adv, F[id(adv)], whole_set_s2=True)
        for c in (tile, border):
            rejected(c, F[id(c)], drop_second_piece=True)
