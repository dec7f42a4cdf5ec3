"""GPU: the resident L2 train set (apds_l2_train_*, apds_dev_l2_train_top2 of csrc/l2_screen.hip) at 64 and 128 elements per row, at the
borders of the screen: query blocks, train tiles and the rows of a thread's second staged piece, the sample (floor and nt / 12), adversarial
bf16 rounding, equal computed distances, candidate overflow and what it leaves on the handle, one handle through many shapes, index bases
above 2^31 and across the wrap of 2^32. Judged by l2_border_cases: the float64 reference with the derived bound
B = (dim + 16) 2^-24 (|q|^2 + |t|^2), and bit equality with the handle's exact mode and with apds_dev_l2_topk.
test_l2_border_inputs_cpu.py shows that the inputs sit where they claim and that the checks reject a screen without its margin, with the
whole set's threshold, or without the second piece's rows.
Left out: the refusal at 2^29 candidate entries (millions of queries); the APDS_L2_PRIO / APDS_L2_SAMPLE_DIV switches."""
from importlib import import_module

import numpy as np
import pytest

import l2_border_cases as bc

pytestmark = pytest.mark.gpu
BIG_BASE = 3_000_000_000       # above 2^31
WRAP_BASE = (1 << 32) - 3      # rows 0, 1, 2 keep the top of the u32 range, row 3 is index 0
SENTINEL = 0x5A5A5A5A5A5A5A5A
WORST = {64: 0.0, 128: 0.0}    # largest |F - D| / B seen per row length (printed, and asserted <= 1 where it is measured)


class _Dev:
    def __init__(self, pkg):
        import torch
        self.torch, self.pkg = torch, pkg
        self.pl = import_module(pkg.__name__ + ".pipeline")
        self.L, self.check = pkg.lib(), pkg._lib.check
        self.stream = torch.cuda.Stream()      # the C ABI reads torch's default stream (handle 0) as "the thread's own": work on an explicit one

    def put(self, x):
        t = self.torch.from_numpy(np.ascontiguousarray(x, np.float32)).to("cuda:0")
        self.torch.cuda.synchronize()
        assert t.data_ptr() % 16 == 0
        return t

    def topk(self, dq, dt, index_base=0, k=2):
        """apds_dev_l2_topk: keys [nq, k] uint64"""
        out = self.torch.empty((dq.shape[0], k), dtype=self.torch.int64, device="cuda:0")
        with self.torch.cuda.stream(self.stream):
            self.check(self.L.apds_dev_l2_topk(dq.data_ptr(), dq.shape[0], dt.data_ptr(), dt.shape[0], dt.shape[1], index_base, k, out.data_ptr(), self.pl.torch_stream()))
        self.torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint64)

    def top2(self, ts, dq, mode="screen", out=None):
        """(keys [nq, 2] uint64, mode used, candidates per query) of one call on the handle"""
        with self.torch.cuda.stream(self.stream):
            res = ts.top2(dq, mode, out=out)
        self.torch.cuda.synchronize()
        return res.cpu().numpy().view(np.uint64), ts.mode_used, ts.candidates_per_query


@pytest.fixture(scope="module")
def dev(gpu_pkg):
    return _Dev(gpu_pkg)


def _note_error(keys, q, t, index_base, dim):
    """largest |F - D| / B over the returned (query, row) pairs, float64 reference of those pairs only"""
    F, rows = bc.split_keys(keys, index_base)
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    worst = 0.0
    for j in range(keys.shape[1]):
        tj = t64[rows[:, j]]
        D = ((q64 - tj) ** 2).sum(1)
        B = (dim + 16) * 2.0 ** -24 * ((q64 * q64).sum(1) + (tj * tj).sum(1))
        worst = max(worst, float((np.abs(F[:, j] - D) / B).max()))
    WORST[dim] = max(WORST[dim], worst)
    print(f"dim {dim}: largest |F - D| / B here {worst:.3f}, so far {WORST[dim]:.3f}")
    assert worst <= 1.0
    return worst


def _handle_agrees(dev, case, index_base=0):
    """The handle's screen (which must have run), its exact mode and apds_dev_l2_topk return the same keys; planted rows in order; copies
    outside the sample lose to the lower row. -> (keys, candidates per query)"""
    dq, dt = dev.put(case["q"]), dev.put(case["t"])
    want = dev.topk(dq, dt, index_base)
    ts = dev.pl.L2TrainSet(dt, index_base=index_base)
    try:
        assert ts.info() == (len(case["t"]), case["dim"], True)
        screen, used, cpq = dev.top2(ts, dq, "screen")
        assert used == "screen", used
        exact, used, _ = dev.top2(ts, dq, "exact")
        assert used == "exact"
    finally:
        ts.close()
    assert np.array_equal(screen, exact), (np.nonzero((exact != screen).any(1))[0][:5], cpq)
    assert np.array_equal(screen, want), np.nonzero((want != screen).any(1))[0][:5]
    _, rows = bc.split_keys(screen, index_base)
    for a, near, second in case.get("planted", []):
        assert tuple(rows[a]) == (near, second), (a, rows[a], near, second)
    for a, r0, r1, copies in case.get("outside_copies", []):
        assert tuple(rows[a]) == (r0, r1), (a, rows[a], copies)
    return screen, cpq


@pytest.mark.parametrize("index_base", [0, BIG_BASE])
@pytest.mark.parametrize("nq", bc.SCREEN_NQ)
@pytest.mark.parametrize("dim", bc.SC_DIMS)
def test_screen_query_blocks(dev, dim, nq, index_base):
    case = bc.screen_case(nq, 300, dim)
    keys, _ = _handle_agrees(dev, case, index_base)
    bc.accept_case(keys, case, index_base=index_base)
    _note_error(keys, case["q"], case["t"], index_base, dim)


@pytest.mark.parametrize("dim,nt", [(dim, nt) for dim in bc.SC_DIMS for nt in bc.SCREEN_NT_BY_DIM[dim]])
def test_train_rows_and_sample_border(dev, dim, nt):
    """nt in 2, 129, 8191, 8192, 8193 and the size at which the sample is nt / 12 in whole tiles (100 000 at dim 64: 8448; 140 000 at dim 128:
    11776). Up to 8193 rows every query is judged against float64; above, the planted and outside-copy queries are."""
    case = bc.screen_case(100, nt, dim)
    keys, cpq = _handle_agrees(dev, case)
    pairs = {p[1:] for p in case["planted"]}
    s = case["sample"]
    if s < nt:
        assert (s - 1, s) in pairs and (s, s - 1) in pairs                     # (both orders came back: _handle_agrees)
    sel = None if nt <= 8193 else bc.screen_case_checked_queries(case)
    bc.accept_case(keys if sel is None else keys[sel], case, sel=sel)
    _note_error(keys, case["q"], case["t"], 0, dim)
    print(f"dim {dim}, 100 x {nt}: sample {s}, {cpq:.1f} candidates per query")


@pytest.mark.parametrize("dim", bc.SC_DIMS)
def test_adversarial_rounding(dev, dim):
    case = bc.adversarial_case(dim)
    keys, cpq = _handle_agrees(dev, case)
    print(f"dim {dim}, adversarial rounding: {cpq:.1f} candidates per query")
    for qi, r0, r1, rivals in case["adv"]:
        assert tuple(int(v & bc.U32) for v in keys[qi]) == (r0, r1), (qi, keys[qi], r0, r1)
    bc.check(keys, case["q"], case["t"], 0, 2)
    _note_error(keys, case["q"], case["t"], 0, dim)


@pytest.mark.parametrize("group", [4, 8])
def test_equal_computed_distances_dim64(dev, group):
    """As test_l2_borders_gpu.py::test_equal_computed_distances, at 64 elements per row: the expected keys are built from the kernel's own
    per-pair values (one-row calls), and the handle's screen, its exact mode and apds_dev_l2_topk must all return them."""
    torch = dev.torch
    case = bc.equal_case(group, 64)
    q, t, rows = case["q"], case["t"], case["rows"]
    dq, dt = dev.put(q), dev.put(t)
    single = torch.empty((rows.shape[1], bc.EQ_NQ, bc.EQ_NQ), dtype=torch.int64, device="cuda:0")
    with torch.cuda.stream(dev.stream):
        for j in range(rows.shape[1]):
            for i in range(bc.EQ_NQ):
                dev.check(dev.L.apds_dev_l2_topk(dq.data_ptr(), bc.EQ_NQ, dt[int(rows[i, j])].data_ptr(), 1, 64, 0, 1, single[j, i].data_ptr(), dev.pl.torch_stream()))
    torch.cuda.synchronize()
    single = single.cpu().numpy().view(np.uint64)
    ar = np.arange(bc.EQ_NQ)
    own = single[:, ar, ar].T                                                            # [query, j]: key of (query, rows[query, j]) as row 0
    assert (own & bc.U32 == 0).all()
    F = (own >> np.uint64(32)).astype(np.uint32).view(np.float32).reshape(own.shape)
    D = np.stack([np.einsum("ij,ij->i", q.astype(np.float64) - t[rows[:, j]], q.astype(np.float64) - t[rows[:, j]]) for j in range(rows.shape[1])], 1)
    assert (np.abs(F - D) <= bc.bound(q, t)[ar[:, None], rows]).all()
    assert (F[:, group] == F[:, 1]).all()                                                # the copy's value is its source's: position plays no part
    collide = np.array([np.unique(f, return_counts=True)[1].max() >= 3 for f in F])
    print(f"dim 64, group {group}: {int(collide.sum())} of {bc.EQ_NQ} queries have >= 3 equal computed distances; {int((F == 0).sum())} of {F.size} values are 0")
    assert collide.mean() >= 0.25
    want = bc.expected_from_pair_values(F, rows)
    got = dev.topk(dq, dt)
    bad = np.nonzero((got != want).any(1))[0]
    assert not len(bad), (len(bad), [(int(i), [int(v & bc.U32) for v in got[i]], [int(v & bc.U32) for v in want[i]]) for i in bad[:4]])
    ts = dev.pl.L2TrainSet(dt)
    try:
        screen, used, _ = dev.top2(ts, dq, "screen")
        assert used == "screen" and np.array_equal(screen, want), np.nonzero((screen != want).any(1))[0][:4]
        exact, used, _ = dev.top2(ts, dq, "exact")
        assert used == "exact" and np.array_equal(exact, want)
    finally:
        ts.close()


def test_candidate_overflow_through_the_handle(dev):
    """70 000 identical rows of 64 elements: every row is a candidate of every query. One block of pass B holds two tiles (274 splits), so
    384 queries give it 2 * 128 * 384 = 98 304 candidates for a region of 73 728: the handle falls back to its exact path. 288 queries
    fill the region to its last entry (2 * 128 * 288 = 73 728) and 17 leave it nearly empty: both must run the screen, on the same
    handle, right after the overflow; then the overflow call again, so that a count or a region left over would show."""
    rng = np.random.default_rng(0x4C64B900)
    q = bc._unit(rng, 384, 64).astype(np.float32)
    t = np.repeat(bc._unit(rng, 1, 64).astype(np.float32), 70_000, axis=0)
    assert bc.split_plan(70_000, 384, bc.SC_TM, bc.SC_Q)[1:] == (274, 2) and 2 * bc.SC_TM * 288 == bc.SC_REGION
    dq, dt = dev.put(q), dev.put(t)
    want = dev.topk(dq, dt)
    D = bc.d2_64(q, t[:1])[:, 0]
    B = bc.bound(q, t[:1])[:, 0]

    def rows_0_and_1(keys, n):
        assert (keys[:, 0] & bc.U32 == 0).all() and (keys[:, 1] & bc.U32 == 1).all() and np.array_equal(keys[:, 0] >> np.uint64(32), keys[:, 1] >> np.uint64(32))
        F = (keys[:, 0] >> np.uint64(32)).astype(np.uint32).view(np.float32)
        assert (np.abs(F - D[:n]) <= B[:n]).all()
        assert np.array_equal(keys, want[:n])

    ts = dev.pl.L2TrainSet(dt)
    try:
        for nq, mode in ((384, "exact"), (288, "screen"), (17, "screen"), (384, "exact"), (289, "exact"), (288, "screen")):
            keys, used, cpq = dev.top2(ts, dq[:nq], "screen")
            print(f"{nq} queries x 70 000 identical rows: {used}, {cpq:.0f} candidates per query, {2 * bc.SC_TM * nq} in a block of two tiles")
            assert used == mode, (nq, used, cpq)
            assert cpq == 70_000 and (2 * bc.SC_TM * nq > bc.SC_REGION) == (mode == "exact")
            rows_0_and_1(keys, nq)
        exact, used, _ = dev.top2(ts, dq, "exact")
        assert used == "exact"
        rows_0_and_1(exact, 384)
    finally:
        ts.close()


@pytest.mark.parametrize("dim", bc.SC_DIMS)
def test_one_handle_many_shapes(dev, dim):
    """nq = 385, 1, 384, 17, 513 on one handle into one output buffer of 600 rows: each result equals apds_dev_l2_topk's and the handle's
    exact mode, the rows past nq keep a sentinel; one more call takes its queries from an aligned view into a larger tensor."""
    torch = dev.torch
    case = bc.screen_case(513, 8193, dim)
    dq, dt = dev.put(case["q"]), dev.put(case["t"])
    want = dev.topk(dq, dt)
    out = torch.empty((600, 2), dtype=torch.int64, device="cuda:0")
    ts = dev.pl.L2TrainSet(dt)
    try:
        for nq in (385, 1, 384, 17, 513):
            for mode in ("screen", "exact"):
                out.fill_(SENTINEL)
                torch.cuda.synchronize()
                keys, used, _ = dev.top2(ts, dq[:nq], mode, out=out)
                assert used == mode and keys.shape == (nq, 2) and np.array_equal(keys, want[:nq]), (nq, mode, used)
                assert (out[nq:].cpu().numpy() == SENTINEL).all(), (nq, mode)
        view = dq[5:]                                                                    # 5 rows = 1280 or 2560 bytes into the tensor
        assert view.data_ptr() % 16 == 0 and view.data_ptr() != dq.data_ptr()
        alone = dev.put(case["q"][5:])
        got_view, used_view, _ = dev.top2(ts, view, "screen")
        got_alone, used_alone, _ = dev.top2(ts, alone, "screen")
        assert used_view == used_alone == "screen"
        assert np.array_equal(got_view, got_alone) and np.array_equal(got_view, want[5:])
    finally:
        ts.close()


@pytest.mark.parametrize("dim", bc.SC_DIMS)
def test_index_base_across_the_wrap(dev, dim):
    """index_base = 2^32 - 3 on 300 rows: rows 0, 1, 2 carry the indices 2^32 - 3 .. 2^32 - 1 and row 3 the index 0, inside one lane's
    four rows of the first tile. Row 2 (index 0xFFFFFFFF, the low word of an empty key) and row 3 are each made the nearest row of a
    query of their own. The keys' low words are (row + base) mod 2^32 and their distance words those of base 0."""
    case = bc.screen_case(385, 300, dim)
    q, t = case["q"].copy(), case["t"]
    rng = np.random.default_rng(0x4C64BA00 + dim)
    assert not {200, 201} & set(case["planted_q"].tolist()) and not {2, 3} & {r for p in case["planted"] for r in p[1:]}
    for qi, row in ((200, 2), (201, 3)):
        q[qi] = (t[row].astype(np.float64) + bc._offset(rng, dim, 0.1)).astype(np.float32)
        D = bc.d2_64(q[[qi]], t)[0]
        assert int(np.argmin(D)) == row and np.sort(D)[1] > 0.5
    wrapped = {**case, "q": q}
    k0, _ = _handle_agrees(dev, wrapped, 0)
    kw, _ = _handle_agrees(dev, wrapped, WRAP_BASE)
    bc.accept_case(kw, wrapped, index_base=WRAP_BASE)
    assert np.array_equal(kw >> np.uint64(32), k0 >> np.uint64(32))
    assert np.array_equal(kw & bc.U32, ((k0 & bc.U32) + np.uint64(WRAP_BASE)) & bc.U32)
    assert int(kw[200, 0] & bc.U32) == 0xFFFFFFFF and int(kw[201, 0] & bc.U32) == 0
    a = case["planted"][2][0]                                                             # row 0 is the nearest row of this planted query
    assert case["planted"][2][1] == 0 and int(kw[a, 0] & bc.U32) == WRAP_BASE
