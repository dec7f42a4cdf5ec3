"""GPU: the float L2 matchers (l2_topk_kernel of csrc/l2_match.hip, the bf16 screen + re-rank of csrc/l2_screen.hip) at the borders of their
tiles, wave slices, splits, dimensions, row paths, index bases and sample, judged by l2_border_cases.accept: a float64 reference with the
derived bound B = (dim + 16) 2^-24 (|q|^2 + |t|^2). test_l2_border_inputs_cpu.py shows that the inputs sit on those borders, that the check
passes an independent implementation and rejects the mistakes it is there for. Keys come from apds_dev_l2_topk / apds_dev_l2_topk_ex on
device tensors.
Left out: the screen's refusal at n_blocks * region > 2^29 candidate entries needs about 2.8 M queries."""
import ctypes as C

import numpy as np
import pytest

import l2_border_cases as bc

pytestmark = pytest.mark.gpu
BIG_BASE = 3_000_000_000       # above 2^31


class _Dev:
    def __init__(self, gpu_pkg):
        import torch
        self.torch = torch
        self.pl = __import__("cubesat_apds_amd.pipeline", fromlist=["x"])
        self.L, self.check = gpu_pkg.lib(), gpu_pkg._lib.check
        self.dev = torch.device("cuda:0")
        self.stream = torch.cuda.Stream(self.dev)

    def put(self, x, shift=0):
        """device copy of a float32 matrix; shift = 1: a view 4 bytes into a larger buffer (not 16-byte aligned)"""
        torch = self.torch
        x = np.ascontiguousarray(x, np.float32)
        buf = torch.empty(x.size + 4, dtype=torch.float32, device=self.dev)
        view = buf[shift:shift + x.size].view(x.shape)
        view.copy_(torch.from_numpy(x))
        assert view.data_ptr() % 16 == (4 * shift) % 16
        return view

    def topk(self, q, t, k=2, index_base=0, mode=None, q_shift=0, t_shift=0):
        """keys [nq, k] uint64 (mode None: apds_dev_l2_topk) or (keys, mode_used, candidates per query) (mode 0 / 1: apds_dev_l2_topk_ex)"""
        torch = self.torch
        with torch.cuda.stream(self.stream):
            dq, dt = (q if torch.is_tensor(q) else self.put(q, q_shift)), (t if torch.is_tensor(t) else self.put(t, t_shift))
            out = torch.empty((dq.shape[0], k), dtype=torch.int64, device=self.dev)
            used, cpq = C.c_int(-1), C.c_double(0)
            if mode is None:
                self.check(self.L.apds_dev_l2_topk(dq.data_ptr(), dq.shape[0], dt.data_ptr(), dt.shape[0], dq.shape[1], index_base, k, out.data_ptr(), self.pl.torch_stream()))
            else:
                self.check(self.L.apds_dev_l2_topk_ex(dq.data_ptr(), dq.shape[0], dt.data_ptr(), dt.shape[0], dq.shape[1], index_base, k, mode, out.data_ptr(),
                                                      self.pl.torch_stream(), C.byref(used), C.byref(cpq)))
            torch.cuda.synchronize()
            keys = out.cpu().numpy().view(np.uint64)
        return keys if mode is None else (keys, used.value, cpq.value)

    def parts_merged(self, q, t, cuts, index_base=0, k=2):
        """top-k of the row ranges between `cuts` with their index_base, merged by apds_dev_merge_topk"""
        torch = self.torch
        with torch.cuda.stream(self.stream):
            dq, dt = self.put(q), self.put(t)
            edges = [0] + list(cuts) + [len(t)]
            parts = torch.empty((len(edges) - 1, len(q), k), dtype=torch.int64, device=self.dev)
            for p, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
                self.check(self.L.apds_dev_l2_topk(dq.data_ptr(), len(q), dt[a:].data_ptr(), b - a, q.shape[1], (index_base + a) % (1 << 32), k, parts[p].data_ptr(),
                                                   self.pl.torch_stream()))
            merged = torch.empty((len(q), k), dtype=torch.int64, device=self.dev)
            self.check(self.L.apds_dev_merge_topk(parts.data_ptr(), len(edges) - 1, len(q), k, merged.data_ptr(), self.pl.torch_stream()))
            torch.cuda.synchronize()
            return merged.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def dev(gpu_pkg):
    return _Dev(gpu_pkg)


# --- exact kernel -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 1])
@pytest.mark.parametrize("nt", bc.TILE_NT)
def test_tile_borders_train_rows(dev, nt, k):
    case = bc.tile_case(129, nt)
    keys = dev.topk(case["q"], case["t"], k)
    bc.accept_case(keys, case, k=k)
    if nt == 1 and k == 2:
        assert (keys[:, 1] == bc.EMPTY_KEY).all() and (keys[:, 0] & bc.U32 == 0).all()


@pytest.mark.parametrize("k", [2, 1])
@pytest.mark.parametrize("nq", bc.TILE_NQ)
def test_tile_borders_queries(dev, nq, k):
    case = bc.tile_case(nq, 128 * 3 + 1)
    bc.accept_case(dev.topk(case["q"], case["t"], k), case, k=k)


def test_wave_slice_borders(dev):
    case = bc.wave_case()
    for k in (2, 1):
        bc.accept_case(dev.topk(case["q"], case["t"], k), case, k=k)


@pytest.mark.parametrize("nt", bc.SPLIT_NT)
def test_split_borders(dev, nt):
    """8200 queries x 17 / 18 train tiles: 6 splits of 3 tiles, the last shorter. All keys are computed; accept runs on the planted and tie
    queries and every 8th query (split_case_checked_queries); every query's keys must also equal those of the three-part merge."""
    case = bc.split_case(nt)
    sel = bc.split_case_checked_queries(case)
    keys = dev.topk(case["q"], case["t"], 2)
    bc.accept_case(keys[sel], case, sel=sel)
    assert np.array_equal(keys, dev.parts_merged(case["q"], case["t"], [383, 1921]))


@pytest.mark.parametrize("dim", bc.DIMS)
def test_dimensions_and_row_paths(dev, dim):
    case = bc.dim_case(dim)
    keys = dev.topk(case["q"], case["t"], 2)
    bc.accept_case(keys, case)
    if dim in (64, 128):       # dim == KP: an aligned pointer takes the FULL_ROWS kernel, a view 4 bytes into a buffer the padded one
        assert np.array_equal(keys, dev.topk(case["q"], case["t"], 2, t_shift=1))
        assert np.array_equal(keys, dev.topk(case["q"], case["t"], 2, q_shift=1))


@pytest.mark.parametrize("index_base", bc.INDEX_BASES)
def test_index_base_and_halves(dev, index_base):
    case = bc.base_case()
    keys = dev.topk(case["q"], case["t"], 2, index_base)
    bc.accept_case(keys, case, index_base=index_base)
    assert np.array_equal(keys, dev.parts_merged(case["q"], case["t"], [len(case["t"]) // 2], index_base))
    if index_base:
        k0 = dev.topk(case["q"], case["t"], 2, 0)
        assert np.array_equal(keys >> np.uint64(32), k0 >> np.uint64(32)) and np.array_equal((keys & bc.U32), (k0 & bc.U32) + np.uint64(index_base))


def test_scales_and_zero_vectors(dev):
    case = bc.scale_case()
    for k in (2, 1):
        keys = dev.topk(case["q"], case["t"], k)
        bc.accept_case(keys, case, k=k)
    keys = dev.topk(case["q"], case["t"], 2)
    sp = case["special"]
    assert list(keys[sp["zero_query"]]) == [33, 160]                                   # distance bits 0, the two zero rows in order
    assert int(keys[sp["equal"][0], 0] & bc.U32) == sp["equal"][1]


@pytest.mark.parametrize("group", [4, 8])
def test_equal_computed_distances(dev, group):
    """Near-duplicates of a query (q + 1e-6 noise) in the four rows of one lane, or the eight rows of two neighbouring lanes, and an exact
    copy elsewhere: their computed d^2 collide (the clamp at 0, the rounding of |q|^2 + u). The expected keys are built from the
    kernel's own per-pair values F(q, t), measured with one-row calls (nt = 1, k = 1): F does not depend on a row's position, so the
    two smallest (F, row) are what every path must return: the one call, the screen, and parts merged."""
    torch = dev.torch
    case = bc.equal_case(group)
    q, t, rows = case["q"], case["t"], case["rows"]
    with torch.cuda.stream(dev.stream):
        dq, dt = dev.put(q), dev.put(t)
        single = torch.empty((rows.shape[1], bc.EQ_NQ, bc.EQ_NQ), dtype=torch.int64, device=dev.dev)
        for j in range(rows.shape[1]):
            for i in range(bc.EQ_NQ):
                dev.check(dev.L.apds_dev_l2_topk(dq.data_ptr(), bc.EQ_NQ, dt[int(rows[i, j])].data_ptr(), 1, 128, 0, 1, single[j, i].data_ptr(), dev.pl.torch_stream()))
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
    print(f"group {group}: {int(collide.sum())} of {bc.EQ_NQ} queries have >= 3 equal computed distances; {int((F == 0).sum())} of {F.size} values are 0")
    assert collide.mean() >= 0.25
    want = bc.expected_from_pair_values(F, rows)
    got = dev.topk(q, t, 2)
    bad = np.nonzero((got != want).any(1))[0]
    assert not len(bad), (len(bad), [(int(i), [int(v & bc.U32) for v in got[i]], [int(v & bc.U32) for v in want[i]]) for i in bad[:4]])
    screen, used, _ = dev.topk(q, t, 2, mode=1)
    assert used == 1 and np.array_equal(screen, want)
    assert np.array_equal(dev.parts_merged(q, t, [258, 516]), want)                      # a group cut in two; every copy apart from its source


# --- screen -------------------------------------------------------------------------------------------------------------------------------------
def _screen_equals_exact(dev, case, index_base):
    torch = dev.torch
    with torch.cuda.stream(dev.stream):
        dq, dt = dev.put(case["q"]), dev.put(case["t"])
    exact, used0, _ = dev.topk(dq, dt, 2, index_base, mode=0)
    screen, used1, cpq = dev.topk(dq, dt, 2, index_base, mode=1)
    assert (used0, used1) == (0, 1)
    assert np.array_equal(exact, screen), (np.nonzero((exact != screen).any(1))[0][:5], cpq)
    _, rows = bc.split_keys(exact, index_base)
    for a, near, second in case["planted"]:
        assert tuple(rows[a]) == (near, second), (a, rows[a], near, second)
    for a, r0, r1, copies in case.get("outside_copies", []):
        assert tuple(rows[a]) == (r0, r1), (a, rows[a])
    return exact, cpq


@pytest.mark.parametrize("index_base", [0, BIG_BASE])
@pytest.mark.parametrize("nq", bc.SCREEN_NQ)
def test_screen_query_blocks(dev, nq, index_base):
    case = bc.screen_case(nq, 300)
    exact, _ = _screen_equals_exact(dev, case, index_base)
    bc.accept_case(exact, case, index_base=index_base)


@pytest.mark.parametrize("index_base", [0, BIG_BASE])
@pytest.mark.parametrize("nt", bc.SCREEN_NT)
def test_screen_train_rows_and_sample_border(dev, nt, index_base):
    """(at 140 000 rows the float64 reference of all pairs is left to the planted rows: the exact mode has its own tests above)"""
    case = bc.screen_case(100, nt)
    exact, _ = _screen_equals_exact(dev, case, index_base)
    if nt <= 8193 and index_base == 0:
        bc.accept_case(exact, case)


def test_screen_adversarial_rounding(dev):
    case = bc.adversarial_case()
    exact, cpq = _screen_equals_exact(dev, {**case, "planted": []}, 0)
    print(f"adversarial rounding: {cpq:.1f} candidates per query")
    for qi, r0, r1, rivals in case["adv"]:
        assert tuple(int(v & bc.U32) for v in exact[qi]) == (r0, r1)
    bc.check(exact, case["q"], case["t"], 0, 2)


def test_screen_fallbacks(dev):
    case = bc.screen_case(100, 300)
    q, t = case["q"], case["t"]
    for kw in ({"k": 1}, {"q_shift": 1}, {"t_shift": 1}):
        exact, used0, _ = dev.topk(q, t, mode=0, **kw)
        screen, used1, _ = dev.topk(q, t, mode=1, **kw)
        assert (used0, used1) == (0, 0) and np.array_equal(exact, screen), kw
        bc.accept_case(exact, case, k=kw.get("k", 2))
    exact, used0, _ = dev.topk(q, t[:1], mode=0)
    screen, used1, _ = dev.topk(q, t[:1], mode=1)
    assert (used0, used1) == (0, 0) and np.array_equal(exact, screen) and (exact[:, 1] == bc.EMPTY_KEY).all()


def test_screen_candidate_overflow(dev):
    """384 queries x 70 000 identical rows: 274 splits of 2 tiles, 2 * 128 * 384 = 98 304 candidates for a region of 73 728: the exact kernel
    takes over. Every row is at the same computed distance: rows 0 and 1."""
    rng = np.random.default_rng(0x4C32B900)
    q = bc._unit(rng, 384, 128).astype(np.float32)
    t = np.repeat(bc._unit(rng, 1, 128).astype(np.float32), 70_000, axis=0)
    exact, used0, _ = dev.topk(q, t, mode=0)
    screen, used1, cpq = dev.topk(q, t, mode=1)
    assert (used0, used1) == (0, 0) and cpq * 384 / 274 > bc.SC_REGION
    assert np.array_equal(exact, screen)
    assert (exact[:, 0] & bc.U32 == 0).all() and (exact[:, 1] & bc.U32 == 1).all() and np.array_equal(exact[:, 0] >> np.uint64(32), exact[:, 1] >> np.uint64(32))
    D = bc.d2_64(q, t[:1])[:, 0]
    F = (exact[:, 0] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    assert (np.abs(F - D) <= bc.bound(q, t[:1])[:, 0]).all()
