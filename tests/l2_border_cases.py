"""Inputs, float64 reference and acceptance check for the float L2 matchers (csrc/l2_match.hip, csrc/l2_screen.hip) at the borders of their
tiles, wave slices, splits, dimensions and sample. Used by test_l2_border_inputs_cpu.py (which shows that every input sits on the border it
names and that the check accepts an independent implementation and rejects six named mistakes), by test_l2_borders_gpu.py (the one-shot
entries) and by test_l2_train_borders_gpu.py (the resident train set). The screen's cases take the row length: 128 or 64.

Reference. d2_64(q, t) = sum_i (q_i - t_i)^2 in numpy float64 on the float32 inputs: its own error (a few 2^-53 relative) is nothing beside
the bound below.

Bound. The kernel computes F = max(fl(Q + fl(T - 2 P)), 0) in binary32 with u = 2^-24, where
  * Q, T are the row norms of row_norms_kernel: every element is squared (one rounding, or none where the compiler contracts the square
    into the add) and then passes through at most 7 adds (one inside its lane, six in the xor-shuffle tree); all terms are >= 0, so
    |Q - |q|^2| <= 8u |q|^2 and |T - |t|^2| <= 8u |t|^2 to first order:                                         8u (|q|^2 + |t|^2)
  * P is a dim-long fmaf chain (the f32 MFMA; zero padding of the k axis adds exact zeros): |P - q.t| <= gamma_dim sum |q_i t_i|
    <= dim u |q| |t|; it enters doubled, and 2 |q| |t| <= |q|^2 + |t|^2:                                     dim u (|q|^2 + |t|^2)
  * fmaf(-2, P, T) rounds once a value of size <= |t|^2 + 2 |q| |t| <= 2 (|q|^2 + |t|^2):                      2u (|q|^2 + |t|^2)
  * the final add rounds once a value of size <= (|q| + |t|)^2 <= 2 (|q|^2 + |t|^2):                           2u (|q|^2 + |t|^2)
  * the clamp at 0 moves F towards the true value, which is >= 0.
First order total (dim + 12) u (|q|^2 + |t|^2); the second order terms (gamma_n = n u / (1 - n u), products of the above) are below
(dim + 12)^2 u^2 < 2e-3 u per unit of (|q|^2 + |t|^2), and 4u is set aside for them and for the double rounding of the emulation's fma:
    B(q, t) = (dim + 16) 2^-24 (|q|^2 + |t|^2),        norms in float64.
The bound was written down before any GPU run and is checked here against a numpy binary32 emulation of the formula only
(test_l2_border_inputs_cpu.py::test_emulation_stays_within_the_bound records the largest error / B seen).

Acceptance (`check`, `accept`), per query and rank j < k, with D = d2_64, s_0, s_1, ... the reference's rows in ascending (D, row):
  * j >= nt: the key is EMPTY_KEY; otherwise it is not, its row (minus index_base, mod 2^32) is in [0, nt), the rows of a query are distinct
    and its keys strictly ascending as u64;
  * |F_j - D(row_j)| <= B(q, row_j);
  * D(row_j) <= max_{m <= j} (D(s_m) + B(q, s_m)) + B(q, row_j): among s_0..s_j one row is not ranked before j, so the kernel's j-th value is at
    most the largest computed value among them (with equal norms this is "the j-th smallest D + 2B");
  * row_j == s_j wherever s_j is DECIDED: |D(r) - D(s_j)| > B(q, r) + B(q, s_j) for every other row r, so that no computed order within the
    bound can differ (with equal norms: the reference's gaps on both sides of rank j exceed 2B).
`accept` returns the share of (query, rank) pairs that are decided. The inputs below are built so that every planted query is decided at
both ranks and at least 99 % of the filler pairs are: filler rows and queries have unit norm (d^2 ~ 2 from each other, B ~ 2e-5 at dim 128),
a planted query has rows at |e| = 0.1 and 0.2 (d^2 = 0.01 and 0.04)."""
import numpy as np

EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
U32 = np.uint64(0xFFFFFFFF)

# --- the launch geometry of the two kernels, restated (test_l2_border_inputs_cpu.py asserts the cases against these) -----------------------
L2_TM = L2_TN = 128          # train rows / queries per block tile of l2_topk_kernel
L2_WAVE_ROWS = 16            # rows of a tile owned by one of the 8 waves
L2_LANE_ROWS = 4             # rows of a wave's slice owned by one lane (k class kc = lane >> 4): rows 16 w + 4 kc + 0..3
L2_BLOCK_TARGET = 512        # blocks the split plan aims at
SC_Q = 384                   # queries per block of l2_screen_kernel
SC_TM = 128                  # train rows per tile of the screen
SC_DIMS = (64, 128)          # the two descriptor lengths the screen is built for (128: the one-shot entry and the train set; 64: the train set)
SC_ROWS_PER_PASS = {128: 32, 64: 64}   # rows that one staged piece of all 512 threads covers: 512 / (dim / 8); a tile is 4 or 2 pieces per thread
SC_PITCH = {128: 272, 64: 160}         # bytes per staged train row in LDS
SC_SAMPLE_DIV = 12           # runtime default of the sample divisor (APDS_L2_SAMPLE_DIV)
SC_SAMPLE_MIN = 8192
SC_REGION = 384 * 192        # candidate entries per block of pass B


def ceil_div(a, b):
    return -(-a // b)


def split_plan(n_rows, n_cols, tile_rows=L2_TM, tile_cols=L2_TN):
    """(t_tiles, splits, tiles_per_split) for n_rows train rows against n_cols queries"""
    q_tiles, t_tiles = ceil_div(n_cols, tile_cols), ceil_div(n_rows, tile_rows)
    splits = max(1, min(t_tiles, ceil_div(L2_BLOCK_TARGET, q_tiles)))
    tiles_per_split = ceil_div(t_tiles, splits)
    return t_tiles, ceil_div(t_tiles, tiles_per_split), tiles_per_split


def screen_sample_rows(nt, div=SC_SAMPLE_DIV):
    return min(nt, max(SC_SAMPLE_MIN, ceil_div(nt // div, SC_TM) * SC_TM))


# --- reference, bound, acceptance --------------------------------------------------------------------------------------------------------------
def d2_64(q, t):
    """[nq, nt] float64 sum of squared differences of float32 rows"""
    q64, t64 = np.asarray(q, np.float32).astype(np.float64), np.asarray(t, np.float32).astype(np.float64)
    out = np.empty((len(q64), len(t64)))
    step = max(1, (1 << 22) // max(1, t64.size))
    for a in range(0, len(q64), step):
        d = q64[a:a + step, None, :] - t64[None, :, :]
        out[a:a + step] = np.einsum("ijk,ijk->ij", d, d)
    return out


def bound(q, t):
    """[nq, nt] B(q, t) = (dim + 16) 2^-24 (|q|^2 + |t|^2)"""
    q64, t64 = np.asarray(q, np.float32).astype(np.float64), np.asarray(t, np.float32).astype(np.float64)
    return (q64.shape[1] + 16) * 2.0 ** -24 * ((q64 * q64).sum(1)[:, None] + (t64 * t64).sum(1)[None, :])


def split_keys(keys, index_base=0):
    """u64 keys -> (d^2 as float64, row minus index_base as int64 in [0, 2^32))"""
    k = np.asarray(keys).view(np.uint64) if np.asarray(keys).dtype == np.int64 else np.asarray(keys, np.uint64)
    f = (k >> np.uint64(32)).astype(np.uint32).view(np.float32).reshape(k.shape).astype(np.float64)
    rows = ((k & U32).astype(np.int64) - int(index_base)) % (1 << 32)
    return f, rows


def make_keys(f32, rows, index_base=0):
    """(float32 d^2 >= 0, rows) -> u64 keys"""
    bits = np.ascontiguousarray(f32, np.float32).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | ((np.asarray(rows, np.int64) + int(index_base)) % (1 << 32)).astype(np.uint64)


def topk_keys(F, k, index_base=0, higher_row_first=False):
    """the k smallest (F, row) of every row of the float32 matrix F as keys [nq, k], EMPTY_KEY where nt < k"""
    nq, nt = F.shape
    rows = np.arange(nt)
    out = np.full((nq, k), EMPTY_KEY, np.uint64)
    for i in range(nq):
        order = np.lexsort((-rows if higher_row_first else rows, F[i]))[:k]
        order = order[np.isfinite(F[i, order])]
        out[i, :len(order)] = make_keys(F[i, order], order, index_base)
    return out


def check(keys, q, t, index_base, k):
    """Raises AssertionError naming the first broken rule; returns the bool [nq, min(k, nt)] mask of decided (query, rank) pairs."""
    keys = np.asarray(keys)
    keys = keys.view(np.uint64) if keys.dtype == np.int64 else keys.astype(np.uint64)
    nq, nt = len(q), len(t)
    assert keys.shape == (nq, k), keys.shape
    kk = min(k, nt)
    assert (keys[:, kk:] == EMPTY_KEY).all(), "a slot past the train rows holds a key"
    assert (keys[:, :kk] != EMPTY_KEY).all(), "EMPTY_KEY where a row exists"
    decided = np.zeros((nq, kk), bool)
    if not kk or not nq:
        return decided
    F, rows = split_keys(keys[:, :kk], index_base)
    assert ((rows >= 0) & (rows < nt)).all(), ("row out of range", rows[(rows < 0) | (rows >= nt)][:4])
    if kk == 2:
        assert (rows[:, 0] != rows[:, 1]).all(), "one row twice"
        assert (keys[:, 0] < keys[:, 1]).all(), ("keys not ascending", np.nonzero(keys[:, 0] >= keys[:, 1])[0][:4])
    D, Bm = d2_64(q, t), bound(q, t)
    ar = np.arange(nq)
    order = np.argsort(D, axis=1, kind="stable")[:, :kk]
    reach = np.full(nq, -np.inf)
    for j in range(kk):
        sj, rj = order[:, j], rows[:, j]
        Dj, Bj = D[ar, sj], Bm[ar, sj]
        err = np.abs(F[:, j] - D[ar, rj])
        assert (err <= Bm[ar, rj]).all(), ("distance off by more than B: worst error / B", float((err / np.maximum(Bm[ar, rj], 1e-300)).max()), j)
        reach = np.maximum(reach, Dj + Bj)
        late = D[ar, rj] > reach + Bm[ar, rj]
        assert not late.any(), ("a nearer row was missed", np.nonzero(late)[0][:4], j)
        sep = np.abs(D - Dj[:, None]) > Bm + Bj[:, None]
        sep[ar, sj] = True
        decided[:, j] = sep.all(1)
        wrong = decided[:, j] & (rj != sj)
        assert not wrong.any(), ("row differs from a decided reference row", np.nonzero(wrong)[0][:4], j)
    return decided


def accept(keys, q, t, index_base, k):
    """The acceptance check; returns the share of (query, rank) pairs decided by the reference's gaps."""
    d = check(keys, q, t, index_base, k)
    return float(d.mean()) if d.size else 1.0


def accept_case(keys, case, index_base=0, k=2, sel=None):
    """`accept` on a case plus the cap: planted queries decided everywhere, filler pairs to >= 99 %, ties to the lower row, bit-equal
    distances of copied rows; a query whose second neighbour has copies outside the sample: nearest decided, the lower row second. `sel`: the subset of query indices that `keys` holds (default all)."""
    sel = np.arange(len(case["q"])) if sel is None else np.asarray(sel)
    d = check(keys, case["q"][sel], case["t"], index_base, k)
    planted = np.isin(sel, case["planted_q"])
    tied = np.isin(sel, [c[0] for c in case["ties"]] + list(case.get("excluded", [])) + [c[0] for c in case.get("outside_copies", [])])
    assert d[planted].all(), "a planted query is not decided"
    filler = ~planted & ~tied
    if filler.any() and d.shape[1]:
        assert d[filler].mean() >= 0.99, d[filler].mean()
    _, rows = split_keys(np.asarray(keys)[:, :d.shape[1]], index_base)
    pos = {int(v): i for i, v in enumerate(sel)}
    for qi, near, second in case["planted"]:
        if qi in pos:
            want = [r for r in (near, second) if r >= 0][:d.shape[1]]
            assert list(rows[pos[qi], :len(want)]) == want, (qi, rows[pos[qi]], want)
    kb = np.asarray(keys).view(np.uint64) if np.asarray(keys).dtype == np.int64 else np.asarray(keys, np.uint64)
    for qi, lo, hi in case["ties"]:
        if qi in pos:
            assert int(rows[pos[qi], 0]) == lo, ("tie not to the lower row", qi, rows[pos[qi]], lo, hi)
            if d.shape[1] == 2:
                assert int(rows[pos[qi], 1]) == hi and kb[pos[qi], 0] >> np.uint64(32) == kb[pos[qi], 1] >> np.uint64(32), (qi, rows[pos[qi]])
    for qi, r0, r1, copies in case.get("outside_copies", []):      # rank 1 has exact copies at higher rows: undecided by the gaps, decided by the row
        if qi in pos:
            assert d[pos[qi], 0] and list(rows[pos[qi]]) == [r0, r1][:d.shape[1]], ("a copy outside the sample won over the lower row", qi, rows[pos[qi]], r0, r1, copies)
    return float(d.mean()) if d.size else 1.0


# --- inputs ------------------------------------------------------------------------------------------------------------------------------------
def _unit(rng, n, dim):
    x = rng.normal(size=(n, dim))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _offset(rng, dim, length, avoid=None):
    e = rng.normal(size=dim)
    if avoid is not None and dim > 1:
        e -= avoid * (e @ avoid) / (avoid @ avoid)
    return e * (length / np.linalg.norm(e))


def query_slots(nq):
    """query indices for planted queries, the borders of the 128-query tiles first"""
    pref = [0, nq - 1, 127, 128, 1, nq - 2, 126, 129, 255, 256, 383, 384, 63, 64]
    seen, out = set(), []
    for v in pref + list(range(2, nq)):
        if 0 <= v < nq and v not in seen:
            seen.add(v)
            out.append(v)
    return out


def tile_pairs(nt, tile=L2_TM):
    """(first row, last existing row) of every tile"""
    return [(a, min(a + tile, nt) - 1) for a in range(0, nt, tile)]


def wave_pairs(nt, tiles=(0, 1), waves=(0, 3, 7)):
    """(first row, last row) of a wave's 16-row slice"""
    return [(L2_TM * T + L2_WAVE_ROWS * w, L2_TM * T + L2_WAVE_ROWS * w + 15) for T in tiles for w in waves if L2_TM * T + L2_WAVE_ROWS * w + 15 < nt]


def make_case(nq, nt, dim, pairs, seed, ties=(), norms=None):
    """Unit-norm filler rows and queries; per (f, l) of `pairs` two planted queries that share the rows f and l: query A has row f at
    |e| = 0.1 and row l at 0.2, query B has row l at 0.1 and row f at 0.2 (t[f] = c, t[l] = c - e1 + e2, A = c - e1, B = c + e2, e1 and e2
    orthogonal where dim allows). A pair with f == l plants one query at 0.1. `ties`: (lo, hi) row pairs, hi an exact copy of lo at 0.1 from
    a query of its own. `norms` (lo, hi): every row, query and planted group is scaled by a factor drawn log-uniformly from that range.
    dim == 1: filler rows are 1 + 0.01 * (a permutation), filler queries -(0.5 + 0.003 i): every distance is distinct; dim < 16: planted
    groups sit at radius 3, away from the unit sphere that 3-D filler rows cover densely. As many pairs are planted as nq has room for.
    -> dict q, t (float32), planted [(query, nearest row, second row or -1)], planted_q, ties [(query, lo, hi)]"""
    rng = np.random.default_rng(seed)
    if dim == 1:
        t = (1.0 + 0.01 * rng.permutation(nt))[:, None].astype(np.float64)
        q = -(0.5 + 0.003 * rng.permutation(nq))[:, None].astype(np.float64)
    else:
        t, q = _unit(rng, nt, dim), _unit(rng, nq, dim)
    if norms is not None:
        t *= np.exp(rng.uniform(np.log(norms[0]), np.log(norms[1]), size=(nt, 1)))
        q *= np.exp(rng.uniform(np.log(norms[0]), np.log(norms[1]), size=(nq, 1)))
    slots = query_slots(nq)
    planted, tie_list = [], []
    radius = 1.0 if dim >= 16 else 3.0
    for f, l in pairs:
        if not slots:
            break
        s = 1.0 if norms is None else float(np.exp(rng.uniform(np.log(norms[0]), np.log(norms[1]))))
        c = (-(5.0 + len(planted)) * np.ones(1) if dim == 1 else radius * _unit(rng, 1, dim)[0])
        e1 = _offset(rng, dim, 0.1)
        e2 = _offset(rng, dim, 0.2, avoid=e1) if dim > 1 else np.array([-0.2])
        a = slots.pop(0)
        t[f], q[a] = s * c, s * (c - e1)
        if f == l:
            planted.append((a, f, -1))
            continue
        t[l] = s * (c - e1 + e2)
        planted.append((a, f, l))
        if slots:
            b = slots.pop(0)
            q[b] = s * (c + e2)
            planted.append((b, l, f))
    for lo, hi in ties:
        if not slots:
            break
        a = slots.pop(0)
        c = (-(40.0 + len(tie_list)) * np.ones(1) if dim == 1 else radius * _unit(rng, 1, dim)[0])
        t[lo] = c
        t[hi] = c
        q[a] = c - _offset(rng, dim, 0.1)
        tie_list.append((a, lo, hi))
    q, t = q.astype(np.float32), t.astype(np.float32)
    # a planted query whose tile has one row takes its second neighbour from the filler: name it, the cap holds for it too
    D = None
    for i, (a, near, second) in enumerate(planted):
        if second < 0 and nt > 1:
            D = d2_64(q[[a]], t)[0]
            planted[i] = (a, near, int(np.argsort(D, kind="stable")[1]))
    return {"q": q, "t": t, "planted": planted, "planted_q": np.array([p[0] for p in planted], np.int64), "ties": tie_list, "dim": dim}


TILE_NT = [1, 2, 15, 16, 17, 127, 128, 129, 128 * 3 - 1, 128 * 3, 128 * 3 + 1]
TILE_NQ = [1, 127, 128, 129, 300]
DIMS = [1, 3, 4, 63, 64, 65, 100, 127, 128]
SPLIT_NQ = 8200
SPLIT_NT = [128 * 17 - 1, 128 * 17, 128 * 17 + 1]
INDEX_BASES = [0, 1, 3_000_000_000]


def tile_case(nq, nt, dim=128):
    return make_case(nq, nt, dim, tile_pairs(nt), seed=0x4C32B000 + 1000 * nq + nt + dim)


def wave_case():
    return make_case(129, 300, 128, wave_pairs(300), seed=0x4C32B101)


def base_case():
    """4 tiles = 4 splits of one tile (2 query tiles): tile borders, a pair across the first and the last split, a tie across two splits"""
    nt = 128 * 3 + 1
    return make_case(129, nt, 128, [(128 * 3, 127), (128, 255), (256, 383)], seed=0x4C32B202, ties=[(130, 300)])


def split_case(nt):
    """8200 queries = 65 query tiles -> at most 8 splits; 17 or 18 train tiles -> 3 tiles per split, 6 splits, the last one shorter.
    Planted: first row of the last split / last row of the first split; the two ends of a middle split; equal rows in two splits."""
    t_tiles, splits, tps = split_plan(nt, SPLIT_NQ)
    first_of_last, last_of_first = (splits - 1) * tps * L2_TM, tps * L2_TM - 1
    pairs = [(first_of_last, last_of_first), (2 * tps * L2_TM, 3 * tps * L2_TM - 1), (nt - 1, 0)]
    return make_case(SPLIT_NQ, nt, 128, pairs, seed=0x4C32B300 + nt, ties=[(tps * L2_TM + 5, 4 * tps * L2_TM + 77)])


def split_case_checked_queries(case):
    """the queries of a split case that `accept` is run on: every planted and tie query and every 8th query (the float64 reference of all
    8200 x 2177 pairs would take longer than the rest of the suite's L2 tests together)"""
    extra = [p[0] for p in case["planted"]] + [c[0] for c in case["ties"]]
    return np.unique(np.concatenate([np.arange(0, len(case["q"]), 8), np.array(extra, np.int64)]))


def dim_case(dim):
    return make_case(130, 257, dim, tile_pairs(257), seed=0x4C32B400 + dim)


def scale_case():
    """Rows and planted groups with norms from 0.01 to 30 (log-uniform), filler queries from 0.01 to 1 (a query much longer than the rows
    it competes among has gaps below B, whatever the kernel); a zero query, two zero train rows, a query equal to a train row. The zero
    rows are at exactly |q|^2 from every query: where they are the reference's two nearest, decided against the third, the query is a tie
    (lower row first, equal distance bits); other queries with a zero row among their three nearest are left out of the filler share."""
    nt = 300
    case = make_case(130, nt, 128, tile_pairs(nt) + [(40, 200)], seed=0x4C32B500, norms=(0.01, 30.0))
    rng = np.random.default_rng(0x4C32B501)
    filler = np.setdiff1d(np.arange(130), case["planted_q"])
    case["q"][filler] = (_unit(rng, len(filler), 128) * np.exp(rng.uniform(np.log(0.01), np.log(1.0), size=(len(filler), 1)))).astype(np.float32)
    case["q"][77] = 0.0
    case["t"][[33, 160]] = 0.0
    case["q"][78] = case["t"][90]
    case["special"] = {"zero_query": 77, "zero_rows": (33, 160), "equal": (78, 90)}
    D, Bm = d2_64(case["q"], case["t"]), bound(case["q"], case["t"])
    case["excluded"] = []
    for i in filler:
        o = np.argsort(D[i], kind="stable")[:3]
        if tuple(o[:2]) == (33, 160) and D[i, o[2]] - D[i, 160] > Bm[i, o[2]] + Bm[i, 160]:
            case["ties"].append((int(i), 33, 160))
        elif 33 in o or 160 in o:
            case["excluded"].append(int(i))
    return case


# --- equal computed distances ------------------------------------------------------------------------------------------------------------------
EQ_NQ, EQ_NT = 64, 128 * 5 + 37
EQ_COPY_ROW0 = 520


def equal_case(group, dim=128):
    """64 queries; query i has `group` (4 or 8) rows q_i + 1e-6 N(0, 1) at rows 8 i + (4 if group == 4 and i odd else 0) + 0..group-1: rows
    128 tile + 16 wave + 4 kc + 0..3 belong to one lane, 8 rows to two neighbouring lanes. Row EQ_COPY_ROW0 + i is an exact copy of the
    second of them. `dim`: 128 or 64 (the same layout; at 64 the values pass through the 64-term chain).
    -> dict q, t, rows [64, group + 1] (the near-duplicates of every query, the copy last)"""
    assert group in (4, 8) and dim in SC_DIMS
    rng = np.random.default_rng((0x4C32B600 if dim == 128 else 0x4C64B600) + group)
    t, q = _unit(rng, EQ_NT, dim).astype(np.float32), _unit(rng, EQ_NQ, dim).astype(np.float32)
    rows = np.zeros((EQ_NQ, group + 1), np.int64)
    for i in range(EQ_NQ):
        r0 = 8 * i + (4 if group == 4 and i % 2 else 0)
        rows[i, :group] = r0 + np.arange(group)
        t[rows[i, :group]] = q[i] + (1e-6 * rng.normal(size=(group, dim))).astype(np.float32)
        rows[i, group] = EQ_COPY_ROW0 + i
        t[EQ_COPY_ROW0 + i] = t[r0 + 1]
    return {"q": q, "t": t, "rows": rows}


def expected_from_pair_values(F, rows, index_base=0):
    """F [nq, m] float32 computed values of the pairs (query i, rows[i, j]) -> the two smallest (F, row) of every query as keys [nq, 2]"""
    out = np.empty((len(F), 2), np.uint64)
    for i in range(len(F)):
        o = np.lexsort((rows[i], F[i]))[:2]
        out[i] = make_keys(F[i, o], rows[i, o], index_base)
    return out


# --- a numpy binary32 emulation of the kernel's formula -----------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two binary32 values is exact in binary64; the sum is rounded to binary64 and then to binary32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_norms(x):
    """row_norms_kernel: lane l accumulates the squares of elements l, l + 64, ...; six xor-shuffle steps; lane 0 holds the sum"""
    x = np.asarray(x, np.float32)
    n, dim = x.shape
    s = np.zeros((n, 64), np.float32)
    for i in range(dim):
        s[:, i % 64] = _fma32(x[:, i], x[:, i], s[:, i % 64])
    off = 32
    while off:
        s = (s + s[:, np.arange(64) ^ off]).astype(np.float32)
        off >>= 1
    return s[:, 0]


def emulate_pairs(q, t):
    """F of the pairs (q[i], t[i]): float32 [n]"""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    dot = np.zeros(len(q), np.float32)
    for i in range(q.shape[1]):
        dot = _fma32(t[:, i], q[:, i], dot)
    u = _fma32(np.full(len(q), -2.0, np.float32), dot, emulate_norms(t))
    return np.maximum((emulate_norms(q) + u).astype(np.float32), np.float32(0))


def emulate_matrix(q, t):
    """F of every pair: float32 [nq, nt]"""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    dot = np.zeros((len(q), len(t)), np.float32)
    for i in range(q.shape[1]):
        dot = _fma32(t[None, :, i], q[:, None, i], dot)
    u = _fma32(np.float32(-2.0) * np.ones_like(dot), dot, np.broadcast_to(emulate_norms(t)[None, :], dot.shape))
    return np.maximum((emulate_norms(q)[:, None] + u).astype(np.float32), np.float32(0))


# --- screen -------------------------------------------------------------------------------------------------------------------------------------
SCREEN_NQ = [47, 48, 49, 383, 384, 385]
SCREEN_NT = [2, 129, 8191, 8192, 8193, 140_000]
# per row length: the same small sizes and one at which the sample is longer than 8192 and shorter than nt (11776 of 140 000 at dim 128;
# 8448 of 100 000 at dim 64, where 100 x 100 000 x 64 is the largest product a test computes)
SCREEN_NT_BY_DIM = {128: SCREEN_NT, 64: SCREEN_NT[:-1] + [100_000]}
SCREEN_NT_LARGE = {dim: nts[-1] for dim, nts in SCREEN_NT_BY_DIM.items()}
_FILLER = {}


def _screen_filler(n, seed, dim=128):
    key = seed if dim == 128 else (seed, dim)
    if key not in _FILLER or len(_FILLER[key]) < n:
        _FILLER[key] = _unit(np.random.default_rng(seed if dim == 128 else 0x4C640000 + seed), max(n, 1000), dim).astype(np.float32)
    return _FILLER[key][:n]


def screen_pairs(nt, dim=128):
    """(f, l) row pairs that screen_case plants: the sample border (s - 1, s) (or the last two rows where the sample is the whole set), the
    tile ends, the divisor-16 border. dim 64 adds the rows that the SECOND staged piece of a thread carries: (63, 64), the border of
    ROWS_PER_PASS, and (127, 128), the tile's end, in the first tile (row 0 is then paired with the last row of the second tile, as row
    127 is taken), and a pair inside the last tile where it is partial: its first row and the middle one (at 8191 rows: row 63 of it)."""
    s = screen_sample_rows(nt)
    if dim == 128:
        pairs = [(0, nt - 1)] if nt <= 129 else [(s - 1, s) if s < nt else (nt - 2, nt - 1), (0, 127)]
    elif nt < 129:
        pairs = [(0, nt - 1)]
    elif nt == 129:
        pairs = [(0, 126), (63, 64), (127, 128)]
    else:
        pairs = [(s - 1, s) if s < nt else (nt - 2, nt - 1), (0, 255), (SC_ROWS_PER_PASS[64] - 1, SC_ROWS_PER_PASS[64]), (SC_TM - 1, SC_TM)]
    s16 = screen_sample_rows(nt, 16)
    if s16 < s < nt:
        pairs.append((s16 - 1, s16))
    if dim == 64 and nt > 129 and nt % SC_TM >= 2:
        last0 = nt // SC_TM * SC_TM
        pairs.append((last0, last0 + (nt - last0 - 1) // 2))
    return pairs


def screen_case(nq, nt, dim=128):
    """Unit filler (shared between the cases, never written to); planted pairs on the tile ends and on both candidate borders of the sample
    (the runtime's default divisor 12 and the 16 of earlier documents), at dim 64 also on the rows of the second staged piece
    (screen_pairs); a query whose second best inside the sample has exact copies outside it."""
    assert dim in SC_DIMS
    s = screen_sample_rows(nt)
    pairs = screen_pairs(nt, dim)
    case = {"dim": dim}
    rng = np.random.default_rng((0x4C32B700 if dim == 128 else 0x4C64B700) + nt + nq)
    t, q = _screen_filler(nt, 11, dim).copy(), _screen_filler(nq, 12, dim).copy()
    slots = query_slots(nq)
    planted, ties = [], []
    for f, l in pairs:
        c = _unit(rng, 1, dim)[0]
        e1 = _offset(rng, dim, 0.1)
        e2 = _offset(rng, dim, 0.2, avoid=e1)
        a, b = slots.pop(0), slots.pop(0)
        t[f], t[l], q[a], q[b] = c, c - e1 + e2, c - e1, c + e2
        planted += [(a, f, l), (b, l, f)]
    if nt - s >= 8:  # nearest and second inside the sample; copies of the second outside it: the lower row keeps rank 1 (at 8193 the
                     # one row outside the sample belongs to the pair above)
        c = _unit(rng, 1, dim)[0]
        e1 = _offset(rng, dim, 0.1)
        e2 = _offset(rng, dim, 0.2, avoid=e1)
        a = slots.pop(0)
        t[300], t[301], q[a] = c, c - e1 + e2, c - e1
        t[s + 5] = t[301]
        t[nt - 2] = t[301]
        ties.append((a, 300, 301, (s + 5, nt - 2)))
    case.update(q=q, t=t, planted=planted, planted_q=np.array([p[0] for p in planted], np.int64), ties=[], outside_copies=ties, sample=s)
    return case


def screen_case_checked_queries(case):
    """the queries of a large screen case that `accept` is run on: the planted ones and the one with copies outside the sample (among
    100 000 unit rows of 64 elements the filler's nearest neighbours lie closer together than 2 B too often for the 99 % cap)"""
    return np.unique(np.concatenate([case["planted_q"], np.array([c[0] for c in case["outside_copies"]], np.int64)]))


def bf16_round(x):
    """float32 -> the nearest bf16 value (ties to even) as float32"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


BESIDE_MIDPOINT = np.float32(1.0 + 2.0 ** -9)
ADV_QUERIES, ADV_RIVALS = 16, 6


ADV_PARAMS = {128: dict(a=0.12, b=0.02, gap0=6e-4, gap_step=2e-4, raised=3, seed=0x4C32B800),
              64: dict(a=0.12, b=0.02, gap0=3e-4, gap_step=1e-4, raised=1, seed=0x4C64B800)}


def adversarial_case(dim=128):
    """Every element is +-m (1 + 2^-9) with m a bf16 value: bf16 rounding takes every element to m, a relative error of -2^-9 each, all in
    the same direction, so q~.t~ = q.t / (1 + 2^-9)^2 exactly: the screen value of a row is too large by ~2^-7 q.t.
    Adversarial query (16 of them, each with its own random signs s): |q_i| = a on the first dim / 2 axes and b on the last dim / 2
    (a = 0.12, b = 0.02). Its true nearest row t0 = s * (b.., a..) and second t1 (t0 with three magnitudes one bf16 step up; one at dim 64)
    have every product q_i t_i > 0: their errors add up to ~2^-7 * 0.31 = 2.4e-3 (half of that at dim 64). Six rivals have magnitude c in
    pairs of axes with signs (+s, -s): q.r = 0 term by term, their screen value has no error; their norms are tuned (pairs at one bf16
    step above c) to put them 6e-4 .. 1.6e-3 FARTHER than t0 in truth (3e-4 .. 8e-4 at dim 64, where the error that must cover them is
    half as large), so the screen ranks all six BEFORE t0 and t1. Filler rows and queries: unit Gaussian, same element form. The
    parameters were fixed on the CPU (test_l2_border_inputs_cpu.py asserts what they must achieve), none against a device result.
    -> dict q, t, adv [(query, t0 row, t1 row, [rival rows])]"""
    P = ADV_PARAMS[dim]
    rng = np.random.default_rng(P["seed"])
    nq, nt, h = 50, 128 * 2 + 72, dim // 2
    form = lambda x: (bf16_round(np.asarray(x, np.float32)) * BESIDE_MIDPOINT).astype(np.float32)
    t, q = form(_unit(rng, nt, dim)), form(_unit(rng, nq, dim))
    a, b = bf16_round(np.float32(P["a"])), bf16_round(np.float32(P["b"]))
    step_a = np.float32(2.0 ** (np.floor(np.log2(a)) - 7))
    adv, row = [], 0
    s0 = rng.choice([-1.0, 1.0], size=dim).astype(np.float32)
    for i in range(ADV_QUERIES):
        # the queries' signs differ by flips of whole axis pairs: a rival of ANOTHER adversarial query then also has q.r = 0 term by term,
        # and is one more rival at the same distances, instead of landing anywhere within +-0.1 of them
        s = s0 * np.repeat(rng.choice([-1.0, 1.0], size=h), 2).astype(np.float32)
        qa = s * np.concatenate([np.full(h, a), np.full(h, b)]).astype(np.float32)
        m0 = np.concatenate([np.full(h, b), np.full(h, a)]).astype(np.float32)
        m1 = m0.copy()
        m1[h:h + P["raised"]] += step_a
        qi = 3 * i
        q[qi] = form(qa)
        t[row], t[row + 1] = form(s * m0), form(s * m1)
        d0 = float(d2_64(q[[qi]], t[[row]])[0, 0])
        qn = float((q[qi].astype(np.float64) ** 2).sum())
        rivals = []
        for k in range(ADV_RIVALS):
            target = d0 - qn + P["gap0"] + P["gap_step"] * k        # the rival's |r|^2: q.r = 0, so d^2 = |q|^2 + |r|^2
            c_lo = (np.array([np.sqrt(target / dim) / float(BESIDE_MIDPOINT)], np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)[0]
            c_hi = np.float32(c_lo + np.float32(2.0 ** (np.floor(np.log2(c_lo)) - 7)))
            lo2, hi2 = (float(c_lo) * float(BESIDE_MIDPOINT)) ** 2, (float(c_hi) * float(BESIDE_MIDPOINT)) ** 2
            n_hi = int(np.clip(np.ceil((target - dim * lo2) / (2 * (hi2 - lo2))), 0, h))
            mags = np.repeat(np.where(rng.permutation(h) < n_hi, c_hi, c_lo).astype(np.float32), 2)
            flip = np.repeat(rng.choice([-1.0, 1.0], size=h), 2).astype(np.float32) * np.tile(np.array([1.0, -1.0], np.float32), h)
            t[row + 2 + k] = form(s * flip * mags)
            rivals.append(row + 2 + k)
        adv.append((qi, row, row + 1, rivals))
        row += 2 + ADV_RIVALS
    return {"q": q, "t": t, "adv": adv, "dim": dim}


def screen_values(q, t):
    """float64 screen value |q|^2 + |t|^2 - 2 q~.t~ with q~, t~ rounded to bf16"""
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    return (q64 * q64).sum(1)[:, None] + (t64 * t64).sum(1)[None, :] - 2.0 * bf16_round(q).astype(np.float64) @ bf16_round(t).astype(np.float64).T


def screen_eps(q, t):
    """eps(q) of screen_theta_kernel in float64: 2 (2u + u^2) |q| Tmax + 2^-13 (|q|^2 + Tmax^2), u = 2^-8, Tmax the largest row norm"""
    qn = (q.astype(np.float64) ** 2).sum(1)
    tm = (t.astype(np.float64) ** 2).sum(1).max()
    u = 2.0 ** -8
    return 2.0 * (2.0 * u + u * u) * np.sqrt(qn) * np.sqrt(tm) + (qn + tm) * 2.0 ** -13


def emulate_screen(q, t, eps_scale=1.0, whole_set_s2=False, drop_second_piece=False, exact=None):
    """The screen in numpy: float64 screen values -> s2 of the sample -> rows with S <= s2 + 2 eps -> their exact values re-ranked.
    `exact`: the float32 [nq, nt] values of the exact kernel (default: emulate_matrix). Three mistakes for the CPU test to reject:
    eps_scale = 0 (no margin); whole_set_s2 (the second smallest screen value of ALL rows as the threshold, no margin: what a sample's
    s2 is not); drop_second_piece (rows 64..127 of every tile never become candidates: the second staged piece at dim 64).
    -> (keys [nq, 2], candidates per query)"""
    S = screen_values(q, t)
    n_s = len(t) if whole_set_s2 else screen_sample_rows(len(t))
    s2 = np.sort(S[:, :n_s], axis=1)[:, 1]
    theta = s2 + (0.0 if whole_set_s2 else 2.0 * eps_scale) * screen_eps(q, t)
    cand = S <= theta[:, None]
    if drop_second_piece:
        cand[:, np.arange(len(t)) % SC_TM >= 64] = False
    F = (emulate_matrix(q, t) if exact is None else exact).copy()
    F[~cand] = np.inf
    return topk_keys(F, 2), float(cand.sum(1).mean())
