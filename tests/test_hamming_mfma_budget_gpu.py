"""GPU: the top-2 matrix-core Hamming kernel inside its 104-register budget computes the keys it computed outside it.

What the budget changed in hamming_mfma_kernel (csrc/hamming_mfma.hip): the LDS-DMA holds ONE per-lane source constant and derives the
other three pieces' (and the popcounts' lane offset) where it issues them, and the queries' popcounts are read in the epilogue, by the
lanes that write, instead of being carried across the tile loop. A wrong DMA constant shows as rows of a tile read from somewhere else; a
wrong popcount as distances off by a constant for some queries. So the matrix-core backend (apds_dev_hamming_topk_backend 2) is compared
with the vector-ALU backend (1) key for key on the smallest shapes around those borders:

  queries     1, 47, 49, 383, 385   the clamp of hm_load_operands (columns past the last query), the epilogue's reload at a wave's
                                    (48 queries) and a workgroup's (384) border
  train rows  2, 127, 129, 257      one partial tile, one row short of a tile, one row into the second and into the third: every DMA piece
                                    of a wave with rows and with padding behind it
  threshold   65 536 + 129 rows x 385 queries: a 4 096-row threshold launch (THR = false) and the main launch behind it (THR = true)

Ties everywhere: a third of the train rows are copies of five patterns, spread over all tiles (and, on the long shape, over both sides of
the sample's end), and the queries are copies of train rows, near misses of them and random rows - equal distances must keep the lower
row, in both kernels alike."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QUERY_COUNTS = (1, 47, 49, 383, 385)
TRAIN_ROWS = (2, 127, 129, 257)
LONG_SHAPE = (65536 + 129, 385)
EMPTY = -7   # what the output holds before a call: no key (distance < 2^10, row < 2^31) looks like it


def _rows(rng, n):
    r = np.zeros((n, 64), np.uint8)
    r[:, :61] = rng.integers(0, 256, (n, 61), dtype=np.uint8)
    r[:, 60] &= 0x3F
    return r


def _case(nt, nq, seed):
    rng = np.random.default_rng(seed)
    db = _rows(rng, nt)
    pool = _rows(rng, 5)
    copies = rng.random(nt) < 1 / 3
    copies[[0, nt - 1]] = True                                   # the first and the last row tie with rows between them
    db[copies] = pool[rng.integers(0, 5, int(copies.sum()))]
    q = _rows(rng, nq)
    kind = rng.integers(0, 4, nq)                                # 0: a pool pattern, 1: a copy of a row, 2: a near miss, 3: random
    src = rng.integers(0, nt, nq)
    q[kind == 0] = pool[rng.integers(0, 5, int((kind == 0).sum()))]
    q[kind == 1] = db[src[kind == 1]]
    q[kind == 2] = db[src[kind == 2]]
    q[kind == 2, 7] ^= 0x11
    return db, q


def _keys(pkg, dq, dt, nq, nt, base, backend):
    import torch
    L, check = pkg.lib(), pkg._lib.check
    out = torch.full((nq, 2), EMPTY, dtype=torch.int64, device=dq.device)
    torch.cuda.synchronize()
    check(L.apds_dev_hamming_topk_backend(dq.data_ptr(), nq, dt.data_ptr(), nt, base, 2, out.data_ptr(), backend, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _differences(pkg, nt, nq, base):
    """-> (keys that differ between the two backends, keys left unwritten, queries whose two keys tie in distance)"""
    import torch
    dev = torch.device("cuda:0")
    db, q = _case(nt, nq, 7919 * nt + nq)
    dq, dt = torch.from_numpy(q).to(dev), torch.from_numpy(db).to(dev)
    want = _keys(pkg, dq, dt, nq, nt, base, 1)
    got = _keys(pkg, dq, dt, nq, nt, base, 2)
    ties = int(((want[:, 0] >> 32) == (want[:, 1] >> 32)).sum())
    return int((got != want).sum()), int((got == EMPTY).sum()), ties


def test_keys_equal_the_vector_backends_at_query_and_tile_borders(gpu_pkg):
    bad, ties = [], 0
    for nt in TRAIN_ROWS:
        for nq in QUERY_COUNTS:
            diff, unwritten, t = _differences(gpu_pkg, nt, nq, base=1000 if nt == 129 else 0)
            print(f"nt {nt} nq {nq}: {diff} keys differ, {unwritten} unwritten, {t} queries with tied keys", flush=True)
            ties += t
            if diff or unwritten:
                bad.append((nt, nq, diff, unwritten))
    assert bad == []
    assert ties > 0   # (the cases are made to tie; a generator that stopped doing so would check less than it says)


def test_keys_equal_the_vector_backends_behind_a_threshold_launch(gpu_pkg):
    nt, nq = LONG_SHAPE
    diff, unwritten, ties = _differences(gpu_pkg, nt, nq, base=0)
    print(f"nt {nt} nq {nq}: {diff} keys differ, {unwritten} unwritten, {ties} queries with tied keys")
    assert (diff, unwritten) == (0, 0) and ties > 0
