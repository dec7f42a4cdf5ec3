"""GPU: the tile loop of the matrix-core Hamming matcher (hm_scan_tiles in csrc/hamming_mfma.hip) around its borders.

The loop reads a train tile from one LDS buffer while the LDS-DMA of the next tile fills the other, reads the first row block of the next
tile right behind the barrier at the end of a tile, and reads every block's operands one block ahead of its MFMAs. What that can get wrong
is silent: a block (or its popcounts) read before its DMA landed, or after the DMA of the tile after next overwrote it - distances of some
other tile's rows. So every query here has its exact copy planted in the first or in the last 16-row block of some tile (every tile gets
both), and the matrix-core backends (apds_dev_hamming_topk_backend 2: top-2 kernel, 3: the K = 4 / K = 8 kernel) are compared with the
vector-ALU backend (1) key for key, all queries, all columns, on shapes around the loop's borders:

  tiles per split   1, 2, 3, 7 (APDS_MATCH_MFMA_SPLITS=4 on 4, 8, 12, 28 tiles) and 121 behind a threshold launch of 8 per split
  n_train           128 m - 1, 128 m, 128 m + 1 for each of those m
  queries           never a multiple of 384 (top-2: 8 waves x 48) nor of 256 (K = 4 / 8: 8 waves x 32)
  threshold launch  without (n_train < 65 536) and with (n_train = 128 * 516 - 1, + 0, + 1: a 4 096-row sample, then the rest)
  plan              the fill model's own (in this process) and four forced splits (a child process: the switches are read once)
  empty splits      6 001 queries x 65 tiles: the fill model takes 13 splits, the XCD pinning rounds that to 16 (5 tiles each) - the
                    workgroups of splits 13 .. 15 have no tile and write empty lists

One run each; every comparison covers the whole key array."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HM_TM = 128
BORDER_TILES = (4, 8, 12, 28)          # x 4 forced splits: 1, 2, 3, 7 tiles per split
THRESHOLD_TILES = 516                  # 66 048 rows: a 32-tile sample, 484 tiles behind it (121 per forced split)
VARIANTS = ((2, 2), (3, 4), (3, 8))    # (backend, k): the top-2 kernel, the K = 4 and the K = 8 kernel


def _rows(rng, n):
    r = np.zeros((n, 64), np.uint8)
    r[:, :61] = rng.integers(0, 256, (n, 61), dtype=np.uint8)
    r[:, 60] &= 0x3F
    return r


def _case(nt, nq, seed):
    """nt random rows; query 2 t is a copy of a row of tile t's first 16-row block, query 2 t + 1 of a row of its last block (the last
    block that exists, for a partial last tile); the queries behind those are random rows with a near miss each."""
    rng = np.random.default_rng(seed)
    db, q = _rows(rng, nt), _rows(rng, nq)
    tiles = -(-nt // HM_TM)
    assert nq >= 2 * tiles and nq % 384 and nq % 256
    planted = np.empty(2 * tiles, np.int64)
    for t in range(tiles):
        lo, hi = t * HM_TM, min(nt, (t + 1) * HM_TM)
        last_block = lo + (hi - 1 - lo) // 16 * 16
        planted[2 * t] = lo + rng.integers(0, min(16, hi - lo))
        planted[2 * t + 1] = last_block + rng.integers(0, hi - last_block)
    q[: 2 * tiles] = db[planted]
    rest = np.arange(2 * tiles, nq)
    q[rest] = db[rng.integers(0, nt, len(rest))]
    q[rest, 7] ^= 0x11                                       # two bits off some row
    return db, q, planted


def _shapes():
    out = []
    for m in BORDER_TILES:
        for d in (-1, 0, 1):
            out.append((HM_TM * m + d, 2 * (m + 1) + 391))      # 401 .. 449 queries: two workgroups of either kernel, the last one partial
    for d in (-1, 0, 1):
        out.append((HM_TM * THRESHOLD_TILES + d, 2 * (THRESHOLD_TILES + 1) + 47))   # 1 081 queries
    return out


def _keys(pkg, dq, dt, nq, nt, k, backend):
    import torch
    L, check = pkg.lib(), pkg._lib.check
    out = torch.full((nq, k), -7, dtype=torch.int64, device=dq.device)
    torch.cuda.synchronize()
    check(L.apds_dev_hamming_topk_backend(dq.data_ptr(), nq, dt.data_ptr(), nt, 0, k, out.data_ptr(), backend, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _compare(pkg, shapes, variants=VARIANTS):
    """-> list of (nt, nq, backend, k, differing keys, planted rows missed); empty when everything agrees."""
    import torch
    dev = torch.device("cuda:0")
    bad = []
    for nt, nq in shapes:
        db, q, planted = _case(nt, nq, nt * 31 + nq)
        dq, dt = torch.from_numpy(q).to(dev), torch.from_numpy(db).to(dev)
        for backend, k in variants:
            want = _keys(pkg, dq, dt, nq, nt, k, 1)
            got = _keys(pkg, dq, dt, nq, nt, k, backend)
            diff = int((got != want).sum())
            missed = int((got[: len(planted), 0] != planted).sum())   # key = distance 0 << 32 | row
            print(f"nt {nt} nq {nq} backend {backend} k {k}: {diff} keys differ, {missed} planted rows missed", flush=True)
            if diff or missed or (got == -7).any():
                bad.append((nt, nq, backend, k, diff, missed))
    return bad


def test_tile_borders_on_the_fill_models_plan(gpu_pkg):
    assert _compare(gpu_pkg, _shapes()) == []


def test_empty_trailing_splits_of_an_xcd_pinned_plan(gpu_pkg):
    """16 query tiles x 65 train tiles: rounds x (tiles per split + 4) is least at 13 splits (one round, 5 tiles each) and as small at 16,
    so the multiple of eight is taken: splits 13, 14, 15 start behind the last tile. The K = 4 / K = 8 kernels get the same shape (their
    24 query tiles make their own plan)."""
    assert _compare(gpu_pkg, [(HM_TM * 65 - 3, 6001)]) == []


def test_tile_borders_with_four_forced_splits(gpu_pkg):
    """The same shapes in a child process with APDS_MATCH_MFMA_SPLITS=4 (and the XCD rounding off, which would overrule it on the long
    shape): 1, 2, 3, 7 and 121 tiles per split, the threshold launch's sample at 8."""
    env = dict(os.environ, APDS_MATCH_MFMA_SPLITS="4", APDS_MATCH_MFMA_XCD="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    print(r.stdout[-6000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"cases": 3 * len(_shapes()), "bad": []}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (first: see tests/conftest.py)
    import __graft_entry__ as graft
    package = graft.load_package()
    package.lib()
    failures = _compare(package, _shapes())
    print(json.dumps({"cases": 3 * len(_shapes()), "bad": failures}))
    sys.exit(1 if failures else 0)
