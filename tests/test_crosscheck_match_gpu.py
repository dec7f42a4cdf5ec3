"""GPU: apds_dev_crosscheck_match - get_bruteforce_matches (BFMatcher(NORM_HAMMING, crossCheck = true), lib.rs:116-126) on device rows -
against the CPU oracle, match list for match list, distance included.

The scan behind it is roles-swapped: the TRAIN rows are the searching side (register columns of the matrix-core kernel: 48 per wave, 384 per
workgroup), the queries are streamed in 128-row tiles. The sizes sit on those borders. The tie cases are built by hand: duplicate train
rows (the lower one wins its query), duplicate queries (the train row chooses the lower one), a train row halfway between two queries,
queries nobody chooses. Both backends: the matrix cores here, the vector ALU in a child process started with APDS_MATCH_MFMA=0."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SENTINEL = 16, 0x5A5A5A5A
N_TRAIN = [1, 2, 47, 48, 49, 383, 384, 385, 4097]
N_QUERY = [1, 127, 128, 129, 300]
# a sparse product: every value of both lists appears, the tile borders of one side meet the column borders of the other
SIZES = [(1, 1), (127, 2), (128, 47), (129, 48), (300, 49), (1, 383), (127, 384), (128, 385), (129, 4097), (300, 4097), (300, 384), (129, 383), (128, 1)]
assert {q for q, _ in SIZES} == set(N_QUERY) and {t for _, t in SIZES} == set(N_TRAIN)


def rows_for(nq, nt, seed):
    """61-byte descriptors: random train rows; half of the queries are train rows with a few bits flipped, the rest random"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (nt, 61), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, 61), dtype=np.uint8)
    for i in range(0, nq, 2):
        q[i] = t[rng.integers(0, nt)]
        q[i, rng.integers(0, 61, 3)] ^= np.uint8(1) << rng.integers(0, 8, 3).astype(np.uint8)
    return q, t


def tie_case(name):
    rng = np.random.default_rng(77)
    t = rng.integers(0, 256, (500, 61), dtype=np.uint8)
    q = rng.integers(0, 256, (200, 61), dtype=np.uint8)
    if name == "duplicate_train_rows":          # rows 5, 140 (another tile column block), 499 are query 3: the lower train index wins
        t[5] = t[140] = t[499] = q[3]
        t[400] = t[20] = q[150]
    elif name == "duplicate_queries":           # queries 7, 130 (another tile), 199 are train row 11: it chooses the lower query
        q[7] = q[130] = q[199] = t[11]
        q[140] = q[2] = t[450]
    elif name == "equidistant_train_row":       # train row 9 is 2 bits from query 60 and 2 bits from query 10
        t[9] = q[10]
        t[9, 0] ^= 0x03
        q[60] = t[9]
        q[60, 1] ^= 0x03
    elif name == "queries_nobody_chooses":      # 200 queries, 30 train rows: at most 30 queries can be chosen
        t = t[:30].copy()
    elif name == "all_rows_equal":              # every pair at distance 0: train row r chooses query 0, query 0 keeps train row 0
        t[:] = q[0]
        q[:] = q[0]
    return q, t


TIES = ["duplicate_train_rows", "duplicate_queries", "equidistant_train_row", "queries_nobody_chooses", "all_rows_equal"]


def rows64(a):
    out = np.zeros((a.shape[0], 64), np.uint8)
    out[:, :a.shape[1]] = a
    return out


def dev_crosscheck(pkg, q, t, index_base=0):
    """-> (matches as DMATCH records, the raw output buffer with its guard rows)"""
    import torch
    L = pkg.lib()
    nq, nt = len(q), len(t)
    dq = torch.from_numpy(rows64(q)).to("cuda:0") if nq else None
    dt = torch.from_numpy(rows64(t)).to("cuda:0") if nt else None
    out = torch.full((nq + GUARD, 4), SENTINEL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    n = C.c_int(-1)
    pkg._lib.check(L.apds_dev_crosscheck_match(dq.data_ptr() if nq else None, nq, dt.data_ptr() if nt else None, nt, index_base, out.data_ptr(), C.byref(n), None))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert 0 <= n.value <= nq and (got[n.value:] == SENTINEL).all()       # nothing behind the matches
    return got[:n.value].copy().view(pkg._lib.DMATCH_DTYPE).ravel()


def same_matches(got, want, index_base=0):
    want = want.copy()
    want["train_idx"] += index_base
    assert len(got) == len(want), (len(got), len(want))
    assert got.tobytes() == want.tobytes()                                  # bit for bit, the f32 distance included


@pytest.fixture(scope="module")
def wanted(oracle_mod):
    """the oracle's answer of every case, computed once"""
    out = {}
    for nq, nt in SIZES:
        q, t = rows_for(nq, nt, 1000 * nq + nt)
        out[(nq, nt)] = (q, t, oracle_mod.get_bruteforce_matches(q, t))
    for name in TIES:
        q, t = tie_case(name)
        out[name] = (q, t, oracle_mod.get_bruteforce_matches(q, t))
    return out


@pytest.mark.parametrize("nq,nt", SIZES)
def test_sizes_at_the_kernel_borders(gpu_pkg, wanted, nq, nt):
    q, t, want = wanted[(nq, nt)]
    same_matches(dev_crosscheck(gpu_pkg, q, t), want)


@pytest.mark.parametrize("name", TIES)
def test_ties(gpu_pkg, wanted, name):
    q, t, want = wanted[name]
    got = dev_crosscheck(gpu_pkg, q, t)
    same_matches(got, want)
    by_q = {int(m["query_idx"]): (int(m["train_idx"]), float(m["distance"])) for m in got}
    if name == "duplicate_train_rows":
        assert by_q[3] == (5, 0.0) and by_q[150] == (20, 0.0)
    elif name == "duplicate_queries":
        assert by_q[7] == (11, 0.0) and 130 not in by_q and 199 not in by_q and by_q[2] == (450, 0.0) and 140 not in by_q
    elif name == "equidistant_train_row":
        assert by_q[10] == (9, 2.0) and by_q.get(60, (-1, 0.0))[0] != 9
    elif name == "queries_nobody_chooses":
        assert 0 < len(got) <= 30
    elif name == "all_rows_equal":
        assert len(got) == 1 and by_q[0] == (0, 0.0)


@pytest.mark.parametrize("key", [(129, 4097), (300, 49), "duplicate_train_rows"])
def test_index_base(gpu_pkg, wanted, key):
    q, t, want = wanted[key]
    same_matches(dev_crosscheck(gpu_pkg, q, t, 0), want, 0)
    same_matches(dev_crosscheck(gpu_pkg, q, t, 1000), want, 1000)


@pytest.mark.parametrize("key", [(300, 4097), (128, 385), "duplicate_queries"])
def test_equals_the_one_call_host_entry(gpu_pkg, wanted, key):
    q, t, _ = wanted[key]
    same_matches(dev_crosscheck(gpu_pkg, q, t), gpu_pkg.feature_extraction.get_bruteforce_matches(q, t))


def test_empty_sides_and_argument_errors(gpu_pkg):
    import torch
    L = gpu_pkg.lib()
    q, t = rows_for(5, 7, 1)
    assert len(dev_crosscheck(gpu_pkg, q[:0], t)) == 0
    assert len(dev_crosscheck(gpu_pkg, q, t[:0])) == 0
    assert len(dev_crosscheck(gpu_pkg, q[:0], t[:0])) == 0
    d = torch.zeros((8, 64), dtype=torch.uint8, device="cuda:0")
    out = torch.zeros((8, 4), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    n = C.c_int(-1)
    # a train side above INT_MAX is refused before anything is read (the rows behind the pointer do not exist)
    assert L.apds_dev_crosscheck_match(d.data_ptr(), 8, d.data_ptr(), (1 << 31), 0, out.data_ptr(), C.byref(n), None) == gpu_pkg._lib.ERR_ASSERT
    assert n.value == 0
    assert L.apds_dev_crosscheck_match(d.data_ptr(), -1, d.data_ptr(), 8, 0, out.data_ptr(), C.byref(n), None) == gpu_pkg._lib.ERR_ASSERT
    assert L.apds_dev_crosscheck_match(d.data_ptr(), 8, d.data_ptr(), 8, 0, out.data_ptr(), None, None) == gpu_pkg._lib.ERR_BAD_ARG
    assert L.apds_dev_crosscheck_match(None, 8, d.data_ptr(), 8, 0, out.data_ptr(), C.byref(n), None) == gpu_pkg._lib.ERR_BAD_ARG


def test_python_wrapper(gpu_pkg, wanted):
    import torch
    from importlib import import_module
    pl = import_module(gpu_pkg.__name__ + ".pipeline")
    q, t, want = wanted[(129, 383)]
    with torch.cuda.stream(torch.cuda.Stream("cuda:0")):
        m = pl.dev_crosscheck_match(torch.from_numpy(rows64(q)).to("cuda:0"), torch.from_numpy(rows64(t)).to("cuda:0"), index_base=7)
        got = m.cpu().numpy().view(gpu_pkg._lib.DMATCH_DTYPE).ravel()
    same_matches(got, want, 7)


def _digest(pkg, cases):
    return {str(k): dev_crosscheck(pkg, q, t).tobytes().hex() for k, (q, t) in cases.items()}


def _cases():
    out = {k: rows_for(k[0], k[1], 1000 * k[0] + k[1]) for k in SIZES}
    out.update({name: tie_case(name) for name in TIES})
    return out


def test_vector_backend_in_a_child_process(gpu_pkg, wanted):
    """every case again under APDS_MATCH_MFMA=0: the vector-ALU kernel serves the swapped scan"""
    be = C.c_int(-1)
    gpu_pkg._lib.check(gpu_pkg.lib().apds_dev_match_backend(C.byref(be)))
    assert be.value == 1                                  # this process ran the matrix cores
    env = dict(os.environ, APDS_MATCH_MFMA="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    there = json.loads(r.stdout.strip().splitlines()[-1])
    assert there["backend_mfma"] == 0
    for k, (q, t, want) in wanted.items():
        assert there["results"][str(k)] == want.tobytes().hex(), k


if __name__ == "__main__" and "--child" in sys.argv:
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the library: one HIP runtime)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg.lib()
    be = C.c_int(-1)
    pkg._lib.check(pkg.lib().apds_dev_match_backend(C.byref(be)))
    print(json.dumps({"backend_mfma": be.value, "results": _digest(pkg, _cases())}))
