"""GPU: Hamming k-NN for 3 <= k <= 8 on the FP4 matrix cores (hamming_mfma_topk_kernel, backend 3 of apds_dev_hamming_topk_backend).
Every comparison is exact: integer keys (distance << 32 | row), ties to the lower train row, -1 where fewer than k rows exist.
What a K-entry list per lane can get wrong and a two-entry list could not - more than K equal rows spread over the four row groups of
a 16-row block, over tiles, over splits, over the threshold sample's border - is planted on purpose; the expected values come from a
numpy popcount with a stable argsort that shares no text with the oracle or the kernels."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HM_TM = 128          # train rows per tile of the matrix-core kernels
HM_Q_TOPK = 256      # queries per workgroup of hamming_mfma_topk_kernel (8 waves x 2 column blocks x 16)
KMAX_DEFAULT = 8     # APDS_MATCH_MFMA_KMAX when the environment does not set it (csrc/runtime.cpp)
EMPTY = np.int64(-1)
_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)


def _rows(rng, n):
    r = rng.integers(0, 256, (n, 61), dtype=np.uint8)
    r[:, 60] &= 0x3F
    return r


def _flipped(row, nbits, seed):
    r = row.copy()
    for b in np.random.default_rng(seed).choice(480, nbits, replace=False):
        r[b >> 3] ^= 1 << (b & 7)
    return r


def _numpy_topk_keys(q, db, k, base=0):
    """Brute force: popcount(xor) by table, stable argsort = ties to the lower row; keys as the library writes them."""
    out = np.full((len(q), k), EMPTY, np.int64)
    m = min(k, len(db))
    for lo in range(0, len(q), 16):
        d = _POP[q[lo:lo + 16, None, :] ^ db[None, :, :]].sum(2, dtype=np.int64)
        order = np.argsort(d, axis=1, kind="stable")[:, :m]
        out[lo:lo + 16, :m] = (np.take_along_axis(d, order, axis=1) << 32) | (order + base)
    return out


def _idx_dist(keys):
    idx = np.where(keys == EMPTY, -1, keys & 0xFFFFFFFF).astype(np.int32)
    dist = np.where(keys == EMPTY, 0x7FFFFFFF, keys >> 32).astype(np.int32)
    return idx, dist


def _pad64(a):
    return np.ascontiguousarray(np.concatenate([a, np.zeros((len(a), 64 - a.shape[1]), np.uint8)], 1))


def _backend_keys(gpu_pkg, q, db, k, backend, base=0):
    """apds_dev_hamming_topk_backend on host rows (61 or 64 bytes wide) -> [nq, k] int64 keys."""
    import torch
    L, check = gpu_pkg.lib(), gpu_pkg._lib.check
    dev = torch.device("cuda:0")
    dq, dt = torch.from_numpy(_pad64(q)).to(dev), torch.from_numpy(_pad64(db)).to(dev)
    out = torch.full((len(q), k), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    check(L.apds_dev_hamming_topk_backend(dq.data_ptr(), len(q), dt.data_ptr(), len(db), base, k, out.data_ptr(), backend, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _shapes(k):
    return [(5, 1, 1000), (5, 2, 1000), (5, k - 1, 0),                                   # fewer rows than k
            (HM_Q_TOPK - 1, HM_TM - 1, 1000), (HM_Q_TOPK, HM_TM, 1000), (HM_Q_TOPK + 1, HM_TM + 1, 7),   # tile borders, rows and queries
            (777, 3 * HM_TM + 5, 1000),
            (3000, 40000, 1000),                                                         # several splits, no threshold launch
            (700, 65536 + 127, 1000),                                                    # threshold launch; the rest is not a whole tile
            (2500, 70000, 0), (300, 300000, 123456)]


@pytest.mark.parametrize("k", [3, 4, 5, 7, 8])
def test_backend_3_gives_the_vector_kernels_keys(gpu_pkg, k):
    """apds_dev_hamming_topk_backend: 1 = xor + popcount on the vector ALU, 3 = the matrix cores, in ONE process on the same device buffers:
    every key identical, empty slots included. On the commit before this kernel existed the call with backend 3 returns APDS_ERR_ASSERT
    (-215: "backend: 0 default, 1 vector ALU, 2 matrix cores (k <= 2)")."""
    import torch
    L, check = gpu_pkg.lib(), gpu_pkg._lib.check
    dev = torch.device("cuda:0")
    for nq, nt, base in _shapes(k):
        g = torch.Generator(device=dev)
        g.manual_seed(nq * 7919 + nt + k)
        db = torch.randint(0, 256, (nt, 64), dtype=torch.uint8, device=dev, generator=g)
        q = torch.randint(0, 256, (nq, 64), dtype=torch.uint8, device=dev, generator=g)
        for t in (db, q):
            t[:, 60] &= 0x3F
            t[:, 61:] = 0
        m = min(nq, nt, 500)
        q[:m] = db[torch.randint(0, nt, (m,), device=dev, generator=g)]
        if nt >= 2000:
            db[nt // 2: nt // 2 + 300] = db[:300]                 # duplicate rows: ties
            db[nt - 20: nt] = db[5]                               # a run of twenty equal rows at the very end (the last, partial tile)
        outs = []
        for backend in (1, 3):
            out = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()   # the library call runs on the library's own stream: torch's writes above must have landed
            check(L.apds_dev_hamming_topk_backend(q.data_ptr(), nq, db.data_ptr(), nt, base, k, out.data_ptr(), backend, None))
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy())
        diff = int((outs[0] != outs[1]).sum())
        print(f"k {k} nq {nq} nt {nt} base {base}: {diff} keys differ")
        assert np.array_equal(outs[0], outs[1]), (nq, nt, base)
        assert (outs[1] != -7).all()
        if nt < k:
            assert (outs[1][:, nt:] == -1).all() and (outs[1][:, :nt] != -1).all()
    # a named backend refuses what it cannot do
    big = torch.empty((4, 9), dtype=torch.int64, device=dev)
    assert L.apds_dev_hamming_topk_backend(q.data_ptr(), 4, db.data_ptr(), nt, 0, 9, big.data_ptr(), 3, None) == -215
    assert L.apds_dev_hamming_topk_backend(q.data_ptr(), 4, db.data_ptr(), nt, 0, 3, big.data_ptr(), 2, None) == -215


@pytest.mark.parametrize("k", [1, 2])
def test_backend_3_runs_the_top2_kernel_for_small_k(gpu_pkg, k):
    rng = np.random.default_rng(k)
    db, q = _rows(rng, 5000), _rows(rng, 300)
    q[:100] = db[rng.integers(0, 5000, 100)]
    assert np.array_equal(_backend_keys(gpu_pkg, q, db, k, 3, 9), _backend_keys(gpu_pkg, q, db, k, 2, 9))


@pytest.mark.parametrize("k", [3, 4, 5, 8])
def test_knn_match_against_a_numpy_popcount(gpu_pkg, k):
    """The anchor of tests/test_match_gpu.py widened to k columns: through feature_extraction.knn_match (the default route) and on
    the matrix cores by name."""
    rng = np.random.default_rng(21 + k)
    db, q = _rows(rng, 3000), _rows(rng, 700)
    q[:200] = db[rng.integers(0, 3000, 200)]                 # exact hits
    db[1500:1600] = db[100:200]                              # duplicate rows: ties between rows 100.. and 1500..
    db[2500:2600] = db[100:200]
    q[200:260] = db[100:160]
    q[260:300, 7] ^= 0x11                                    # near misses of random rows
    want = _numpy_topk_keys(q, db, k)
    wi, wd = _idx_dist(want)
    idx, dist = gpu_pkg.feature_extraction.knn_match(q, db, k)
    assert np.array_equal(dist, wd) and np.array_equal(idx, wi)
    assert np.array_equal(_backend_keys(gpu_pkg, q, db, k, 3), want)
    assert (idx[200:260, 1] == idx[200:260, 0] + 1400).all() and (idx[200:260, 2] == idx[200:260, 0] + 2400).all()


@pytest.mark.parametrize("k", [4, 8])
def test_against_the_oracle_on_150000_rows(gpu_pkg, oracle_mod, k):
    """Threshold launch on (150 000 rows: a 9 344-row sample, then the rest): default route and backend 3 against oracle.knn_hamming."""
    db = gpu_pkg.synth.make_descriptor_db(150000, seed=199 + k)
    db[1000] = db[10]
    db[100000] = db[10]
    q, _ = gpu_pkg.synth.make_queries(db, 700, seed=15 + k)
    q[0] = db[10]
    oracle_mod.set_threads(8)
    oi, od = oracle_mod.knn_hamming(q, db, k)
    idx, dist = gpu_pkg.feature_extraction.knn_match(q, db, k)
    assert np.array_equal(dist, od) and np.array_equal(idx, oi)
    bi, bd = _idx_dist(_backend_keys(gpu_pkg, q, db, k, 3))
    assert np.array_equal(bd, od) and np.array_equal(bi, oi)
    assert tuple(idx[0, :3]) == (10, 1000, 100000)


def _tie_case(nt, seed, K):
    """A DB of nt random rows with, for one query each, more than K equal rows (or the rows named) placed where a K-entry list per lane, the
    fold over the four lanes of a query column, the split merge or the threshold launch could lose one or keep the wrong one."""
    rng = np.random.default_rng(seed)
    db, qs = _rows(rng, nt), []
    n_eq = K + 3
    sample = 0 if nt < 65536 else min(16384, nt // 16 // HM_TM * HM_TM)

    def query():
        qs.append(_rows(rng, 1)[0])
        return qs[-1]

    # (a) the four row groups of one 16-row block (lane group kq holds rows 4 kq .. 4 kq + 3 of it): rows 0 4 8 12 1 5 9 13 2 6 10 of a block
    q = query()
    twin = _flipped(q, 6, seed + 1)
    block = 16 * 37
    for r in sorted([0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10][:n_eq]):
        db[block + r] = twin
    # ... and the whole block equal, K < 16: the first K rows of it
    q = query()
    db[16 * 50: 16 * 51] = _flipped(q, 4, seed + 2)
    # (b) different tiles
    q = query()
    twin = _flipped(q, 7, seed + 3)
    for t in range(n_eq):
        db[HM_TM * (3 + 2 * t) + 7 + t] = twin
    # (c) different splits: over the whole index range, the last row included
    q = query()
    twin = _flipped(q, 5, seed + 4)
    for r in np.linspace(11, nt - 1, n_eq).astype(np.int64):
        db[r] = twin
    # (e) an exact copy of the query after K worse rows (same lane group, then a later tile)
    q = query()
    for j in range(K):
        db[16 * (70 + j) + 1] = _flipped(q, 3, seed + 10 + j)
    db[16 * (70 + K) + 1] = q
    db[min(nt - 2, 30000)] = q
    # the distance range: an all-zero and an all-ones (486 bits) query, with an all-zero and an all-ones row in the DB
    ones = np.full(61, 0xFF, np.uint8)
    ones[60] = 0x3F
    qs.append(np.zeros(61, np.uint8))
    qs.append(ones)
    db[200], db[201] = 0, ones
    if sample:
        # (d) both sides of the sample / rest border with the K-th place contested: K - 1 better rows and the K-th inside the sample, equal
        # rows in the rest (its first row, a row later on, the last row): the sample's row must keep the K-th place
        q = query()
        for j in range(K - 1):
            db[1000 + 17 * j] = _flipped(q, 2, seed + 20 + j)
        kth = _flipped(q, 9, seed + 30)
        for r in (sample - 300, sample, sample + 5000, nt - 1):
            db[r] = kth
        # a run of equal rows straddling the border: the last four of the sample, the first seven of the rest
        q = query()
        db[sample - 4: sample + 7] = _flipped(q, 8, seed + 31)
        # equal rows in the rest only, better than everything in the sample
        q = query()
        twin = _flipped(q, 3, seed + 32)
        for r in np.linspace(sample + 1, nt - 3, n_eq).astype(np.int64):
            db[r] = twin
    return db, np.stack(qs)


@pytest.mark.parametrize("nt", [4000, 40000, 90000])   # two tiles per split | twenty | a threshold launch (a 5 504-row sample) in front
@pytest.mark.parametrize("k", [3, 4, 7, 8])
def test_ties_in_a_k_entry_list(gpu_pkg, k, nt):
    K = 4 if k <= 4 else 8
    db, q = _tie_case(nt, 1000 * k + nt % 977, K)
    q = np.concatenate([q, _rows(np.random.default_rng(3), 300)])      # (more than one workgroup's worth of query columns in flight)
    want = _numpy_topk_keys(q, db, k, 77)
    got = _backend_keys(gpu_pkg, q, db, k, 3, 77)
    bad = np.nonzero((got != want).any(1))[0]
    print(f"k {k} nt {nt}: queries that differ: {bad[:10].tolist()}")
    assert np.array_equal(got, want)
    assert np.array_equal(_backend_keys(gpu_pkg, q, db, k, 1, 77), want)
    idx, dist = gpu_pkg.feature_extraction.knn_match(q, db, k)           # the default route
    wi, wd = _idx_dist(_numpy_topk_keys(q, db, k))
    assert np.array_equal(idx, wi) and np.array_equal(dist, wd)
    assert dist[5].min() == 0 and dist[5].max() <= 486 and dist[6].max() <= 486 and (dist[5, 0], dist[6, 0]) == (0, 0)


def _launches(L, check, name):
    ms, n = C.c_float(0), C.c_int(0)
    check(L.apds_dev_last_kernel_ms(name, C.byref(ms), C.byref(n)))
    return n.value


def test_the_default_route_runs_the_new_kernel(gpu_pkg):
    """With timing on, a default apds_dev_hamming_topk(k = 4) records its main launch under "hamming_topk_mfma_k" (and under
    "hamming_topk", like every main match launch) when the matrix cores serve the match and APDS_MATCH_MFMA_KMAX >= 4; k = 9 never does."""
    import torch
    L, check = gpu_pkg.lib(), gpu_pkg._lib.check
    dev = torch.device("cuda:0")
    mc = C.c_int(-1)
    check(L.apds_dev_match_backend(C.byref(mc)))
    kmax = int(os.environ.get("APDS_MATCH_MFMA_KMAX", KMAX_DEFAULT))
    rng = np.random.default_rng(4)
    db, q = torch.from_numpy(_pad64(_rows(rng, 70000))).to(dev), torch.from_numpy(_pad64(_rows(rng, 500))).to(dev)
    check(L.apds_dev_timing_enable(1))
    try:
        _launches(L, check, b"hamming_topk_mfma_k"), _launches(L, check, b"hamming_topk")      # (drain what earlier calls left)
        for k, nt in ((4, 70000), (4, 3000), (8, 70000), (3, 3000)):
            out = torch.empty((500, k), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            check(L.apds_dev_hamming_topk(q.data_ptr(), 500, db.data_ptr(), nt, 0, k, out.data_ptr(), None))
            torch.cuda.synchronize()
            n_k, n_all = _launches(L, check, b"hamming_topk_mfma_k"), _launches(L, check, b"hamming_topk")
            print(f"k {k} nt {nt}: matrix cores {mc.value}, KMAX {kmax}: {n_k} launches as hamming_topk_mfma_k, {n_all} as hamming_topk")
            assert n_k == (1 if mc.value == 1 and k <= kmax else 0) and n_all >= 1
        for k in (9, 2):
            out = torch.empty((500, k), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            check(L.apds_dev_hamming_topk(q.data_ptr(), 500, db.data_ptr(), 70000, 0, k, out.data_ptr(), None))
            torch.cuda.synchronize()
            assert _launches(L, check, b"hamming_topk_mfma_k") == 0 and _launches(L, check, b"hamming_topk") >= 1
    finally:
        check(L.apds_dev_timing_enable(0))


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_k4_equals_the_unsharded_vector_keys(gpu_pkg, world):
    """Threads as ranks over the loopback transport (the choreography of tests/cpp/shard_loopback_test.cpp), k = 4: every rank's keys for its
    own queries, and the replicated form's keys on every rank, equal apds_dev_hamming_topk_backend(backend 1) over the unsharded rows -
    with a run of seven equal rows straddling every shard border."""
    L, check, lib_mod = gpu_pkg.lib(), gpu_pkg._lib.check, gpu_pkg._lib
    k, nt = 4, 6000
    rng = np.random.default_rng(50 + world)
    db = _rows(rng, nt)
    queries = [_rows(rng, n) for n in (300, 257, 100)[:world]]
    for r in range(1, world):
        border = r * nt // world
        twin = _flipped(queries[0][r], 5, r)
        db[border - 3: border + 4] = twin
    for qr in queries:
        qr[10:60] = db[rng.integers(0, nt, 50)]
    want = [_backend_keys(gpu_pkg, qr, db, k, 1) for qr in queries]
    for r in range(1, world):
        border = r * nt // world
        assert (want[0][r] & 0xFFFFFFFF).tolist() == [border - 3, border - 2, border - 1, border]
    db64 = _pad64(db)
    cid = lib_mod.CommId()
    check(L.apds_comm_id_create(lib_mod.TRANSPORT_LOOPBACK, C.byref(cid)))
    got, rep, errors = [None] * world, [None] * world, []

    def rank_main(rank):
        try:
            check(L.apds_set_device(0))
            lo, hi = rank * nt // world, (rank + 1) * nt // world
            q64, q0 = _pad64(queries[rank]), _pad64(queries[0])
            bufs, hosts = [], []

            def dev_buf(nbytes, host=None):
                p = C.c_void_p()
                check(L.apds_dev_alloc(nbytes + 64, C.byref(p)))
                bufs.append(p)
                if host is not None:
                    hosts.append(host)                           # (the upload is asynchronous: the rows stay alive until the rank is done)
                    check(L.apds_dev_upload(p, host.ctypes.data, host.nbytes, None))
                return p
            rows = dev_buf((hi - lo) * 64, np.ascontiguousarray(db64[lo:hi]))
            dq, dq0 = dev_buf(q64.nbytes, q64), dev_buf(q0.nbytes, q0)
            dk, dr = dev_buf(len(q64) * k * 8), dev_buf(len(q0) * k * 8)
            check(L.apds_stream_synchronize(None))
            shard = C.c_void_p()
            check(L.apds_shard_create(C.byref(shard), rank, world, lib_mod.TRANSPORT_LOOPBACK, C.byref(cid), None, rows, hi - lo, lo))
            check(L.apds_shard_knn(shard, dq, len(q64), None, k, dk, None))
            keys = np.zeros((len(q64), k), np.int64)
            check(L.apds_dev_download(keys.ctypes.data, dk, keys.nbytes, None))
            got[rank] = keys
            check(L.apds_shard_knn_replicated(shard, dq0, len(q0), -1, k, dr, None))
            keys0 = np.zeros((len(q0), k), np.int64)
            check(L.apds_dev_download(keys0.ctypes.data, dr, keys0.nbytes, None))
            rep[rank] = keys0
            check(L.apds_shard_destroy(shard))
            for p in bufs:
                check(L.apds_dev_release(p))
            check(L.apds_thread_release())
        except Exception as e:   # noqa: BLE001 - reported by the main thread
            errors.append((rank, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not errors and not any(t.is_alive() for t in threads), errors
    for r in range(world):
        assert np.array_equal(got[r], want[r]), ("rank", r)
        assert np.array_equal(rep[r], want[0]), ("replicated form, rank", r)


def test_keypoint_table_view_k4(gpu_pkg):
    """apds_db_knn_match with k = 4 on a selection == knn_match on the downloaded selection == the numpy anchor (before this change the
    call returned APDS_ERR_ASSERT: "k in {1,2}")."""
    fd = gpu_pkg.feature_database
    rng = np.random.default_rng(8)
    n = 5000
    kp = np.zeros(n, gpu_pkg._lib.KEYPOINT_DTYPE)
    kp["x"], kp["y"] = rng.random(n).astype(np.float32) * 512, rng.random(n).astype(np.float32) * 512
    kp["size"], kp["response"] = 4.8, (rng.random(n) * 0.05 + 0.001).astype(np.float32)
    d = _rows(rng, n)
    d[3000:3006] = d[17]

    class Ex:
        keypoints, descriptors = kp, d
    t = fd.KeypointTable(2 * n)
    try:
        t.create_keypoints(Ex, 1, 0)
        rows = t.read_keypoints_from_lod(0)
        assert len(rows) == n
        q = _rows(rng, 400)
        q[:100] = d[rng.integers(0, n, 100)]
        q[0] = d[17]
        for k in (4, 3, 8, 11):
            idx, dist = t.knn_match_view(q, k)
            ki, kd = gpu_pkg.feature_extraction.knn_match(q, rows.descriptors, k)
            wi, wd = _idx_dist(_numpy_topk_keys(q, rows.descriptors, k))
            assert np.array_equal(idx, ki) and np.array_equal(dist, kd)
            assert np.array_equal(idx, wi) and np.array_equal(dist, wd)
            assert (dist[0, :min(k, 7)] == 0).all()
    finally:
        t.close()
