"""GPU: the resident L2 train set (apds_l2_train_*, csrc/l2_screen.hip) - apds_dev_l2_train_top2 in screen mode against the keys of
apds_dev_l2_topk(k = 2) on the same rows, np.array_equal, at dim 64 (the M-SURF length: two k-steps, 160-byte LDS rows, two staged pieces per
thread) and dim 128.

Sizes: nt in 2, 127, 128, 129 (the 128-row tile), 8191, 8192, 8193 (the sample floor) and 20001 (more than one split: 157 tiles over the
512-block target); nq in 1, 15, 16, 17 (a 16-query column block), 383, 384, 385 (Q = 384 queries per block at both lengths: three column
blocks per wave) and 511, 512, 513 (a block and a third; the sizes of a four-block build, Q = 512, that was measured, found slower and
removed: kept as sizes). With at most 20001 rows a block of pass B sees at most 128 rows, fewer than the 192 candidates per query its
region holds: the candidate buffer cannot overflow here, so the screen must have run wherever the handle is screen_ready and the query
pointer aligned. The structural borders of the screen (sample, staged pieces, adversarial rounding, overflow, index bases) are in
test_l2_train_borders_gpu.py."""
import ctypes as C
import gc
from importlib import import_module

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EXACT, SCREEN = 0, 1
NTS = [2, 127, 128, 129, 8191, 8192, 8193, 20001]
NQS = [1, 15, 16, 17, 383, 384, 385, 511, 512, 513]
NQ_MAX = max(NQS)


class Dev:
    def __init__(self, pkg):
        import torch
        self.torch, self.pkg = torch, pkg
        self.pl = import_module(pkg.__name__ + ".pipeline")
        self.L, self.check = pkg.lib(), pkg._lib.check
        self.stream = torch.cuda.Stream()      # the C ABI reads torch's default stream (handle 0) as "the thread's own": work on an explicit one

    def up(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        self.torch.cuda.synchronize()
        return t

    def topk(self, dq, dt, index_base=0):
        """apds_dev_l2_topk(k = 2): the keys every case is compared with"""
        out = self.torch.empty((dq.shape[0], 2), dtype=self.torch.int64, device="cuda:0")
        with self.torch.cuda.stream(self.stream):
            self.check(self.L.apds_dev_l2_topk(dq.data_ptr(), dq.shape[0], dt.data_ptr(), dt.shape[0], dt.shape[1], index_base, 2, out.data_ptr(), self.pl.torch_stream()))
        self.torch.cuda.synchronize()
        return out.cpu().numpy()

    def top2(self, ts, dq, mode="screen"):
        with self.torch.cuda.stream(self.stream):
            out = ts.top2(dq, mode)
        self.torch.cuda.synchronize()
        return out.cpu().numpy(), ts.mode_used, ts.candidates_per_query


@pytest.fixture(scope="module")
def dev(gpu_pkg):
    return Dev(gpu_pkg)


def rows_of(synth, kind, nt, dim):
    """(train [nt, dim], queries [NQ_MAX, dim]) float32"""
    rng = np.random.default_rng(0x4C3264 + 131 * nt + dim + len(kind))
    if kind == "unit":                      # unit rows, 30 % of the queries a row + noise
        t, q, _ = synth.make_l2_set(nt, NQ_MAX, dim=dim, seed=0x4C326400 + nt)
        return t, q
    if kind == "gauss":                     # raw Gaussian rows, norms log-uniform in 0.01 .. 30
        t = rng.standard_normal((nt, dim))
        t *= (np.exp(rng.uniform(np.log(0.01), np.log(30.0), nt)) / np.linalg.norm(t, axis=1))[:, None]
        q = t[rng.integers(0, nt, NQ_MAX)] * (1.0 + 0.02 * rng.standard_normal((NQ_MAX, dim)))
        q[::3] = rng.standard_normal((len(q[::3]), dim)) * rng.uniform(0.01, 4.0, (len(q[::3]), 1))
        return t.astype(np.float32), q.astype(np.float32)
    assert kind == "dup"                    # every row about ten times: exact ties everywhere, decided by the lower row
    base = rng.standard_normal((max(1, nt // 10), dim)).astype(np.float32)
    t = base[rng.integers(0, len(base), nt)]
    q = base[rng.integers(0, len(base), NQ_MAX)].copy()
    q[1::2] += (0.01 * rng.standard_normal((len(q[1::2]), dim))).astype(np.float32)
    return np.ascontiguousarray(t), q


@pytest.mark.parametrize("kind", ["unit", "gauss", "dup"])
@pytest.mark.parametrize("dim", [64, 128])
def test_screen_keys_equal_the_exact_keys(dev, dim, kind):
    for nt in NTS:
        t, q = rows_of(dev.pkg.synth, kind, nt, dim)
        dt, dq = dev.up(t), dev.up(q)
        want = dev.topk(dq, dt)
        ts = dev.pl.L2TrainSet(dt)
        try:
            assert ts.info() == (nt, dim, True)
            for nq in NQS:
                got, used, _ = dev.top2(ts, dq[:nq])
                assert used == "screen", (nt, nq)                     # (fails on a tree without the dim-64 screen)
                assert np.array_equal(got, want[:nq]), (nt, nq, np.flatnonzero((got != want[:nq]).any(1))[:8])
            got, used, _ = dev.top2(ts, dq, "exact")                  # the handle's exact path: its own norms
            assert used == "exact" and np.array_equal(got, want), nt
        finally:
            ts.close()


@pytest.mark.parametrize("dim", [64, 128])
def test_index_base(dev, dim):
    base = 1 << 20
    t, q = rows_of(dev.pkg.synth, "unit", 8193, dim)
    dt, dq = dev.up(t), dev.up(q[:385])
    want = dev.topk(dq, dt, base)
    assert (want & 0xFFFFFFFF).min() >= base
    ts = dev.pl.L2TrainSet(dt, index_base=base)
    try:
        got, used, _ = dev.top2(ts, dq)
        assert used == "screen" and np.array_equal(got, want)
    finally:
        ts.close()


def test_zero_rows_among_queries_and_train_rows(dev):
    # M-SURF gives an all-zero descriptor for a flat patch
    t, q = rows_of(dev.pkg.synth, "unit", 8193, 64)
    t[[0, 77, 8192]] = 0
    q[[0, 5, 384]] = 0
    dt, dq = dev.up(t), dev.up(q)
    want = dev.topk(dq, dt)
    ts = dev.pl.L2TrainSet(dt)
    try:
        got, used, _ = dev.top2(ts, dq)                               # (either mode may have run)
        assert used in ("screen", "exact") and np.array_equal(got, want)
        assert [int(k & 0xFFFFFFFF) for k in got[0]] == [0, 77]       # the zero query's nearest: the zero rows, lower row first
    finally:
        ts.close()


@pytest.mark.parametrize("dim", [64, 128])
def test_misaligned_query_pointer_runs_the_exact_kernel(dev, dim):
    t, q = rows_of(dev.pkg.synth, "unit", 8193, dim)
    q = q[:385]
    flat = dev.torch.zeros(q.size + 1, dtype=dev.torch.float32, device="cuda:0")
    flat[1:] = dev.up(q).reshape(-1)
    dq = flat[1:].view(q.shape[0], dim)                                # 4 bytes past a 16-byte boundary
    assert dq.data_ptr() % 16 == 4
    dt = dev.up(t)
    want = dev.topk(dev.up(q), dt)
    ts = dev.pl.L2TrainSet(dt)
    try:
        got, used, cpq = dev.top2(ts, dq)
        assert used == "exact" and cpq == 0 and np.array_equal(got, want)
    finally:
        ts.close()


def test_unsupported_dim_and_single_row(dev):
    t, q = rows_of(dev.pkg.synth, "unit", 2000, 32)
    dt, dq = dev.up(t), dev.up(q[:100])
    ts = dev.pl.L2TrainSet(dt)
    try:
        assert ts.info() == (2000, 32, False)
        got, used, _ = dev.top2(ts, dq)
        assert used == "exact" and np.array_equal(got, dev.topk(dq, dt))
    finally:
        ts.close()
    t, q = rows_of(dev.pkg.synth, "unit", 2, 64)
    d1, dq = dev.up(t[:1]), dev.up(q[:17])
    ts = dev.pl.L2TrainSet(d1)                                         # one row: no second neighbour, no screen
    try:
        assert ts.info() == (1, 64, False)
        got, used, _ = dev.top2(ts, dq)
        assert used == "exact" and np.array_equal(got, dev.topk(dq, d1)) and (got[:, 1] == -1).all()
    finally:
        ts.close()
    L, BAD = dev.L, dev.pkg._lib.ERR_BAD_ARG
    assert L.apds_l2_train_info(None, None, None, None) == BAD
    assert L.apds_dev_l2_train_top2(None, dq.data_ptr(), 17, SCREEN, None, None, None, None) == BAD
    ts = dev.pl.L2TrainSet(dev.up(t))
    try:
        assert L.apds_dev_l2_train_top2(ts._h, dq.data_ptr(), 17, 2, None, None, None, None) == BAD
    finally:
        ts.close()


def test_two_hundred_calls_do_not_grow_the_workspace(dev):
    torch = dev.torch
    t, q = rows_of(dev.pkg.synth, "unit", 20001, 64)
    dt, dq = dev.up(t), dev.up(q)
    ts = dev.pl.L2TrainSet(dt)
    out = torch.empty((NQ_MAX, 2), dtype=torch.int64, device="cuda:0")
    try:
        with torch.cuda.stream(dev.stream):
            for mode in ("screen", "exact", "screen"):                # the thread's workspace has been through both paths
                ts.top2(dq, mode, out=out)
        torch.cuda.synchronize()
        first = out.cpu().numpy().copy()
        gc.collect()                                                  # (earlier tests' objects give their device memory back now, not in between)
        torch.cuda.synchronize()
        info = dev.pkg._lib.workspace_info
        slabs0, free0 = info(), torch.cuda.mem_get_info()[0]
        with torch.cuda.stream(dev.stream):
            for i in range(200):
                ts.top2(dq, "exact" if i % 50 == 49 else "screen", out=out)
        torch.cuda.synchronize()
        assert info() == slabs0 and slabs0[0] > 0                     # the thread's workspace: not a byte, not an allocation
        assert abs(torch.cuda.mem_get_info()[0] - free0) < 4 << 20
        assert np.array_equal(out.cpu().numpy(), first)
    finally:
        ts.close()


def test_real_descriptors_of_a_frame_and_its_shifted_view(dev, capsys):
    fe, synth = dev.pkg.feature_extraction, dev.pkg.synth
    tile = synth.make_tile(352, 640, frame_index=31)
    a = fe.akaze_keypoint_descriptor_extraction(tile, descriptor="kaze")
    b = fe.akaze_keypoint_descriptor_extraction(np.roll(tile, (13, 29), axis=(0, 1)).copy(), descriptor="kaze")
    qa, tb = np.ascontiguousarray(a.descriptors, np.float32), np.ascontiguousarray(b.descriptors, np.float32)
    assert qa.shape[1] == 64 and len(qa) >= 50 and len(tb) >= 50
    dq, dt = dev.up(qa), dev.up(tb)
    want = dev.topk(dq, dt)
    ts = dev.pl.L2TrainSet(dt)
    try:
        got, used, cpq = dev.top2(ts, dq)
        with capsys.disabled():
            print(f"\n[l2 train set] M-SURF rows: {len(qa)} queries x {len(tb)} train rows, candidates per query {cpq:.2f}")
        assert used == "screen" and np.array_equal(got, want) and cpq >= 2.0
    finally:
        ts.close()
