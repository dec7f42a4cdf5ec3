"""GPU: apds_dev_l2_ratio_filter (csrc/match_filter.hip) on the keys of apds_dev_l2_topk against get_knn_matches_l2, record for record:
query order, train index, distance = sqrtf(d^2) bit for bit, kept iff d0 < d1 * filter_strength in f32 with both keys present.

nq in 1, 1023, 1024, 1025 (SCAN_BLOCK = 1024 queries per block of the ordered compaction); a train set of exactly two rows; one of a
single row (every second key empty: no matches, where the host front raises for want of a second neighbour); a planted exact tie
d0 == d1 * fs (duplicate rows, fs = 1.0: dropped, the test is strict); fs = 0 and fs above 1."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM = 64


class Dev:
    def __init__(self, pkg):
        import torch
        self.torch, self.pkg = torch, pkg
        self.pl = import_module(pkg.__name__ + ".pipeline")
        self.L, self.check = pkg.lib(), pkg._lib.check
        self.stream = torch.cuda.Stream()      # the C ABI reads torch's default stream (handle 0) as "the thread's own": work on an explicit one

    def keys(self, q, t):
        torch = self.torch
        dq, dt = torch.from_numpy(q).to("cuda:0"), torch.from_numpy(t).to("cuda:0")
        out = torch.empty((len(q), 2), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            self.check(self.L.apds_dev_l2_topk(dq.data_ptr(), len(q), dt.data_ptr(), len(t), DIM, 0, 2, out.data_ptr(), self.pl.torch_stream()))
        torch.cuda.synchronize()
        return out

    def filtered(self, keys, fs):
        with self.torch.cuda.stream(self.stream):
            m = self.pl.dev_l2_ratio_filter(keys, fs)
        self.torch.cuda.synchronize()
        return m.cpu().numpy().view(self.pkg._lib.DMATCH_DTYPE).reshape(-1)


@pytest.fixture(scope="module")
def dev(gpu_pkg):
    return Dev(gpu_pkg)


def same_records(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in ("query_idx", "train_idx", "img_idx"):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(got["distance"].view(np.uint32), want["distance"].view(np.uint32))


@pytest.mark.parametrize("nq", [1, 1023, 1024, 1025])
def test_equals_get_knn_matches_l2(dev, nq):
    fe = dev.pkg.feature_extraction
    t, q, _ = dev.pkg.synth.make_l2_set(3000, nq, dim=DIM, seed=0x4C32F000 + nq, planted=0.5)
    keys = dev.keys(q, t)
    kept = []
    for fs in (0.0, 0.5, 0.8, 1.0, 1.5):
        want = fe.get_knn_matches_l2(q, t, 2, fs)
        same_records(dev.filtered(keys, fs), want)
        kept.append(len(want))
    assert kept[0] == 0 and kept[-1] == nq                            # fs = 0 keeps nothing; above 1 every query (d0 <= d1, d1 > 0)
    assert nq == 1 or 0 < kept[2] < nq                                # 0.8 really selects


def test_two_rows_and_one_row(dev):
    fe = dev.pkg.feature_extraction
    t, q, _ = dev.pkg.synth.make_l2_set(2, 1025, dim=DIM, seed=0x4C32F0A0)
    for fs in (0.8, 1.0, 1.2):
        same_records(dev.filtered(dev.keys(q, t), fs), fe.get_knn_matches_l2(q, t, 2, fs))
    keys = dev.keys(q, t[:1])                                           # one row: the second key of every query is empty
    assert (keys[:, 1] == -1).all() and (keys[:, 0] != -1).all()
    for fs in (0.8, 1e30):
        assert len(dev.filtered(keys, fs)) == 0
    with pytest.raises(dev.pkg.ApdsError):                              # (the host front has no second neighbour to compare)
        fe.get_knn_matches_l2(q, t[:1], 2, 0.8)


def test_exact_tie_is_dropped(dev):
    fe = dev.pkg.feature_extraction
    t, q, _ = dev.pkg.synth.make_l2_set(1500, 1025, dim=DIM, seed=0x4C32F0B0, planted=0.5)
    t[700] = t[3]                                                       # duplicate rows: queries near row 3 see d0 == d1
    q[10] = t[3] + np.float32(0.01)
    q[1024] = t[3]                                                      # the row itself: d0 == d1, zero up to the rounding of |q|^2 + |t|^2 - 2 q.t
    keys = dev.keys(q, t)
    k = keys.cpu().numpy()
    for i in (10, 1024):
        assert k[i, 0] >> 32 == k[i, 1] >> 32 and [int(k[i, 0] & 0xFFFFFFFF), int(k[i, 1] & 0xFFFFFFFF)] == [3, 700]
    got = dev.filtered(keys, 1.0)
    same_records(got, fe.get_knn_matches_l2(q, t, 2, 1.0))
    assert 10 not in got["query_idx"] and 1024 not in got["query_idx"] and len(got) >= 1000
    above = dev.filtered(keys, 1.0000001)                               # the next f32 above 1: a non-zero tie passes (d1 * fs rounds above d1)
    assert k[10, 0] >> 32 != 0 and 10 in above["query_idx"]
    same_records(above, fe.get_knn_matches_l2(q, t, 2, 1.0000001))


def test_contract(dev):
    L, lib = dev.L, dev.pkg._lib
    n = C.c_int(-1)
    assert L.apds_dev_l2_ratio_filter(None, 4, 1, 0.8, None, C.byref(n), None) == lib.ERR_OUT_OF_RANGE     # as apds_dev_ratio_filter: k >= 2
    assert L.apds_dev_l2_ratio_filter(None, 4, 2, 0.8, None, None, None) == lib.ERR_BAD_ARG
    assert L.apds_dev_l2_ratio_filter(None, 0, 2, 0.8, None, C.byref(n), None) == 0 and n.value == 0
