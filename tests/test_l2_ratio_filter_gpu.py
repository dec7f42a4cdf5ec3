"""GPU: apds_dev_l2_ratio_filter (csrc/match_filter.hip) on the keys of apds_dev_l2_topk against get_knn_matches_l2, record for record:
query order, train index, distance = sqrtf(d^2) bit for bit, kept iff d0 < d1 * filter_strength in f32 with both keys present.

nq in 1, 1023, 1024, 1025 (SCAN_BLOCK = 1024 queries per block of the ordered compaction); a train set of exactly two rows; one of a
single row (every second key empty: no matches, where the host front raises for want of a second neighbour); a planted exact tie
d0 == d1 * fs (duplicate rows, fs = 1.0: dropped, the test is strict); fs = 0 and fs above 1.
test_keys_built_by_hand needs no matcher: d^2 bit patterns a matcher rarely produces (zero, subnormal, beside perfect squares, the ends of
the exponent range) with the second key placed beside d0 / fs^2, against the host rule restated in numpy."""
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


def hand_made_d2_bits():
    """uint32 bit patterns of d^2: 0, the smallest and the largest subnormal, the smallest normal; n^2 and its binary32 neighbours for n in
    1..64 (where a root that is one ulp off shows: the exact root is representable); 2^e and its neighbours for e = -126, -119 .. 126 (odd
    and even exponents alternate); the largest finite value; 4096 random positive finite patterns"""
    f = lambda x: int(np.float32(x).view(np.uint32))
    bits = [0, 1, 0x007FFFFF, 0x00800000]
    for n in range(1, 65):
        bits += [f(n * n) - 1, f(n * n), f(n * n) + 1]
    for e in range(-126, 127, 7):
        b = f(2.0 ** e)
        bits += [b - 1, b, b + 1] if e > -126 else [b, b + 1]          # (below 2^-126: the largest subnormal, listed above)
    bits.append(0x7F7FFFFF)
    bits += np.random.default_rng(0x4C32F0C0).integers(1, 0x7F800000, 4096).tolist()
    return np.array(bits, np.uint32)


@pytest.mark.parametrize("k", [2, 3])
def test_keys_built_by_hand(dev, k):
    """4097 queries per call; the key stride is k (the third key of k = 3 is never read). Expected: distance = the correctly rounded binary32
    root of the key's d^2; kept iff both keys are present and root(d0) < float32(root(d1) * float32(fs)) - get_knn_matches_l2's rule."""
    torch, NQ = dev.torch, 4097
    d0 = hand_made_d2_bits()
    root = lambda bits: np.sqrt(bits.view(np.float32))
    r64 = np.sqrt(d0.view(np.float32).astype(np.float64)).astype(np.float32)
    assert np.array_equal(root(d0).view(np.uint32), r64.view(np.uint32))           # numpy's binary32 root is the float64 root rounded once
    n = np.arange(1, 65)
    assert np.array_equal(root((n * n).astype(np.float32).view(np.uint32)), n.astype(np.float32))
    rng = np.random.default_rng(0x4C32F0C1 + k)
    seen = {"kept": 0, "dropped": 0, "equal": 0, "subnormal_product": 0}
    for fs in (0.5, 0.8, 1.0, 1.25, 2.0 ** -60):
        fs32 = np.float32(fs)
        with np.errstate(over="ignore"):
            beside = np.minimum(d0.view(np.float32).astype(np.float64) / (float(fs32) * float(fs32)), float(np.finfo(np.float32).max)).astype(np.float32).view(np.uint32)
        a = np.repeat(d0, 3).astype(np.int64)
        b = np.clip(np.repeat(beside, 3).astype(np.int64) + np.tile(np.array([-1, 0, 1]), len(d0)), 0, 0x7F7FFFFF)
        for start in range(0, len(a), NQ):
            idx = np.arange(start, start + NQ) % len(a)                            # (the last batch wraps round to the first pairs)
            keys = np.empty((NQ, k), np.uint64)
            low = rng.integers(0, 1 << 32, (NQ, k), dtype=np.uint64)
            keys[:, 0] = (a[idx].astype(np.uint64) << np.uint64(32)) | low[:, 0]
            keys[:, 1] = (b[idx].astype(np.uint64) << np.uint64(32)) | low[:, 1]
            if k == 3:
                keys[:, 2] = rng.integers(0, 1 << 63, NQ, dtype=np.uint64)
            keys[5::7, 1] = np.uint64(0xFFFFFFFFFFFFFFFF)                          # no second neighbour
            keys[11::97, :2] = np.uint64(0xFFFFFFFFFFFFFFFF)                       # no neighbour at all
            present = (keys[:, 0] != np.uint64(0xFFFFFFFFFFFFFFFF)) & (keys[:, 1] != np.uint64(0xFFFFFFFFFFFFFFFF))
            r0 = root((keys[:, 0] >> np.uint64(32)).astype(np.uint32))
            with np.errstate(invalid="ignore"):
                r1 = root((keys[:, 1] >> np.uint64(32)).astype(np.uint32))         # (nan where the key is empty: not present)
                product = (r1.astype(np.float64) * float(fs32)).astype(np.float32)  # exact in binary64, rounded once: the binary32 product, subnormal results included
                keep = present & (r0 < product)
            want = np.zeros(int(keep.sum()), dev.pkg._lib.DMATCH_DTYPE)
            want["query_idx"] = np.flatnonzero(keep)
            want["train_idx"] = (keys[keep, 0] & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
            want["distance"] = r0[keep]
            dk = torch.from_numpy(keys.view(np.int64)).to("cuda:0")
            torch.cuda.synchronize()
            same_records(dev.filtered(dk, fs), want)
            seen["kept"] += int(keep.sum())
            seen["dropped"] += int((present & ~keep).sum())
            seen["equal"] += int((present & (r0 == product)).sum())
            seen["subnormal_product"] += int((present & (product > 0) & (product < np.finfo(np.float32).tiny)).sum())
    print(f"k = {k}: {seen}")
    assert min(seen.values()) > 0, seen                                           # both sides of the test, exact equality, a subnormal product


def test_contract(dev):
    L, lib = dev.L, dev.pkg._lib
    n = C.c_int(-1)
    assert L.apds_dev_l2_ratio_filter(None, 4, 1, 0.8, None, C.byref(n), None) == lib.ERR_OUT_OF_RANGE     # as apds_dev_ratio_filter: k >= 2
    assert L.apds_dev_l2_ratio_filter(None, 4, 2, 0.8, None, None, None) == lib.ERR_BAD_ARG
    assert L.apds_dev_l2_ratio_filter(None, 0, 2, 0.8, None, C.byref(n), None) == 0 and n.value == 0
