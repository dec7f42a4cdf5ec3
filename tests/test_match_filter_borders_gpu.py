"""GPU: csrc/match_filter.hip at its borders, through the device entry points apds_dev_ratio_filter and apds_dev_cross_check on hand-built
u64 keys: the ratio test cell by cell on the grid of all distance pairs, the rows it must not read, the three-kernel ordered compaction at
and beyond the 1024 blocks its offsets kernel scans per trip, and the cross-check scatter under contention. Exact equality with the numpy
references of filter_border_cases.py (pinned to the oracle by test_filter_border_inputs_cpu.py), match records and count; every output buffer
ends in guard records that must come back untouched."""
import ctypes as C

import numpy as np
import pytest

import filter_border_cases as bc

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def dev(gpu_pkg):
    import torch
    return torch, torch.device("cuda:0"), gpu_pkg._lib.lib(), gpu_pkg._lib.check


def _upload(dev, keys):
    torch, d = dev[0], dev[1]
    return torch.from_numpy(np.ascontiguousarray(keys).view(np.int64)).to(d)


def _out(dev, nq):
    torch, d = dev[0], dev[1]
    out = torch.full((nq + GUARD, 4), SENTINEL, dtype=torch.int32, device=d)
    torch.cuda.synchronize()                      # the library runs on a stream of its own
    return out


def _compare(dev, out, n, want):
    dev[0].cuda.synchronize()
    got = out.cpu().numpy()
    assert n == len(want)
    assert np.array_equal(got[:n].copy().view(bc.DMATCH_DTYPE).ravel(), want)
    assert (got[n:] == SENTINEL).all()            # nothing written behind the matches, the guard records included


def _ratio(dev, tkeys, nq, K, fs, want):
    L, check = dev[2], dev[3]
    out, n = _out(dev, nq), C.c_int(-1)
    check(L.apds_dev_ratio_filter(tkeys.data_ptr(), nq, K, float(fs), out.data_ptr(), C.byref(n), None))
    _compare(dev, out, n.value, want)


@pytest.fixture(scope="module")
def grid(dev):
    keys = bc.ratio_grid_keys()
    return keys, _upload(dev, keys)


@pytest.mark.parametrize("fs", bc.RATIO_FS, ids=bc.RATIO_FS_IDS)
def test_ratio_grid(dev, grid, fs):
    """Every pair (d0, d1) of 0..512: `d0 < d1 * fs` with one f32 product. The subnormal fs passes d0 = 0 against every d1 > 0 only where f32
    denormals are not flushed."""
    keys, tkeys = grid
    _ratio(dev, tkeys, len(keys), 2, fs, bc.ratio_reference(keys, 2, fs))


@pytest.mark.parametrize("K", bc.RATIO_STRUCTURE_K)
@pytest.mark.parametrize("nq", bc.RATIO_STRUCTURE_NQ)
def test_ratio_structure(dev, nq, K):
    """Only columns 0 and 1 of K are read; a missing first or second neighbour fails the row; train indices 0 and 2^31 - 1 come through."""
    keys = bc.ratio_structure_keys(nq, K)
    _ratio(dev, _upload(dev, keys), nq, K, bc.RATIO_STRUCTURE_FS, bc.ratio_reference(keys, K, bc.RATIO_STRUCTURE_FS))


@pytest.mark.parametrize("pattern", bc.FLAG_PATTERNS)
@pytest.mark.parametrize("nq", bc.COMPACTION_NQ)
def test_compaction_sizes(dev, nq, pattern):
    """scan_flags_device + the emit kernel under the ratio entry: from one flag to 2 * 1024^2 + 1025 of them (2050 blocks: three trips of the
    offsets kernel's loop, the last for two blocks)."""
    keys = bc.compaction_keys(bc.flag_pattern(pattern, nq))
    _ratio(dev, _upload(dev, keys), nq, 2, 1.0, bc.ratio_reference(keys, 2, 1.0))


_CROSS_CHECK = bc.cross_check_cases()


@pytest.mark.parametrize("name", sorted(_CROSS_CHECK))
def test_cross_check(dev, name):
    L, check = dev[2], dev[3]
    train_best, nq = _CROSS_CHECK[name]
    tb = _upload(dev, train_best)
    out, n = _out(dev, nq), C.c_int(-1)
    check(L.apds_dev_cross_check(tb.data_ptr(), len(train_best), nq, out.data_ptr(), C.byref(n), None))
    _compare(dev, out, n.value, bc.cross_check_reference(train_best, nq))
