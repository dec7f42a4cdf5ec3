"""GPU: apds_db_delete_ids / apds_db_delete_where on a FLOAT keypoint table (csrc/keypoint_delete.hip: the staging row is 10 + 64 + 6 dwords,
the chunk 2^18 rows), with a byte table put through the same deletes beside it. The expectation is db_float_cases.Model: the numpy table
with the victims removed - survivors keep their order and every bit of every column, ids included; the world points move with them.

Victims at rows 0, 1023, 1024 (TB = 1024 rows per block) and the last row; a deleted tail (nothing moves); every other row; a level of
detail and a region through apds_db_delete_where; with and
without current world points; ids go on after a delete and views select from the closed-up table. One case of 2 * 2^18 + 3 rows with
victims and survivors on both sides of both chunk borders, filled from device tensors and compared on the device."""
import numpy as np
import pytest

import db_float_cases as cases
from db_float_cases import Ex, Model, bits

pytestmark = pytest.mark.gpu

N = 2049
DGT = [9.0, 1e-4, 0, 57.0, 0, -1e-4]


def fresh(pkg, seed, room=64):
    """2049 rows over three images, the level of detail alternating every 50 rows; both tables with `room` free rows"""
    img = np.repeat([1, 2, 3], [700, 700, N - 1400])
    model = Model(cases.keypoints(pkg, N, seed), img, (np.arange(N) // 50) % 2, cases.unit_rows(N, seed + 1), cases.byte_rows(N, seed + 2))
    tf, tb = cases.make_tables(pkg, model, N + room)
    return model, tf, tb


def elevation(pkg):
    et = pkg.feature_database.ElevationTable()
    et.create_geotransform("dataset", DGT)
    return et


VICTIMS = {
    "borders": lambda n: np.isin(np.arange(n), [0, 1023, 1024, n - 1]),
    "tail": lambda n: np.arange(n) >= n - 300,
    "first": lambda n: np.arange(n) == 0,
    "block": lambda n: (np.arange(n) >= 1000) & (np.arange(n) < 1100),
    "odd": lambda n: np.arange(n) % 2 == 1,                    # every other row
}


@pytest.mark.parametrize("with_xyz", [False, True])
@pytest.mark.parametrize("which", sorted(VICTIMS))
def test_delete_ids(gpu_pkg, which, with_xyz):
    pkg = gpu_pkg
    model, tf, tb = fresh(pkg, 500)
    try:
        xyz = None
        if with_xyz:
            assert tf.world_coordinates(elevation(pkg)) == 0 and tb.world_coordinates(elevation(pkg)) == 0
            xyz = cases.Snapshot(pkg, tf, [1, 2, 3], [0, 1]).xyz
            assert xyz is not None and len(np.unique(xyz, axis=0)) > 100
        victims = VICTIMS[which](N)
        ids = model.ids[victims].copy()
        want = model.delete(victims)
        shuffled = np.random.default_rng(1).permutation(np.concatenate([ids, ids[:2], [N + 50, 0]]))     # duplicates and unknown ids
        assert tf.delete_keypoints(shuffled) == want and tb.delete_keypoints(shuffled) == want
        sf, sb = cases.assert_model(pkg, model, tf, tb, which)
        if with_xyz:
            assert sf.xyz is not None and sf.xyz.tobytes() == xyz[~victims].tobytes() and sb.xyz.tobytes() == sf.xyz.tobytes()
        else:
            assert sf.xyz is None and sb.xyz is None
    finally:
        tf.close()
        tb.close()


@pytest.mark.parametrize("with_xyz", [False, True])
def test_delete_where_then_insert_and_select(gpu_pkg, with_xyz):
    """a level of detail leaves (every second run of 50 rows), then a region; then rows are added: ids go on, and views read the closed-up table"""
    pkg = gpu_pkg
    model, tf, tb = fresh(pkg, 600)
    try:
        if with_xyz:
            tf.world_coordinates(elevation(pkg))
            tb.world_coordinates(elevation(pkg))
            xyz = cases.Snapshot(pkg, tf, [1, 2, 3], [0, 1]).xyz
        victims = model.lod == 1
        want = model.delete(victims)
        assert want > 900 and tf.delete_keypoints_from_lod(1) == want and tb.delete_keypoints_from_lod(1) == want
        sf, _ = cases.assert_model(pkg, model, tf, tb, "lod")
        if with_xyz:
            assert sf.xyz.tobytes() == xyz[~victims].tobytes()
            xyz = xyz[~victims]
        box = (50.0, 50.0, 300.0, 300.0)
        victims = model.mask(2, 0, box)
        want = model.delete(victims)
        assert want > 100
        assert tf.delete_keypoints_from_coordinates(*box, 0) == want and tb.delete_keypoints_from_coordinates(*box, 0) == want
        sf, _ = cases.assert_model(pkg, model, tf, tb, "box")
        if with_xyz:
            assert sf.xyz.tobytes() == xyz[~victims].tobytes()
        # ids continue behind the highest id ever given, whatever was deleted
        more = Model(cases.keypoints(pkg, 40, 601), np.full(40, 9), np.ones(40, np.int64), cases.unit_rows(40, 602), cases.byte_rows(40, 603))
        tf.create_keypoints(Ex(more.src_kp, more.desc_f), 9, 1)
        tb.create_keypoints(Ex(more.src_kp, more.desc_b), 9, 1)
        more.ids = np.arange(N + 1, N + 41, dtype=np.int32)
        for name in ("kp", "src_kp", "img", "lod", "desc_f", "desc_b", "ids"):
            setattr(model, name, np.concatenate([getattr(model, name), getattr(more, name)]))
        cases.assert_model(pkg, model, tf, tb, "insert after delete")
        # views and the table's own selection on the closed-up table
        vf, vb = tf.view(100), tb.view(100)
        try:
            for mode, value, bx in ((1, 0, None), (0, 9, None), (1, 1, None), (2, 0, (0.0, 0.0, 200.0, 400.0)), (0, 2, None)):
                w = model.select(mode, value, bx, limit=100)
                cases.check_views(pkg, model, vf, vb, cases.select(vf, mode, value, bx), cases.select(vb, mode, value, bx), w)
            old = tf.read_keypoints_from_image_id(9)
            w = model.select(0, 9)
            assert np.array_equal(old.ids, model.ids[w]) and np.array_equal(bits(old.descriptors), bits(model.desc_f[w]))
        finally:
            vf.close()
            vb.close()
    finally:
        tf.close()
        tb.close()


def test_delete_across_both_chunk_borders(gpu_pkg):
    """2 * 2^18 + 3 rows (134 MB of float rows) from device tensors; victims and survivors on both sides of rows 2^18 and 2^19; compared by
    torch.equal on the device, the table's columns read in place"""
    import torch
    from importlib import import_module
    pkg = gpu_pkg
    pl = import_module(pkg.__name__ + ".pipeline")
    C18 = 1 << 18
    n = 2 * C18 + 3
    g = torch.Generator(device="cuda:0").manual_seed(7)
    kps = torch.rand((n, 7), generator=g, device="cuda:0", dtype=torch.float32) + 1.0          # (every field read as bits; the lift at level 0 is v * 1 + 0)
    desc_f = torch.rand((n, 64), generator=g, device="cuda:0", dtype=torch.float32) - 0.5
    desc_b = torch.randint(0, 256, (n, 64), generator=g, device="cuda:0", dtype=torch.uint8)
    victims = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    rows = [0, 5, 1023, 1024, C18 - 2, C18 - 1, C18, C18 + 2, 2 * C18 - 1, 2 * C18, 2 * C18 + 2]
    victims[rows] = True
    victims[C18 - 700:C18 - 600] = True
    victims[2 * C18 - 50:2 * C18 - 10] = True
    keep = ~victims
    assert bool(keep[C18 - 3]) and bool(keep[C18 + 1]) and bool(keep[2 * C18 - 2]) and bool(keep[2 * C18 + 1])      # survivors beside every border
    ids = (torch.arange(n, device="cuda:0", dtype=torch.int32) + 1)
    victim_ids = ids[victims].cpu().numpy()
    torch.cuda.synchronize()
    fd = pkg.feature_database
    tf, tb = fd.KeypointTable(n, descriptor="kaze"), fd.KeypointTable(n)
    try:
        tf.create_keypoints_device(kps.data_ptr(), desc_f.data_ptr(), n, 7, 0)
        tb.create_keypoints_device(kps.data_ptr(), desc_b.data_ptr(), n, 7, 0)
        desc_b[:, 61:] = 0
        for t, desc, row_bytes, dtype in ((tf, desc_f, 256, torch.float32), (tb, desc_b, 64, torch.uint8)):
            assert t.delete_keypoints(victim_ids) == len(victim_ids)
            m = n - len(victim_ids)
            r, k, _, rows_now = t.device_table()
            assert rows_now == len(t) == m
            got_desc = pl._table_tensor(r, m * row_bytes, "cuda:0", dtype, (m, 64))
            got_kps = pl._table_tensor(k, m * 28, "cuda:0", torch.int32, (m, 7))
            assert torch.equal(got_desc.view(torch.uint8), desc[keep].view(torch.uint8)), row_bytes
            assert torch.equal(got_kps, kps[keep].view(torch.int32)), row_bytes
            assert np.array_equal(t.ids(), ids[keep].cpu().numpy()), row_bytes
            assert len(t.read_keypoints_from_image_id(8)) == 0
    finally:
        tf.close()
        tb.close()
