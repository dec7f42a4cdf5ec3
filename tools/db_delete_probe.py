#!/usr/bin/env python3
"""What a delete costs on a 1 M-row keypoint table, on one GPU, beside the only thing a table without deletes can do: build the resulting
table anew.

The table: 1000 images of --db-rows / 1000 rows each (device rows, apds_db_insert_batch_dev), levels of detail 0 and 1 in turn by groups
of 125 images, world points computed. Four deletes, each on a freshly filled table, --repeats times, medians of the wall time of the call
(it returns when the table is final):
  front / middle / tail : apds_db_delete_where mode 0 of image 2 / 500 / 1000 (about a thousand rows each)
  lod                   : apds_db_delete_where mode 1 of level of detail 1 (half the table, in four runs)
Beside each, in the same process and alternating with it, the baseline: the same surviving rows inserted into an empty table of the same
capacity by the same apds_db_insert_batch_dev calls (counts of the deleted images zero), alone and followed by the
apds_db_world_coordinates run a rebuilt table needs before it has world points again (a delete keeps them).

moved_bytes = survivors behind the first deleted row x 128 B (ten 4-byte columns, the 64-byte descriptor row, three doubles). The
compaction reads and writes them twice (table -> staging -> table) and scans a flag byte and the predicate's column per row:
traffic_bytes = 4 x moved_bytes + rows x 5 B (image id or level of detail read, the flag written; the gather's flag read, 1 B beside
512, is left out). hbm_fraction = traffic_bytes / time / 8 TB/s (the spec peak).

    python tools/db_delete_probe.py [--db-rows 1000000] [--repeats 7] [--out profiles/db_delete/db_delete_probe.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
ROW_BYTES = 128
IMAGES, GROUP = 1000, 125


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db-rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import __graft_entry__ as graft
    pkg = graft.load_package()
    L, check, ptr = pkg.lib(), pkg._lib.check, pkg._lib.ptr
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    check(L.apds_set_device(0))
    per = args.db_rows // IMAGES
    n = per * IMAGES

    g = torch.Generator(device=dev).manual_seed(3)
    kp = torch.rand((n, 7), generator=g, device=dev) * 256.0
    kp[:, 5:7] = 0
    desc = torch.randint(0, 256, (n, 64), generator=g, device=dev, dtype=torch.uint8)
    torch.cuda.synchronize()
    et = pkg.feature_database.ElevationTable()
    et.create_geotransform("dataset", [9.0, 1e-4, 0, 57.0, 0, -1e-4])
    cr = np.zeros((GROUP, 2), np.uint32)

    def fill(table, without_image=None, without_lod=None):
        """the 1000 images in groups of 125 (one call each, levels of detail 0, 1, 0, 1, ..); an image or a level of detail left out"""
        for gi in range(IMAGES // GROUP):
            lod = gi % 2
            if lod == without_lod:
                continue
            counts = np.full(GROUP, per, np.int32)
            first = gi * GROUP + 1
            if without_image is not None and first <= without_image < first + GROUP:
                counts[without_image - first] = 0
            check(L.apds_db_insert_batch_dev(table._h, kp.data_ptr() + gi * GROUP * per * 28, desc.data_ptr() + gi * GROUP * per * 64, GROUP, per, ptr(counts),
                                             first, lod, ptr(cr), 256, 256, None))

    def columns(table):
        r, k, x, m = table.device_table()
        out = [np.zeros((m, 64), np.uint8), np.zeros(m, pkg._lib.KEYPOINT_DTYPE), np.zeros((m, 3), np.float64)]
        for a, p in zip(out, (r, k, x)):
            check(L.apds_dev_download(ptr(a), p, a.nbytes, None))
        return out

    table, rebuilt = pkg.feature_database.KeypointTable(n), pkg.feature_database.KeypointTable(n)
    cases = {"front": (0, 2), "middle": (0, 500), "tail": (0, 1000), "lod": (1, 1)}
    results = {}
    for name, (mode, value) in cases.items():
        t_del, t_ins, t_ins_xyz, deleted = [], [], [], 0
        for r in range(args.repeats + 1):
            table.delete_keypoints_from_lod(0), table.delete_keypoints_from_lod(1)
            rebuilt.delete_keypoints_from_lod(0), rebuilt.delete_keypoints_from_lod(1)
            fill(table)
            assert len(table) == n and table.world_coordinates(et) == 0
            torch.cuda.synchronize()
            nd = C.c_int64(0)
            t0 = time.perf_counter()
            check(L.apds_db_delete_where(table._h, mode, value, 0.0, 0.0, 0.0, 0.0, C.byref(nd)))
            t1 = time.perf_counter()
            fill(rebuilt, without_image=value if mode == 0 else None, without_lod=value if mode == 1 else None)
            t2 = time.perf_counter()
            assert rebuilt.world_coordinates(et) == 0
            t3 = time.perf_counter()
            deleted = nd.value
            assert len(table) == len(rebuilt) == n - deleted
            if r == 0:          # (warm-up round) the two tables hold the same rows
                for a, b in zip(columns(table), columns(rebuilt)):
                    assert a.tobytes() == b.tobytes()
            else:
                t_del.append((t1 - t0) * 1e3)
                t_ins.append((t2 - t1) * 1e3)
                t_ins_xyz.append((t3 - t1) * 1e3)
        if mode == 0:
            moved_rows = n - value * per
        else:
            moved_rows = sum(per * GROUP for gi in range(IMAGES // GROUP) if gi % 2 == 0 and gi > 1)
        ms = float(np.median(t_del))
        traffic = 4 * moved_rows * ROW_BYTES + n * 5
        results[name] = dict(deleted_rows=int(deleted), moved_rows=int(moved_rows), moved_bytes=int(moved_rows * ROW_BYTES), traffic_bytes=int(traffic),
                             delete_ms=round(ms, 3), delete_ms_min=round(float(np.min(t_del)), 3), hbm_fraction=round(traffic / (ms * 1e-3) / HBM_PEAK, 4),
                             rebuild_insert_ms=round(float(np.median(t_ins)), 3), rebuild_insert_world_ms=round(float(np.median(t_ins_xyz)), 3),
                             rebuild_over_delete=round(float(np.median(t_ins)) / ms, 2))
        print(name, results[name], flush=True)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    summary = dict(db_rows=n, rows_per_image=per, repeats=args.repeats, row_bytes=ROW_BYTES, hbm_peak_bytes_per_s=HBM_PEAK, cases=results, parent_commit=commit,
                   device=torch.cuda.get_device_name(0))
    line = json.dumps(summary)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    table.close()
    rebuilt.close()


if __name__ == "__main__":
    main()
