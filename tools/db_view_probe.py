#!/usr/bin/env python3
"""What a per-frame select costs beside the scan, on one GPU, on a 1 M-row keypoint table (the rolled copies of the frames, then random rows;
one level of detail, coordinates spread over a 16384^2 mosaic).

 1. the two fronts of the one selection engine (csrc/keypoint_select.hip) in one process, the two calls alternating, medians of the wall
    time until the view is complete: apds_db_view_select (a view object's buffers, the caller's stream; view_select_ms) and apds_db_select
    (the table's current view, scratch from the thread's workspace, synchronised; db_select_ms - up to profiles/db_view/ that key timed a
    host-driven implementation of its own, the keys are kept so the runs stay comparable). Two cases: a bounding box that qualifies
    fewer rows than the 262143-row limit, and a level-of-detail select that qualifies every row (radix cut + the full 2^18 sort).
 2. frames/s of a pipeline whose train set is selected per frame (every selection returns the full 262143 rows) against the whole-table
    pipeline on the same table and frames, off / on alternating, and the select's share of the per-frame-view frame period.

    python tools/db_view_probe.py [--steps 30] [--warmup 3] [--rounds 2] [--out profiles/db_view/db_view_probe.json]

 --float: the select of a FLOAT table instead (profiles/db_float/). A float table and a byte table of --db-rows rows with the same keypoints
 (random rows inserted from the device; every row qualifies, so a select returns the 262143 best). Three things are timed in one run, the
 calls alternating, medians over --repeats: the byte view's select; the float view's select, whose gather also writes the L2 train side
 (fused); and the unfused alternative for the same rows - apds_db_select on the float table (the plain gather into the table's own view)
 followed by apds_l2_train_create over those rows. Host time of the whole call until the result is complete, and the GPU time of the gather
 launch ("db_select_gather") and of apds_l2_train_create's three launches ("l2_train_prepare") from apds_dev_last_kernel_ms. The gather's
 algorithmic bytes per selected row (256 read; 256 + 128 + 4 written on a float view, 64 + 64 on a byte view) over its GPU time, as a share
 of the HBM peak (--hbm-gbs, 8000).

    python tools/db_view_probe.py --float [--db-rows 1000000] [--repeats 9] [--out profiles/db_float/db_view_probe_float.json]"""
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


class _Ex:
    def __init__(self, kp, d):
        self.keypoints, self.descriptors = kp, d


def float_select(args):
    import torch
    import __graft_entry__ as graft
    pkg = graft.load_package()
    L, check, fd = pkg.lib(), pkg._lib.check, pkg.feature_database
    torch.cuda.set_device(0)
    check(L.apds_set_device(0))
    NDB, dev = args.db_rows, torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    tf, tb = fd.KeypointTable(NDB, descriptor="kaze"), fd.KeypointTable(NDB)
    at, chunk = 0, 250_000
    while at < NDB:         # the same keypoints into both tables, rows of either kind, all from device tensors
        m = min(chunk, NDB - at)
        kps = torch.zeros((m, 7), dtype=torch.float32, device=dev)
        kps[:, 0:2] = torch.rand((m, 2), device=dev, generator=g) * 16384
        kps[:, 4] = torch.rand(m, device=dev, generator=g)
        rows_f = torch.randn((m, 64), device=dev, generator=g)
        rows_f /= rows_f.norm(dim=1, keepdim=True)
        rows_b = torch.randint(0, 256, (m, 64), device=dev, generator=g, dtype=torch.uint8)
        torch.cuda.synchronize()
        tf.create_keypoints_device(kps.data_ptr(), rows_f.data_ptr(), m, 1 + at // chunk, 0)
        tb.create_keypoints_device(kps.data_ptr(), rows_b.data_ptr(), m, 1 + at // chunk, 0)
        at += m
    del kps, rows_f, rows_b
    vf, vb = tf.view(), tb.view()
    check(L.apds_dev_timing_enable(1))
    n, t = C.c_int(0), {k: [] for k in ("byte_view_select", "float_view_select_fused", "float_select_plain", "l2_train_create")}
    gpu = {k: [] for k in ("byte_gather", "float_gather_fused", "float_gather_plain", "l2_train_prepare")}
    box = (0.0, 0.0, 0.0, 0.0)

    def gather_ms(key):
        ms, launches = pkg._lib.kernel_ms("db_select_gather")
        assert launches == 1, launches
        gpu[key].append(ms)

    for r in range(args.repeats + 2):
        t0 = time.perf_counter()
        check(L.apds_db_view_select(vb._h, 1, 0, *box, 0, None, C.byref(n)))
        check(L.apds_stream_synchronize(None))
        tb_end = time.perf_counter()
        rows = n.value
        gather_ms("byte_gather")
        t1 = time.perf_counter()
        check(L.apds_db_view_select(vf._h, 1, 0, *box, 0, None, C.byref(n)))
        check(L.apds_stream_synchronize(None))
        t2 = time.perf_counter()
        assert n.value == rows
        gather_ms("float_gather_fused")
        t3 = time.perf_counter()
        check(L.apds_db_select(tf._h, 1, 0, *box, C.byref(n)))             # the plain gather: the table's own view has no train side
        t4 = time.perf_counter()
        assert n.value == rows
        r64 = tf.view_device_pointers()[0]
        h = C.c_void_p()
        check(L.apds_l2_train_create(C.byref(h), r64, rows, 64, 0))      # norms, bf16 copy, largest norm: three launches and a synchronise
        t5 = time.perf_counter()
        check(L.apds_l2_train_destroy(h))
        gather_ms("float_gather_plain")
        ms, launches = pkg._lib.kernel_ms("l2_train_prepare")
        assert launches == 1, launches
        gpu["l2_train_prepare"].append(ms)
        if r >= 2:
            t["byte_view_select"].append((tb_end - t0) * 1e3)
            t["float_view_select_fused"].append((t2 - t1) * 1e3)
            t["float_select_plain"].append((t4 - t3) * 1e3)
            t["l2_train_create"].append((t5 - t4) * 1e3)
        else:
            for v in gpu.values():
                v.pop()
    med = lambda a: round(float(np.median(a)), 4)     # noqa: E731
    host = {k: med(v) for k, v in t.items()}
    host["float_unfused_whole"] = round(host["float_select_plain"] + host["l2_train_create"], 4)
    gpu_ms = {k: med(v) for k, v in gpu.items()}
    gpu_ms["float_unfused_gather_plus_prepare"] = round(gpu_ms["float_gather_plain"] + gpu_ms["l2_train_prepare"], 4)
    bytes_row = dict(float_fused=256 + 256 + 128 + 4, float_plain=256 + 256, byte=64 + 64)
    gbs = lambda b, ms: round(b * rows / (ms * 1e-3) / 1e9, 1)      # noqa: E731
    achieved = dict(float_fused=gbs(bytes_row["float_fused"], gpu_ms["float_gather_fused"]), float_plain=gbs(bytes_row["float_plain"], gpu_ms["float_gather_plain"]),
                    byte=gbs(bytes_row["byte"], gpu_ms["byte_gather"]))
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    summary = dict(probe="db_view_float", db_rows=NDB, selected_rows=rows, repeats=args.repeats, host_ms=host, gpu_ms=gpu_ms,
                   fused_beats_unfused_whole_call=bool(host["float_view_select_fused"] < host["float_unfused_whole"]),
                   algorithmic_bytes_per_row=bytes_row, gather_gb_per_s=achieved, hbm_peak_gb_per_s=args.hbm_gbs,
                   gather_share_of_hbm_peak={k: round(v / args.hbm_gbs, 4) for k, v in achieved.items()}, parent_commit=commit,
                   device=torch.cuda.get_device_name(0))
    line = json.dumps(summary)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    vf.close()
    vb.close()
    tf.close()
    tb.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--db-rows", type=int, default=1_000_000)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--filter-strength", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--float", dest="float_table", action="store_true", help="time the select of a float table: fused gather against gather + apds_l2_train_create")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    args = ap.parse_args()
    if args.float_table:
        return float_select(args)

    import torch
    import __graft_entry__ as graft
    pkg = graft.load_package()
    from cubesat_apds_amd import pipeline as pl
    L, check, synth = pkg.lib(), pkg._lib.check, pkg.synth
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    check(L.apds_set_device(0))
    T, NDB = args.tile, args.db_rows

    # ---- the table: every frame rolled (extracted and inserted on the device), then random rows
    frames_np = [synth.make_tile(T, T, frame_index=i) for i in range(args.frames)]
    frames = [torch.from_numpy(f).to(dev) for f in frames_np]
    cap = pkg.feature_extraction.MAX_POINTS
    kps = torch.empty((cap, 7), dtype=torch.float32, device=dev)
    desc = torch.empty((cap, 64), dtype=torch.uint8, device=dev)
    table = pkg.feature_database.KeypointTable(NDB)
    torch.cuda.synchronize()
    for i, f in enumerate(frames_np):
        rolled = torch.from_numpy(np.roll(f, (37, 52), axis=(0, 1)).copy()).to(dev)
        torch.cuda.synchronize()
        n = C.c_int(0)
        check(L.apds_dev_akaze_extract(rolled.data_ptr(), T, T, rolled.shape[2], rolled.stride(0), cap, kps.data_ptr(), desc.data_ptr(), cap, C.byref(n), None))
        table.create_keypoints_device(kps.data_ptr(), desc.data_ptr(), min(n.value, NDB - len(table)), i + 1, 0, i, 0, (T, T))
    rng = np.random.default_rng(7)
    while len(table) < NDB:
        m = min(200_000, NDB - len(table))
        kp = np.zeros(m, pkg._lib.KEYPOINT_DTYPE)
        kp["x"], kp["y"], kp["response"] = rng.uniform(0, 16384, m), rng.uniform(0, 16384, m), rng.uniform(0, 1e-9, m)     # below every extracted response: the frames' rows survive the cut
        table.create_keypoints(_Ex(kp, synth.make_descriptor_db(m, seed=synth.DB_SEED + len(table))), 100, 0)
    view = table.view()

    # ---- 1. the two fronts of the selection engine, alternating
    cases = {"box_below_limit": (2, 0, (0.0, 0.0, 7000.0, 7000.0)), "lod_all_rows": (1, 0, (0.0, 0.0, 0.0, 0.0))}
    select = {}
    for name, (mode, value, box) in cases.items():
        old, new, n_old, n_new = [], [], C.c_int(0), C.c_int(0)
        for r in range(args.repeats + 2):
            t0 = time.perf_counter()
            check(L.apds_db_select(table._h, mode, value, *box, C.byref(n_old)))
            t1 = time.perf_counter()
            check(L.apds_db_view_select(view._h, mode, value, *box, 0, None, C.byref(n_new)))
            check(L.apds_stream_synchronize(None))
            t2 = time.perf_counter()
            if r >= 2:
                old.append((t1 - t0) * 1e3)
                new.append((t2 - t1) * 1e3)
        assert n_old.value == n_new.value
        select[name] = dict(rows=n_new.value, db_select_ms=round(float(np.median(old)), 3), view_select_ms=round(float(np.median(new)), 3),
                            factor=round(float(np.median(old) / np.median(new)), 2), not_slower=bool(np.median(new) <= np.median(old)))
        print(name, select[name], flush=True)

    # ---- 2. the pipeline: whole table against a per-frame view of 262143 rows
    sel = pl.StreamedFramePipeline.selection(1, 0)
    res = pkg._lib.FrameResult()

    def timed(per_frame):
        pipe = pl.StreamedFramePipeline.from_table(table, device=str(dev), per_frame_view=per_frame)
        try:
            handle = pipe.prepare(frames[0].shape, filter_strength=args.filter_strength)
            fargs = [pipe.frame_args(x) for x in frames]

            def stream(count):
                for i in range(count):
                    ptr, stride, on_dev = fargs[i % len(fargs)]
                    if per_frame:
                        check(L.apds_pipeline_submit_select(handle, ptr, stride, on_dev, C.byref(sel), None))
                    else:
                        check(L.apds_pipeline_submit(handle, ptr, stride, on_dev, None))
                for i in range(count):
                    check(L.apds_pipeline_poll(handle, C.byref(res), 1))
                    if res.status != 0:
                        raise RuntimeError(f"frame {res.frame} failed: status {res.status}")
                return res.n_matches

            stream(args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = stream(args.steps)
            torch.cuda.synchronize()
            return args.steps / (time.perf_counter() - t0), m
        finally:
            pipe.close()

    runs, matches = {"whole_table": [], "per_frame_view": []}, {}
    for r in range(args.rounds):
        for mode in ("whole_table", "per_frame_view"):
            fps, matches[mode] = timed(mode == "per_frame_view")
            runs[mode].append(fps)
            print(f"round {r} {mode}: {fps:.2f} frames/s", flush=True)
    whole, per = float(np.median(runs["whole_table"])), float(np.median(runs["per_frame_view"]))
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    summary = dict(tile=T, db_rows=NDB, view_rows=select["lod_all_rows"]["rows"], steps=args.steps, warmup=args.warmup, rounds=args.rounds, select=select,
                   fps_whole_table=[round(v, 2) for v in runs["whole_table"]], fps_per_frame_view=[round(v, 2) for v in runs["per_frame_view"]],
                   fps_whole_table_median=round(whole, 2), fps_per_frame_view_median=round(per, 2), matches_last_frame=matches,
                   select_share_of_frame_period=round(select["lod_all_rows"]["view_select_ms"] / (1e3 / per), 3),
                   parent_commit=commit, device=torch.cuda.get_device_name(0))
    line = json.dumps(summary)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    view.close()
    table.close()


if __name__ == "__main__":
    main()
