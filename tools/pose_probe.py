#!/usr/bin/env python3
"""What the pipeline's pose stage costs on the headline shape: 4096^2 frames against a 1 M-row descriptor DB, built the way bench.py builds
it (a shifted copy of every frame + i.i.d. random rows), streamed through StreamedFramePipeline with pose off and pose on (EPnP) in one
process, alternating off / on / off / on so that a drift of the box is not read as the stage's cost. World points of the DB rows: the DB
keypoints back-projected from a camera looking straight down at a plane 1000 m away, with a 3 % relief.

    python tools/pose_probe.py [--steps 50] [--warmup 3] [--rounds 2] [--out profiles/pose/pose_probe.json]

Prints one line per timed run and a JSON summary: frames/s off and on (median of the rounds), the drop, and the pose stage's own time per
frame (gather + PnP RANSAC on one frame's matches, timed alone on the host thread) as a share of the pose-off frame period."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--db-rows", type=int, default=1_000_000)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--filter-strength", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import __graft_entry__ as graft
    pkg = graft.load_package()
    from cubesat_apds_amd import pipeline as pl
    L, check, synth = pkg.lib(), pkg._lib.check, pkg.synth
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    check(L.apds_set_device(0))
    T, NDB = args.tile, args.db_rows

    # ---- the DB, as bench.py builds it for one GPU
    shift = (37, 52)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max(1, min(args.frames, 4))) as pool:
        frames_np = list(pool.map(lambda i: synth.make_tile(T, T, frame_index=i), range(args.frames)))
    frames = [torch.from_numpy(f).to(dev) for f in frames_np]
    cap = pkg.feature_extraction.MAX_POINTS
    kps = torch.empty((cap, 7), dtype=torch.float32, device=dev)
    desc = torch.empty((cap, 64), dtype=torch.uint8, device=dev)
    rows, xy = [], []
    setup_stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(setup_stream):
        for f in frames_np:
            rolled = torch.from_numpy(np.roll(f, shift, axis=(0, 1)).copy()).to(dev)
            n = C.c_int(0)
            check(L.apds_dev_akaze_extract(rolled.data_ptr(), T, T, rolled.shape[2], rolled.stride(0), cap, kps.data_ptr(), desc.data_ptr(), cap, C.byref(n),
                                           pl.torch_stream()))
            rows.append(desc[:n.value].clone())
            xy.append(kps[:n.value, 0:2].clone())
        rows, xy = torch.cat(rows), torch.cat(xy)
        P = min(rows.shape[0], NDB)
        pad = np.zeros((NDB - P, 64), np.uint8)
        pad[:, :61] = synth.make_descriptor_db(NDB - P, seed=synth.DB_SEED + P)
        db = torch.cat([rows[:P], torch.from_numpy(pad).to(dev)]).contiguous()
        db_xy = torch.zeros((NDB, 2), dtype=torch.float32, device=dev)
        db_xy[:P] = xy[:P]
    torch.cuda.synchronize()

    # ---- world points: a plane 1000 m below a downward camera (f = 4000 px), 3 % relief
    f, c, Z0 = 4000.0, T / 2.0, 1000.0
    uv = db_xy.cpu().numpy().astype(np.float64)
    Z = Z0 * (1 + 0.03 * np.sin(uv[:, 0] / 97.0) * np.cos(uv[:, 1] / 61.0))
    xyz = np.stack([(uv[:, 0] - c) * Z / f, (uv[:, 1] - c) * Z / f, Z], 1)
    K = np.array([[f, 0, c], [0, f, c], [0, 0, 1]])
    pose = pl.PoseStage(xyz, K, method=pl.SOLVEPNP_EPNP)

    streamed = pl.StreamedFramePipeline(db, db_xy, device=str(dev))
    fr = pkg._lib.FrameResult
    fp = pkg._lib.FramePose()

    def timed(with_pose):
        streamed.enable_pose(pose if with_pose else None)
        handle = streamed.prepare(frames[0].shape, filter_strength=args.filter_strength)
        fargs = [streamed.frame_args(x) for x in frames]
        res = fr()

        def stream(count):
            poses = []
            for i in range(count):
                ptr, stride, on_dev = fargs[i % len(fargs)]
                check(L.apds_pipeline_submit(handle, ptr, stride, on_dev, None))
            for i in range(count):
                check(L.apds_pipeline_poll_pose(handle, C.byref(res), C.byref(fp) if with_pose else None, 1))
                if res.status != 0:
                    raise RuntimeError(f"frame {res.frame} failed: status {res.status}")
                if with_pose:
                    poses.append((fp.status, fp.found, fp.n_correspondences, fp.n_inliers))
            return poses

        stream(args.warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        poses = stream(args.steps)
        torch.cuda.synchronize()
        return args.steps / (time.perf_counter() - t0), poses

    runs = {"off": [], "on": []}
    last_poses = None
    for r in range(args.rounds):
        for mode in ("off", "on"):
            fps, poses = timed(mode == "on")
            runs[mode].append(fps)
            if poses:
                last_poses = poses
            print(f"round {r} pose {mode}: {fps:.2f} frames/s", flush=True)
    streamed.close()

    # ---- the pose stage alone: one frame's matches (serial path) -> gather + PnP RANSAC, timed on this thread
    serial = pl.FramePipeline(db, db_xy, device=str(dev))
    out = serial.step(frames[0], filter_strength=args.filter_strength)
    M, Kp = out["n_matches"], out["n_keypoints"]
    img = torch.empty((M, 2), dtype=torch.float32, device=dev)
    obj = torch.empty((M, 3), dtype=torch.float32, device=dev)
    rv, tv, ni, found = np.zeros(3), np.zeros(3), C.c_int(0), C.c_int(0)
    o = np.ascontiguousarray(pose.origin)
    Kc = np.ascontiguousarray(K)
    torch.cuda.synchronize()
    solo = []
    for i in range(12):
        t0 = time.perf_counter()
        check(L.apds_dev_pnp_correspondences(serial.kps.data_ptr(), Kp, pose.db_xyz_dev.data_ptr(), NDB, pkg._lib.ptr(o), serial.matches.data_ptr(), M,
                                             img.data_ptr(), obj.data_ptr(), None))
        check(L.apds_dev_pnp_solver_ransac(obj.data_ptr(), img.data_ptr(), M, pkg._lib.ptr(Kc), pose.iter_count, pose.reproj_thres, pose.confidence, pose.method,
                                           pkg._lib.ptr(rv), pkg._lib.ptr(tv), None, C.byref(ni), C.byref(found), None))
        if i >= 2:
            solo.append((time.perf_counter() - t0) * 1e3)
    off, on = float(np.median(runs["off"])), float(np.median(runs["on"]))
    summary = dict(tile=T, db_rows=NDB, steps=args.steps, warmup=args.warmup, rounds=args.rounds, method="EPNP",
                   fps_pose_off=[round(v, 2) for v in runs["off"]], fps_pose_on=[round(v, 2) for v in runs["on"]],
                   fps_off_median=round(off, 2), fps_on_median=round(on, 2), drop_percent=round(100.0 * (off - on) / off, 2),
                   pose_stage_ms_per_frame_alone=round(float(np.median(solo)), 3), matches_per_frame=M,
                   pose_stage_share_of_frame_period=round(float(np.median(solo)) / (1e3 / off), 3),
                   last_run_poses=[list(p) for p in (last_poses or [])[:4]], inliers_frame0=ni.value, found_frame0=found.value,
                   device=torch.cuda.get_device_name(0))
    line = json.dumps(summary)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
