#!/usr/bin/env python3
"""What the lens costs on the headline shape.

 1. The frame undistort alone: apds_dev_undistort_image on a 4096^2 BGRA frame resident on the device (coefficient set (-0.12, 0.03,
    1e-3, -5e-4), f = 3000), timed with device events over --reps launches after a warm-up, as a fraction of the HBM roofline for the
    128 MiB it has to move (64 MiB read once, 64 MiB written; 6.3 TB/s achievable). One host call of apds_warp_perspective on the same
    frame runs beside it so that a kernel trace of this program (rocprofv3 --kernel-trace --stats, a run of its own) shows
    warp_perspective_kernel and undistort_image_kernel side by side.
 2. The streamed pipeline with the lens off and on (pose on in both), alternating off / on --rounds times in one process, as
    tools/pose_probe.py does for the pose stage; --parent-fps records the parent commit's "off" figure (from the same script run on
    that commit) beside it.

    python tools/lens_probe.py [--steps 50] [--warmup 3] [--rounds 2] [--reps 200] [--parent-fps X] [--out profiles/lens/lens_probe.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SET_A = np.array([-0.12, 0.03, 1e-3, -5e-4])
HBM_ACHIEVABLE = 6.3e12     # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--db-rows", type=int, default=1_000_000)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--filter-strength", type=float, default=0.3)
    ap.add_argument("--parent-fps", type=float, default=None)
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import __graft_entry__ as graft
    pkg = graft.load_package()
    from cubesat_apds_amd import pipeline as pl
    L, check, synth, ptr = pkg.lib(), pkg._lib.check, pkg.synth, pkg._lib.ptr
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    check(L.apds_set_device(0))
    T, NDB = args.tile, args.db_rows
    has_lens = hasattr(L, "apds_dev_undistort_image")     # (the parent commit runs part 2's "off" half only)

    frames_np = [synth.make_tile(T, T, frame_index=i) for i in range(args.frames)]
    frames = [torch.from_numpy(f).to(dev) for f in frames_np]
    summary = dict(tile=T, db_rows=NDB, device=torch.cuda.get_device_name(0))

    # ---- 1. the image kernel alone
    if has_lens:
        K = np.array([[3000.0, 0, (T - 1) / 2], [0, 3000.0, (T - 1) / 2], [0, 0, 1]])
        src, dst = frames[0], torch.empty_like(frames[0])
        stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(stream):
            run = lambda: check(L.apds_dev_undistort_image(src.data_ptr(), T, T, 4, ptr(K), ptr(SET_A), 4, None, dst.data_ptr(), pl.torch_stream()))     # noqa: E731
            for _ in range(10):
                run()
            stream.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                run()
            b.record()
            stream.synchronize()
        ms = a.elapsed_time(b) / args.reps     # launches back to back on one stream: the weight-table copy of each call is inside
        moved = 2 * T * T * 4
        floor_ms = moved / HBM_ACHIEVABLE * 1e3
        summary.update(undistort_image_ms=round(ms, 4), undistort_image_bytes=moved, hbm_floor_ms=round(floor_ms, 4),
                       undistort_image_fraction_of_hbm_roofline=round(floor_ms / ms, 3))
        print(f"undistort_image {T}x{T} BGRA: {ms:.4f} ms per call, {moved / ms / 1e6:.0f} GB/s, {floor_ms / ms:.3f} of the HBM roofline", flush=True)
        M = np.array([[1.0, 0.01, 3.0], [-0.01, 1.0, -2.0], [1e-6, 0, 1.0]])
        out = np.empty_like(frames_np[0])
        check(L.apds_warp_perspective(ptr(frames_np[0]), T, T, 4, ptr(M), T, T, ptr(out)))     # (for the kernel trace)

    # ---- 2. the pipeline, lens off / on
    if not args.skip_pipeline:
        shift = (37, 52)
        cap = pkg.feature_extraction.MAX_POINTS
        kps = torch.empty((cap, 7), dtype=torch.float32, device=dev)
        desc = torch.empty((cap, 64), dtype=torch.uint8, device=dev)
        rows, xy = [], []
        with torch.cuda.stream(torch.cuda.Stream(dev)):
            for f in frames_np:
                rolled = torch.from_numpy(np.roll(f, shift, axis=(0, 1)).copy()).to(dev)
                n = C.c_int(0)
                check(L.apds_dev_akaze_extract(rolled.data_ptr(), T, T, 4, rolled.stride(0), cap, kps.data_ptr(), desc.data_ptr(), cap, C.byref(n), pl.torch_stream()))
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
        f, c, Z0 = 4000.0, T / 2.0, 1000.0
        uv = db_xy.cpu().numpy().astype(np.float64)
        Z = Z0 * (1 + 0.03 * np.sin(uv[:, 0] / 97.0) * np.cos(uv[:, 1] / 61.0))
        xyz = np.stack([(uv[:, 0] - c) * Z / f, (uv[:, 1] - c) * Z / f, Z], 1)
        Kp = np.array([[f, 0, c], [0, f, c], [0, 0, 1]])
        pose = pl.PoseStage(xyz, Kp, method=pl.SOLVEPNP_EPNP)
        res, fp = pkg._lib.FrameResult(), pkg._lib.FramePose()

        def timed(lens_on):
            kw = dict(lens=(Kp, SET_A, 5)) if lens_on else {}
            streamed = pl.StreamedFramePipeline(db, db_xy, device=str(dev), pose=pose, **kw)
            try:
                handle = streamed.prepare(frames[0].shape, filter_strength=args.filter_strength)
                fargs = [streamed.frame_args(x) for x in frames]

                def stream_frames(count):
                    matches = 0
                    for i in range(count):
                        p, stride, on_dev = fargs[i % len(fargs)]
                        check(L.apds_pipeline_submit(handle, p, stride, on_dev, None))
                    for i in range(count):
                        check(L.apds_pipeline_poll_pose(handle, C.byref(res), C.byref(fp), 1))
                        if res.status != 0:
                            raise RuntimeError(f"frame {res.frame} failed: status {res.status}")
                        matches = res.n_matches
                    return matches

                stream_frames(args.warmup)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                matches = stream_frames(args.steps)
                torch.cuda.synchronize()
                return args.steps / (time.perf_counter() - t0), matches
            finally:
                streamed.close()

        runs, matches = {"off": [], "on": []}, 0
        for r in range(args.rounds):
            for mode in (("off", "on") if has_lens else ("off",)):
                fps, matches = timed(mode == "on")
                runs[mode].append(fps)
                print(f"round {r} lens {mode}: {fps:.2f} frames/s", flush=True)
        off = float(np.median(runs["off"]))
        summary.update(steps=args.steps, warmup=args.warmup, rounds=args.rounds, matches_per_frame=matches, fps_lens_off=[round(v, 2) for v in runs["off"]],
                       fps_off_median=round(off, 2), fps_off_parent_commit=args.parent_fps)
        if runs["on"]:
            on = float(np.median(runs["on"]))
            summary.update(fps_lens_on=[round(v, 2) for v in runs["on"]], fps_on_median=round(on, 2), drop_percent=round(100.0 * (off - on) / off, 2))

    line = json.dumps(summary)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
