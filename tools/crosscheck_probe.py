#!/usr/bin/env python3
"""What the pipeline's cross-check matcher (apds_pipeline_set_matcher, get_bruteforce_matches, lib.rs:116-126) costs beside the ratio
matcher on the headline shape: 4096^2 frames against a 1 M-row descriptor DB, built the way bench.py builds it (a shifted copy of every
frame + i.i.d. random rows). A ratio pipeline and a cross-check pipeline alternate (ratio / crosscheck / ratio / crosscheck) in one
process, so that a drift of the box is not read as a difference of the matchers.

    python tools/crosscheck_probe.py [--steps 40] [--warmup 4] [--rounds 2] [--out profiles/pipeline_crosscheck/crosscheck_probe.json]

Prints one line per timed run and a JSON summary: frames/s, matches and inliers per frame of both matchers, and the main scan's kernel
time per frame (HIP events, the counter "hamming_topk": the forward k = 2 scan of the ratio matcher, the roles-swapped top-1 scan of the
cross-check) with what runs in front of it ("hamming_topk_sample": the expansions, the threshold launch of the forward scan)."""
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
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
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
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(dev)):
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

    be = C.c_int(-1)
    check(L.apds_dev_match_backend(C.byref(be)))
    pipes = {m: pl.StreamedFramePipeline(db, db_xy, device=str(dev), matcher=m) for m in ("ratio", "crosscheck")}
    runs = {m: [] for m in pipes}
    try:
        for r in range(args.rounds):
            for m, pipe in pipes.items():
                pipe.run(frames, args.warmup, filter_strength=args.filter_strength, timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res, timers = pipe.run(frames, args.steps, filter_strength=args.filter_strength, timing=True)
                torch.cuda.synchronize()
                fps = args.steps / (time.perf_counter() - t0)
                scan_ms, scan_n = timers["hamming_topk"]
                pre_ms, _ = timers["hamming_topk_sample"]
                one = dict(fps=round(fps, 2), keypoints_per_frame=round(float(np.mean([x["n_keypoints"] for x in res])), 1),
                           matches_per_frame=round(float(np.mean([x["n_matches"] for x in res])), 1),
                           inliers_per_frame=round(float(np.mean([x["n_inliers"] for x in res])), 1),
                           homographies=sum(x["H"] is not None for x in res), scan_ms_per_frame=round(scan_ms / args.steps, 3), scan_launches=scan_n,
                           before_scan_ms_per_frame=round(pre_ms / args.steps, 3))
                runs[m].append(one)
                print(f"round {r} {m}: " + json.dumps(one), flush=True)
    finally:
        for pipe in pipes.values():
            pipe.close()

    def med(m, k):
        return round(float(np.median([x[k] for x in runs[m]])), 3)

    summary = dict(tile=T, db_rows=NDB, steps=args.steps, warmup=args.warmup, rounds=args.rounds, filter_strength=args.filter_strength, matrix_cores=be.value,
                   runs=runs, device=torch.cuda.get_device_name(0))
    for m in runs:
        summary[m] = {k: med(m, k) for k in ("fps", "matches_per_frame", "inliers_per_frame", "scan_ms_per_frame", "before_scan_ms_per_frame")}
    summary["swapped_over_forward_scan"] = round(summary["crosscheck"]["scan_ms_per_frame"] / max(summary["ratio"]["scan_ms_per_frame"], 1e-9), 3)
    line = json.dumps(summary)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
