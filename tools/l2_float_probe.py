#!/usr/bin/env python3
"""The float path's numbers (profiles/pipeline_float/): one JSON line per measurement, appended to --out as well.

  match-synth   apds_dev_l2_train_top2 (screen, exact) and apds_dev_l2_topk_ex at dim 64 on unit-norm rows, 35 312 x 983 616 x 64 (the
                pipeline's own shape): median of --runs timed calls after --warmup, candidates per query, keys compared between the modes
  match-real    the same on M-SURF rows: a DB extracted from --tiles distinct 1024 x 1024 synthetic tiles (apds_akaze_extract_float_batch),
                queries = the descriptors of shifted views of the first tiles
  screen128     the dim-128 screen through apds_dev_l2_topk_ex at --q128 x 1 000 000 x 128 (the shape of profiles/r04), before / after
  pipeline      frames/s of StreamedFramePipeline(matcher="l2") beside the Hamming pipeline's, same frames (4096 x 4096), same session
  pipeline-table  the same frames and rows with the rows in a float keypoint table and a region select per frame (262143 rows of the view):
                what selecting per frame costs beside the fixed-train-set figure of `pipeline`

(The committed match_synth_nc4.jsonl is the same probe on a build that also instantiated four column blocks per wave at dim 64, picked
per process; that variant lost and is gone, so every record made now says nc64 = 3.)"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("cubesat-apds_amd")
pl = importlib.import_module("cubesat-apds_amd.pipeline")
L, check = pkg._lib.lib(), pkg._lib.check
DEV = torch.device("cuda:0")
NQ, NT = 35312, 983616


def emit(args, **rec):
    rec["nc64"] = 3
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def match(args, name, q, db):
    nq, nt, dim = int(q.shape[0]), int(db.shape[0]), int(q.shape[1])
    ts = pl.L2TrainSet(db)
    outs = {}
    try:
        for mode in ("screen", "exact"):
            out = torch.empty((nq, 2), dtype=torch.int64, device=DEV)
            med, lo, hi = timed(lambda: ts.top2(q, mode, out=out), args.warmup, args.runs)
            outs[mode] = out
            emit(args, probe=name, call="apds_dev_l2_train_top2", mode=mode, mode_used=ts.mode_used, nq=nq, nt=nt, dim=dim, ms_median=med, ms_min=lo, ms_max=hi,
                 candidates_per_query=ts.candidates_per_query, runs=args.runs)
        emit(args, probe=name, check="screen keys == exact keys", equal=bool(torch.equal(outs["screen"], outs["exact"])))
    finally:
        ts.close()
    out = torch.empty((nq, 2), dtype=torch.int64, device=DEV)
    used, cpq = C.c_int(-1), C.c_double(0)
    med, lo, hi = timed(lambda: check(L.apds_dev_l2_topk_ex(q.data_ptr(), nq, db.data_ptr(), nt, dim, 0, 2, 1, out.data_ptr(), pl.torch_stream(), C.byref(used), C.byref(cpq))),
                        args.warmup, args.runs)
    emit(args, probe=name, call="apds_dev_l2_topk_ex", mode="screen", mode_used=("exact", "screen")[used.value], nq=nq, nt=nt, dim=dim, ms_median=med, ms_min=lo,
         ms_max=hi, runs=args.runs, equal_to_train_set=bool(torch.equal(out, outs["exact"])))


def unit_rows(n, dim, g):
    return torch.nn.functional.normalize(torch.randn((n, dim), device=DEV, generator=g), dim=1).contiguous()


def match_synth(args):
    g = torch.Generator(device=DEV)
    g.manual_seed(7)
    db, q = unit_rows(NT, 64, g), unit_rows(NQ, 64, g)
    npl = int(0.3 * NQ)
    src = torch.randint(0, NT, (npl,), device=DEV, generator=g)
    q[:npl] = torch.nn.functional.normalize(db[src] + 0.05 * torch.randn((npl, 64), device=DEV, generator=g), dim=1)
    match(args, "match-synth", q, db)


def match_real(args):
    fe, synth = pkg.feature_extraction, pkg.synth
    tiles = np.stack([synth.make_tile(1024, 1024, frame_index=900 + i, blobs_per_mpx=20000) for i in range(args.tiles)])
    db = np.concatenate([np.asarray(e.descriptors, np.float32) for e in fe.akaze_keypoint_descriptor_extraction_batch(tiles, descriptor="kaze")])
    shifted = np.stack([np.roll(t, (19, 23), axis=(0, 1)) for t in tiles[:max(1, args.tiles // 4)]])
    q = np.concatenate([np.asarray(e.descriptors, np.float32) for e in fe.akaze_keypoint_descriptor_extraction_batch(shifted, descriptor="kaze")])[:NQ]
    norms = np.linalg.norm(db, axis=1)
    emit(args, probe="match-real", tiles=args.tiles, db_rows=len(db), queries=len(q), norm_min=float(norms.min()), norm_median=float(np.median(norms)),
         norm_max=float(norms.max()), zero_rows=int((norms == 0).sum()))
    match(args, "match-real", torch.from_numpy(q).to(DEV), torch.from_numpy(db).to(DEV))


def screen128(args):
    g = torch.Generator(device=DEV)
    g.manual_seed(7)
    nq, nt = args.q128, 1000000
    db, q = unit_rows(nt, 128, g), unit_rows(nq, 128, g)
    npl = int(0.3 * nq)
    src = torch.randint(0, nt, (npl,), device=DEV, generator=g)
    q[:npl] = torch.nn.functional.normalize(db[src] + 0.05 * torch.randn((npl, 128), device=DEV, generator=g), dim=1)
    out = torch.empty((nq, 2), dtype=torch.int64, device=DEV)
    used, cpq = C.c_int(-1), C.c_double(0)
    check(L.apds_dev_timing_enable(1))
    med, lo, hi = timed(lambda: check(L.apds_dev_l2_topk_ex(q.data_ptr(), nq, db.data_ptr(), nt, 128, 0, 2, 1, out.data_ptr(), pl.torch_stream(), C.byref(used), C.byref(cpq))),
                        args.warmup, args.runs)
    ms_s, n_s = pkg._lib.kernel_ms("l2_screen")
    emit(args, probe="screen128", label=args.label, call="apds_dev_l2_topk_ex", mode_used=("exact", "screen")[used.value], nq=nq, nt=nt, dim=128, ms_median=med, ms_min=lo,
         ms_max=hi, candidates_per_query=cpq.value, runs=args.runs, l2_screen_kernel_ms_last=ms_s, l2_screen_launches_last=n_s)


def pipeline(args):
    fe, synth = pkg.feature_extraction, pkg.synth
    T = args.tile
    tiles = [synth.make_tile(T, T, frame_index=i) for i in range(2)]
    frames = [torch.from_numpy(t).to(DEV) for t in tiles]
    rolled = [np.roll(t, (19, 23), axis=(0, 1)).copy() for t in tiles]
    g = torch.Generator(device=DEV)
    g.manual_seed(11)
    for kind in ("l2", "ratio"):
        ex = [fe.akaze_keypoint_descriptor_extraction(r, descriptor="kaze" if kind == "l2" else "mldb") for r in rolled]
        kps = np.concatenate([np.asarray(e.keypoints) for e in ex])
        n_real = len(kps)
        xy = torch.rand((NT, 2), device=DEV, generator=g) * (T - 1)
        xy[:n_real] = torch.from_numpy(np.stack([kps["x"], kps["y"]], 1).astype(np.float32)).to(DEV)
        if kind == "l2":
            db = unit_rows(NT, 64, g)
            db[:n_real] = torch.from_numpy(np.concatenate([np.asarray(e.descriptors, np.float32) for e in ex])).to(DEV)
        else:
            db = torch.randint(0, 256, (NT, 64), device=DEV, generator=g, dtype=torch.uint8)
            db[:, 60] &= 0x3F
            db[:, 61:] = 0
            db[:n_real, :61] = torch.from_numpy(np.concatenate([e.descriptors for e in ex])).to(DEV)
        torch.cuda.synchronize()
        pipe = pl.StreamedFramePipeline(db, xy, matcher=kind)
        try:
            pipe.run(frames, args.warmup + 1, filter_strength=args.fs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res, _ = pipe.run(frames, args.frames, filter_strength=args.fs)
            dt = time.perf_counter() - t0
        finally:
            pipe.close()
        emit(args, probe="pipeline", matcher=kind, l2_mode="screen" if kind == "l2" else None, tile=T, db_rows=NT, frames=args.frames,
             frames_per_s=args.frames / dt, n_keypoints=res[0]["n_keypoints"], n_matches=res[0]["n_matches"], n_inliers=res[0]["n_inliers"], filter_strength=args.fs)
        del db, xy


def pipeline_table(args):
    """the float pipeline's frame and rows, the rows in a FLOAT keypoint table and the train set selected per frame: a region select that
    qualifies every row and returns the 262143 best (the frames' own rows among them: the random rows' responses lie below theirs)"""
    fe, synth, fd = pkg.feature_extraction, pkg.synth, pkg.feature_database
    T = args.tile
    tiles = [synth.make_tile(T, T, frame_index=i) for i in range(2)]
    frames = [torch.from_numpy(t).to(DEV) for t in tiles]
    ex = [fe.akaze_keypoint_descriptor_extraction(np.roll(t, (19, 23), axis=(0, 1)).copy(), descriptor="kaze") for t in tiles]
    kps_real = np.concatenate([np.asarray(e.keypoints) for e in ex])
    n_real = len(kps_real)
    g = torch.Generator(device=DEV)
    g.manual_seed(11)
    kps = torch.zeros((NT, 7), dtype=torch.float32, device=DEV)
    kps[:, 0:2] = torch.rand((NT, 2), device=DEV, generator=g) * (T - 1)
    kps[:, 4] = torch.rand(NT, device=DEV, generator=g) * 1e-9
    kps[:n_real] = torch.from_numpy(kps_real.view(np.float32).reshape(n_real, 7)).to(DEV)
    db = unit_rows(NT, 64, g)
    db[:n_real] = torch.from_numpy(np.concatenate([np.asarray(e.descriptors, np.float32) for e in ex])).to(DEV)
    torch.cuda.synchronize()
    table = fd.KeypointTable(NT, descriptor="kaze")
    table.create_keypoints_device(kps.data_ptr(), db.data_ptr(), NT, 1, 0)
    del db, kps
    sel = pl.StreamedFramePipeline.selection(2, 0, (0.0, 0.0, float(T), float(T)))
    pipe = pl.StreamedFramePipeline.from_table(table, per_frame_view=True)
    try:
        pipe.run(frames, args.warmup + 1, filter_strength=args.fs, selections=[sel])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res, _ = pipe.run(frames, args.frames, filter_strength=args.fs, selections=[sel])
        dt = time.perf_counter() - t0
    finally:
        pipe.close()
        table.close()
    emit(args, probe="pipeline-table", matcher="l2", l2_mode="screen", train_set="per-frame region select of a float table: 262143 of %d rows" % NT, tile=T,
         db_rows=NT, view_rows=(1 << 18) - 1, frames=args.frames, frames_per_s=args.frames / dt, n_keypoints=res[0]["n_keypoints"], n_matches=res[0]["n_matches"],
         n_inliers=res[0]["n_inliers"], filter_strength=args.fs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="+", choices=["match-synth", "match-real", "screen128", "pipeline", "pipeline-table"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tiles", type=int, default=48)
    ap.add_argument("--q128", type=int, default=262144)
    ap.add_argument("--label", default="")
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--fs", type=float, default=0.8)
    args = ap.parse_args()
    torch.cuda.set_stream(torch.cuda.Stream(DEV))
    for w in args.what:
        {"match-synth": match_synth, "match-real": match_real, "screen128": screen128, "pipeline": pipeline, "pipeline-table": pipeline_table}[w](args)


if __name__ == "__main__":
    main()
