"""What the mask support costs: apds_dev_akaze_extract_masked[_support] on resident BGRA frames with their own alpha as the mask.
usage: mask_support_probe.py [--lib PATH] [--mode frame|batch|count] [--label NAME]
  --lib   another build of libapds_hip.so (the parent commit's: only the calls it has are timed)
  frame   one 4096^2 frame (4 x 4 copies of a 1024^2 synthetic tile), 20 back-to-back calls per round, three rounds
  batch   256 tiles of 1024^2 in one batched call, 3 calls per round, three rounds
  count   one 1024^2 extraction per variant and nothing else (for a kernel trace: the launch count)
The alpha is 0 on a swath edge (the left 300 columns) and in one block, 255 elsewhere."""
import argparse
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=os.path.join(ROOT, "cubesat-apds_amd", "libapds_hip.so"))
ap.add_argument("--mode", default="frame")
ap.add_argument("--label", default="change")
ap.add_argument("--variants", default="masked,support15,sat")
args = ap.parse_args()
pkg = importlib.import_module("cubesat-apds_amd")
dev = torch.device("cuda:0")
torch.cuda.init()
L = C.CDLL(args.lib)
vp, i, sz, ip = C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_int)
L.apds_dev_akaze_extract_masked.argtypes = [vp, i, i, i, sz, vp, sz, i, vp, vp, i, ip, vp]
L.apds_dev_akaze_extract_batch_masked.argtypes = [vp, i, sz, i, i, i, sz, vp, sz, sz, i, vp, vp, i, ip, vp]
has_support = hasattr(L, "apds_dev_akaze_extract_masked_support")
if has_support:
    L.apds_dev_akaze_extract_masked_support.argtypes = [vp, i, i, i, sz, vp, sz, i, i, vp, vp, i, ip, vp]
    L.apds_dev_akaze_extract_batch_masked_support.argtypes = [vp, i, sz, i, i, i, sz, vp, sz, sz, i, i, vp, vp, i, ip, vp]
    L.apds_dev_mask_zero_sat.argtypes = [vp, i, i, sz, sz, vp, vp]


def frame(side):
    tile = pkg.synth.make_tile(1024, 1024, frame_index=3, channels=4)
    f = np.tile(tile, (side // 1024, side // 1024, 1))
    f[..., 3] = 255
    f[:, :300, 3] = 0
    f[side // 2: side // 2 + 200, side // 2: side // 2 + 300, 3] = 0
    return np.ascontiguousarray(f)


def check(rc):
    if rc != 0:
        raise SystemExit(f"library call failed: {rc}")


def timed(name, call, calls, rounds, what):
    for r in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            n = call()
        torch.cuda.synchronize()
        print(f"{args.label} round {r} {name}: {(time.perf_counter() - t0) / calls * 1e3:.3f} ms per {what}, {n} keypoints", flush=True)


variants = [v for v in args.variants.split(",") if v == "masked" or has_support]
if args.mode in ("frame", "count"):
    side = 4096 if args.mode == "frame" else 1024
    f = torch.from_numpy(frame(side)).to(dev)
    cap = (1 << 18) - 1
    kps = torch.empty((cap, 7), dtype=torch.float32, device=dev)
    desc = torch.empty((cap, 64), dtype=torch.uint8, device=dev)
    sat = torch.empty(((side + 1) * (side + 1),), dtype=torch.int32, device=dev)
    n = C.c_int(0)
    alpha = f.data_ptr() + 3

    def masked():
        # the alpha as a plane mask: base = image + 3 with the image's row stride would need a pixel stride; the public device call takes
        # planes, so the probe passes a copy of the alpha plane
        check(L.apds_dev_akaze_extract_masked(f.data_ptr(), side, side, 4, side * 4, plane.data_ptr(), side, cap, kps.data_ptr(), desc.data_ptr(), cap, C.byref(n), None))
        return n.value

    def support15():
        check(L.apds_dev_akaze_extract_masked_support(f.data_ptr(), side, side, 4, side * 4, plane.data_ptr(), side, 15, cap, kps.data_ptr(), desc.data_ptr(), cap,
                                                      C.byref(n), None))
        return n.value

    def sat_plane():
        check(L.apds_dev_mask_zero_sat(plane.data_ptr(), side, side, side, 1, sat.data_ptr(), None))
        return 0

    def sat_alpha():
        check(L.apds_dev_mask_zero_sat(alpha, side, side, side * 4, 4, sat.data_ptr(), None))
        return 0

    plane = f[..., 3].contiguous()
    calls = {"masked": [("support 0 (apds_dev_akaze_extract_masked)", masked)], "support15": [("support 15", support15)],
             "sat": [("table of a plane alone", sat_plane), ("table of the BGRA alpha alone", sat_alpha)]}
    for v in variants:
        for name, fn in calls[v]:
            if args.mode == "count":
                fn()
                torch.cuda.synchronize()
                print(f"{args.label} {name}: one call done", flush=True)
            else:
                timed(name, fn, 20, 3, "4096^2 call")
else:
    B, side = 256, 1024
    one = torch.from_numpy(frame(side)).to(dev)
    imgs = one.unsqueeze(0).repeat(B, 1, 1, 1).contiguous()
    planes = imgs[..., 3].contiguous()
    cap = 4096
    kps = torch.empty((B, cap, 7), dtype=torch.float32, device=dev)
    desc = torch.empty((B, cap, 64), dtype=torch.uint8, device=dev)
    counts = (C.c_int * B)()

    def masked():
        check(L.apds_dev_akaze_extract_batch_masked(imgs.data_ptr(), B, side * side * 4, side, side, 4, side * 4, planes.data_ptr(), side, side * side, cap,
                                                    kps.data_ptr(), desc.data_ptr(), cap, counts, None))
        return sum(counts)

    def support15():
        check(L.apds_dev_akaze_extract_batch_masked_support(imgs.data_ptr(), B, side * side * 4, side, side, 4, side * 4, planes.data_ptr(), side, side * side, 15,
                                                            cap, kps.data_ptr(), desc.data_ptr(), cap, counts, None))
        return sum(counts)

    for v in variants:
        if v == "masked":
            timed("support 0 (apds_dev_akaze_extract_batch_masked)", masked, 3, 3, "256 x 1024^2 call")
        if v == "support15":
            timed("support 15", support15, 3, 3, "256 x 1024^2 call")
