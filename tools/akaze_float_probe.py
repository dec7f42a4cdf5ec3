"""GPU time of the float (M-SURF, 64 x f32) extraction beside the M-LDB extraction of the same frames: detection is shared, so the difference
is the describe kernel (csrc/akaze_describe_msurf.hip against mldb_kernel). Times are the library's own event pairs around the whole
extraction (apds_dev_timing_enable, "akaze_extract" of apds_dev_last_kernel_ms), frames resident, one stream, nothing else on the GPU.

    python tools/akaze_float_probe.py [--reps 10]          # one 4096^2 frame, one 1024^2 frame, a batch of 16 x 1024^2; JSON lines
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("cubesat-apds_amd")
L, check, kernel_ms = pkg._lib.lib(), pkg._lib.check, pkg._lib.kernel_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.init()
    check(L.apds_dev_timing_enable(1))
    for side, batch in ((4096, 1), (1024, 1), (1024, 16)):
        frames = torch.from_numpy(pkg.synth.make_tile(side, side, frame_index=0)).to(dev).unsqueeze(0).repeat(batch, 1, 1, 1).contiguous()
        for i in range(1, min(batch, 4)):      # a few different frames in a batch; the rest repeat them
            frames[i::4] = torch.from_numpy(pkg.synth.make_tile(side, side, frame_index=i)).to(dev)
        torch.cuda.synchronize()
        cap = (1 << 18) - 1 if batch == 1 else 32768
        kps = torch.empty((batch * cap, 7), dtype=torch.float32, device=dev)
        rows = {"mldb": torch.empty((batch * cap, 64), dtype=torch.uint8, device=dev), "kaze": torch.empty((batch * cap, 64), dtype=torch.float32, device=dev)}
        counts = (C.c_int * batch)()
        image_stride, row_stride = frames.stride(0), frames.stride(1)

        def extract(kind):
            fn = L.apds_dev_akaze_extract_batch_masked_support if kind == "mldb" else L.apds_dev_akaze_extract_float_batch
            check(fn(frames.data_ptr(), batch, image_stride, side, side, 4, row_stride, None, 0, 0, 0, cap, kps.data_ptr(), rows[kind].data_ptr(), cap, counts, None))

        out = {"side": side, "batch": batch}
        for kind in ("mldb", "kaze"):
            for _ in range(args.warmup):
                extract(kind)
            check(L.apds_stream_synchronize(None))
            kernel_ms("akaze_extract")          # drop what the warm-up recorded
            for _ in range(args.reps):
                extract(kind)
            check(L.apds_stream_synchronize(None))
            ms, calls = kernel_ms("akaze_extract")
            out[kind + "_ms"] = round(ms / max(calls, 1), 4)       # (the call returns the sum over the recorded extractions)
            out[kind + "_calls"] = calls
            out["keypoints"] = int(sum(counts))
        out["kaze_over_mldb"] = round(out["kaze_ms"] / out["mldb_ms"], 3) if out["mldb_ms"] else None
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
