#!/usr/bin/env python3
"""Builds the level-of-detail 0..2 database of one synthetic mosaic three ways, alternating in one process:

    (a) host MosaicedDataset, nearest   - the path before the device mosaic: numpy windows, three band uploads per tile
    (b) DeviceMosaic, nearest           - apds_mosaic_tile_extract_batch, the same rows bit for bit
    (c) DeviceMosaic, Lanczos           - the reference's read_as(.., Lanczos)

and, with --overviews, a fourth:

    (d) DeviceMosaic with overviews, Lanczos - the read of the reference's COG: level k of the cubic pyramid serves level of detail k

with `--tile`-pixel tiles (the mosaic is cut as a 4-level pyramid, so --size 8192 gives 1024 x 1024 tiles: 64 + 16 + 4) and batch = all
tiles of a level. Prints, per level and way: seconds (host clock around calls that end in a device synchronise), the resampling kernels'
own time (hipEvents, apds_dev_last_kernel_ms "mosaic_resample"), the algorithmic bytes of the level (12 H W read + 12 H W / 4^lod
written; way (d) copies an overview: 12 H W / 4^lod read and as much written) over that time, and the keypoint count; with --overviews
also the build of the pyramid (host seconds and the kernels' own time on fresh handles, median, against 12 bytes per source pixel read
plus 12 per destination pixel written, summed over the steps); last line: one JSON object with everything.

    python tools/mosaic_probe.py --size 8192 --reps 2 [--overviews]

With --db-build N it does one other thing instead: the whole table of the mosaic (--levels levels, --batch tiles per call, nearest) is
built through the two-step path (batch extraction to the host, one apds_db_insert_image per tile) and through the device path
(apds_mosaic_tiles_to_db per group), alternating in one process: one warm-up of each, then N timed builds of each (host clock around calls
that end in a device synchronise). Prints every time, the medians and the spread (max - min) of each path, and checks that both paths
store the same number of rows per image.

    python tools/mosaic_probe.py --size 4096 --levels 3 --batch 16 --db-build 5
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def synthetic_mosaic(pkg, size):
    base = pkg.synth.make_tile(2048, 2048, frame_index=11, channels=3).astype(np.float32)
    reps = (size + 2047) // 2048
    bands = np.empty((3, size, size), np.float32)
    yy, xx = np.meshgrid(np.linspace(0.8, 1.2, size, dtype=np.float32), np.linspace(0.9, 1.1, size, dtype=np.float32), indexing="ij")
    for b, (ch, gain, off) in enumerate(((2, 3.0, 10.0), (1, 2.0, -5.0), (0, 1.5, 0.0))):
        bands[b] = np.tile(base[:, :, ch], (reps, reps))[:size, :size] * gain * yy * xx + off
    bands[0, 5:9, 7:12] = np.nan
    return bands


def db_build(pkg, args):
    """the same table through both paths, alternating: seconds per whole build"""
    ge, pp, fd = pkg.geotiff_extractor, pkg.preprocessor, pkg.feature_database
    dev = ge.DeviceMosaic(synthetic_mosaic(pkg, args.size))
    dev.datasets_min_max()
    times, rows = {"host insert": [], "device insert": []}, {}
    for rep in range(args.db_build + 1):                                      # rep 0 warms every shape up and is not reported
        for name, device_insert in (("host insert", False), ("device insert", True)):
            table, images = fd.KeypointTable(6_000_000), pp.ImageTable()
            s = time.perf_counter()
            out = pp.process_lod_from_mosaic(table, images, dev, args.levels, batch=args.batch, device_insert=device_insert)
            e = time.perf_counter()
            assert len(table) == sum(n for level in out for _, n in level)
            rows.setdefault(name, out)
            assert rows[name] == out and rows["host insert"] == out, "the two paths store different rows per image"
            if rep:
                times[name].append(e - s)
            table.close()
    tiles = sum(len(level) for level in rows["host insert"])
    total = sum(n for level in rows["host insert"] for _, n in level)
    tile, _, _ = pp.tile_grid(dev.raster_size(), args.levels, 0)
    print(f"DB build of a {args.size} x {args.size} mosaic: {args.levels} levels, {tiles} tiles of {tile[0]} x {tile[1]}, batch {args.batch}, {total} rows; "
          f"{args.db_build} timed builds of each path after one warm-up, alternating")
    summary = {}
    for name, t in times.items():
        summary[name] = dict(seconds=t, median=float(np.median(t)), spread=float(max(t) - min(t)))
        print(f"{name:14s}: median {summary[name]['median']:.4f} s, spread (max - min) {summary[name]['spread']:.4f} s  [{' '.join('%.4f' % x for x in t)}]")
    print(json.dumps(dict(size=args.size, levels=args.levels, batch=args.batch, tiles=tiles, tile=tile[0], rows=total, db_build=summary)))
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--overviews", action="store_true", help="also build the overview pyramid and read the levels of detail from it (way d)")
    ap.add_argument("--db-build", type=int, default=0, metavar="N", help="instead: build the whole table N times through the two-step path and "
                    "N times through the device path (apds_mosaic_tiles_to_db), alternating, and print both times")
    ap.add_argument("--batch", type=int, default=16, help="tiles per library call of --db-build")
    args = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first, as bench.py does)
    pkg = graft.load_package()
    L = pkg.lib()
    assert L.apds_device_count() > 0, "no HIP device: this probe measures on the GPU"
    if args.db_build > 0:
        return db_build(pkg, args)
    ge, pp, fd = pkg.geotiff_extractor, pkg.preprocessor, pkg.feature_database
    t0 = time.perf_counter()
    bands = synthetic_mosaic(pkg, args.size)
    host = ge.MosaicedDataset(bands)
    t1 = time.perf_counter()
    dev = host.to_device()
    t2 = time.perf_counter()
    mm_host = host.datasets_min_max().as_array()
    t3 = time.perf_counter()
    L.apds_dev_timing_enable(1)
    mm_dev = dev.datasets_min_max().as_array()
    t4 = time.perf_counter()
    minmax_ms, _ = pkg._lib.kernel_ms("mosaic_minmax")
    assert np.array_equal(mm_host, mm_dev), (mm_host, mm_dev)
    n_bytes = 12.0 * args.size * args.size
    print(f"mosaic {args.size} x {args.size} x 3 f32 ({n_bytes / 1e9:.2f} GB): synthesis {t1 - t0:.2f} s, upload {t2 - t1:.3f} s")
    print(f"min/max: host nanmin/nanmax {t3 - t2:.3f} s | device call {t4 - t3:.4f} s, kernels {minmax_ms:.3f} ms = {n_bytes / minmax_ms / 1e6:.0f} GB/s of the {n_bytes / 1e9:.2f} GB read")
    amount = 4                                                                # tile = size / 8
    tile, _, _ = pp.tile_grid(host.raster_size(), amount, 0)
    ways = [("a host nearest", host, "nearest"), ("b device nearest", dev, "nearest"), ("c device lanczos", dev, "lanczos")]
    build = None
    if args.overviews:
        runs = []
        for rep in range(args.reps + 1):                                      # a fresh handle each time: a handle builds once; rep 0 warms up
            dev_ov = host.to_device()
            pkg._lib.kernel_ms("mosaic_overviews")
            s = time.perf_counter()
            n_levels = dev_ov.build_overviews()
            e = time.perf_counter()
            ms, launches = pkg._lib.kernel_ms("mosaic_overviews")
            if rep:
                runs.append((e - s, ms, launches))
            if rep < args.reps:
                dev_ov.close()
        sizes = [dev_ov.level_size(k) for k in range(n_levels + 1)]
        algo = sum(12.0 * (sizes[k - 1][0] * sizes[k - 1][1] + sizes[k][0] * sizes[k][1]) for k in range(1, n_levels + 1))
        ms = float(np.median([r[1] for r in runs]))
        build = dict(levels=n_levels, sizes=sizes, seconds=float(np.median([r[0] for r in runs])), kernel_ms=ms, launches=runs[0][2], algorithmic_bytes=algo)
        print(f"overviews: {n_levels} levels {' '.join('%dx%d' % s for s in sizes[1:])}, build call {build['seconds']:.4f} s, kernels ({runs[0][2]} launches) "
              f"{ms:.3f} ms [{' '.join('%.3f' % r[1] for r in runs)}] = {algo / ms / 1e6:.0f} GB/s of the {algo / 1e9:.2f} GB read + written")
        assert np.array_equal(dev_ov.datasets_min_max().as_array(), mm_dev)
        ways.append(("d device overviews", dev_ov, "lanczos"))
    results = {w[0]: {lod: [] for lod in range(args.levels)} for w in ways}
    for rep in range(args.reps + 1):                                          # rep 0 warms every shape up and is not reported
        for name, ds, mode in ways:
            table, images = fd.KeypointTable(6_000_000), pp.ImageTable()
            for lod in range(args.levels):
                _, columns, rows = pp.tile_grid(ds.raster_size(), amount, lod)
                pkg._lib.kernel_ms("mosaic_resample")                         # drop what is pending
                s = time.perf_counter()
                out = pp.downscale_from_lod(table, images, ds, amount, lod, batch=columns * rows, resample=mode)
                e = time.perf_counter()
                ms, launches = pkg._lib.kernel_ms("mosaic_resample")
                if rep:
                    results[name][lod].append(dict(seconds=e - s, resample_ms=ms, resample_calls=launches, tiles=len(out), keypoints=sum(n for _, n in out)))
            table.close()
    print(f"tiles of {tile[0]} x {tile[1]}, batch = all tiles of a level, {args.reps} timed repetitions after one warm-up (median shown)")
    for lod in range(args.levels):
        for name, _, _ in ways:
            algo = n_bytes * (2.0 * 0.25 ** lod if name.startswith("d") else 1.0 + 0.25 ** lod)
            r = results[name][lod]
            sec = float(np.median([x["seconds"] for x in r]))
            ms = float(np.median([x["resample_ms"] for x in r]))
            rate = f"{algo / ms / 1e6:8.0f} GB/s of {algo / 1e9:.2f} GB" if ms > 0 else "       - (no resampling kernel)"
            print(f"lod {lod} {name:18s}: {r[0]['tiles']:3d} tiles {sec:8.3f} s  [{' '.join('%.3f' % x['seconds'] for x in r)}]  resample {ms:8.3f} ms {rate}  keypoints {r[0]['keypoints']}")
    print(json.dumps(dict(size=args.size, tile=tile[0], reps=args.reps, minmax_ms=minmax_ms, host_minmax_s=t3 - t2, upload_s=t2 - t1, overviews=build,
                          results={k: {str(l): v for l, v in d.items()} for k, d in results.items()})))
    dev.close()
    if args.overviews:
        dev_ov.close()


if __name__ == "__main__":
    main()
