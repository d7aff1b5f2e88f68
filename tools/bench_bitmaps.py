#!/usr/bin/env python3
"""Restitch from resident bitmaps against the paths that decode or upload again: nine 4032 x 3024 photo-like JPEG files (made from a
seed), a vertical stitch, four legs timed call by call with a device synchronisation around each call, after a warm-up, the legs
alternating so that drift hits all four alike:
  (a) stitch_files(paths)                    every call reads and decodes the files again, PNG out
  (b) stitch_png(bitmaps)                    decoded once by decode_bitmaps, PNG out
  (c) stitch(host arrays)                    the decoded pixels cross PCIe on every call, pixels out
  (d) stitch(bitmaps)                        pixels out, nothing goes up
Prints one JSON line: per leg the median, min, max and spread (p90 - p10) in milliseconds.
Usage: python tools/bench_bitmaps.py [--reps 15] [--warmup 3] [--seed 0]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import imagestitching_amd as ist  # noqa: E402


def photos(seed, n=9, h=3024, w=4032):
    yy, xx = np.mgrid[0:h, 0:w]
    for k in range(n):
        a = np.stack([128 + 90 * np.sin(xx / (37.0 + k) + yy / 91.0), 128 + 80 * np.cos(xx / 53.0 - yy / (29.0 + k)), 100 + 0.03 * xx + 0.02 * yy], -1)
        yield (a + np.random.default_rng(seed + k).normal(0, 3.0, a.shape)).clip(0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    paths = []
    for k, px in enumerate(photos(a.seed)):
        p = os.path.join(tmp, "in%d.jpg" % k)
        Image.fromarray(px).save(p, "JPEG", quality=90, subsampling=2)
        paths.append(p)
    bitmaps = ist.decode_bitmaps(paths)
    host = [{"width": b.width, "height": b.height, "orientation": b.orientation, "opaque": b.opaque, "fileSize": b.file_size, "data": b.download()}
            for b in bitmaps]
    legs = {
        "a_stitch_files": lambda: ist.stitch_files(paths, "vertical"),      # (both PNG legs hand the file to Python as bytes: one copy each)
        "b_stitch_png_bitmaps": lambda: ist.stitch_png(bitmaps, "vertical"),
        "c_stitch_host_arrays": lambda: ist.stitch(host, "vertical"),
        "d_stitch_bitmaps": lambda: ist.stitch(bitmaps, "vertical"),
    }
    times = {k: [] for k in legs}
    for rep in range(a.warmup + a.reps):
        for name, f in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = f()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            del r
            if rep >= a.warmup:
                times[name].append(dt)
    res = {"bench": "bitmaps", "images": "9 x 4032x3024 JPEG q90 4:2:0", "direction": "vertical", "reps": a.reps, "warmup": a.warmup,
           "jpeg_mb": round(sum(os.path.getsize(p) for p in paths) / 1e6, 2), "device": torch.cuda.get_device_name(0)}
    for name, v in times.items():
        v = np.array(v)
        res[name] = {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(v.min()), 3), "max_ms": round(float(v.max()), 3),
                     "p10_p90_ms": round(float(np.percentile(v, 90) - np.percentile(v, 10)), 3)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
