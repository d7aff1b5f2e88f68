#!/usr/bin/env python3
"""The grid of thumbnails (ist_bitmaps_thumbs) on the bitmaps a grid is for: 9 (the page's cap, index.js:311) and 64 (BASELINE
configs[4]'s count) resident 12 MP opaque bitmaps, 4032 x 3024, every second one with EXIF orientation 6, into 96 x 96 'fill' cells.
Two arms, in the same process, alternated call by call, host clock around each (the call returns host pixels):
  thumbnails    ONE thumbnails(bitmaps, (96, 96)) call: a launch pair, one table copy, one copy down
  preview_loop  Bitmap.preview(96, 96) bitmap after bitmap - all a host had before: per image two launches, a stream wait and a small
                copy; it applies no crop and no turn, and reads every bitmap whole (48.8 MB) where the grid reads its 3024 x 3024
                window (36.6 MB): the same source bytes or more
Per workload and arm: median / min / max / p10-p90 spread in microseconds over --iters timed repeats after --warmup.  window_bytes is
4 * sum of the windows' pixels: divide it by the stage-1 time of a kernel trace (rocprofv3 --kernel-trace --stats -- python
tools/bench_thumbs.py --trace) for the reduce's share of 8 TB/s.  --trace runs only the thumbnails arm, a few calls per workload.
Prints one JSON line.  Usage: python tools/bench_thumbs.py [--iters 60] [--warmup 10] [--counts 9,64] [--trace]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import imagestitching_amd as ist  # noqa: E402
from imagestitching_amd import _lib as L  # noqa: E402

W, H, CELL = 4032, 3024, (96, 96)


def bitmaps(n):
    """n resident opaque bitmaps: three different pixel sets in rotation, every second bitmap stored for a quarter turn"""
    rng = np.random.default_rng(11)
    px = []
    for _ in range(3):
        a = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        a[..., 3] = 255
        px.append(a)
    return [ist.upload_bitmap({"width": W, "height": H, "data": px[k % 3], "opaque": True, "orientation": 6 if k & 1 else 1}) for k in range(n)]


def stats(us):
    v = np.array(us)
    return {"median_us": round(float(np.median(v)), 1), "min_us": round(float(v.min()), 1), "max_us": round(float(v.max()), 1),
            "p10_p90_us": round(float(np.percentile(v, 90) - np.percentile(v, 10)), 1)}


def clock(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e6, r


def bench(n, a):
    bms = bitmaps(n)
    lay = ist.thumbnail_layout(bms, CELL, "fill")
    window_bytes = 4 * sum(t["window"][2] * t["window"][3] for t in lay)
    pairs = L.lib.ist_debug_thumb_launches()
    new, old = [], []
    reps = (2 if a.trace else a.warmup) + (3 if a.trace else a.iters)
    for it in range(reps):
        t, r = clock(lambda: ist.thumbnails(bms, CELL))
        del r
        if it >= a.warmup:
            new.append(t)
        if a.trace:
            continue
        t, r = clock(lambda: [b.preview(*CELL) for b in bms])
        del r
        if it >= a.warmup:
            old.append(t)
    assert L.lib.ist_debug_thumb_launches() == pairs + reps      # one launch pair per call: every bitmap is opaque
    res = {"bitmaps": n, "window_bytes": window_bytes, "bitmap_bytes": 4 * W * H * n}
    if not a.trace:
        res["thumbnails"] = stats(new)
        res["preview_loop"] = stats(old)
        res["speedup"] = round(res["preview_loop"]["median_us"] / res["thumbnails"]["median_us"], 2)
        res["thumbnails_minus_loop_us"] = round(res["thumbnails"]["median_us"] - res["preview_loop"]["median_us"], 1)
    for b in bms:
        b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--counts", default="9,64")
    ap.add_argument("--trace", action="store_true", help="a short run of the thumbnails arm alone, for a kernel trace")
    a = ap.parse_args()
    res = {"bench": "thumbs", "cell": list(CELL), "mode": "fill", "bitmap": [W, H], "iters": a.iters, "warmup": a.warmup, "trace": a.trace,
           "device": torch.cuda.get_device_name(0), "workloads": {}}
    for n in [int(c) for c in a.counts.split(",")]:
        res["workloads"][str(n)] = bench(n, a)
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
