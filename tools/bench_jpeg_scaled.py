#!/usr/bin/env python3
"""Reduced-size JPEG decode (decode_bitmaps(files, scale=d)) on the files it is for: nine 12 MP 4:2:0 baseline JPEGs, 4032 x 3024 (the
page's cap, index.js:311), at d = 1, 2, 4, 8 in ONE process.  The comparator is d = 1 of the same run: the full-size code path.
Per d:
  decode_ms       host clock around decode_bitmaps (files in, bitmaps resident), median / min over --iters after --warmup; the arms
                  alternate call by call in an order that rotates, so --iters and --warmup are multiples of 4
  reconstruct_ms  IST_PHASE_RECONSTRUCT of a call with phase timing on (every phase then ends with a stream synchronisation)
  resident_bytes  ist_debug_bitmap_bytes of the nine bitmaps (exact: 4 sw sh + the tail, rounded to 256 per bitmap)
Then two uses:
  thumbnails      the 3 x 3 grid of 96 x 96 'fill' cells from files: decode at 1 / 1 + thumbnails + release, against
                  thumbnails_from_files (which decodes every photo at 1 / 8)
  restitch        the Android-capped vertical plan (platform 'android': bilinear, edge anti-aliasing on) from resident d = 1 bitmaps against resident
                  d = 4 bitmaps: the same plan and canvas, a sixteenth of the source bytes
Prints one JSON line.  Usage: python tools/bench_jpeg_scaled.py [--iters 16] [--warmup 4]"""
import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import imagestitching_amd as ist  # noqa: E402
from imagestitching_amd import _lib as L  # noqa: E402

W, H, N, CELL = 4032, 3024, 9, (96, 96)
SCALES = (1, 2, 4, 8)


def photos():
    """nine photo-like files: smooth colour fields + noise, three pixel sets in rotation at three qualities"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    files = []
    for k in range(3):
        rng = np.random.default_rng(20 + k)
        a = np.empty((H, W, 3), np.float32)
        for c in range(3):
            fx, fy, ph = rng.uniform(0.5, 3.0, 3)
            a[..., c] = 127.5 + 100 * np.sin(fx * xx / W * 6.28 + fy * yy / H * 6.28 + ph * 2)
        a += rng.integers(-12, 13, a.shape)
        im = Image.fromarray(np.clip(a, 0, 255).astype(np.uint8))
        for q in (92, 88, 84):
            b = io.BytesIO()
            im.save(b, "JPEG", quality=q, subsampling=2)
            files.append(b.getvalue())
    return files[:N]


def stats(ms):
    v = np.array(ms)
    return {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3)}


def clock(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def close(bms):
    for b in bms:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    files = photos()
    res = {"bench": "jpeg_scaled", "files": N, "size": [W, H], "file_bytes": sum(len(f) for f in files), "iters": a.iters, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "scales": {}}
    reps = a.warmup + a.iters
    wall = {d: [] for d in SCALES}
    recon = {d: [] for d in SCALES}
    for it in range(reps):                               # the arms alternate call by call, and the order rotates: where a call stands in
        for d in SCALES[it % 4:] + SCALES[:it % 4]:      # the round moves its wall time by up to 1 ms whatever its scale (it follows the
            t, bms = clock(lambda: ist.decode_bitmaps(files, scale=d))      # release of the previous arm's bitmaps), so every arm takes every place
            close(bms)
            if it >= a.warmup:
                wall[d].append(t)
    ist.set_phase_timing(True)
    for it in range(reps):
        for d in SCALES:
            close(ist.decode_bitmaps(files, scale=d))
            if it >= a.warmup:
                recon[d].append(ist.last_phase_times()["reconstruct"])
    ist.set_phase_timing(False)
    for d in SCALES:
        base = L.lib.ist_debug_bitmap_bytes()
        bms = ist.decode_bitmaps(files, scale=d)
        res["scales"][str(d)] = {"decode_ms": stats(wall[d]), "reconstruct_ms": stats(recon[d]), "resident_bytes": L.lib.ist_debug_bitmap_bytes() - base,
                                 "bitmap": list(bms[0].shape[1::-1])}
        close(bms)
    for d in SCALES[1:]:
        s, one = res["scales"][str(d)], res["scales"]["1"]
        s["decode_vs_full"] = round(s["decode_ms"]["median"] / one["decode_ms"]["median"], 3)
        s["reconstruct_vs_full"] = round(s["reconstruct_ms"]["median"] / one["reconstruct_ms"]["median"], 3)

    def grid_full():
        bms = ist.decode_bitmaps(files)
        r = ist.thumbnails(bms, CELL)
        close(bms)
        return r
    full, fast = [], []
    for it in range(reps):
        t, r1 = clock(grid_full)
        t2, r2 = clock(lambda: ist.thumbnails_from_files(files, CELL))
        if it >= a.warmup:
            full.append(t)
            fast.append(t2)
    diff = max(int(np.abs(x.astype(np.int32) - y.astype(np.int32)).max()) for x, y in zip(r1, r2))
    res["thumbnails"] = {"cell": list(CELL), "from_full_bitmaps_ms": stats(full), "thumbnails_from_files_ms": stats(fast),
                         "speedup": round(float(np.median(full) / np.median(fast)), 2), "max_abs_difference": diff}

    opts = {"platform": "android"}
    b1, b4 = ist.decode_bitmaps(files), ist.decode_bitmaps(files, scale=4)
    p = ist.plan(b1, "vertical", opts)
    t1, t4 = [], []
    for it in range(reps):
        t, r1 = clock(lambda: ist.stitch(b1, "vertical", opts))
        t2, r4 = clock(lambda: ist.stitch(b4, "vertical", opts))
        if it >= a.warmup:
            t1.append(t)
            t4.append(t2)
    assert (r1["width"], r1["height"]) == (r4["width"], r4["height"]) == (p.canvas_w, p.canvas_h)
    res["restitch"] = {"plan": "android, vertical", "canvas": [p.canvas_w, p.canvas_h], "scale_down": round(float(p.scale_down), 4),
                       "from_scale_1_ms": stats(t1), "from_scale_4_ms": stats(t4), "speedup": round(float(np.median(t1) / np.median(t4)), 2)}
    close(b1 + b4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
