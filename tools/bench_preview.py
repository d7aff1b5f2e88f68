#!/usr/bin/env python3
"""The preview reduce (ist_preview_device) on the canvases a preview is for, fitted into the reference's 343 x 457 node:
  vertical     4032 x 27216  ->  68 x 457   (nine 12 MP photos)
  horizontal  36288 x  3024  -> 343 x  29
  long         8000 x 384000 ->  10 x 457   (BASELINE configs[4])
Opaque sources in HBM, at least 3 buffer sets per shape in rotation, every launch timed with device events after a warm-up.  Per
shape: median / min / max / p10-p90 spread in microseconds, and 4 * w * h over the median as a share of 8 TB/s.
The comparator is the path a host had before: the same shrink as a one-draw filter 'area' job (Stitcher.compile_ops).  It runs in
the same process, alternating with the reduce, on the first two shapes only - on the third it is per-pixel taps by the hundred
thousand, a kernel that would run for seconds.
--e2e adds stitch_files of nine 12 MP JPEG files with and without the 'preview' option, alternating, host clock around each call.
Prints one JSON line.  Usage: python tools/bench_preview.py [--iters 60] [--warmup 10] [--sets 3] [--e2e] [--skip-long]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import imagestitching_amd as ist  # noqa: E402
from imagestitching_amd import _lib as L  # noqa: E402

S = importlib.import_module("imagestitching_amd.stitch")
BOX = (343, 457)
SHAPES = [("vertical", 4032, 27216, True), ("horizontal", 36288, 3024, True), ("long", 8000, 384000, False)]     # (name, w, h, run the comparator)


def source(w, h, seed):
    """an opaque w x h image made on the device, a band of rows at a time"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    step = max(1, (256 << 20) // (4 * w))
    for y in range(0, h, step):
        n = min(step, h - y)
        t[y:y + n] = torch.randint(0, 256, (n, w, 4), dtype=torch.uint8, device="cuda", generator=g)
    t[..., 3] = 255
    return t


def area_job(w, h, pw, ph):
    ops = (L.Op * 1)()
    ops[0].kind, ops[0].image = 1, 0
    ops[0].m[:] = [1, 0, 0, 1, 0, 0]
    ops[0].s[:] = [0, 0, w, h]
    ops[0].d[:] = [0, 0, pw, ph]
    descs = S._descs([{"width": w, "height": h, "opaque": True}])
    return ist.Stitcher(0).compile_ops(pw, ph, ops, 1, descs, 1, filter="area")


def stats(us, nbytes=None):
    v = np.array(us)
    r = {"median_us": round(float(np.median(v)), 2), "min_us": round(float(v.min()), 2), "max_us": round(float(v.max()), 2),
         "p10_p90_us": round(float(np.percentile(v, 90) - np.percentile(v, 10)), 2)}
    if nbytes:
        r["tb_per_s"] = round(nbytes / (float(np.median(v)) * 1e-6) / 1e12, 3)
        r["share_of_8_tb_s"] = round(nbytes / (float(np.median(v)) * 1e-6) / 8e12, 4)
        r["ps_per_source_byte"] = round(float(np.median(v)) * 1e6 / nbytes, 4)
    return r


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def bench_shape(name, w, h, compare, a):
    pw, ph = ist.preview_fit(w, h, *BOX)
    sets = [source(w, h, 100 + k) for k in range(a.sets)]
    outs = [torch.empty((ph, pw, 4), dtype=torch.uint8, device="cuda") for _ in range(a.sets)]
    job = area_job(w, h, pw, ph) if compare else None
    job_outs = [torch.empty((ph, pw, 4), dtype=torch.uint8, device="cuda") for _ in range(a.sets)] if compare else None
    before = L.lib.ist_debug_preview_launches()
    new, old = [], []
    for it in range(a.warmup + a.iters):
        k = it % a.sets
        t = timed(lambda: ist.preview_device(sets[k], pw, ph, out=outs[k], opaque=True))
        if it >= a.warmup:
            new.append(t)
        if compare:
            t = timed(lambda: job.launch([sets[k]], job_outs[k]))
            if it >= a.warmup:
                old.append(t)
    assert L.lib.ist_debug_preview_launches() == before + a.warmup + a.iters
    res = {"shape": "%dx%d -> %dx%d" % (w, h, pw, ph), "ratio": [round(w / pw, 1), round(h / ph, 1)], "source_mb": round(4 * w * h / 1e6, 1),
           "preview": stats(new, 4 * w * h)}
    if compare:
        res["area_job"] = stats(old, 4 * w * h)
        res["speedup"] = round(res["area_job"]["median_us"] / res["preview"]["median_us"], 2)
        d = (outs[0].to(torch.int16) - job_outs[0].to(torch.int16)).abs()
        res["max_abs_diff_vs_area_job"] = int(d.max())
        res["bytes_differing_vs_area_job"] = int((d != 0).sum())
    return res


def bench_e2e(a):
    from PIL import Image
    tmp = tempfile.mkdtemp()
    paths = []
    yy, xx = np.mgrid[0:3024, 0:4032]
    for k in range(9):
        px = np.stack([128 + 90 * np.sin(xx / (37.0 + k) + yy / 91.0), 128 + 80 * np.cos(xx / 53.0 - yy / (29.0 + k)), 100 + 0.03 * xx + 0.02 * yy], -1)
        px = (px + np.random.default_rng(k).normal(0, 3.0, px.shape)).clip(0, 255).astype(np.uint8)
        paths.append(os.path.join(tmp, "in%d.jpg" % k))
        Image.fromarray(px).save(paths[-1], "JPEG", quality=90, subsampling=2)
    legs = {"without_preview": {}, "with_preview": {"preview": BOX}}
    times = {k: [] for k in legs}
    for rep in range(a.warmup + a.iters):
        for name, opts in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = ist.stitch_files(paths, "vertical", opts, copy=False)
            dt = (time.perf_counter() - t0) * 1e3
            del r
            if rep >= a.warmup:
                times[name].append(dt)
    out = {}
    for name, v in times.items():
        v = np.array(v)
        out[name] = {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(v.min()), 3), "max_ms": round(float(v.max()), 3),
                     "p10_p90_ms": round(float(np.percentile(v, 90) - np.percentile(v, 10)), 3)}
    out["preview_adds_ms"] = round(out["with_preview"]["median_ms"] - out["without_preview"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--skip-long", action="store_true")
    a = ap.parse_args()
    assert a.iters >= 50 and a.sets >= 3, "at least 50 timed iterations over at least 3 buffer sets"
    res = {"bench": "preview", "box": list(BOX), "iters": a.iters, "warmup": a.warmup, "buffer_sets": a.sets, "device": torch.cuda.get_device_name(0),
           "shapes": {}}
    for name, w, h, compare in SHAPES:
        if name == "long" and a.skip_long:
            continue
        res["shapes"][name] = bench_shape(name, w, h, compare, a)
        torch.cuda.empty_cache()
    if a.e2e:
        res["files_to_png_9x12mp"] = bench_e2e(a)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
