"""Batched PNG export against a loop of single stitch_png() calls, on one MI355X.  Prints ONE JSON line.

Workloads (what a stitching service receives: many small independent onStitch requests, each ending in the export step
wx.canvasToTempFilePath({fileType: 'png'}), utils/canvas.js:205-242, pages/index/index.js:1577-1579):
  A  tools/bench_batch.py's A: 64 requests of 9 x 1080x1920, vertical, identity widths
  B  tools/bench_batch.py's B: 64 requests of 4-9 images of mixed sizes, bilinear, seeded
  C  64 requests shaped like the reference's device-capped plans: 9 images resampled into a ~606x4096 vertical canvas
At PNG levels 1 (Paeth + run-length + Huffman) and 0 (stored), each with warm-up and the two variants alternated in one process:
a loop of stitch_png(), every file released before the next request, vs ONE stitch_png_batch() (wall clock: host buffers in, PNG
files out).  Reported: microseconds per request, batch / loop, and the compression launches the batch made.  Every batch file is
checked against the loop's: the same IHDR and the same zlib stream byte for byte.

  python tools/bench_png_batch.py [--workloads ABC] [--levels 10] [--reps 5] [--warmup 2]
  rocprofv3 --kernel-trace --stats -d DIR -o png_batch -- python tools/bench_png_batch.py --reps 1 --warmup 0     (launch counts)
"""
import argparse
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import bench_batch  # noqa: E402  (workloads A and B, their host pixels)
import imagestitching_amd as ist  # noqa: E402
from imagestitching_amd import _lib as L  # noqa: E402


def workload(name):
    if name in "AB":
        return bench_batch.workload(name)
    # C: 9 photos of mixed aspect, width-normalised to 606 px and stacked to ~4096 rows (the reference caps a plan's canvas by the
    # device's limits; BASELINE.md section 1 lists 606x4096 as a typical such plan)
    rng = np.random.default_rng(20261016)
    reqs = []
    for _ in range(bench_batch.N_REQ):
        widths = [606] + [int(rng.integers(700, 1300)) for _ in range(8)]           # mode 'min': every image scaled to 606 px wide
        sizes = [(int(w), int(round(int(w) * 4096 / 9 / 606))) for w in rng.permutation(widths)]
        reqs.append((sizes, "vertical", {"filter": "bilinear", "mode": "min"}))
    return reqs


def zstream(png):
    """(IHDR, concatenated IDAT data) of a PNG file"""
    png = bytes(png)
    at, ihdr, idat = 8, b"", b""
    while at < len(png):
        n, = struct.unpack(">I", png[at:at + 4])
        kind = png[at + 4:at + 8]
        if kind == b"IHDR":
            ihdr = png[at + 8:at + 8 + n]
        elif kind == b"IDAT":
            idat += png[at + 8:at + 8 + n]
        at += 12 + n
    return ihdr, idat


def leg(requests, level, reps, warmup):
    opts = [dict(o, pngLevel=level) for _, _, o in requests]
    before = L.lib.ist_debug_png_batch_launches()
    got = ist.stitch_png_batch(requests, level=level)
    launches = L.lib.ist_debug_png_batch_launches() - before
    identical, png_bytes, canvas_bytes = True, 0, 0
    for r, o, g in zip(requests, opts, got):
        w = ist.stitch_png(r[0], r[1], o)
        identical = identical and zstream(g["png"]) == zstream(w["png"])
        png_bytes += len(g["png"])
        canvas_bytes += 4 * g["width"] * g["height"]
    del got
    times = {"loop": [], "batch": []}

    def loop():                      # every file released before the next request
        for r, o in zip(requests, opts):
            ist.stitch_png(r[0], r[1], o)

    def batch():
        ist.stitch_png_batch(requests, level=level)

    for i in range(warmup + reps):
        for name, fn in (("loop", loop), ("batch", batch)) if i % 2 == 0 else (("batch", batch), ("loop", loop)):
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if i >= warmup:
                times[name].append(dt * 1e6)
    lu, bu = statistics.median(times["loop"]), statistics.median(times["batch"])
    n = len(requests)
    return {"us_per_request_loop": round(lu / n, 1), "us_per_request_batch": round(bu / n, 1), "batch_over_loop": round(bu / lu, 4),
            "compression_launches": int(launches), "identical_zlib": bool(identical), "png_over_raw": round(png_bytes / canvas_bytes, 4),
            "samples_us_per_request": {k: [round(v / n, 1) for v in vs] for k, vs in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="ABC")
    ap.add_argument("--levels", default="10")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    guard = bench.StdoutGuard()
    assert torch.cuda.is_available(), "bench_png_batch needs a GPU"
    line = {"metric": "batched PNG export: us per request, loop of stitch_png vs one stitch_png_batch", "requests": bench_batch.N_REQ,
            "device": torch.cuda.get_device_name(0), "kernel_source_sha": bench.kernel_source_sha()}
    what = {"A": "64 x 9 x 1080x1920 vertical, identity widths (COPY)", "B": "64 mixed-size requests of 4-9 images, bilinear, seeded",
            "C": "64 x 9 images resampled into ~606x4096 vertical canvases (device-capped plans)"}
    for w in args.workloads:
        reqs = workload(w)
        pixels = bench_batch.host_images(reqs)
        requests = [([{"width": a.shape[1], "height": a.shape[0], "data": a, "opaque": True} for a in imgs], d, o)
                    for (_, d, o), imgs in zip(reqs, pixels)]
        r = {"what": what[w], "images": sum(len(s) for s, _, _ in reqs)}
        for lv in args.levels:
            r["level_" + lv] = leg(requests, int(lv), args.reps, args.warmup)
        line["workload_" + w] = r
    guard.emit(json.dumps(line))


if __name__ == "__main__":
    main()
