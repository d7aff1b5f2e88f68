#!/usr/bin/env python3
"""The overlap search (find_overlaps) on the strip it is for: nine synthetic 1170 x 2532 screenshots of one scrolled page, resident in
HBM (107 MB), each with the same status / title bar on top, the same tab bar below, and a body that repeats part of the shot above.
Reported, from one run:
  find_overlaps       the whole call (tables up, three launches, two waits, the host rules): host clock, median / min / max / spread
  signature_us        the signature launch alone - the one pass over every pixel - and signature_share_of_8TBps = its bytes / its time
                      against the 8 TB/s HBM peak
  cost_us, edge_us    the cost launch (pairs x k) and the edge launch
  preview_reduce_us   stage 1 of the preview reduce (ist_bitmap_preview, 96 x 208 box) per bitmap, in the same run: the in-tree comparator
                      for one source-stationary read of the same bitmap; preview_share_of_8TBps likewise
Kernel times come from a kernel trace of a short child run of this script (rocprofv3 --kernel-trace --stats -- python
tools/bench_overlap.py --trace), averaged per launch; without rocprofv3 they are null and the line says so.
Prints one JSON line.  Usage: python tools/bench_overlap.py [--iters 40] [--warmup 5] [--trace] [--no-kernels]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import imagestitching_amd as ist  # noqa: E402
from imagestitching_amd import _lib as L  # noqa: E402

W, H, N = 1170, 2532, 9
HEADER, FOOTER = 132, 249                      # status + title bar, tab bar + home indicator (rows)
BODY = H - HEADER - FOOTER
STEPS = [700, 1500, 333, 2000, 1100, 2135, 900, 1800]      # page rows scrolled between neighbouring shots (all < BODY: every pair overlaps)
PEAK = 8.0e12


def shots():
    """a page of rendered-text-like rows (runs of a few colours, every row different) cut into N shots"""
    rng = np.random.default_rng(5)
    offsets = np.concatenate([[0], np.cumsum(STEPS)])
    rows = int(offsets[-1]) + BODY
    palette = rng.integers(0, 256, (16, 4), dtype=np.uint8)
    page = palette[rng.integers(0, 16, (rows, W // 6 + 1))].repeat(6, axis=1)[:, :W]
    head = palette[rng.integers(0, 16, (HEADER, W // 6 + 1))].repeat(6, axis=1)[:, :W]
    foot = palette[rng.integers(0, 16, (FOOTER, W // 6 + 1))].repeat(6, axis=1)[:, :W]
    out = []
    for off in offsets:
        s = np.ascontiguousarray(np.concatenate([head, page[off:off + BODY], foot], axis=0))
        s[..., 3] = 255
        out.append(s)
    return out, [(HEADER, FOOTER, BODY - st) for st in STEPS]


def stats(us):
    v = np.array(us)
    return {"median_us": round(float(np.median(v)), 1), "min_us": round(float(v.min()), 1), "max_us": round(float(v.max()), 1),
            "p10_p90_us": round(float(np.percentile(v, 90) - np.percentile(v, 10)), 1)}


def kernel_times():
    """average microseconds per launch of the kernels of a traced child run, by a substring of their names; None without rocprofv3"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--trace"],
                           capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return None
        out = {}
        for row in csv.DictReader(open(files[0])):
            for key in ("ist_overlap_signature_kernel", "ist_overlap_edge_kernel", "ist_overlap_cost_kernel", "ist_preview_partial_kernel"):
                if key in row.get("Name", ""):
                    calls, total = float(row["Calls"]), float(row["TotalDurationNs"])
                    c0, t0 = out.get(key, (0.0, 0.0))
                    out[key] = (c0 + calls, t0 + total)
        return {k: round(t / c / 1e3, 2) for k, (c, t) in out.items() if c}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="a short run for a kernel trace: a few find_overlaps calls and one preview per bitmap")
    ap.add_argument("--no-kernels", action="store_true", help="skip the traced child run")
    a = ap.parse_args()
    px, want = shots()
    bms = [ist.upload_bitmap({"width": W, "height": H, "data": s, "opaque": True}) for s in px]
    got = ist.find_overlaps(bms)
    assert [(p["header"], p["footer"], p["overlap"]) for p in got] == want, got
    if a.trace:
        for _ in range(4):
            ist.find_overlaps(bms)
        for b in bms:
            b.preview(96, 208)
        return
    launches = L.lib.ist_debug_overlap_launches()
    call = []
    for it in range(a.warmup + a.iters):
        t0 = time.perf_counter()
        ist.find_overlaps(bms)
        if it >= a.warmup:
            call.append((time.perf_counter() - t0) * 1e6)
    assert L.lib.ist_debug_overlap_launches() == launches + 3 * (a.warmup + a.iters)
    for b in bms:
        b.close()
    bytes_read = 4 * W * H * N
    res = {"bench": "overlap", "device": torch.cuda.get_device_name(0), "bitmaps": N, "bitmap": [W, H], "bytes_read": bytes_read,
           "iters": a.iters, "warmup": a.warmup, "find_overlaps": stats(call), "records": got}
    k = None if a.no_kernels else kernel_times()
    if k is None:
        res["kernels"] = "not measured (no kernel trace)"
    else:
        sig, pre = k.get("ist_overlap_signature_kernel"), k.get("ist_preview_partial_kernel")
        res.update({"signature_us": sig, "edge_us": k.get("ist_overlap_edge_kernel"), "cost_us": k.get("ist_overlap_cost_kernel"),
                    "preview_reduce_us": pre,
                    "signature_share_of_8TBps": round(bytes_read / (sig * 1e-6) / PEAK, 3) if sig else None,
                    "preview_share_of_8TBps": round(4 * W * H / (pre * 1e-6) / PEAK, 3) if pre else None})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
