#!/usr/bin/env python3
"""The lossless JPEG join on the files it is for: nine 12 MP 4:2:0 baseline JPEGs of one quality (4032 x 3024, synthesised as
tools/bench_jpeg_scaled.py synthesises its photos, but at ONE quality: a join needs one set of quantisation tables), stitched 1:1 into
one 4032 x 27216 JPEG, by two routes in ONE process:
  join    join_jpeg(files, 'vertical'): Huffman decode -> the join kernel -> Huffman code; no pixel exists
  pixels  decode_bitmaps(files) then stitch_jpeg(bitmaps, quality=90, subsampling='420'): the route there was before
The arms alternate call by call and the order rotates ('reduced-size decode': where a call stands in the round moves its
wall time whatever it does), so --iters and --warmup are multiples of 2.  Reported:
  wall_ms        host clock around each route (files in, file out; both end in a synchronised read-back), median / min / max
  file_bytes     both files against the sum of the sources
  join_kernel    the join kernel's time from a rocprofv3 --kernel-trace --stats run of its own (a child process: tracing slows the host,
                 so no wall time is taken there), and that time as a fraction of the floor: 4 bytes per coefficient (2 read, 2
                 written) at 8 TB/s.  Skipped with --no-trace or where rocprofv3 is missing ('not measured').
Prints one JSON line and, with --out, writes it.  Usage: python tools/bench_jpeg_join.py [--iters 10] [--warmup 2] [--out FILE]"""
import argparse
import csv
import glob
import io
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

W, H, N, QUALITY = 4032, 3024, 9, 90
PEAK_BYTES_PER_S = 8e12


def photos(w=W, h=H, n=N):
    """photo-like files: smooth colour fields + noise, three pixel sets in rotation, one quality"""
    from PIL import Image
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    files = []
    for k in range(3):
        rng = np.random.default_rng(20 + k)
        a = np.empty((h, w, 3), np.float32)
        for c in range(3):
            fx, fy, ph = rng.uniform(0.5, 3.0, 3)
            a[..., c] = 127.5 + 100 * np.sin(fx * xx / w * 6.28 + fy * yy / h * 6.28 + ph * 2)
        a += rng.integers(-12, 13, a.shape)
        b = io.BytesIO()
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(b, "JPEG", quality=QUALITY, subsampling=2)
        files.append(b.getvalue())
    return [files[k % 3] for k in range(n)]


def coefficients(w, h, n):
    """coefficients of the joined 4:2:0 file: 6 blocks of 64 per 16 x 16 MCU"""
    return n * (-(-w // 16)) * (-(-h // 16)) * 6 * 64


def stats(ms):
    v = np.array(ms)
    return {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3)}


def clock(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def traced_kernel_us(size):
    """the join kernel's durations (us) in a rocprofv3 --kernel-trace --stats run of a child that joins the same files"""
    if shutil.which("rocprofv3") is None:
        return None
    out = tempfile.mkdtemp(prefix="join_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "t", "--",
           sys.executable, os.path.abspath(__file__), "--child", "--size", "%dx%dx%d" % size]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=out)
    found = glob.glob(out + "/**/*_kernel_trace.csv", recursive=True)
    if r.returncode != 0 or not found:
        sys.stderr.write(r.stdout[-1000:] + r.stderr[-2000:])
        return None
    rows = sorted((row for row in csv.DictReader(open(found[0])) if "ist_jpeg_join_kernel" in row["Kernel_Name"]), key=lambda row: int(row["Start_Timestamp"]))
    us = [(int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3 for row in rows]      # in launch order
    shutil.rmtree(out, ignore_errors=True)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", default="%dx%dx%d" % (W, H, N), help="WxHxN of the sources")
    ap.add_argument("--out")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true", help="(the traced run: four joins, nothing printed)")
    a = ap.parse_args()
    w, h, n = (int(v) for v in a.size.split("x"))
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_jpeg_join: needs a GPU (nothing is measured without one)")
    import imagestitching_amd as ist
    files = photos(w, h, n)
    if a.child:
        for _ in range(4):
            ist.join_jpeg(files, "vertical")
        return
    check = ist.jpeg_join_check(files, "vertical")
    assert check["ok"], check

    def pixels():
        bms = ist.decode_bitmaps(files)
        try:
            return ist.stitch_jpeg(bms, "vertical", {"quality": QUALITY, "subsampling": "420"})["jpeg"]
        finally:
            for b in bms:
                b.close()
    arms = {"join": lambda: ist.join_jpeg(files, "vertical"), "pixels": pixels}
    order = ("join", "pixels")
    wall = {k: [] for k in order}
    size = {}
    for it in range(a.warmup + a.iters):
        for k in order[it % 2:] + order[:it % 2]:
            t, f = clock(arms[k])
            size[k] = len(f)
            if it >= a.warmup:
                wall[k].append(t)
    src = sum(len(f) for f in files)
    res = {"bench": "jpeg_join", "files": n, "size": [w, h], "joined": [check["width"], check["height"]], "quality": QUALITY, "iters": a.iters,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "run": "one run",
           "wall_ms": {k: stats(v) for k, v in wall.items()},
           "join_vs_pixels_wall": round(float(np.median(wall["join"]) / np.median(wall["pixels"])), 3),
           "file_bytes": {"sources": src, "join": size["join"], "pixels": size["pixels"],
                          "join_vs_sources": round(size["join"] / src, 4), "pixels_vs_sources": round(size["pixels"] / src, 4)}}
    coef = coefficients(w, h, n)
    floor_us = 4 * coef / PEAK_BYTES_PER_S * 1e6
    us = None if a.no_trace else traced_kernel_us((w, h, n))
    res["join_kernel"] = {"coefficients": coef, "bytes_moved": 4 * coef, "floor_us_at_8TBps": round(floor_us, 1)}
    if us and len(us) % 4 == 0:
        per = len(us) // 4                                   # launches (slabs) of one call; the first call is left out
        calls = [float(sum(us[k * per:(k + 1) * per])) for k in range(1, 4)]
        res["join_kernel"].update({"launches_per_call": per, "launch_us": stats(us[per:]), "us_per_call": stats(calls),
                                   "floor_over_kernel": round(floor_us / float(np.median(calls)), 3),
                                   "bytes_per_s": round(4 * coef / (float(np.median(calls)) * 1e-6)),
                                   "source": "rocprofv3 --kernel-trace --stats, a run of its own: four calls, the first left out; a call's time is the sum of its slabs' launches"})
    else:
        res["join_kernel"]["us"] = "not measured"
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
