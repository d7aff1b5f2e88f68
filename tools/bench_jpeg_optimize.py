"""The JPEG export with the file's own Huffman tables (optimize=True, IST_JPEG_OPTIMIZE) beside the standard-table export of the same
canvas on one MI355X.  Prints ONE JSON line.

  canvases  the bench canvas (4032x27216: the strip of nine 12 MP images; six slabs of the encoder's scratch, so the optimised file is
            transformed twice) and one phone-sized canvas (1170x2532: one slab, transformed once); photo-like content (smooth colour
            + noise, tools/bench_jpeg.py), quality 90, 4:2:0.
  timed     encode_jpeg_device, standard and optimised alternated inside one process after warm-ups, canvases and output buffers
            rotating between two sets.  The calls are synchronous (the host lays the intervals out and, with optimize, builds the
            tables), so the time is the wall clock of the call: median and minimum of the per-call milliseconds, the file sizes, and
            the ratios optimised / standard.
  kernels   with --trace DIR: one child process per canvas under `rocprofv3 --kernel-trace` (tracing only, a run of its own, BEFORE the
            timed run so that the profiler is gone when the clock runs): the histogram kernel's own time per call, its rate over the
            bytes it reads (the coefficient scratch once: 128 B per block) as a fraction of the HBM peak, the time of one transform pass
            over the canvas, and the share of the extra time (optimised - standard, from the timed run) that is the second transform.
            Without --trace, or without rocprofv3, these read "not measured".

  python tools/bench_jpeg_optimize.py [--iters 9] [--warmup 2] [--trace DIR]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CANVASES = ((4032, 27216), (1170, 2532))
TRACE_CALLS = 4


def setup(w, h):
    import torch

    import bench_jpeg
    from imagestitching_amd import _lib as L
    dev = torch.device("cuda", 0)
    canvases = [bench_jpeg.photo_like(h, w, s, dev) for s in (1, 2)]
    cap = int(L.lib.ist_jpeg_bound(w, h, 0x101))
    outs = [torch.empty(cap + 16, dtype=torch.uint8, device=dev) for _ in (0, 1)]
    return canvases, outs


def trace_child(w, h):
    """under rocprofv3: two warm-up calls of each kind, then TRACE_CALLS optimised and TRACE_CALLS standard calls; prints the launch counts"""
    import imagestitching_amd as ist
    from imagestitching_amd import _lib as L
    canvases, outs = setup(w, h)
    for k in range(2 + TRACE_CALLS):
        before = L.lib.ist_debug_jpeg_encode_launches(), L.lib.ist_debug_jpeg_histogram_launches()
        ist.encode_jpeg_device(canvases[k & 1], 90, "420", out=outs[k & 1], optimize=True)
        opt = L.lib.ist_debug_jpeg_encode_launches() - before[0], L.lib.ist_debug_jpeg_histogram_launches() - before[1]
        before = L.lib.ist_debug_jpeg_encode_launches()
        ist.encode_jpeg_device(canvases[k & 1], 90, "420", out=outs[k & 1])
        std = L.lib.ist_debug_jpeg_encode_launches() - before
    print(json.dumps({"calls": 2 + TRACE_CALLS, "transforms_optimised": opt[0], "histograms": opt[1], "transforms_standard": std}), flush=True)


def traced(w, h, out_dir):
    """kernel times of one canvas from a rocprofv3 kernel trace of trace_child, per call (all calls of a kind are the same work)"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return "not measured (no rocprofv3)"
    d = os.path.join(out_dir, "%dx%d" % (w, h))
    os.makedirs(d, exist_ok=True)
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                        "--trace-child", "%dx%d" % (w, h)], capture_output=True, text=True, timeout=900)
    files = glob.glob(d + "/**/*_kernel_trace.csv", recursive=True)
    if r.returncode != 0 or not files or not r.stdout.strip():
        return "not measured (the traced run failed: exit %d: %s)" % (r.returncode, r.stderr[-300:])
    counts = json.loads([x for x in r.stdout.strip().splitlines() if x.startswith("{")][-1])
    us = {}
    for row in csv.DictReader(open(files[0])):
        for name in ("ist_jpeg_histogram_kernel", "ist_jpeg_transform_kernel", "ist_jpeg_entropy_wide_kernel", "ist_jpeg_entropy_kernel", "ist_jpeg_gather_kernel"):
            if name in row["Kernel_Name"]:
                us.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    calls = counts["calls"]
    slabs = counts["transforms_standard"]
    passes = calls * (counts["transforms_optimised"] + counts["transforms_standard"]) / slabs        # transform passes over the whole canvas
    blocks = -(-w // 16) * 6 * -(-h // 16)
    hist_ms = sum(us.get("ist_jpeg_histogram_kernel", [0.0])) / calls / 1e3
    import bench
    return {"slabs": slabs, "transform_launches_per_optimised_call": counts["transforms_optimised"], "histogram_launches_per_call": counts["histograms"],
            "histogram_ms_per_call": round(hist_ms, 4), "histogram_bytes_read": blocks * 128,
            "histogram_GBs": round(blocks * 128 / (hist_ms * 1e-3) / 1e9, 1) if hist_ms > 0 else None,
            "histogram_hbm_frac": round(blocks * 128 / (hist_ms * 1e-3) / 1e9 / bench.HBM_PEAK_GBS, 4) if hist_ms > 0 else None,
            "transform_ms_per_pass": round(sum(us.get("ist_jpeg_transform_kernel", [0.0])) / passes / 1e3, 4),
            "entropy_wide_ms_per_call": round(sum(us.get("ist_jpeg_entropy_wide_kernel", [0.0])) / calls / 1e3, 4),
            "entropy_standard_ms_per_call": round(sum(us.get("ist_jpeg_entropy_kernel", [0.0])) / calls / 1e3, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace", default=None, help="directory for the rocprofv3 kernel traces (one child process per canvas)")
    ap.add_argument("--trace-child", default=None, help="WxH: the traced workload, in this process")
    a = ap.parse_args()
    if a.trace_child:
        w, h = (int(v) for v in a.trace_child.split("x"))
        trace_child(w, h)
        return
    kernels = {"%dx%d" % c: (traced(c[0], c[1], a.trace) if a.trace else "not measured (no --trace)") for c in CANVASES}
    import torch

    import bench
    import bench_jpeg
    import imagestitching_amd as ist
    assert torch.cuda.is_available(), "bench_jpeg_optimize needs a GPU"
    res = {"metric": "JPEG export with optimised Huffman tables (quality 90, 4:2:0): ms per encode_jpeg_device call and file bytes beside the standard tables",
           "iters": a.iters, "warmup": a.warmup, "hbm_peak_GBs": bench.HBM_PEAK_GBS, "kernel_source_sha": bench.kernel_source_sha(), "canvases": {}}
    for w, h in CANVASES:
        canvases, outs = setup(w, h)
        arms = {"standard": lambda k: ist.encode_jpeg_device(canvases[k & 1], 90, "420", out=outs[k & 1])[1],
                "optimised": lambda k: ist.encode_jpeg_device(canvases[k & 1], 90, "420", out=outs[k & 1], optimize=True)[1]}
        r = bench_jpeg.timed(arms, a.iters, a.warmup)
        r["raw_bytes"] = w * h * 4
        r["ms_ratio_optimised_over_standard"] = round(r["optimised"]["ms_median"] / r["standard"]["ms_median"], 3)
        r["bytes_ratio_optimised_over_standard"] = round(r["optimised"]["bytes"] / r["standard"]["bytes"], 4)
        k = kernels["%dx%d" % (w, h)]
        r["kernels"] = k
        if isinstance(k, dict):
            extra = r["optimised"]["ms_median"] - r["standard"]["ms_median"]
            second = k["transform_ms_per_pass"] if k["transform_launches_per_optimised_call"] > k["slabs"] else 0.0
            r["extra_ms"] = round(extra, 3)
            r["second_transform_share_of_extra"] = round(second / extra, 3) if extra > 0 else None
            r["histogram_share_of_extra"] = round(k["histogram_ms_per_call"] / extra, 3) if extra > 0 else None
        res["canvases"]["%dx%d" % (w, h)] = r
        del canvases, outs
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
