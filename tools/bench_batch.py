"""Batched stitching against a loop of single stitches, on one MI355X.  Prints ONE JSON line.

Workloads (what a stitching service receives: many small independent onStitch requests, each capped at 9 images by
pages/index/index.js:311):
  A  64 requests of 9 x 1080x1920, vertical, identity widths (every draw is a copy: the COPY path)
  B  64 requests of 4-9 images of mixed sizes, bilinear resampling, seeded

Legs, each with warm-up and the two variants alternated in one process:
  (a) device-resident: back-to-back ist_job_launch per request  vs  ONE ist_jobs_launch (device events around each variant)
  (b) host path:       a loop of stitch(), every result released before the next request  vs  stitch_batch()  (wall clock: host
                       buffers in, host buffers out)
Reported: microseconds per request for each, and the batch kernel's share of the HBM peak from algorithmic bytes (the byte count
bench.py uses: ist_job_info.algorithmic_bytes).  Batch and loop outputs are checked byte for byte.

  python tools/bench_batch.py [--workloads AB] [--legs ab] [--reps 5] [--warmup 2]
  rocprofv3 --kernel-trace --stats -d DIR -o batch -- python tools/bench_batch.py --legs a --reps 3     (dispatch count, table copy)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (HBM peak, input synthesis, pre-roll)
import imagestitching_amd as ist  # noqa: E402
from imagestitching_amd import _lib as L  # noqa: E402

DEV = "cuda:0"
N_REQ = 64


def workload(name):
    """[(sizes [(w, h)], direction, opts)] per request"""
    if name == "A":
        return [([(1080, 1920)] * 9, "vertical", {"filter": "bilinear"}) for _ in range(N_REQ)]
    rng = np.random.default_rng(20261015)
    reqs = []
    for _ in range(N_REQ):
        n = int(rng.integers(4, 10))
        sizes = [(int(rng.integers(480, 1600)), int(rng.integers(480, 1600))) for _ in range(n)]
        reqs.append((sizes, str(rng.choice(["vertical", "horizontal"])), {"filter": "bilinear", "mode": str(rng.choice(["min", "max"])),
                                                                           "gap": int(rng.choice([0, 4]))}))
    return reqs


def host_images(reqs):
    """host pixels: one synthetic bitmap per distinct size (requests share them, as they would share nothing but the shape)"""
    cache = {}
    out = []
    for sizes, _, _ in reqs:
        imgs = []
        for k, (w, h) in enumerate(sizes):
            key = (w, h, k)
            if key not in cache:
                cache[key] = bench.synth_np(len(cache), w, h)
            imgs.append(cache[key])
        out.append(imgs)
    return out


def leg_device(reqs, pixels, reps, warmup):
    st = ist.Stitcher(0)
    jobs, srcs, outs_loop, outs_batch = [], [], [], []
    dev_cache = {}
    alg = 0
    for (sizes, direction, opts), imgs in zip(reqs, pixels):
        p, job = st.compile([{"width": a.shape[1], "height": a.shape[0], "opaque": True} for a in imgs], direction, opts)
        jobs.append(job)
        alg += int(job.info["algorithmic_bytes"])
        ss = []
        for a in imgs:
            key = id(a)
            if key not in dev_cache:
                dev_cache[key] = torch.from_numpy(a).to(DEV)
            ss.append(dev_cache[key])
        srcs.append(ss)
        outs_loop.append(torch.empty((p.canvas_h, p.canvas_w, 4), dtype=torch.uint8, device=DEV))
        outs_batch.append(torch.empty((p.canvas_h, p.canvas_w, 4), dtype=torch.uint8, device=DEV))

    def loop():
        for j, s, o in zip(jobs, srcs, outs_loop):
            j.launch(s, o)

    def batch():
        ist.launch_jobs(jobs, srcs, outs_batch)

    bench.preroll(loop, torch)
    before = L.lib.ist_debug_batch_launches()
    batch()
    torch.cuda.synchronize()
    launches = L.lib.ist_debug_batch_launches() - before
    identical = all(torch.equal(a, b) for a, b in zip(outs_loop, outs_batch))
    times = {"loop": [], "batch": []}
    for i in range(warmup + reps):
        for name, fn in (("loop", loop), ("batch", batch)) if i % 2 == 0 else (("batch", batch), ("loop", loop)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    lu, bu = statistics.median(times["loop"]), statistics.median(times["batch"])
    return {"us_per_request_loop": round(lu / len(jobs), 2), "us_per_request_batch": round(bu / len(jobs), 2),
            "batch_over_loop": round(bu / lu, 4), "batch_kernel_launches": int(launches),
            "algorithmic_bytes": alg, "hbm_frac_batch": round(alg / (bu * 1e-6) / 1e9 / bench.HBM_PEAK_GBS, 4),
            "hbm_frac_loop": round(alg / (lu * 1e-6) / 1e9 / bench.HBM_PEAK_GBS, 4),
            "table_bytes_per_launch": table_bytes(jobs), "identical": bool(identical),
            "samples_us": {k: [round(v, 1) for v in vs] for k, vs in times.items()}}


def table_bytes(jobs):
    """the per-launch job table ist_jobs_launch copies (ist_batch.cpp): per kernel form, 2112 B of LaunchArgs per job + the tile
    prefix (8 B per job + 8) + the chunk table (4 B per 64 tiles + 4), each section padded to 256 B"""
    def up(v):
        return (v + 255) // 256 * 256
    n = len(jobs)
    tiles = sum(int(j.info["n_tiles"]) for j in jobs)
    return up(2112 * n) + up(8 * (n + 1)) + up(4 * ((tiles + 63) // 64 + 1))


def leg_host(reqs, pixels, reps, warmup):
    requests = [([{"width": a.shape[1], "height": a.shape[0], "data": a, "opaque": True} for a in imgs], d, o)
                for (_, d, o), imgs in zip(reqs, pixels)]
    got = ist.stitch_batch(requests)
    identical = True
    for k, r in enumerate(requests):
        identical = identical and np.array_equal(got[k], ist.stitch(*r)["data"])
    del got
    times = {"loop": [], "batch": []}

    def loop():                      # every result released before the next request (its pinned block is reused)
        for r in requests:
            ist.stitch(*r)

    def batch():                     # all 64 results held until the call returns, then released
        ist.stitch_batch(requests)

    # (the two variants draw their result blocks from separate classes of the library's pinned pool: neither changes what the
    # other finds there)
    for i in range(warmup + reps):
        for name, fn in (("loop", loop), ("batch", batch)) if i % 2 == 0 else (("batch", batch), ("loop", loop)):
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if i >= warmup:
                times[name].append(dt * 1e6)
    lu, bu = statistics.median(times["loop"]), statistics.median(times["batch"])
    return {"us_per_request_loop": round(lu / len(requests), 1), "us_per_request_batch": round(bu / len(requests), 1),
            "batch_over_loop": round(bu / lu, 4), "identical": bool(identical),
            "samples_us_per_request": {k: [round(v / len(requests), 1) for v in vs] for k, vs in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="AB")
    ap.add_argument("--legs", default="ab")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    guard = bench.StdoutGuard()
    assert torch.cuda.is_available(), "bench_batch needs a GPU"
    line = {"metric": "batched stitching: us per request, loop of single stitches vs one batch", "requests": N_REQ,
            "device": torch.cuda.get_device_name(0), "kernel_source_sha": bench.kernel_source_sha()}
    for w in args.workloads:
        reqs = workload(w)
        pixels = host_images(reqs)
        r = {"what": "64 x 9 x 1080x1920 vertical, identity widths (COPY)" if w == "A" else "64 mixed-size requests of 4-9 images, bilinear, seeded",
             "images": sum(len(s) for s, _, _ in reqs)}
        if "a" in args.legs:
            r["a_device"] = leg_device(reqs, pixels, args.reps, args.warmup)
            torch.cuda.empty_cache()
        if "b" in args.legs:
            r["b_host"] = leg_host(reqs, pixels, args.reps, args.warmup)
        line["workload_" + w] = r
    guard.emit(json.dumps(line))


if __name__ == "__main__":
    main()
