"""The JPEG export on one MI355X, beside the PNG export of the same canvas.  Prints ONE JSON line.

  encode   encode_jpeg_device of the two bench canvases (4032x27216 and 36288x3024, photo-like content: smooth colour + noise) at
           quality 90 in 4:2:0 and 4:4:4, and encode_png_device (level 1) of the same canvas as the comparator.  The calls are
           synchronous (the host lays the restart intervals out), so the time is the wall clock of the call.
  stitch   stitch_jpeg over nine resident 12 MP bitmaps beside stitch_png (level 1) over the same bitmaps: bitmaps in HBM, file in
           host memory.
Arms are alternated inside one process after warm-ups, canvases and output buffers rotate between two sets; median and minimum of
the per-call milliseconds, and the file sizes beside them.

  python tools/bench_jpeg.py [--iters 7] [--warmup 2]
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


def photo_like(h, w, seed, dev):
    """smooth colour + noise of +-12, opaque: an HxWx4 uint8 CUDA tensor"""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    yy = torch.arange(h, device=dev, dtype=torch.float32)[:, None]
    xx = torch.arange(w, device=dev, dtype=torch.float32)[None, :]
    out = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
    for c in range(3):
        v = 127.5 + 100 * torch.sin(xx * (0.002 + 0.001 * c) + yy * (0.003 - 0.0007 * c) + seed + c)
        v = v + torch.randint(-12, 13, (h, w), device=dev, generator=g).float()
        out[..., c] = v.clamp(0, 255).round().to(torch.uint8)
    out[..., 3] = 255
    return out


def timed(arms, iters, warmup):
    """arms: {name: callable(k) -> file length}; alternated; returns {name: {ms_median, ms_min, bytes}}"""
    ms = {n: [] for n in arms}
    size = {}
    for k in range(warmup + iters):
        for n, fn in arms.items():
            t0 = time.perf_counter()
            size[n] = int(fn(k))
            dt = (time.perf_counter() - t0) * 1e3
            if k >= warmup:
                ms[n].append(dt)
    return {n: {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "bytes": size[n]} for n, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch

    import imagestitching_amd as ist
    from imagestitching_amd import _lib as L
    assert torch.cuda.is_available(), "bench_jpeg needs a GPU"
    dev = torch.device("cuda", 0)
    res = {"metric": "JPEG export (quality 90): ms per call beside the PNG export (level 1) of the same canvas", "iters": a.iters, "warmup": a.warmup,
           "encode": {}, "stitch": {}}
    for w, h in ((4032, 27216), (36288, 3024)):
        canvases = [photo_like(h, w, s, dev) for s in (1, 2)]
        cap = max(int(L.lib.ist_jpeg_bound(w, h, 0)), int(L.lib.ist_png_bound(w, h)))
        outs = [torch.empty(cap + 16, dtype=torch.uint8, device=dev) for _ in (0, 1)]
        arms = {
            "jpeg_420": lambda k: ist.encode_jpeg_device(canvases[k & 1], 90, "420", out=outs[k & 1])[1],
            "jpeg_444": lambda k: ist.encode_jpeg_device(canvases[k & 1], 90, "444", out=outs[k & 1])[1],
            "png_level1": lambda k: ist.encode_png_device(canvases[k & 1], out=outs[k & 1], level=1)[1],
        }
        r = timed(arms, a.iters, a.warmup)
        r["raw_bytes"] = w * h * 4
        res["encode"]["%dx%d" % (w, h)] = r
        del canvases, outs
        torch.cuda.empty_cache()
    imgs = [photo_like(3024, 4032, 10 + k, dev).cpu().numpy() for k in range(9)]
    bms = [ist.upload_bitmap(x) for x in imgs]
    arms = {
        "stitch_jpeg_420": lambda k: len(ist.stitch_jpeg(bms, "vertical", {"quality": 90})["jpeg"]),
        "stitch_jpeg_444": lambda k: len(ist.stitch_jpeg(bms, "vertical", {"quality": 90, "subsampling": "444"})["jpeg"]),
        "stitch_png_level1": lambda k: len(ist.stitch_png(bms, "vertical", {"pngLevel": 1})["png"]),
    }
    res["stitch"]["9x4032x3024_vertical"] = timed(arms, a.iters, a.warmup)
    for b in bms:
        b.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
