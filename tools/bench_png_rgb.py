"""The RGB form of the compressing PNG export (pngColor 'rgb') beside the RGBA form, on one MI355X.  Prints ONE JSON line.

The bench canvas - nine 4032 x 3024 images stitched vertically, 4032 x 27216, photo-like content (smooth colour + noise, opaque) -
goes through the two paths a caller has, RGBA against RGB in alternation on one context in one process:

  encode   encode_png_device of the canvas resident in HBM into a device buffer (level 1): the compression alone.
  stitch   stitch_png over the nine resident bitmaps (level 1): render, compression and the file's trip to host memory.

Median and minimum of the per-call wall-clock milliseconds after warm-ups, and the file sizes beside them.  Both files are decoded
once and compared with the canvas before anything is timed.

  python tools/bench_png_rgb.py [--iters 9] [--warmup 2]
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


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
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import numpy as np
    import torch

    import imagestitching_amd as ist
    from imagestitching_amd import _lib as L
    from bench_jpeg import photo_like
    assert torch.cuda.is_available(), "bench_png_rgb needs a GPU"
    dev = torch.device("cuda", 0)
    imgs = [photo_like(3024, 4032, 10 + k, dev).cpu().numpy() for k in range(9)]
    bms = [ist.upload_bitmap(x) for x in imgs]
    canvas_np = np.concatenate(imgs, 0)
    canvas = torch.from_numpy(canvas_np).to(dev)
    h, w = canvas_np.shape[:2]
    outs = [torch.empty(int(L.lib.ist_png_bound(w, h)) + 16, dtype=torch.uint8, device=dev) for _ in (0, 1)]
    # both forms decode to the canvas (once, untimed)
    from PIL import Image
    Image.MAX_IMAGE_PIXELS = None
    for color, mode in (("rgba", "RGBA"), ("rgb", "RGB")):
        png = ist.stitch_png(bms, "vertical", {"pngLevel": 1, "pngColor": color})["png"]
        im = Image.open(io.BytesIO(bytes(png)))
        assert im.mode == mode and np.array_equal(np.asarray(im), canvas_np[..., :len(mode)]), color
        del im, png
    res = {"metric": "PNG export (level 1) of the 4032x27216 bench canvas: RGB (colour type 2) beside RGBA (colour type 6), ms per call and file bytes",
           "iters": a.iters, "warmup": a.warmup, "raw_bytes": w * h * 4}
    res["encode_png_device"] = timed({
        "rgba": lambda k: ist.encode_png_device(canvas, out=outs[k & 1], level=1, color="rgba")[1],
        "rgb": lambda k: ist.encode_png_device(canvas, out=outs[k & 1], level=1, color="rgb")[1],
    }, a.iters, a.warmup)
    res["stitch_png_bitmaps"] = timed({
        "rgba": lambda k: len(ist.stitch_png(bms, "vertical", {"pngLevel": 1, "pngColor": "rgba"})["png"]),
        "rgb": lambda k: len(ist.stitch_png(bms, "vertical", {"pngLevel": 1, "pngColor": "rgb"})["png"]),
    }, a.iters, a.warmup)
    for arm in ("encode_png_device", "stitch_png_bitmaps"):
        r = res[arm]
        r["bytes_ratio"] = round(r["rgb"]["bytes"] / r["rgba"]["bytes"], 4)
        r["ms_ratio"] = round(r["rgb"]["ms_median"] / r["rgba"]["ms_median"], 4)
    for b in bms:
        b.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
