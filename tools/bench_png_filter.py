"""The adaptive row filters of the compressing PNG export (pngFilter 'adaptive') beside Paeth on every row, on one MI355X.  Prints ONE
JSON line.

The bench canvas - nine 4032 x 3024 images stitched vertically, 4032 x 27216, photo-like content (smooth colour + noise, opaque) -
goes through the two paths a caller has, in both colour forms, Paeth against adaptive in alternation on one context in one process:

  encode   encode_png_device of the canvas resident in HBM into a device buffer (level 1): the pre-pass and the compression alone.
  stitch   stitch_png over the nine resident bitmaps (level 1): render, pre-pass, compression and the file's trip to host memory.

Median and minimum of the per-call wall-clock milliseconds after warm-ups, and the file sizes beside them; bytes_ratio and ms_ratio
are adaptive / Paeth of the same colour form in the same run.  Every file is decoded once and compared with the canvas before
anything is timed.

  python tools/bench_png_filter.py [--iters 9] [--warmup 2]
"""
import argparse
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FORMS = [(c, f) for c in ("rgba", "rgb") for f in ("paeth", "adaptive")]


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
    from bench_png_rgb import timed
    assert torch.cuda.is_available(), "bench_png_filter needs a GPU"
    dev = torch.device("cuda", 0)
    imgs = [photo_like(3024, 4032, 10 + k, dev).cpu().numpy() for k in range(9)]
    bms = [ist.upload_bitmap(x) for x in imgs]
    canvas_np = np.concatenate(imgs, 0)
    canvas = torch.from_numpy(canvas_np).to(dev)
    h, w = canvas_np.shape[:2]
    outs = [torch.empty(int(L.lib.ist_png_bound(w, h)) + 16, dtype=torch.uint8, device=dev) for _ in (0, 1)]
    # every form decodes to the canvas (once, untimed)
    from PIL import Image
    Image.MAX_IMAGE_PIXELS = None
    for color, filt in FORMS:
        png = ist.stitch_png(bms, "vertical", {"pngLevel": 1, "pngColor": color, "pngFilter": filt})["png"]
        im = Image.open(io.BytesIO(bytes(png)))
        assert im.mode == color.upper() and np.array_equal(np.asarray(im), canvas_np[..., :len(color)]), (color, filt)
        del im, png
    res = {"metric": "PNG export (level 1) of the 4032x27216 bench canvas: adaptive row filters beside Paeth on every row, in both colour forms, ms per call and file bytes",
           "iters": a.iters, "warmup": a.warmup, "raw_bytes": w * h * 4}
    tag = lambda c, f: c + "_" + f
    res["encode_png_device"] = timed({tag(c, f): (lambda k, c=c, f=f: ist.encode_png_device(canvas, out=outs[k & 1], level=1, color=c, row_filter=f)[1])
                                      for c, f in FORMS}, a.iters, a.warmup)
    res["stitch_png_bitmaps"] = timed({tag(c, f): (lambda k, c=c, f=f: len(ist.stitch_png(bms, "vertical", {"pngLevel": 1, "pngColor": c, "pngFilter": f})["png"]))
                                       for c, f in FORMS}, a.iters, a.warmup)
    for arm in ("encode_png_device", "stitch_png_bitmaps"):
        r = res[arm]
        for c in ("rgba", "rgb"):
            r[c + "_bytes_ratio"] = round(r[tag(c, "adaptive")]["bytes"] / r[tag(c, "paeth")]["bytes"], 4)
            r[c + "_ms_ratio"] = round(r[tag(c, "adaptive")]["ms_median"] / r[tag(c, "paeth")]["ms_median"], 4)
    for b in bms:
        b.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
