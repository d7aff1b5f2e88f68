"""The window matches of the compressing PNG export (pngMatch 'window') beside the run form, on one MI355X.  Prints ONE JSON line
(profiles/r17_png_match.json is such a line).

Two canvases of 4032 x 27216, nine 4032 x 3024 images stitched vertically:

  photo   the bench canvas: photo-like content (smooth colour + noise, opaque).
  text    white pages with dark text in PIL's default font, lines of words out of a vocabulary of 300 random letter strings.

Each goes through the two paths a caller has, 'run' against 'window' in alternation on one context in one process (RGBA, Paeth):

  encode   encode_png_device of the canvas resident in HBM into a device buffer (level 1): the compression alone.
  stitch   stitch_png over the nine resident bitmaps (level 1): render, compression and the file's trip to host memory.

Median and minimum of the per-call wall-clock milliseconds after warm-ups, and the file sizes beside them; bytes_ratio and ms_ratio
are window / run on the same canvas in the same run.  Every window file is decoded once and compared with the canvas before anything
is timed.

  python tools/bench_png_match.py [--iters 9] [--warmup 2]
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

MATCHES = ("run", "window")


def text_page(h, w, seed, vocab=300):
    """an HxWx4 uint8 array: white with lines of dark words"""
    import numpy as np
    from PIL import Image, ImageDraw, ImageFont
    rng = np.random.RandomState(seed)
    words = ["".join(chr(97 + c) for c in rng.randint(0, 26, rng.randint(2, 9))) for _ in range(vocab)]
    im = Image.new("RGBA", (w, h), (255, 255, 255, 255))
    draw, font = ImageDraw.Draw(im), ImageFont.load_default()
    per_line = max(1, w // 52)
    for y in range(4, h - 10, 14):
        draw.text((4, y), " ".join(words[i] for i in rng.randint(0, vocab, per_line)), fill=(20, 20, 20, 255), font=font)
    return np.asarray(im).copy()


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
    assert torch.cuda.is_available(), "bench_png_match needs a GPU"
    dev = torch.device("cuda", 0)
    from PIL import Image
    Image.MAX_IMAGE_PIXELS = None
    res = {"metric": "PNG export (level 1, RGBA, Paeth) of two 4032x27216 canvases, photo-like and rendered text: window matches beside the run form, ms per call and file bytes",
           "iters": a.iters, "warmup": a.warmup}
    contents = {"photo": lambda k: photo_like(3024, 4032, 10 + k, dev).cpu().numpy(), "text": lambda k: text_page(3024, 4032, 10 + k)}
    for what, make in contents.items():
        imgs = [make(k) for k in range(9)]
        bms = [ist.upload_bitmap(x) for x in imgs]
        canvas_np = np.concatenate(imgs, 0)
        canvas = torch.from_numpy(canvas_np).to(dev)
        h, w = canvas_np.shape[:2]
        res["raw_bytes"] = w * h * 4
        outs = [torch.empty(int(L.lib.ist_png_bound(w, h)) + 16, dtype=torch.uint8, device=dev) for _ in (0, 1)]
        png = ist.stitch_png(bms, "vertical", {"pngLevel": 1, "pngMatch": "window"})["png"]      # decodes to the canvas (once, untimed)
        im = Image.open(io.BytesIO(bytes(png)))
        assert im.mode == "RGBA" and np.array_equal(np.asarray(im), canvas_np), what
        del im, png
        r = res[what] = {}
        r["encode_png_device"] = timed({m: (lambda k, m=m: ist.encode_png_device(canvas, out=outs[k & 1], level=1, match=m)[1]) for m in MATCHES}, a.iters, a.warmup)
        r["stitch_png_bitmaps"] = timed({m: (lambda k, m=m: len(ist.stitch_png(bms, "vertical", {"pngLevel": 1, "pngMatch": m})["png"])) for m in MATCHES}, a.iters, a.warmup)
        for arm in ("encode_png_device", "stitch_png_bitmaps"):
            t = r[arm]
            t["bytes_ratio"] = round(t["window"]["bytes"] / t["run"]["bytes"], 4)
            t["ms_ratio"] = round(t["window"]["ms_median"] / t["run"]["ms_median"], 4)
        for b in bms:
            b.close()
        del canvas, outs, bms, imgs, canvas_np
    print(json.dumps(res))


if __name__ == "__main__":
    main()
