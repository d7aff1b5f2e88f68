"""The batched JPEG export on one MI355X, beside a loop of the single-file encoder over the same canvases.  Prints ONE JSON line.

Three shapes, all at quality 90 in 4:2:0, canvases resident in HBM (photo-like content: smooth colour + noise):
  64 x 96x96       a thumbnail grid
  256 x 750x1334   phone screenshots
  9 x 4032x3024    twelve-megapixel photos
Two arms per shape: `loop`, one encode_jpeg_device call per canvas, and `batch`, one encode_jpeg_batch_device call for all of them.
Both are synchronous (the host lays the restart intervals out), so the time is the wall clock of the arm.  Arms are alternated inside
one process after warm-ups, canvases and output buffers rotate between two sets; median and minimum of the per-arm milliseconds, the
total file bytes beside them (equal in both arms: the files are the same).

  python tools/bench_jpeg_batch.py [--iters 7] [--warmup 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_jpeg import photo_like, timed  # noqa: E402

SHAPES = ((64, 96, 96), (256, 750, 1334), (9, 4032, 3024))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch

    import imagestitching_amd as ist
    from imagestitching_amd import _lib as L
    assert torch.cuda.is_available(), "bench_jpeg_batch needs a GPU"
    dev = torch.device("cuda", 0)
    res = {"metric": "JPEG export of n canvases (quality 90, 4:2:0): ms per n files, one batch call beside a loop of single-file calls",
           "iters": a.iters, "warmup": a.warmup, "shapes": {}}
    for n, w, h in SHAPES:
        sets = [[photo_like(h, w, 1000 * s + k, dev) for k in range(n)] for s in (0, 1)]
        cap = int(L.lib.ist_jpeg_bound(w, h, 1))
        outs = [[torch.empty(cap + 16, dtype=torch.uint8, device=dev) for _ in range(n)] for _ in (0, 1)]
        before = L.lib.ist_debug_jpeg_batch_launches()
        arms = {
            "loop": lambda k: sum(ist.encode_jpeg_device(c, 90, "420", out=o)[1] for c, o in zip(sets[k & 1], outs[k & 1])),
            "batch": lambda k: sum(m for _, m in ist.encode_jpeg_batch_device(sets[k & 1], 90, "420", outs=outs[k & 1])),
        }
        r = timed(arms, a.iters, a.warmup)
        assert r["loop"]["bytes"] == r["batch"]["bytes"]
        r["rounds_per_batch_call"] = (L.lib.ist_debug_jpeg_batch_launches() - before) // (a.iters + a.warmup)
        r["loop_over_batch_median"] = round(r["loop"]["ms_median"] / r["batch"]["ms_median"], 2)
        r["raw_bytes"] = n * w * h * 4
        res["shapes"]["%dx%dx%d" % (n, w, h)] = r
        del sets, outs, arms
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
