#!/usr/bin/env python3
"""The colour conversion (profile='srgb') on the files it is for: nine 12 MP Display-P3-tagged 4:2:0 baseline JPEGs, 4032 x 3024 (the
page's cap, index.js:311), in ONE process.
  kernel      convert_color_device alone, timed with device events over --iters after --warmup, on buffer sets that rotate: nine
              48.8 MB bitmaps per set, six sets = 2.6 GB, so no launch finds its pixels in the 256 MiB Infinity Cache.  Input = the decoded
              photos (the lookups are data-dependent: real pixels, not noise).  The kernel's bytes are 8 per pixel (each pixel read
              once and written once); the floor is those bytes at the 8 TB/s HBM peak, fraction_of_peak = floor / measured.
              `dense` = dense rows, 16-byte aligned; `offset` = the same pixels in a box that starts 28 bytes behind a 16-byte
              boundary at a pitch of 4 w + 48 (the direct-to-canvas case); `pitch_only` and `offset_only` take the two apart.
  decode      host clock around decode_bitmaps (files in, bitmaps resident) with profile='srgb' against profile='ignore', the arms
              alternating call by call in an order that flips; added = median(srgb) - median(ignore).
  stitch      stitch_files of the nine files (vertical, equal widths: every image is converted in its box of the canvas) with and
              without opts['colorProfile'] = 'srgb'.
Prints one JSON line.  Usage: python tools/bench_colour.py [--iters 20] [--warmup 4] [--out FILE]"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import icc_writer  # noqa: E402
import imagestitching_amd as ist  # noqa: E402

W, H, N, SETS = 4032, 3024, 9, 6
HBM_PEAK = 8.0e12


def photos(icc):
    """nine photo-like files: smooth colour fields + noise, three pixel sets in rotation at three qualities, tagged with icc"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    files = []
    for k in range(3):
        rng = np.random.default_rng(20 + k)
        a = np.empty((H, W, 3), np.float32)
        for c in range(3):
            fx, fy, ph = rng.uniform(0.5, 3.0, 3)
            a[..., c] = 127.5 + 100 * np.sin(fx * xx / W * 6.28 + fy * yy / H * 6.28 + ph * 2)
        a += rng.integers(-12, 13, a.shape)
        im = Image.fromarray(np.clip(a, 0, 255).astype(np.uint8))
        for q in (92, 88, 84):
            b = io.BytesIO()
            im.save(b, "JPEG", quality=q, subsampling=2, icc_profile=icc)
            files.append(b.getvalue())
    return files[:N]


def stats(ms):
    v = np.array(ms)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


def clock(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def close(bms):
    for b in bms:
        b.close()


def kernel_times(sets, fresh, icc, iters, warmup):
    """ms per launch (one image), device events around each set's nine launches.  The conversion is in place, so a set is refilled
    with the decoded pixels before it is used again - half a rotation ahead of its turn, outside the timed window, so that the two
    sets timed in between (0.9 GB of traffic each) push the refill out of the Infinity Cache."""
    out = []
    for it in range(warmup + iters):
        views = sets[it % len(sets)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for v in views:
            ist.convert_color_device(v, icc)
        e1.record()
        e1.synchronize()
        if it >= warmup:
            out.append(e0.elapsed_time(e1) / len(views))
        for v, t in zip(sets[(it + len(sets) // 2) % len(sets)], fresh):
            v.copy_(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    icc = icc_writer.fixtures()["p3_para3"]
    files = photos(icc)
    assert all(ist.image_color(f) == "convert" for f in files)
    res = {"bench": "colour", "files": N, "size": [W, H], "file_bytes": sum(len(f) for f in files), "iters": a.iters, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "profile": "Display P3, para type 3"}

    # ---- the kernel alone
    tensors, _ = ist.decode_files_device(files)
    dense = [[t.clone() for t in tensors] for _ in range(SETS)]
    pitch = 4 * W + 48
    flats = [[torch.empty(64 + pitch * H, dtype=torch.uint8, device="cuda") for _ in tensors] for _ in range(SETS)]
    offset = [[torch.as_strided(f, (H, W, 4), (pitch, 4, 1), 28) for f in fs] for fs in flats]
    padded = [[torch.as_strided(f, (H, W, 4), (pitch, 4, 1), 0) for f in fs] for fs in flats]       # (the same blocks: timed after `offset`)
    shifted = [[torch.as_strided(f, (H, W, 4), (4 * W, 4, 1), 28) for f in fs] for fs in flats]
    for vs in offset:
        for v, t in zip(vs, tensors):
            v.copy_(t)
    torch.cuda.synchronize()
    floor_ms = 8.0 * W * H / HBM_PEAK * 1e3
    res["kernel"] = {"bytes_per_pixel": 8, "floor_ms_at_8TBps": round(floor_ms, 4), "buffer_sets": SETS}
    for name, sets in (("dense", dense), ("offset", offset), ("pitch_only", padded), ("offset_only", shifted)):
        t = kernel_times(sets, tensors, icc, a.iters, a.warmup)
        s = stats(t)
        res["kernel"][name] = {"ms_per_image": s, "TBps": round(8.0 * W * H / (s["median"] * 1e-3) / 1e12, 3), "fraction_of_peak": round(floor_ms / s["median"], 3)}
    del dense, flats, offset, padded, shifted, tensors
    torch.cuda.empty_cache()

    # ---- decode_bitmaps with and without the conversion, in the same run
    arms = ("ignore", "srgb")
    wall = {p: [] for p in arms}
    for it in range(a.warmup + a.iters):
        for p in (arms if it % 2 == 0 else arms[::-1]):
            t, bms = clock(lambda: ist.decode_bitmaps(files, profile=p))
            close(bms)
            if it >= a.warmup:
                wall[p].append(t)
    res["decode_bitmaps_ms"] = {p: stats(wall[p]) for p in arms}
    res["decode_bitmaps_ms"]["added"] = round(res["decode_bitmaps_ms"]["srgb"]["median"] - res["decode_bitmaps_ms"]["ignore"]["median"], 4)
    res["decode_bitmaps_ms"]["added_fraction"] = round(res["decode_bitmaps_ms"]["added"] / res["decode_bitmaps_ms"]["ignore"]["median"], 4)

    # ---- the file pipeline
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for k, f in enumerate(files):
            paths.append(os.path.join(d, "p%d.jpg" % k))
            with open(paths[-1], "wb") as fh:
                fh.write(f)
        wall = {p: [] for p in arms}
        for it in range(a.warmup // 2 + a.iters // 2):
            for p in (arms if it % 2 == 0 else arms[::-1]):
                t, r = clock(lambda: ist.stitch_files(paths, "vertical", {"colorProfile": p}))
                if it >= a.warmup // 2:
                    wall[p].append(t)
        res["stitch_files_ms"] = {p: stats(wall[p]) for p in arms}
        res["stitch_files_ms"]["added"] = round(res["stitch_files_ms"]["srgb"]["median"] - res["stitch_files_ms"]["ignore"]["median"], 4)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
