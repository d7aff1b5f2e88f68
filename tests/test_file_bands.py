"""The index rules of the file pipeline (ist_file_bands.cpp: how a stitch of files is cut into bands, which draws only move their
image and are reconstructed straight into the canvas, which bands a request of the PNG encoder submits) against a statement of
the same rules made here from the planner's op list.  tools/file_bands.cpp prints the C++ side.  Pure CPU."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import imagestitching_amd as ist
from imagestitching_amd.stitch import _filter_of, _merge, edge_aa_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _images(sizes, orientations=None):
    return [{"width": w, "height": h, "orientation": (orientations or {}).get(k, 1), "opaque": True} for k, (w, h) in enumerate(sizes)]


PHOTOS = [(640, 480), (480, 640), (600, 450), (333, 517)]
ODD = [(317, 203), (251, 64), (317, 120), (90, 33), (318, 77)]        # (width, height) of test_gpu_jpeg.py's direct-placement layout
# name -> (images, direction, opts, banded, direct parts or None: whatever the restatement says)
CASES = {
    "same width": (_images([(512, 300), (512, 411), (512, 96)]), "vertical", {}, True, 3),
    "same width, gap": (_images([(512, 300), (512, 411), (512, 96)]), "vertical", {"gap": 9}, True, 3),
    "mixed widths, min": (_images(PHOTOS), "vertical", {"mode": "min"}, True, None),
    "mixed widths, max": (_images(PHOTOS), "vertical", {"mode": "max"}, True, None),
    "horizontal": (_images(PHOTOS), "horizontal", {"gap": 5}, True, None),
    "phone caps": (_images([(3000, 4000)] * 8), "vertical", {"platform": "ios", "edgeAA": False}, True, 0),
    "one turned, vertical": (_images(ODD, {3: 6}), "vertical", {"filter": "nearest", "mode": "original", "gap": 7}, True, 4),
    "one turned, horizontal": (_images(ODD, {3: 6}), "horizontal", {"filter": "nearest", "mode": "original", "gap": 7}, True, 4),
    "orientation 7": (_images([(200, 120), (160, 90), (120, 200)], {1: 7}), "vertical", {"platform": "ios", "gap": 3}, False, None),
    "single image": (_images([(640, 480)]), "vertical", {}, False, None),
    "image listed twice": (_images([(300, 200), (300, 150), (300, 200)]), "vertical", {"filter": "nearest"}, True, 1),
    "more draws than images": (_images([(300, 200), (300, 150), (300, 200)]), "vertical", {"filter": "nearest"}, False, None),
    "a turned image drawn upright": (_images([(512, 300), (512, 411), (512, 96)]), "vertical", {}, True, 2),
    "rows above the first band": (_images([(512, 300), (512, 411), (512, 96)]), "vertical", {}, True, 3),
}


TOP = 40          # "rows above the first band": every draw moved down by this many rows on a canvas as much taller


def _ops(name, images, direction, opts):
    """canvas width, canvas height, the planner's op list and the images the pipeline would be given"""
    p = ist.plan(images, direction, opts)
    ops, canvas_h = p.ops_as_dicts(), p.canvas_h
    if name in ("image listed twice", "more draws than images"):      # the third draw takes the first image's bitmap again
        assert ops[-1]["kind"] == "draw" and ops[-1]["image"] == 2
        ops[-1]["image"] = 0
        if name == "more draws than images":
            images = images[:2]
    if name == "a turned image drawn upright":   # (no plan does that: the orientation rule alone keeps the draw from being direct)
        images = [dict(im, orientation=3 if k == 1 else 1) for k, im in enumerate(images)]
    if name == "rows above the first band":     # (no plan leaves them: the schedule's "none" answer is only reached this way)
        for o in ops:
            if o["kind"] == "draw":
                o["m"][5] += TOP
        canvas_h += TOP
    return p.canvas_w, canvas_h, ops, images


def _sequences(rng, canvas_h, band_rows):
    """non-decreasing requests that end at canvas_h: random ones, then the two the encoder issues (a short first slab followed
    by slabs of about one band; the whole canvas at once - phase timing, PNG level 0)"""
    out = []
    for _ in range(40):
        k = int(rng.integers(1, 7))
        out.append(sorted(int(v) for v in rng.integers(1, canvas_h + 1, size=k - 1)) + [canvas_h])
    first = max(1, min(canvas_h, band_rows // 5))
    out.append(list(range(first, canvas_h, max(1, band_rows))) + [canvas_h])
    out.append([canvas_h])
    return out


def _stdin_case(cw, ch, ops, images, filt, seqs):
    out = ["%d %d %d %d %d %d" % (cw, ch, filt, len(images), len(ops), len(seqs))]
    out += ["%d %d %d 0 0 1" % (im["width"], im["height"], im["orientation"]) for im in images]
    out += [" ".join([str(0 if o["kind"] == "fill" else 1), str(o["image"])] + [repr(float(v)) for v in o["m"] + o["s"] + o["d"]] + [str(v) for v in o["rgba"]])
            for o in ops]
    out += [" ".join(str(v) for v in [len(s)] + s) for s in seqs]
    return "\n".join(out) + "\n"


def _parse(text):
    cases = []
    for line in text.splitlines():
        t = line.split()
        if t[0] == "case":
            cur = {"banded": int(t[1]) == 1, "parts": [], "boxes": [], "moves": [], "seqs": []}
            cases.append(cur)
        elif t[0] == "part":
            assert int(t[1]) == len(cur["parts"])
            cur["parts"].append(dict(zip(("image", "op", "X0", "Y0", "X1", "Y1"), map(int, t[2:]))))
        elif t[0] == "box":
            cur["boxes"].append(tuple(map(int, t[2:])))
        elif t[0] == "moves":
            cur["moves"].append((int(t[2]) == 1, int(t[3]) == 1))
        elif t[0] == "seq":
            cur["seqs"].append([])
        elif t[0] == "req":
            cur["seqs"][-1].append(tuple(map(int, t[1:])))
        else:
            assert t[0] == "end", t
    return cases


# ---- the rules, stated from the op list ------------------------------------------------------------------------------------
def _box(o, canvas_w, canvas_h, edge_aa):
    """canvas pixels of a draw: those whose CENTRE lies in the transformed destination rectangle (with edge anti-aliasing: every
    pixel the rectangle touches), clipped to the canvas"""
    a, b, c, d, e, f = o["m"]
    rx, ry, rw, rh = o["d"]
    xs = [a * u + c * v + e for u in (rx, rx + rw) for v in (ry, ry + rh)]
    ys = [b * u + d * v + f for u in (rx, rx + rw) for v in (ry, ry + rh)]
    lo = (lambda v: math.floor(v)) if edge_aa else (lambda v: math.ceil(v - 0.5))
    hi = (lambda v: math.ceil(v)) if edge_aa else (lambda v: math.ceil(v - 0.5))
    X0, X1 = max(0, lo(min(xs))), min(canvas_w, hi(max(xs)))
    Y0, Y1 = max(0, lo(min(ys))), min(canvas_h, hi(max(ys)))
    return (X0, Y0, X1, Y1) if X1 > X0 and Y1 > Y0 else None


def _expected_cut(ops, n_images, canvas_w, canvas_h, edge_aa):
    """one part per draw, in canvas row order (op order among equals); None unless there are at least two, they share no pixel, and
    there are no more of them than images"""
    parts = []
    for k, o in enumerate(ops):
        if o["kind"] != "draw":
            continue
        box = _box(o, canvas_w, canvas_h, edge_aa)
        if box:
            parts.append({"image": o["image"], "op": k, "X0": box[0], "Y0": box[1], "X1": box[2], "Y1": box[3]})
    for i, p in enumerate(parts):
        for q in parts[i + 1:]:
            if p["X0"] < q["X1"] and q["X0"] < p["X1"] and p["Y0"] < q["Y1"] and q["Y0"] < p["Y1"]:
                return None
    if len(parts) < 2 or len(parts) > n_images:
        return None
    return sorted(parts, key=lambda p: p["Y0"])


def _expected_direct(ops, images, canvas_w, canvas_h):
    """ops (indices) whose draw only moves an upright image that no other draw uses"""
    used = [o["image"] for o in ops if o["kind"] == "draw"]
    out = set()
    for k, o in enumerate(ops):
        if o["kind"] != "draw":
            continue
        im = images[o["image"]]
        w, h = im["width"], im["height"]
        x, y = o["m"][4] + o["d"][0], o["m"][5] + o["d"][1]
        if (o["m"][:4] == [1, 0, 0, 1] and o["s"] == [0, 0, w, h] and o["d"][2:] == [w, h] and x == int(x) and y == int(y)
                and 0 <= x and x + w <= canvas_w and 0 <= y and y + h <= canvas_h and im["orientation"] == 1 and used.count(o["image"]) == 1):
            out.add(k)
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cut_direct_placement_and_band_schedule(tmp_path):
    exe = str(tmp_path / "file_bands")
    csrc = os.path.join(ROOT, "imagestitching_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "file_bands.cpp")] +
                   [os.path.join(csrc, f) for f in ("ist_file_bands.cpp", "ist_plan.cpp", "ist_shard.cpp", "ist_compile.cpp")] + ["-o", exe],
                   check=True, capture_output=True, timeout=300)
    rng = np.random.default_rng(808)
    made, stdin = [], ""
    for name, (images, direction, opts, _, _) in CASES.items():
        cw, ch, ops, images = _ops(name, images, direction, opts)
        o = _merge(opts)
        band_rows = max(im["height"] for im in images)
        seqs = _sequences(rng, ch, band_rows)
        made.append((name, cw, ch, ops, images, o, seqs))
        stdin += _stdin_case(cw, ch, ops, images, _filter_of(o), seqs)
    out = subprocess.run([exe], input=stdin, check=True, capture_output=True, text=True, timeout=300).stdout
    got = _parse(out)
    assert len(got) == len(CASES)
    n_direct_seen = n_none_seen = 0
    for (name, cw, ch, ops, images, o, seqs), c in zip(made, got):
        _, _, _, want_banded, want_direct = CASES[name]
        # ---- the cut
        want = _expected_cut(ops, len(images), cw, ch, edge_aa_of(o))
        assert c["banded"] == want_banded == (want is not None), name
        if not c["banded"]:
            continue
        parts = c["parts"]
        assert parts == want, name
        assert [q["Y0"] for q in parts] == sorted(q["Y0"] for q in parts), name
        assert 2 <= len(parts) <= len(images), name
        assert c["boxes"] == [(q["X0"], q["Y0"], q["X1"] - q["X0"], q["Y1"] - q["Y0"]) for q in parts], name
        # ---- direct placement: the geometry (C++), the band's tiles (the compiler), one draw per image (the caller's three rules
        # but the first - every file of these cases is a JPEG)
        direct = [k for k, (moves, copy_only) in enumerate(c["moves"])
                  if moves and copy_only and sum(1 for q in parts if q["image"] == parts[k]["image"]) == 1]
        assert {parts[k]["op"] for k in direct} == _expected_direct(ops, images, cw, ch), name
        if want_direct is not None:
            assert len(direct) == want_direct, name
        for k in direct:
            q = parts[k]
            assert 0 <= q["X0"] < q["X1"] <= cw and 0 <= q["Y0"] < q["Y1"] <= ch, (name, k)
            for j in direct:
                r = parts[j]
                assert j == k or not (q["X0"] < r["X1"] and r["X0"] < q["X1"] and q["Y0"] < r["Y1"] and r["Y0"] < q["Y1"]), (name, k, j)
        n_direct_seen += len(direct)
        # ---- the schedule
        y0 = [q["Y0"] for q in parts]
        assert y0[0] == (TOP if name == "rows above the first band" else 0), name   # (a plan starts at row 0: its first request finds a band)
        assert len(c["seqs"]) == len(seqs), name
        for seq, reqs in zip(seqs, c["seqs"]):
            assert [r[0] for r in reqs] == seq, name
            submitted = 0
            for n_req, (y_end, begin, end, cover) in enumerate(reqs):
                what = (name, seq, n_req)
                assert begin == submitted and begin <= end <= len(parts), what        # every part once, in sorted order
                started = [k for k in range(len(parts)) if y0[k] < y_end]              # the parts rows [0, y_end) may touch
                if submitted == 0:
                    assert list(range(begin, end)) == started, what                   # the first request: those alone
                else:
                    assert end == len(parts), what                                    # the second: nothing is left
                assert y0[0] > 0 or n_req == 0 or end == len(parts), what             # (the first request of a plan is the first one made)
                submitted = end
                assert all(k < submitted for k in started), what
                assert cover == (started[-1] if started else -1), what                # none: exactly when no band starts above y_end
                assert cover < submitted, what
                n_none_seen += cover == -1
            assert submitted == len(parts), (name, seq)
    assert n_direct_seen >= 3 + 3 + 4 + 4 + 1 + 2 + 3 and n_none_seen > 0
