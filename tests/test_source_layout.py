"""Where the host entry points put the caller's sources in device scratch (SourceLayout, ist_sources.cpp): one request or several in
one block (the batch), whole bitmaps (the one-shot path, the batch, the duplex bands) or the rows a slot of a cut holds (the device
group: dist.py's rows_needed, which tests/test_shard_ops.py holds equal to shard_holdings).  tools/source_layout.cpp prints the
sections, the placed pointers and the copy items; this checks them against the rule, and the checks' codes and messages.  Pure CPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from imagestitching_amd import _lib as L
from imagestitching_amd import dist as D
from tests.test_shard_holdings import SLOTS, SPLITS, _random_job

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = 256                 # kSourceTail
E_INVALID, E_DECODE = -1, -6


def _up(v):
    return (v + 255) & ~255


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("source_layout") / "source_layout")
    csrc = os.path.join(ROOT, "imagestitching_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "source_layout.cpp")] + [os.path.join(csrc, f) for f in ("ist_plan.cpp", "ist_sources.cpp")] +
                   ["-o", exe], check=True, capture_output=True, timeout=300)
    return exe


class Img:
    def __init__(self, w, h, bw=0, bh=0, pitch=None, null=False):
        self.w, self.h, self.bw, self.bh, self.null = w, h, bw, bh, null
        self.pitch = 4 * self.bitmap_w if pitch is None else pitch

    @property
    def bitmap_w(self):
        return self.bw if self.bw > 0 else self.w

    @property
    def bitmap_h(self):
        return self.bh if self.bh > 0 else self.h


def _run(tool, cases):
    """cases: [(requests, copies)]; a request is (images, {image: (y0, y1)}, dense).  Returns one dict per case."""
    text = []
    for reqs, copies in cases:
        text.append(str(len(reqs)))
        for imgs, held, dense in reqs:
            text.append("%d %d %d" % (len(imgs), len(held), int(dense)))
            text += ["%d %d %d %d %d %d" % (m.w, m.h, m.bw, m.bh, m.pitch, int(m.null)) for m in imgs]
            text += ["%d %d %d" % (i, a, b) for i, (a, b) in sorted(held.items())]
        text.append(str(len(copies)))
        text += ["%d %d %d" % c for c in copies]
    out = subprocess.run([tool], input="\n".join(text) + "\n", check=True, capture_output=True, text=True, timeout=300).stdout
    got, cur = [], None
    for line in out.splitlines():
        t = line.split(" ", 2) if line.startswith("add ") else line.split()
        if t[0] == "add":
            if cur is None:
                cur = {"add": [], "place": {}, "copy": [], "all": []}
            cur["add"].append((int(t[1]), t[2]))
        elif t[0] == "bytes":
            cur["bytes"] = int(t[1])
        elif t[0] == "place":
            cur["place"][int(t[1])] = (int(t[2]), int(t[3]))
        elif t[0] == "copy":
            cur["copy"].append(tuple(map(int, t[1:])))
        elif t[0] == "all":
            cur["all"].append(tuple(map(int, t[1:])))
        else:
            assert t[0] == "end", line
            got.append(cur)
            cur = None
    assert len(got) == len(cases)
    return got


def _check_layout(reqs, copies, c):
    """the sections, pointers and copy items of a case whose every request was accepted"""
    assert c["add"] == [(0, "-")] * len(reqs)
    flat = [(m, held.get(i), dense) for imgs, held, dense in reqs for i, m in enumerate(imgs)]
    assert sorted(c["place"]) == list(range(len(flat)))
    want_bytes = sum(_up((rows[1] - rows[0]) * 4 * m.bitmap_w + TAIL) for m, rows, _ in flat if rows)
    assert c["bytes"] == max(want_bytes, 256)
    sections, start_of = [], {}
    for g, (m, rows, dense) in enumerate(flat):
        off, pitch = c["place"][g]
        if rows is None:
            assert (off, pitch) == (-1, 0), g
            continue
        row = 4 * m.bitmap_w
        assert pitch == row, g
        start = off + rows[0] * row                  # the biased pointer addresses row 0: row y0 is the section's first byte
        assert start % 256 == 0 and start >= 0, g
        end = start + (rows[1] - rows[0]) * row + TAIL
        assert end <= c["bytes"], g                  # the held rows and the tail lie inside the block
        sections.append((start, end))
        start_of[g] = start
    sections.sort()
    assert all(a[1] <= b[0] for a, b in zip(sections, sections[1:])), sections   # disjoint
    # copy(i, r0, r1): rows [r0, r1) of the caller's image, row by row into the section's rows r0 - y0 ..
    assert len(c["copy"]) == len(copies)
    for (g, r0, r1), got in zip(copies, c["copy"]):
        m, rows, dense = flat[g]
        hp = 4 * m.bitmap_w if dense else m.pitch
        assert got == (g, r0, r1, start_of[g] + (r0 - rows[0]) * 4 * m.bitmap_w, r0 * hp, hp, 4 * m.bitmap_w, r1 - r0), (g, r0, r1)
    # copy_all: every held image whole, in index order across the requests
    want = []
    for g, (m, rows, dense) in enumerate(flat):
        if rows:
            hp = 4 * m.bitmap_w if dense else m.pitch
            want.append((start_of[g], rows[0] * hp, hp, 4 * m.bitmap_w, rows[1] - rows[0]))
    assert c["all"] == want


def _copies(rng, reqs):
    out, g = [], 0
    for imgs, held, _ in reqs:
        for i in range(len(imgs)):
            if i in held:
                a, b = held[i]
                out.append((g + i, a, b))
                r0 = int(rng.integers(a, b))
                out.append((g + i, r0, int(rng.integers(r0 + 1, b + 1))))
        g += len(imgs)
    return out


def _random_image(rng):
    w, h = int(rng.integers(1, 300)), int(rng.integers(1, 300))
    bw, bh = (int(rng.integers(1, 300)), int(rng.integers(1, 300))) if rng.random() < 0.3 else (0, 0)
    m = Img(w, h, bw, bh)
    m.pitch = 4 * m.bitmap_w + 4 * int(rng.choice([0, 0, 1, 13, 1000]))
    return m


def test_whole_bitmaps_of_one_or_several_requests(tool):
    rng = np.random.default_rng(2024)
    cases = []
    for _ in range(200):
        reqs = []
        for _ in range(int(rng.integers(1, 4))):
            imgs = [_random_image(rng) for _ in range(int(rng.integers(1, 7)))]
            held = {i: (0, m.bitmap_h) for i, m in enumerate(imgs) if rng.random() < 0.8}
            reqs.append((imgs, held, bool(rng.random() < 0.3)))
        cases.append((reqs, _copies(rng, reqs)))
    for (reqs, copies), c in zip(cases, _run(tool, cases)):
        _check_layout(reqs, copies, c)


def test_holdings_of_random_cuts(tool):
    rng = np.random.default_rng(6061)
    cases = []
    for _ in range(16):
        sizes, ori, direction, opts = _random_job(rng)
        descs = [{"width": w, "height": h, "orientation": o} for (w, h), o in zip(sizes, ori)]
        for split in SPLITS:
            for world in SLOTS:
                try:
                    sh = D.ShardedStitch(descs, direction, opts, 0, world, 0, split=split)
                except L.StitchError as e:      # the per-draw cuts refuse draws that share canvas pixels
                    assert split in ("image", "band") and "rows" in e.reason, e
                    continue
                imgs = [Img(w, h, pitch=4 * w + 4 * int(rng.integers(0, 3))) for w, h in sizes]
                for s in range(world):
                    held = sh.rows_needed(s)
                    assert all(0 <= a < b <= imgs[i].bitmap_h for i, (a, b) in held.items())
                    reqs = [(imgs, held, False)]
                    cases.append((reqs, _copies(rng, reqs)))
    assert any(a > 0 for reqs, _ in cases for _, held, _ in reqs for a, _ in held.values())   # holdings that start below row 0
    for (reqs, copies), c in zip(cases, _run(tool, cases)):
        _check_layout(reqs, copies, c)


def test_refused_sources_first_image_first(tool):
    ok = lambda: Img(40, 30, pitch=160)                           # noqa: E731
    null, empty, empty_bmp = Img(40, 30, null=True), Img(0, 30), Img(40, 0)
    short = Img(40, 30, pitch=156)
    bmp_short = Img(40, 30, bw=50, pitch=196)                     # the pitch is checked against the bitmap width
    whole = lambda imgs: {i: (0, max(1, m.bitmap_h)) for i, m in enumerate(imgs)}  # noqa: E731
    table = [
        ([ok(), null, ok()], None, (E_DECODE, "图片1解码异常")),
        ([ok(), ok(), empty], None, (E_DECODE, "图片2解码异常")),
        ([empty_bmp, ok()], None, (E_DECODE, "图片0解码异常")),
        ([ok(), short], None, (E_INVALID, "src_pitch too small")),
        ([bmp_short], None, (E_INVALID, "src_pitch too small")),
        ([ok(), short, null], None, (E_INVALID, "src_pitch too small")),         # two faults: the first image's
        ([ok(), null, short], None, (E_DECODE, "图片1解码异常")),
        ([short, ok(), empty], None, (E_INVALID, "src_pitch too small")),
        ([null, short, ok()], {1: (0, 30), 2: (0, 30)}, (E_INVALID, "src_pitch too small")),   # an image nobody holds is not checked
        ([null, ok()], {1: (5, 9)}, (0, "-")),
    ]
    cases = [([(imgs, whole(imgs) if held is None else held, False)], []) for imgs, held, _ in table]
    got = _run(tool, cases)
    for (imgs, held, want), c in zip(table, got):
        assert c["add"] == [want], (want, c["add"])
    # a dense request (src_pitch NULL) has no pitch to refuse; in a batch the first refused request ends the layout
    ok_req = ([ok(), ok()], whole([ok(), ok()]), False)
    cases = [([([short], {0: (0, 30)}, True)], []), ([ok_req, ([ok(), null], {0: (0, 30), 1: (0, 30)}, False), ok_req], [])]
    got = _run(tool, cases)
    assert got[0]["add"] == [(0, "-")]
    assert got[1]["add"] == [(0, "-"), (E_DECODE, "图片1解码异常")] and "bytes" not in got[1]
