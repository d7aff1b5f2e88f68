"""Thumbnails at the C-ABI and in the Python host, CPU only: the crop / turn / fit rule of include/imagestitch.h (the grid of chosen
images, pages/index/index.wxml:4-22: one <image mode="aspectFill"> per image; the modal image of index.wxml:202 is aspectFit) against a
numpy restatement, the struct layouts, and the argument errors that need no device."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import imagestitching_amd as ist
from imagestitching_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL, FIT = L.THUMB_FILL, L.THUMB_FIT


def turned(a, o):
    """the displayed image of a stored array under EXIF orientation o: the header's table, as numpy writes it"""
    return {1: a, 2: a[:, ::-1], 3: a[::-1, ::-1], 4: a[::-1], 5: a.swapaxes(0, 1), 6: a.swapaxes(0, 1)[:, ::-1],
            7: a.swapaxes(0, 1)[::-1, ::-1], 8: a.swapaxes(0, 1)[::-1]}[o]


def rule(bw, bh, o, tw, th, mode, orient=True):
    """section 1 of the rule, line by line (Python floats are IEEE doubles): (width, height, stored window x, y, w, h)"""
    o = o if orient and 1 <= o <= 8 else 1
    W, H = (bw, bh) if o <= 4 else (bh, bw)
    if mode == FILL:
        if tw / W >= th / H:
            cw, ch = W, min(max(math.floor(th * W / tw + 0.5), 1), H)
        else:
            cw, ch = min(max(math.floor(tw * H / th + 0.5), 1), W), H
        cx, cy = (W - cw) // 2, (H - ch) // 2
        ow, oh = tw, th
    else:
        cx, cy, cw, ch = 0, 0, W, H
        ow, oh = ist.preview_fit(W, H, tw, th)
    # the window in stored space: where the displayed window's pixels come from (an index map turned like the image)
    idx = turned(np.arange(bw * bh, dtype=np.int64).reshape(bh, bw), o)[cy:cy + ch, cx:cx + cw] if bw * bh <= 1 << 16 else None
    if idx is not None:
        ys, xs = idx // bw, idx % bw
        window = (int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1))
    else:                                                   # large images: the same map in closed form
        x, y, w, h = (cy, cx, ch, cw) if o >= 5 else (cx, cy, cw, ch)
        if o in (2, 3, 7, 8):
            x = bw - x - w
        if o in (3, 4, 6, 7):
            y = bh - y - h
        window = (x, y, w, h)
    return (ow, oh) + window


def layout(cases, tw, th, mode, orient=True):
    n = len(cases)
    descs = (L.ImageDesc * max(1, n))(*[L.ImageDesc(bw, bh, o, 0, 0, 0, 0) for bw, bh, o in cases])
    items = (L.ThumbItem * max(1, n))()
    total = C.c_int64(-1)
    spec = L.ThumbSpec(tw, th, mode, 1 if orient else 0)
    rc = L.lib.ist_thumb_layout(descs, n, C.byref(spec), items, C.byref(total))
    return rc, [(t.width, t.height, t.src_x, t.src_y, t.src_w, t.src_h) for t in items[:n]], items, total.value


TURN_OF = {1: 0, 2: 1, 3: 3, 4: 2, 5: 4, 6: 6, 7: 7, 8: 5}       # FLIP_X = 1, FLIP_Y = 2, then TRANSPOSE = 4


def test_the_turn_bits_are_the_exif_table():
    """mirrors inside the stored array, then the transposition: the eight displayed images of the header's table"""
    a = np.arange(5 * 7).reshape(5, 7)
    for o, turn in TURN_OF.items():
        b = a
        if turn & L.TURN_FLIP_X:
            b = b[:, ::-1]
        if turn & L.TURN_FLIP_Y:
            b = b[::-1]
        if turn & L.TURN_TRANSPOSE:
            b = b.T
        assert np.array_equal(b, turned(a, o)), o
    rc, _, items, _ = layout([(7, 5, o) for o in range(0, 10)], 3, 3, FILL)
    assert rc == 0 and [t.turn for t in items[:10]] == [0] + [TURN_OF[o] for o in range(1, 9)] + [0]       # 0 and 9 count as 1
    from PIL import Image
    pil = {2: Image.FLIP_LEFT_RIGHT, 3: Image.ROTATE_180, 4: Image.FLIP_TOP_BOTTOM, 5: Image.TRANSPOSE, 6: Image.ROTATE_270,
           7: Image.TRANSVERSE, 8: Image.ROTATE_90}
    img = np.random.default_rng(1).integers(0, 256, (5, 7, 4), dtype=np.uint8)
    for o, method in pil.items():
        assert np.array_equal(np.asarray(Image.fromarray(img).transpose(method)), turned(img, o)), o


def test_layout_matches_the_rule_on_random_cases():
    rng = np.random.default_rng(20)
    for mode in (FILL, FIT):
        for orient in (True, False):
            cases, cells = [], []
            for _ in range(500):
                small = rng.random() < 0.4                  # (small images also check the window through the index map)
                hi = 200 if small else 5000
                cases.append((int(rng.integers(1, hi + 1)), int(rng.integers(1, hi + 1)), int(rng.integers(1, 9))))
                cells.append((int(rng.integers(1, 401)), int(rng.integers(1, 401))))
            for (bw, bh, o), (tw, th) in zip(cases, cells):
                rc, got, items, total = layout([(bw, bh, o)], tw, th, mode, orient)
                want = rule(bw, bh, o, tw, th, mode, orient)
                assert rc == 0 and got[0] == want, ((bw, bh, o, tw, th, mode, orient), got[0], want)
                assert items[0].turn == (TURN_OF[o] if orient else 0) and items[0].offset == 0 and total == 4 * want[0] * want[1]
                x, y, w, h = want[2:]
                assert 0 <= x and 0 <= y and w >= 1 and h >= 1 and x + w <= bw and y + h <= bh


def test_known_values():
    # a phone photo held upright: stored 4032 x 3024 landscape, displayed 3024 x 4032, the middle square of it
    rc, got, items, _ = layout([(4032, 3024, 6)], 96, 96, FILL)
    assert rc == 0 and got[0] == (96, 96, 504, 0, 3024, 3024) and items[0].turn == (L.TURN_FLIP_Y | L.TURN_TRANSPOSE)
    assert rule(4032, 3024, 6, 96, 96, FILL) == got[0]       # displayed window 3024 x 3024 at cy = 504 -> stored x0 = 504
    assert layout([(4032, 3024, 6)], 96, 96, FIT)[1][0] == (72, 96, 0, 0, 4032, 3024)
    assert layout([(4032, 3024, 6)], 96, 96, FILL, orient=False)[1][0] == (96, 96, 504, 0, 3024, 3024)
    assert layout([(4032, 3024, 6)], 96, 96, FIT, orient=False)[1][0] == (96, 72, 0, 0, 4032, 3024)
    # 1-pixel images: the window is the pixel, whatever the cell
    for o in range(1, 9):
        assert layout([(1, 1, o)], 96, 40, FILL)[1][0] == (96, 40, 0, 0, 1, 1)
        assert layout([(1, 1, o)], 96, 40, FIT)[1][0] == (40, 40, 0, 0, 1, 1)
        assert layout([(1, 9, o)], 5, 5, FILL)[1][0][2:] == (0, 4, 1, 1)
    # the cell's aspect ratio is the image's: the window is the whole image, in both modes
    for o in range(1, 9):
        cell = (100, 75) if o <= 4 else (75, 100)
        assert layout([(4000, 3000, o)], cell[0], cell[1], FILL)[1][0] == cell + (0, 0, 4000, 3000)
        assert layout([(4000, 3000, o)], cell[0], cell[1], FIT)[1][0] == cell + (0, 0, 4000, 3000)
    # bmp_width / bmp_height are the stored size when given
    descs = (L.ImageDesc * 1)(L.ImageDesc(4000, 3000, 1, 400, 300, 0, 0))
    items = (L.ThumbItem * 1)()
    assert L.lib.ist_thumb_layout(descs, 1, C.byref(L.ThumbSpec(10, 10, FILL, 1)), items, None) == 0
    assert (items[0].src_x, items[0].src_y, items[0].src_w, items[0].src_h) == (50, 0, 300, 300)


def test_the_floor_side_of_an_odd_margin_follows_the_orientation():
    """W - cw odd: the displayed window starts at floor((W - cw) / 2), so a mirrored axis leaves the spare pixel at the stored
    array's OTHER end"""
    for o in range(1, 9):
        bw, bh = (10, 7) if o <= 4 else (7, 10)              # displayed 10 x 7, a square cell: cw = 7, margin 3 -> cx = 1
        rc, got, _, _ = layout([(bw, bh, o)], 4, 4, FILL)
        assert rc == 0 and got[0] == rule(bw, bh, o, 4, 4, FILL)
        x, y, w, h = got[0][2:]
        # displayed columns 1..7 of 0..9; stored: along x for o <= 4 (mirrored for 2, 3), along y for o >= 5 (mirrored for 6, 7)
        want = {1: (1, 0, 7, 7), 2: (2, 0, 7, 7), 3: (2, 0, 7, 7), 4: (1, 0, 7, 7), 5: (0, 1, 7, 7), 6: (0, 2, 7, 7), 7: (0, 2, 7, 7), 8: (0, 1, 7, 7)}[o]
        assert (x, y, w, h) == want, o
        bw, bh = (7, 10) if o <= 4 else (10, 7)              # displayed 7 x 10: ch = 7, cy = 1
        x, y, w, h = layout([(bw, bh, o)], 4, 4, FILL)[1][0][2:]
        want = {1: (0, 1, 7, 7), 2: (0, 1, 7, 7), 3: (0, 2, 7, 7), 4: (0, 2, 7, 7), 5: (1, 0, 7, 7), 6: (1, 0, 7, 7), 7: (2, 0, 7, 7), 8: (2, 0, 7, 7)}[o]
        assert (x, y, w, h) == want, o


def test_offsets_are_dense_and_the_count_is_capped():
    rng = np.random.default_rng(3)
    cases = [(int(rng.integers(1, 3000)), int(rng.integers(1, 3000)), int(rng.integers(1, 9))) for _ in range(4096)]
    rc, got, items, total = layout(cases, 60, 45, FIT)
    assert rc == 0
    at = 0
    for k in range(4096):
        assert items[k].offset == at
        at += 4 * items[k].width * items[k].height
    assert total == at
    rc, _, _, total = layout(cases + [(5, 5, 1)], 60, 45, FIT)
    assert rc == -7 and total == 0 and "4096" in L.last_error()          # IST_E_UNSUPPORTED
    assert layout([], 4, 4, FILL)[0] == 0


def test_layout_argument_errors():
    for tw, th, mode in [(0, 5, FILL), (5, 0, FILL), (-2, 5, FIT), (5, 5, 2), (5, 5, -1)]:
        assert layout([(10, 10, 1)], tw, th, mode)[0] == -1, (tw, th, mode)
    assert layout([(10, 10, 1), (0, 10, 1)], 4, 4, FILL)[0] == -1 and "image 1" in L.last_error()
    assert layout([(10, -3, 1)], 4, 4, FIT)[0] == -1
    descs = (L.ImageDesc * 1)(L.ImageDesc(4, 4, 1, 0, 0, 0, 0))
    items = (L.ThumbItem * 1)()
    spec = L.ThumbSpec(4, 4, FILL, 1)
    assert L.lib.ist_thumb_layout(None, 1, C.byref(spec), items, None) == -1
    assert L.lib.ist_thumb_layout(descs, 1, None, items, None) == -1
    assert L.lib.ist_thumb_layout(descs, 1, C.byref(spec), None, None) == -1
    assert L.lib.ist_thumb_layout(descs, -1, C.byref(spec), items, None) == -1
    with pytest.raises(ist.StitchError) as e:
        ist.thumbnail_layout([(10, 10)], (0, 4), "fill")
    assert e.value.code == -1
    with pytest.raises(ValueError, match="'fill' or 'fit'"):
        ist.thumbnail_layout([(10, 10)], (4, 4), "cover")
    with pytest.raises(TypeError, match="cell"):
        ist.thumbnail_layout([(10, 10)], 4, "fill")


def test_the_python_rule_takes_every_kind_of_image():
    got = ist.thumbnail_layout([(4032, 3024, 6), {"width": 601, "height": 777, "orientation": 3}, np.zeros((30, 40, 4), np.uint8)], (96, 96), "fill")
    assert [g["window"] for g in got] == [(504, 0, 3024, 3024), (0, 88, 601, 601), (5, 0, 30, 30)]
    assert [g["offset"] for g in got] == [0, 36864, 73728] and [g["turn"] for g in got] == [6, 3, 0]
    assert ist.thumbnail_layout([(4032, 3024, 6)], (96, 96), "fit", orient=False)[0]["width"] == 96


def test_struct_layouts_match_the_header(tmp_path):
    assert C.sizeof(L.ThumbSpec) == 16 and C.sizeof(L.ThumbItem) == 40
    assert [getattr(L.ThumbItem, f).offset for f, _ in L.ThumbItem._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32]
    c = tmp_path / "t.c"
    c.write_text('#include <stddef.h>\n#include "imagestitch.h"\n'
                 "int main(void){ ist_thumb_spec s; ist_thumb_item t; (void)s; (void)t;\n"
                 "  return sizeof(ist_thumb_spec) == 16 && offsetof(ist_thumb_spec, mode) == 8 && offsetof(ist_thumb_spec, apply_orientation) == 12 &&\n"
                 "  sizeof(ist_thumb_item) == 40 && offsetof(ist_thumb_item, src_x) == 8 && offsetof(ist_thumb_item, src_h) == 20 &&\n"
                 "  offsetof(ist_thumb_item, turn) == 24 && offsetof(ist_thumb_item, offset) == 32 && IST_THUMB_FILL == 0 && IST_THUMB_FIT == 1 &&\n"
                 "  IST_TURN_FLIP_X == 1 && IST_TURN_FLIP_Y == 2 && IST_TURN_TRANSPOSE == 4 && IST_ABI_VERSION == 2 ? 0 : 1; }\n")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


def test_the_entry_points_need_a_context():
    """the context is checked first, and no context can be made without a device: the other argument errors of ist_thumbs_device and
    ist_bitmaps_thumbs are in tests/test_gpu_thumbs.py"""
    descs = (L.ImageDesc * 1)(L.ImageDesc(4, 4, 1, 0, 0, 0, 0))
    items = (L.ThumbItem * 1)()
    spec = L.ThumbSpec(4, 4, FILL, 1)
    assert L.lib.ist_thumbs_device(None, descs, None, None, 1, C.byref(spec), None, 0, items, None) == -4
    assert "绘图上下文" in L.last_error()
    out = C.cast(1, C.POINTER(C.c_uint8))
    assert L.lib.ist_bitmaps_thumbs(None, None, 1, C.byref(spec), items, C.byref(out)) == -4 and not out
    assert L.lib.ist_debug_thumb_launches() == 0 or L.lib.ist_device_count() > 0
    if L.lib.ist_device_count() == 0:
        import torch
        assert ist.thumbnails([], (4, 4)) == [] and ist.thumbnails_device([], (4, 4)) == []
        with pytest.raises(TypeError, match="CUDA tensors"):
            ist.thumbnails_device([torch.zeros((4, 4, 4), dtype=torch.uint8)], (2, 2))
        with pytest.raises(TypeError, match="Bitmaps"):
            ist.thumbnails([np.zeros((4, 4, 4), np.uint8)], (2, 2))
