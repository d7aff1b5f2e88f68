"""The CPU statement of the adaptive PNG row filters (tests/png_filter_reference.py) judged on its own, and the inputs of the GPU
tests (tests/png_filter_cases.py) judged by it: every file decodes to its canvas, every regime the inputs were built for is reached,
and each near miss of the rule changes a file.  CPU only.  Reference anchor: the PNG export of onStitch (utils/canvas.js:205-242,
pages/index/index.js:1577-1579) - a file that decodes to the same pixels."""
import io
import zlib

import numpy as np
import pytest

from tests import png_deflate_reference as R
from tests import png_filter_cases as K
from tests import png_filter_reference as F
from tests import png_rgb_reference as G

BPPS = (4, 3)


def test_the_inputs_reach_their_regimes():
    K.check_regimes()


def _unfilter(filt, h, w, bpp):
    """PNG specification 9.2, byte by byte, from the filtered stream alone"""
    filt = np.frombuffer(filt, np.uint8).reshape(h, bpp * w + 1)
    out = np.zeros((h + 1, bpp * (w + 1)), np.int64)          # a zero row above and a zero pixel to the left
    for y in range(h):
        ft, line = int(filt[y, 0]), filt[y, 1:].astype(np.int64)
        row, up = out[y + 1], out[y]
        for i in range(bpp * w):
            a, b, c = int(row[i]), int(up[i + bpp]), int(up[i])
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            pred = (0, a, b, (a + b) >> 1, a if pa <= pb and pa <= pc else (b if pb <= pc else c))[ft]
            row[i + bpp] = (int(line[i]) + pred) & 255
    return out[1:, bpp:].astype(np.uint8).reshape(h, w, bpp)


@pytest.mark.parametrize("bpp", BPPS)
def test_the_filtered_stream_unfilters_to_the_canvas(bpp):
    """a plain decoder of the five types, on the small canvases that between them hold every type (in either colour form)"""
    seen = set()
    for name, a in K.shape_cases(4):
        h, w = a.shape[:2]
        if h * w > 12000:
            continue
        rep = K.report(name, a, bpp)
        seen |= set(rep.filtered[::bpp * w + 1])
        assert np.array_equal(_unfilter(rep.filtered, h, w, bpp), a[..., :bpp]), name
    assert seen == {0, 1, 2, 3, 4}, seen


@pytest.mark.parametrize("bpp", BPPS)
def test_every_reference_file_decodes_to_its_canvas(bpp):
    from PIL import Image
    for name, a in K.all_cases(bpp):
        rep = K.report(name, a, bpp)
        assert zlib.decompress(rep.stream) == rep.filtered, name
        im = Image.open(io.BytesIO(F.file_bytes_adaptive(a, bpp, rep.stream)))
        assert im.mode == ("RGBA" if bpp == 4 else "RGB") and np.array_equal(np.asarray(im), a[..., :bpp]), name
    name, a = K.slab_cut_case(bpp)
    im = Image.open(io.BytesIO(F.host_file_bytes_adaptive(a, bpp, K.report(name, a, bpp))))
    assert np.array_equal(np.asarray(im), a[..., :bpp]), name


def test_a_canvas_on_which_paeth_wins_every_row_gives_the_default_file():
    cases = dict(K.shape_cases(4))
    for name in ("filter white 64x33", "filter photo 1x1"):
        a = cases[name]
        assert set(F.row_filters(a, 4).tolist()) == {F.PAETH}, name
        assert F.file_bytes_adaptive(a, 4) == R.file_bytes(a), name
        assert F.file_bytes_adaptive(a, 3) == G.file_bytes_rgb(a), name
    a = cases["filter photo 257x19"]                                    # (and one where it does not: another file, never a larger filtered cost)
    assert F.file_bytes_adaptive(a, 4) != R.file_bytes(a)


def test_the_cost_and_the_tie_order_by_hand():
    a = np.zeros((2, 2, 4), np.uint8)
    a[0] = [[10, 250, 128, 0], [10, 250, 128, 0]]
    a[1] = [[12, 250, 128, 0], [10, 252, 128, 0]]
    cost = F.row_costs(a, 4)
    # row 0: None 2 x (10 + 6 + 128 + 0); Sub = Paeth: the first pixel only; Up = None; Average: x - (left >> 1) on the second pixel
    assert cost[0].tolist() == [288, 144, 288, 144 + 5 + 125 + 64, 144]
    # row 1: Average predicts (5, 125, 64, 0) and then (11, 250, 128, 0); Paeth predicts up, then left (both pixels above are alike)
    assert cost[1].tolist() == [12 + 6 + 128 + 10 + 4 + 128, 12 + 6 + 128 + 2 + 2, 2 + 2, 7 + 125 + 64 + 1 + 2, 2 + 2 + 2]
    assert F.row_filters(a, 4).tolist() == [F.PAETH, F.UP]             # row 0: Sub = Paeth, and Paeth wins the tie
    assert F.row_filters(a, 4, F.NEAR_MISSES["tie order 0,1,2,3,4"]).tolist() == [F.SUB, F.UP]
    assert F.row_costs(a, 3)[0].tolist() == cost[0].tolist() and F.row_costs(a[:, :, [0, 1, 3, 2]], 3)[0, 0] == 32
    b = np.zeros((1, 2, 4), np.uint8)
    b[0, 1] = 200                                                        # residual 200 costs 56, not 200
    assert F.row_costs(b, 4)[0, 0] == 4 * 56 and F.row_costs(b, 4, F.NEAR_MISSES["unsigned cost"])[0, 0] == 800


def test_the_choice_does_not_depend_on_the_grid():
    """rows of a canvas and the same rows cut out with the row above them choose alike"""
    name, a = K.shape_cases(4)[4]                                       # the 257 x 19 rows of chosen kinds
    types = F.row_filters(a, 4)
    for y in range(1, a.shape[0]):
        assert F.row_filters(a[y - 1:y + 1], 4)[1] == types[y], y
