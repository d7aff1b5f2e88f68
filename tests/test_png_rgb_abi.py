"""The RGB PNG option at the C-ABI and in the Python host, CPU only: the two new entry points (ist_ctx_set_png_color,
ist_debug_png_grid), the chunk grid of both colour forms against the CPU references, ist_png_bound as an upper bound of both forms,
and the option parser, which refuses an unknown colour before it asks for a device.  Reference anchor: the PNG export of onStitch
(utils/canvas.js:205-242, pages/index/index.js:1577-1579)."""
import ctypes as C
import sys

import pytest

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests import png_deflate_reference as R
from tests import png_rgb_cases as K
from tests import png_rgb_reference as G

S = sys.modules["imagestitching_amd.stitch"]      # (the package's attribute `stitch` is the function)
RGBA, RGB = 0, 1                # IST_PNG_RGBA / IST_PNG_RGB
E_INVALID, E_NO_CONTEXT = -1, -4
SLOT = R.CH + 128               # bytes a chunk may take in the file (stored form + framing + alignment pads)

# ist_png_bound(w, h) of the commit before the colour setting existed (read from its library): the setting must not move it
BOUND_BEFORE = {(1, 1): 16680, (3, 5): 16680, (100, 130): 66216, (2730, 5): 82728, (2731, 3): 49704, (4096, 2): 66216, (5461, 3): 99240,
                (5462, 2): 66216, (10923, 2): 99240, (5462, 400): 13209768, (4032, 27216): 449390760}


def _grid(w, h, color):
    out = (C.c_int64 * 4)(-7, -7, -7, -7)
    rc = L.lib.ist_debug_png_grid(w, h, color, out)
    return rc, tuple(out)


def test_the_symbols_exist():
    assert hasattr(L.lib, "ist_ctx_set_png_color") and hasattr(L.lib, "ist_debug_png_grid")
    assert ist.debug_png_grid(100, 130, "rgb") == (3, 54, 0, 0) and ist.debug_png_grid(100, 130) == (4, 40, 0, 0)


@pytest.mark.parametrize("w,h", K.SHAPES + K.BOUNDARY_SHAPES + ((5462, 400),))
def test_grid_is_the_references_in_both_forms(w, h):
    rc, got = _grid(w, h, RGB)
    assert rc == 0 and got == G.grid_numbers_rgb(w, h) and got[0] == len(G.make_grid_rgb(w, h))
    rc, got4 = _grid(w, h, RGBA)
    assert rc == 0 and got4 == G.grid_numbers_rgba(w, h) and got4[0] == len(R.make_grid(w, h))
    assert got[0] <= got4[0]
    if (w, h) in K.CHUNK_BYTES:
        assert got[0] == len(K.CHUNK_BYTES[(w, h)])


def test_grid_on_both_sides_of_both_boundaries():
    assert _grid(5461, 3, RGB)[1] == (3, 1, 0, 0) and _grid(5462, 3, RGB)[1] == (6, 0, 2, 5461)         # R = 16384 | 16387
    assert _grid(4095, 3, RGBA)[1] == (3, 1, 0, 0) and _grid(4096, 3, RGBA)[1] == (6, 0, 2, 4095)       # R = 16381 | 16385
    assert _grid(4096, 3, RGB)[1] == (3, 1, 0, 0)                                                        # the RGBA boundary is not special
    assert _grid(2730, 5, RGB)[1] == (3, 2, 0, 0) and _grid(2731, 5, RGB)[1] == (5, 1, 0, 0)             # two rows per chunk | one
    assert _grid(10922, 1, RGB)[1] == (2, 0, 2, 5461) and _grid(10923, 1, RGB)[1] == (3, 0, 3, 5461)     # a third piece of one pixel


def test_grid_refuses_bad_arguments():
    for args in ((0, 1, RGB), (1, 0, RGB), (-3, 5, RGBA), (5, 5, 2), (5, 5, -1)):
        rc, out = _grid(*args)
        assert rc == E_INVALID and out == (-7, -7, -7, -7), args
    assert L.lib.ist_debug_png_grid(5, 5, RGB, None) == E_INVALID
    with pytest.raises(L.StitchError):
        ist.debug_png_grid(0, 4)


def test_set_png_color_needs_a_context():
    assert L.lib.ist_ctx_set_png_color(None, RGB) == E_NO_CONTEXT
    assert L.lib.ist_ctx_set_png_color(None, 7) == E_NO_CONTEXT      # (the context is looked at first, as by ist_ctx_set_png_level)


@pytest.mark.parametrize("w,h", sorted(BOUND_BEFORE))
def test_png_bound_is_unchanged_and_bounds_the_rgb_form(w, h):
    bound = L.lib.ist_png_bound(w, h)
    assert bound == BOUND_BEFORE[(w, h)]
    n_rgb = G.grid_numbers_rgb(w, h)[0]
    data = n_rgb * SLOT + 16                                          # png_deflate_bound: every chunk stored, in its slot
    assert bound >= 64 + data + (data // (1 << 30) + 2) * 12 + 64
    assert n_rgb <= G.grid_numbers_rgba(w, h)[0]


def test_the_option_parser_refuses_an_unknown_colour_before_any_device(monkeypatch):
    import numpy as np

    def no_device(*a, **k):
        raise AssertionError("a context was asked for")

    monkeypatch.setattr(S, "_ctx", no_device)
    img = np.zeros((4, 4, 4), np.uint8)
    assert "pngColor" in ist.DEFAULT_OPTS and ist.DEFAULT_OPTS["pngColor"] is None
    for call in (lambda: ist.stitch_png([img], "vertical", {"pngColor": "rgbx"}),
                 lambda: ist.stitch_png_batch([([img], "vertical")], color="rgbx"),
                 lambda: ist.stitch_files(["/nonexistent.png"], "vertical", {"pngColor": "rgbx"}),
                 lambda: ist.encode_png(img, color="rgbx"),
                 lambda: ist.encode_png_device(img, color="rgbx"),
                 lambda: ist.encode_png_batch_device([img], color="rgbx"),
                 lambda: ist.stitch_png([img], "vertical", {"pngColor": 1}),
                 lambda: ist.debug_png_grid(4, 4, "RGB")):
        with pytest.raises(ValueError, match="pngColor must be 'rgba' or 'rgb'"):
            call()
    with pytest.raises(TypeError, match="pngColor"):                 # one colour form for a whole batch, like pngLevel
        ist.stitch_png_batch([([img], "vertical", {"pngColor": "rgb"})])
    assert S._png_color(None) == RGBA and S._png_color("rgba") == RGBA and S._png_color("rgb") == RGB
