"""The adaptive-row-filter PNG option at the C-ABI and in the Python host, CPU only: the new entry point (ist_ctx_set_png_filter), which
looks at its context first, ist_png_bound, which the setting does not move, and the option parser, which refuses an unknown filter
before it asks for a device and a per-request filter in a batch.  (What needs a context - IST_E_INVALID for an unknown value,
IST_E_UNSUPPORTED at level 0 on every *_png entry point - is in tests/test_gpu_png_filter.py: without a device there is no context.)
Reference anchor: the PNG export of onStitch (utils/canvas.js:205-242, pages/index/index.js:1577-1579)."""
import sys

import numpy as np
import pytest

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests import test_png_rgb_abi as A

S = sys.modules["imagestitching_amd.stitch"]      # (the package's attribute `stitch` is the function)
PAETH, ADAPTIVE = 0, 1          # IST_PNG_FILTER_PAETH / IST_PNG_FILTER_ADAPTIVE
E_NO_CONTEXT = -4


def test_the_symbol_exists_and_needs_a_context():
    assert hasattr(L.lib, "ist_ctx_set_png_filter")
    assert L.lib.ist_ctx_set_png_filter(None, ADAPTIVE) == E_NO_CONTEXT
    assert L.lib.ist_ctx_set_png_filter(None, PAETH) == E_NO_CONTEXT
    assert L.lib.ist_ctx_set_png_filter(None, 7) == E_NO_CONTEXT      # (the context is looked at first, as by ist_ctx_set_png_color)


@pytest.mark.parametrize("w,h", sorted(A.BOUND_BEFORE))
def test_png_bound_is_unchanged(w, h):
    """the grid does not change and the bound counts every chunk as stored: the numbers of the commit before the colour setting"""
    assert L.lib.ist_png_bound(w, h) == A.BOUND_BEFORE[(w, h)]


def test_the_option_parser_refuses_an_unknown_filter_before_any_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a context was asked for")

    monkeypatch.setattr(S, "_ctx", no_device)
    img = np.zeros((4, 4, 4), np.uint8)
    assert "pngFilter" in ist.DEFAULT_OPTS and ist.DEFAULT_OPTS["pngFilter"] is None
    for call in (lambda: ist.stitch_png([img], "vertical", {"pngFilter": "sub"}),
                 lambda: ist.stitch_png_batch([([img], "vertical")], row_filter="sub"),
                 lambda: ist.stitch_files(["/nonexistent.png"], "vertical", {"pngFilter": "sub"}),
                 lambda: ist.encode_png(img, row_filter="sub"),
                 lambda: ist.encode_png_device(img, row_filter="sub"),
                 lambda: ist.encode_png_batch_device([img], row_filter="sub"),
                 lambda: ist.stitch_png([img], "vertical", {"pngFilter": 1}),
                 lambda: ist.stitch_png([img], "vertical", {"pngFilter": "Adaptive"})):
        with pytest.raises(ValueError, match="pngFilter must be 'paeth' or 'adaptive'"):
            call()
    with pytest.raises(ValueError, match="pngColor"):                # (and the colour is still checked, in front of the filter)
        ist.encode_png(img, color="rgbx", row_filter="sub")
    assert S._png_filter(None) == PAETH and S._png_filter("paeth") == PAETH and S._png_filter("adaptive") == ADAPTIVE


def test_a_batch_takes_one_filter_for_all_its_requests():
    img = np.zeros((4, 4, 4), np.uint8)
    assert "pngFilter" in S._BATCH_REFUSED
    for batch in (ist.stitch_png_batch, ist.stitch_batch):
        with pytest.raises(TypeError, match="pngFilter"):
            batch([([img], "vertical", {"pngFilter": "adaptive"})])
