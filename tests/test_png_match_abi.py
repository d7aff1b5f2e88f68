"""The PNG window-match option at the C-ABI and in the Python host, CPU only: the new entry point (ist_ctx_set_png_match), which looks at
its context first, the enum of the header, ist_png_bound, which the setting does not move, and the option parser, which refuses an
unknown value with a TypeError before it asks for a device and a per-request pngMatch in a batch.  (What needs a context -
IST_E_INVALID for an unknown value, IST_E_UNSUPPORTED at level 0 on every *_png entry point - is in tests/test_gpu_png_match.py: without
a device there is no context.)  Reference anchor: the PNG export of onStitch (utils/canvas.js:205-242, pages/index/index.js:1577-1579)."""
import os
import re
import sys

import numpy as np
import pytest

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests import test_png_rgb_abi as A

S = sys.modules["imagestitching_amd.stitch"]      # (the package's attribute `stitch` is the function)
RUN, WINDOW = 0, 1              # IST_PNG_MATCH_RUN / IST_PNG_MATCH_WINDOW
E_NO_CONTEXT = -4
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "imagestitch.h")


def test_the_symbol_exists_and_looks_at_its_context_first():
    assert hasattr(L.lib, "ist_ctx_set_png_match")
    assert L.lib.ist_ctx_set_png_match(None, WINDOW) == E_NO_CONTEXT
    assert L.lib.ist_ctx_set_png_match(None, RUN) == E_NO_CONTEXT
    assert L.lib.ist_ctx_set_png_match(None, 7) == E_NO_CONTEXT        # (a bad value behind a NULL context: the context is looked at first)
    assert b"\xe6\x97\xa0\xe6\xb3\x95" in L.lib.ist_last_error()       # (the reference's message for a missing context)


def test_the_header_declares_the_enum_and_the_setter():
    text = open(HEADER, encoding="utf-8").read()
    assert re.search(r"enum\s*\{\s*IST_PNG_MATCH_RUN\s*=\s*0\s*,\s*IST_PNG_MATCH_WINDOW\s*=\s*1\s*\}\s*;", text)
    assert re.search(r"IST_API\s+int\s+ist_ctx_set_png_match\(ist_ctx\*\s*ctx,\s*int\s+match\);", text)
    assert S.PNG_MATCHES == {"run": RUN, "window": WINDOW}


@pytest.mark.parametrize("w,h", sorted(A.BOUND_BEFORE))
def test_png_bound_is_unchanged(w, h):
    """a window chunk is never larger than its stored form: the numbers of the commit before the colour setting"""
    assert L.lib.ist_png_bound(w, h) == A.BOUND_BEFORE[(w, h)]


def test_the_option_parser_refuses_an_unknown_match_before_any_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a context was asked for")

    monkeypatch.setattr(S, "_ctx", no_device)
    img = np.zeros((4, 4, 4), np.uint8)
    assert "pngMatch" in ist.DEFAULT_OPTS and ist.DEFAULT_OPTS["pngMatch"] is None
    for call in (lambda: ist.stitch_png([img], "vertical", {"pngMatch": "lz77"}),
                 lambda: ist.stitch_png_batch([([img], "vertical")], match="lz77"),
                 lambda: ist.stitch_files(["/nonexistent.png"], "vertical", {"pngMatch": "lz77"}),
                 lambda: ist.encode_png(img, match="lz77"),
                 lambda: ist.encode_png_device(img, match="lz77"),
                 lambda: ist.encode_png_batch_device([img], match="lz77"),
                 lambda: ist.stitch_png([img], "vertical", {"pngMatch": 1}),
                 lambda: ist.stitch_png([img], "vertical", {"pngMatch": "Window"})):
        with pytest.raises(TypeError, match="pngMatch must be 'run' or 'window'"):
            call()
    with pytest.raises(ValueError, match="pngColor"):                # (colour and filter are still checked, in front of the match)
        ist.encode_png(img, color="rgbx", match="lz77")
    with pytest.raises(ValueError, match="pngFilter"):
        ist.encode_png(img, row_filter="sub", match="lz77")
    assert S._png_match(None) == RUN and S._png_match("run") == RUN and S._png_match("window") == WINDOW


def test_a_batch_takes_one_match_setting_for_all_its_requests():
    img = np.zeros((4, 4, 4), np.uint8)
    assert "pngMatch" in S._BATCH_REFUSED
    for batch in (ist.stitch_png_batch, ist.stitch_batch):
        with pytest.raises(TypeError, match="pngMatch"):
            batch([([img], "vertical", {"pngMatch": "window"})])
