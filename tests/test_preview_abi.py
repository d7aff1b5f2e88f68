"""Previews at the C-ABI and in the Python host, CPU only: the fit rule (pages/index/index.js:1600-1602) against a restatement of the
reference's three lines for every canvas the captured traces export, the struct layout, the argument errors that need no device,
and the calls that refuse the 'preview' option."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import imagestitching_amd as ist
from imagestitching_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = (343.0, 457.0)            # the preview node of the reference page


def _js_round(x):
    return math.floor(x + 0.5)  # Math.round


def _fit_js(export_w, export_h, box_w, box_h):
    """index.js:1600-1602, line by line (Python floats are IEEE doubles, like JavaScript numbers)"""
    scale_fit = min(box_w / export_w, box_h / export_h)
    pv_w = _js_round(export_w * scale_fit)
    pv_h = _js_round(export_h * scale_fit)
    return pv_w, pv_h


def _fit(w, h, box_w, box_h):
    pw, ph = C.c_int32(-7), C.c_int32(-7)
    rc = L.lib.ist_preview_fit(w, h, box_w, box_h, C.byref(pw), C.byref(ph))
    return rc, pw.value, ph.value


def _exported_sizes():
    with open(os.path.join(ROOT, "tests", "golden", "plan_goldens.json")) as f:
        cases = json.load(f)["cases"]
    sizes = []
    for c in cases:
        for call in c["calls"] or []:
            if call["op"] == "export":
                sizes.append((int(call["a"][4]), int(call["a"][5])))
    return sizes


def test_fit_is_the_reference_rule_on_every_exported_canvas():
    sizes = _exported_sizes()
    assert len(sizes) >= 40
    for w, h in sizes:
        want = _fit_js(w, h, *BOX)
        assert _fit(w, h, *BOX) == (0, max(1, want[0]), max(1, want[1])), (w, h)
        assert ist.preview_fit(w, h, *BOX) == (max(1, want[0]), max(1, want[1]))
        assert _fit(h, w, 457.0, 343.0)[1:] == tuple(reversed(_fit(w, h, *BOX)[1:]))     # the rule does not know its axes


@pytest.mark.parametrize("w,h,pw,ph", [(4032, 27216, 68, 457), (36288, 3024, 343, 29), (8000, 384000, 10, 457), (1664, 3744, 203, 457),
                                         (100, 120, 343, 412), (40, 200000, 1, 457)])
def test_fit_known_values(w, h, pw, ph):
    assert _fit(w, h, *BOX) == (0, pw, ph)
    js = _fit_js(w, h, *BOX)
    assert (max(1, js[0]), max(1, js[1])) == (pw, ph)


def test_fit_never_returns_an_empty_side():
    """the one stated deviation: for a strip thin enough the reference computes 0 and draws nothing"""
    assert _fit_js(40, 200000, *BOX)[0] == 0
    assert _fit(40, 200000, *BOX) == (0, 1, 457)
    assert _fit(10 ** 6, 3, *BOX) == (0, 343, 1)
    assert _fit(1, 1, *BOX) == (0, 343, 343)               # like the reference, the rule enlarges


def test_fit_argument_errors():
    for bw, bh in [(0.0, 457.0), (343.0, 0.0), (-1.0, 457.0), (float("nan"), 457.0), (343.0, float("inf")), (float("-inf"), 1.0)]:
        assert _fit(100, 100, bw, bh) == (-1, 0, 0), (bw, bh)
        assert "box" in L.last_error()
    assert _fit(0, 10, *BOX)[0] == -1 and _fit(10, 0, *BOX)[0] == -1 and _fit(-4, 10, *BOX)[0] == -1
    assert L.lib.ist_preview_fit(10, 10, 343.0, 457.0, None, None) == -1
    with pytest.raises(ist.StitchError) as e:
        ist.preview_fit(10, 10, 0, 5)
    assert e.value.code == -1


def test_preview_struct_layout_matches_the_header(tmp_path):
    assert C.sizeof(L.Preview) == 32
    assert [getattr(L.Preview, f).offset for f, _ in L.Preview._fields_] == [0, 8, 16, 20, 24]
    c = tmp_path / "t.c"
    c.write_text('#include <stddef.h>\n#include "imagestitch.h"\n'
                 "int main(void){ return sizeof(ist_preview) == 32 && offsetof(ist_preview, box_w) == 0 && offsetof(ist_preview, box_h) == 8 &&\n"
                 "  offsetof(ist_preview, width) == 16 && offsetof(ist_preview, height) == 20 && offsetof(ist_preview, pixels) == 24 &&\n"
                 "  IST_ABI_VERSION == 2 ? 0 : 1; }\n")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


def _png_call_args():
    plan, out, n = L.Plan(), C.POINTER(C.c_uint8)(), C.c_int64(0)
    return plan, out, n


def test_every_preview_entry_point_needs_a_context():
    """The entry points check the context first, like every other one of the header, and no context can be made without a device: so
    of the argument errors only those of ist_preview_fit (above) and the NULL-context codes are reachable here.  Short pitches, pw / ph
    < 1 and bad boxes on a live context are in tests/test_gpu_preview.py::test_argument_errors_on_the_device; a bitmap of another
    device than the context's needs two GPUs and is tested nowhere."""
    pv = L.Preview(343.0, 457.0, 5, 5, None)
    descs = (L.ImageDesc * 1)(L.ImageDesc(4, 4, 1, 0, 0, 0, 0))
    plan, out, n = _png_call_args()
    assert L.lib.ist_preview_device(None, None, 0, 4, 4, 0, None, 0, 1, 1, None) == -4
    assert "绘图上下文" in L.last_error()
    assert L.lib.ist_bitmap_preview(None, None, 1, 1, None, 0) == -4
    assert L.lib.ist_stitch_png_preview(None, descs, None, None, 1, 0, 0, 0.0, None, 1, C.byref(plan), C.byref(out), C.byref(n), C.byref(pv)) == -4
    assert L.lib.ist_stitch_bitmaps_png_preview(None, None, 1, 0, 0, 0.0, None, 1, C.byref(plan), C.byref(out), C.byref(n), C.byref(pv)) == -4
    assert L.lib.ist_stitch_files_png_preview(None, None, None, 1, 0, 0, 0.0, None, 1, C.byref(plan), C.byref(out), C.byref(n), C.byref(pv)) == -4
    assert L.lib.ist_stitch_paths_png_preview(None, None, 1, 0, 0, 0.0, None, 1, C.byref(plan), C.byref(out), C.byref(n), C.byref(pv)) == -4
    assert not out and n.value == 0
    # whatever fails, and however early: nothing is returned through the struct
    for call in (lambda pv: L.lib.ist_stitch_png_preview(None, descs, None, None, 1, 0, 0, 0.0, None, 1, C.byref(plan), C.byref(out), C.byref(n), C.byref(pv)),
                 lambda pv: L.lib.ist_stitch_bitmaps_png_preview(None, None, 1, 0, 0, 0.0, None, 1, C.byref(plan), C.byref(out), C.byref(n), C.byref(pv)),
                 lambda pv: L.lib.ist_stitch_files_png_preview(None, None, None, 1, 0, 0, 0.0, None, 1, C.byref(plan), C.byref(out), C.byref(n), C.byref(pv)),
                 lambda pv: L.lib.ist_stitch_paths_png_preview(None, None, 1, 0, 0, 0.0, None, 1, C.byref(plan), C.byref(out), C.byref(n), C.byref(pv))):
        stale = L.Preview(343.0, 457.0, 5, 6, C.cast(1, C.POINTER(C.c_uint8)))
        assert call(stale) == -4 and not stale.pixels and (stale.width, stale.height) == (0, 0)
    assert L.lib.ist_debug_preview_launches() == 0 or L.lib.ist_device_count() > 0


def test_no_device_means_no_context_and_no_fallback():
    if L.lib.ist_device_count() > 0:
        return                                             # (with a GPU the call succeeds: tests/test_gpu_preview.py)
    a = np.zeros((8, 8, 4), np.uint8)
    with pytest.raises(ist.StitchError) as e:
        ist.stitch_png([a], "vertical", {"preview": BOX})
    assert e.value.code == -5                              # IST_E_NO_DEVICE, from ist_ctx_create
    assert L.lib.ist_debug_preview_launches() == 0


def test_the_option_is_refused_where_no_canvas_stays_behind_an_export():
    a = np.zeros((8, 8, 4), np.uint8)
    with pytest.raises(TypeError, match="caller gets the pixels"):
        ist.stitch([a], "vertical", {"preview": BOX})
    with pytest.raises(TypeError, match="do not apply to a batch"):
        ist.stitch_batch([([a], "vertical", {"preview": BOX})])
    with pytest.raises(TypeError, match="do not apply to a batch"):
        ist.stitch_png_batch([([a], "vertical", {"preview": BOX})])
    with pytest.raises(TypeError, match="devices="):
        ist.stitch_png([a], "vertical", {"preview": BOX, "devices": [0, 1]})
    with pytest.raises(TypeError, match="devices="):
        ist.stitch_files(["/nonexistent.jpg"], "vertical", {"preview": BOX, "devices": [0]})
    with pytest.raises(TypeError, match="box_w, box_h"):
        ist.stitch_png([a], "vertical", {"preview": 343})
    assert ist.DEFAULT_OPTS["preview"] is None               # off unless asked for
