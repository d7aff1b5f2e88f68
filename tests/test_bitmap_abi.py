"""Resident bitmaps (ist_bitmap_*, include/imagestitch.h) without a GPU: every entry point answers with its documented code, and the
Python and Node hosts refuse what they must refuse before any device work.  CPU only."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import imagestitching_amd as ist
from imagestitching_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "node", "imagestitch.node")
needs_node = pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")


def test_bitmap_entry_points_refuse_null_arguments():
    lib = L.lib
    desc = L.ImageDesc(4, 4, 1, 0, 0, 0, 0)
    px = np.zeros((4, 4, 4), np.uint8)
    assert lib.ist_bitmap_upload(None, C.byref(desc), px.ctypes.data, 16) is None
    assert "无法获取绘图上下文" in L.last_error()
    out = (C.c_void_p * 1)()
    files = (C.c_char_p * 1)(b"\xff\xd8")
    lens = (C.c_int64 * 1)(2)
    assert lib.ist_bitmaps_decode(None, files, lens, 1, out) == -4
    assert lib.ist_bitmap_desc(None, C.byref(desc)) == -1
    assert lib.ist_bitmap_download(None, px.ctypes.data, 16, 4) == -1
    lib.ist_bitmap_retain(None)                    # no-ops
    lib.ist_bitmap_release(None)
    plan, pixels, ln = L.Plan(), C.POINTER(C.c_uint8)(), C.c_int64(0)
    bms = (C.c_void_p * 1)()
    assert lib.ist_stitch_bitmaps_rgba8(None, bms, 1, 0, 0, 0.0, None, 1, C.byref(plan), C.byref(pixels)) == -4
    assert lib.ist_stitch_bitmaps_png(None, bms, 1, 0, 0, 0.0, None, 1, C.byref(plan), C.byref(pixels), C.byref(ln)) == -4
    assert lib.ist_debug_bitmap_bytes() == 0


def test_bitmap_entry_points_without_a_device():
    """no context can be made without a device (IST_E_NO_DEVICE), so every call that needs one stops at the context"""
    _no_gpu()
    lib = L.lib
    assert lib.ist_ctx_create(0) is None and "no HIP device" in L.last_error()
    with pytest.raises(ist.StitchError) as e:
        ist.upload_bitmap(np.zeros((4, 4, 4), np.uint8))
    assert e.value.code == -5
    with pytest.raises(ist.StitchError) as e:
        ist.decode_bitmaps([b"\xff\xd8\xff\xd9"])
    assert e.value.code == -5
    assert lib.ist_debug_bitmap_bytes() == 0


def test_nothing_to_do_and_too_many_bitmaps_are_answered_before_the_context_is_used():
    """n == 0 and n > 128 need no device: a context pointer that is never dereferenced stands in for one"""
    lib = L.lib
    fake = C.c_void_p(8)                           # (never dereferenced on these paths)
    plan, pixels, ln = L.Plan(), C.POINTER(C.c_uint8)(), C.c_int64(0)
    bms = (C.c_void_p * 129)()
    assert lib.ist_stitch_bitmaps_rgba8(fake, bms, 0, 0, 0, 0.0, None, 1, C.byref(plan), C.byref(pixels)) == 1
    assert lib.ist_stitch_bitmaps_png(fake, bms, 0, 0, 0, 0.0, None, 1, C.byref(plan), C.byref(pixels), C.byref(ln)) == 1
    assert not pixels and plan.canvas_w == 0
    assert lib.ist_bitmaps_decode(fake, None, None, 0, None) == 1
    assert lib.ist_stitch_bitmaps_rgba8(fake, None, 2, 0, 0, 0.0, None, 1, C.byref(plan), C.byref(pixels)) == -1
    assert lib.ist_stitch_bitmaps_rgba8(fake, bms, 2, 0, 0, 0.0, None, 1, None, C.byref(pixels)) == -1
    assert lib.ist_stitch_bitmaps_png(fake, bms, 2, 0, 0, 0.0, None, 1, C.byref(plan), C.byref(pixels), None) == -1
    assert lib.ist_stitch_bitmaps_rgba8(fake, bms, 129, 0, 0, 0.0, None, 1, C.byref(plan), C.byref(pixels)) == -7
    files = (C.c_char_p * 129)()
    lens = (C.c_int64 * 129)()
    out = (C.c_void_p * 129)()
    assert lib.ist_bitmaps_decode(fake, files, lens, 129, out) == -7
    assert lib.ist_bitmaps_decode(fake, None, lens, 1, out) == -1
    # a NULL entry is the reference's missing bitmap, '图片N解码异常'
    assert lib.ist_stitch_bitmaps_rgba8(fake, bms, 3, 0, 0, 0.0, None, 1, C.byref(plan), C.byref(pixels)) == -6
    assert L.last_error() == "图片0解码异常"


def test_python_host_keeps_a_request_all_bitmaps_or_all_host_images():
    fake = ist.Bitmap.__new__(ist.Bitmap)          # (no device here: a Bitmap that was never made stands in for one)
    fake._h, fake.device, fake._desc = None, 0, L.ImageDesc(4, 4, 1, 0, 0, 1, 0)
    host = {"width": 4, "height": 4, "data": np.zeros((4, 4, 4), np.uint8)}
    with pytest.raises(TypeError):
        ist.stitch([fake, host], "vertical")
    with pytest.raises(TypeError):
        ist.stitch_png([host, fake], "vertical")
    with pytest.raises(TypeError):
        ist.plan([fake, host], "vertical")
    with pytest.raises(TypeError):
        ist.stitch([fake], "vertical", {"devices": [0]})
    with pytest.raises(TypeError):
        ist.stitch_batch([([fake], "vertical")])
    # the planner reads a bitmap's desc
    p = ist.plan([fake, fake], "vertical")
    assert (p.canvas_w, p.canvas_h) == (4, 8)
    with pytest.raises(ValueError):                # a closed bitmap is not used
        ist.stitch([fake], "vertical")


NODE_CPU_JS = r"""
const api = require(process.argv[1]);
const out = {};
const fake = Object.create(api.Bitmap.prototype);
const host = { width: 2, height: 2, data: new Uint8Array(16) };
const err = (f) => { try { f(); return null; } catch (e) { return [e.constructor.name, e.code === undefined ? null : e.code]; } };
out.mixedSync = err(() => api.stitchSync([fake, host], 'vertical'));
out.devicesSync = err(() => api.stitchSync([fake], 'vertical', { devices: [0] }));
out.planMixed = err(() => api.plan([host, fake], 'vertical'));
out.batch = err(() => api.stitchBatchSync([{ images: [fake], direction: 'vertical' }]));
out.pngBatch = err(() => api.stitchPngBatchSync([{ images: [fake], direction: 'vertical' }]));
out.construct = err(() => new api.Bitmap());
out.upload = err(() => api.uploadBitmap(host));
out.bytes = api.debugBitmapBytes();
(async () => {
  const rej = async (p) => { try { await p; return null; } catch (e) { return [e.constructor.name, e.code === undefined ? null : e.code, String(e.message)]; } };
  out.mixed = await rej(api.stitch([host, fake], 'vertical'));
  out.devices = await rej(api.stitchPng([fake], 'vertical', { devices: [0, 1] }));
  out.batchAsync = await rej(api.stitchBatch([{ images: [fake], direction: 'vertical' }]));
  out.decode = await rej(api.decodeBitmaps([Buffer.from([0xff, 0xd8, 0xff, 0xd9])]));
  out.decodeNone = await api.decodeBitmaps([]);
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(String(e && e.stack || e)); process.exit(3); });
"""


@needs_node
def test_node_host_refuses_mixed_requests_and_devices_and_rejects_without_a_gpu():
    import torch
    r = subprocess.run([NODE, "-e", NODE_CPU_JS, os.path.join(ROOT, "node", "index.js")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("mixedSync", "devicesSync", "planMixed", "batch", "pngBatch", "construct"):
        assert out[k] is not None and out[k][0] == "TypeError", (k, out[k])
    for k in ("mixed", "devices", "batchAsync"):
        assert out[k] is not None and out[k][0] == "TypeError", (k, out[k])
    assert out["decodeNone"] == []
    if not torch.cuda.is_available():
        assert out["upload"] == ["Error", "-5"]
        assert out["decode"][:2] == ["Error", "-5"] and out["decode"][2].startswith("拼图失败：")
        assert out["bytes"] == 0
