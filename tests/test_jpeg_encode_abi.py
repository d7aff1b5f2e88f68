"""The CPU side of the JPEG export: the quantisation tables and the size bound of the C-ABI against the numpy reference, every
argument error without a device, the Python wrappers' own checks and the Node exports."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests import jpeg_encode_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "node", "imagestitch.node")
needs_node = pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
J444, J420 = 0, 1
INVALID, NO_CONTEXT, UNSUPPORTED = -1, -4, -7


def test_quant_tables_equal_the_reference():
    luma, chroma = (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
    for q in range(1, 101):
        assert L.lib.ist_jpeg_quant_tables(q, luma, chroma) == 0
        rl, rc = R.quant_tables(q)
        assert list(luma) == rl.tolist() and list(chroma) == rc.tolist(), q
    for q in (0, 101, -5):
        assert L.lib.ist_jpeg_quant_tables(q, luma, chroma) == INVALID
    assert L.lib.ist_jpeg_quant_tables(50, None, chroma) == INVALID


def _noise(w, h):
    a = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w, 4), dtype=np.uint8)
    return a


def _pixel_checker(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    v = (((yy + xx) & 1) * 255).astype(np.uint8)
    return np.stack([v, v, v, v], -1)


@pytest.mark.parametrize("layout,ss", (("420", J420), ("444", J444)))
def test_bound_holds_for_the_worst_contents(layout, ss):
    for w, h in ((1, 1), (7, 9), (17, 33), (48, 64), (100, 150)):
        bound = L.lib.ist_jpeg_bound(w, h, ss)
        for make in (_noise, _pixel_checker):
            n = len(R.encode(make(w, h), 100, layout))
            assert bound >= n, (w, h, layout, make.__name__, bound, n)


def test_bound_is_monotone_and_rejects_bad_arguments():
    for ss in (J444, J420):
        for w in (1, 8, 9, 16, 17, 1000, 65535):
            assert L.lib.ist_jpeg_bound(w + 1 if w < 65535 else w, 40, ss) >= L.lib.ist_jpeg_bound(w, 40, ss) > 0
            assert L.lib.ist_jpeg_bound(40, w + 1 if w < 65535 else w, ss) >= L.lib.ist_jpeg_bound(40, w, ss) > 0
        prev = 0
        for side in range(1, 70):
            b = L.lib.ist_jpeg_bound(side, side, ss)
            assert b >= prev
            prev = b
    for w, h, ss in ((0, 1, J420), (1, 0, J420), (-3, 5, J444), (65536, 1, J420), (1, 65536, J444), (8, 8, 2), (8, 8, -1)):
        assert L.lib.ist_jpeg_bound(w, h, ss) < 0, (w, h, ss)


def test_error_codes_without_a_device():
    fake = C.c_void_p(8)                                   # (never dereferenced: every argument is checked before the context is used)
    px = np.zeros((4, 4, 4), np.uint8)
    p, buf = px.ctypes.data, C.c_void_p(4096)              # (a 16-byte aligned "device" address, never dereferenced either)
    n, out, plan = C.c_int64(0), C.POINTER(C.c_uint8)(), L.Plan()
    launches = L.lib.ist_debug_jpeg_encode_launches()
    dev = lambda ctx=fake, canvas=p, pitch=16, w=4, h=4, q=90, ss=J420, o=buf, cap=1 << 20, ln=C.byref(n): \
        L.lib.ist_jpeg_encode_device(ctx, canvas, pitch, w, h, q, ss, o, cap, ln, None)
    assert dev(ctx=None) == NO_CONTEXT
    assert dev(q=0) == dev(q=101) == INVALID
    assert dev(ss=2) == dev(ss=-1) == INVALID
    assert dev(canvas=None) == dev(o=None) == dev(ln=None) == INVALID
    assert dev(w=0) == dev(h=0) == INVALID
    assert dev(pitch=12) == dev(pitch=18) == INVALID
    assert dev(cap=L.lib.ist_jpeg_bound(4, 4, J420) - 1) == INVALID and "ist_jpeg_bound" in L.last_error()
    assert dev(o=C.c_void_p(4100)) == INVALID and "aligned" in L.last_error()
    assert dev(w=65536, pitch=4 * 65536) == UNSUPPORTED and "width" in L.last_error()
    assert dev(h=65536) == UNSUPPORTED and "height" in L.last_error()

    host = lambda ctx=fake, pixels=p, pitch=16, w=4, h=4, q=90, ss=J420, o=C.byref(out), ln=C.byref(n): \
        L.lib.ist_jpeg_encode_rgba8(ctx, pixels, pitch, w, h, q, ss, o, ln)
    assert host(ctx=None) == NO_CONTEXT
    assert host(q=0) == host(ss=3) == host(pixels=None) == host(w=0) == host(pitch=8) == host(o=None) == host(ln=None) == INVALID
    assert host(h=65536) == UNSUPPORTED

    descs = (L.ImageDesc * 1)(L.ImageDesc(4, 4, 1, 0, 0, 0, 0))
    ptrs, pitches = (C.c_void_p * 1)(p), (C.c_size_t * 1)(16)
    st = lambda ctx=fake, q=90, ss=J420, pl=C.byref(plan), o=C.byref(out), ln=C.byref(n): \
        L.lib.ist_stitch_jpeg(ctx, descs, ptrs, pitches, 1, 0, 0, 0.0, None, 1, q, ss, pl, o, ln)
    assert st(ctx=None) == NO_CONTEXT
    assert st(q=0) == st(q=101) == st(ss=7) == st(pl=None) == st(o=None) == st(ln=None) == INVALID
    bms = (C.c_void_p * 1)()
    sb = lambda ctx=fake, nb=1, q=90, ss=J420, pl=C.byref(plan), o=C.byref(out), ln=C.byref(n): \
        L.lib.ist_stitch_bitmaps_jpeg(ctx, bms, nb, 0, 0, 0.0, None, 1, q, ss, pl, o, ln)
    assert sb(ctx=None) == NO_CONTEXT
    assert sb(q=0) == sb(ss=7) == sb(pl=None) == sb(o=None) == INVALID
    assert sb(nb=0) == 1                                   # IST_NOTHING_TO_DO
    assert sb() == -6                                      # a NULL bitmap: '图片0解码异常'
    assert L.lib.ist_debug_jpeg_encode_launches() == launches


def test_python_wrappers_check_their_arguments():
    px = np.zeros((4, 4, 4), np.uint8)
    for q in (0, 101, -1):
        with pytest.raises(ValueError):
            ist.encode_jpeg(px, quality=q)
        with pytest.raises(ValueError):
            ist.stitch_jpeg([px], "vertical", {"quality": q})
    for q in (90.5, "90", None, True):
        with pytest.raises(TypeError):
            ist.encode_jpeg(px, quality=q)
    for ss in ("422", "4:2:0", 2, None):
        with pytest.raises(ValueError):
            ist.encode_jpeg(px, subsampling=ss)
        with pytest.raises(ValueError):
            ist.stitch_jpeg([px], "vertical", {"subsampling": ss})
    for bad in (np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 4), np.float32), np.zeros((4, 4), np.uint8), np.zeros((0, 4, 4), np.uint8)):
        with pytest.raises(TypeError):
            ist.encode_jpeg(bad)
    with pytest.raises(TypeError, match="preview"):
        ist.stitch_jpeg([px], "vertical", {"preview": (8, 8)})
    with pytest.raises(TypeError, match="devices"):
        ist.stitch_jpeg([px], "vertical", {"devices": [0]})
    with pytest.raises(TypeError, match="unknown"):
        ist.stitch_jpeg([px], "vertical", {"qualty": 3})
    assert ist.stitch_jpeg([], "vertical") is None
    assert "quality" not in ist.DEFAULT_OPTS and "subsampling" not in ist.DEFAULT_OPTS      # the other hosts keep refusing them
    with pytest.raises(TypeError, match="unknown"):
        ist.plan([{"width": 4, "height": 4}], "vertical", {"quality": 90})


@needs_node
def test_node_exports_and_option_checks():
    code = """
const api = require('%s/node/index.js');
const out = {types: [typeof api.stitchJpeg, typeof api.encodeJpeg, typeof api.native.encodeJpeg], errors: []};
const px = new Uint8Array(64);
for (const o of [{quality: 0}, {quality: 101}, {quality: 1.5}, {subsampling: '422'}])
  try { api.encodeJpeg(px, 4, 4, o); out.errors.push('accepted'); } catch (e) { out.errors.push(e.constructor.name); }
const img = [{width: 4, height: 4, data: px}];
Promise.all([{preview: {width: 8, height: 8}}, {devices: [0]}, {quality: 0}, {subsampling: 'x'}, {nonsense: 1}].map(
  (o) => api.stitchJpeg(img, 'vertical', o).then(() => 'accepted', (e) => e.constructor.name + ':' + e.message)))
  .then((r) => { out.rejected = r; return api.stitchJpeg([], 'vertical', {quality: 80}); })
  .then((r) => { out.empty = r; console.log(JSON.stringify(out)); });
""" % ROOT
    r = subprocess.run([NODE, "-e", code], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    import json
    out = json.loads(r.stdout)
    assert out["types"] == ["function"] * 3
    assert out["errors"] == ["RangeError", "RangeError", "RangeError", "TypeError"]
    assert [x.split(":")[0] for x in out["rejected"]] == ["TypeError", "TypeError", "RangeError", "TypeError", "TypeError"]
    assert "preview" in out["rejected"][0] and "devices" in out["rejected"][1] and "unknown" in out["rejected"][4]
    assert out["empty"] is None
    dts = open(os.path.join(ROOT, "node", "index.d.ts")).read()
    assert "export function stitchJpeg(" in dts and "export function encodeJpeg(" in dts


@needs_node
def test_canvas_shim_names_a_jpeg_export_without_a_gpu():
    """recordOnly (no device): fileType 'jpg' still only names a path, as before; the file is made where a GPU renders the canvas"""
    code = """
const shim = require('%s/node/canvas_shim.js');
const env = shim.makeEnvironment({recordOnly: true});
const c = env.wx.createOffscreenCanvas({type: '2d', width: 8, height: 8});
c.getContext('2d').fillRect(0, 0, 8, 8);
const r = env.exportCanvas(c, {fileType: 'jpg', quality: 0.8});
console.log(JSON.stringify({path: r.tempFilePath, keys: Object.keys(env.exports[r.tempFilePath]).sort()}));
""" % ROOT
    r = subprocess.run([NODE, "-e", code], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    import json
    out = json.loads(r.stdout)
    assert out["path"].endswith(".jpg") and out["keys"] == ["data", "height", "width"]
