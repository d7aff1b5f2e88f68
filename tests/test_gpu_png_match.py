"""The window matches of the compressing PNG export (pngMatch 'window': ist_ctx_set_png_match, IST_PNG_MATCH_WINDOW) byte for byte
against their CPU statement (tests/png_match_reference.py), in both colour forms and with either row filter, on every entry point that
writes a PNG.  The inputs (tests/png_match_cases.py) are judged on the CPU first (tests/test_png_match_reference.py).  Reference anchor:
wx.canvasToTempFilePath({fileType: 'png'}) (utils/canvas.js:205-242, pages/index/index.js:1577-1579) - a file that decodes to the same
pixels."""
import ctypes
import io

import numpy as np
import pytest
import torch

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests import png_deflate_reference as R
from tests import png_filter_reference as F
from tests import png_match_cases as K
from tests import png_match_reference as M
from tests import png_rgb_reference as G
from tests import test_gpu_png_rgb as TG
from tests import test_gpu_png_stream as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOX = (40, 60)
E_UNSUPPORTED = -7
COLOR = {4: "rgba", 3: "rgb"}
FILTER = {False: "paeth", True: "adaptive"}
NAMES = [n for n, _ in K.shape_cases()]


def _bpp(a):
    return 3 if a.shape[1] == K.RGB_SHAPE[0] else 4


def check_stream(name, a, png, bpp=4, adaptive=False, how=""):
    """the file's IDAT data is the reference's window stream for canvas a, and PIL reads the file as the canvas; returns the IDATs"""
    from PIL import Image
    rep = K.report(name, a, bpp, adaptive)
    h, w = a.shape[:2]
    idat = (T.walk if bpp == 4 else TG.walk)(png, w, h)
    bad = T.stream_difference(b"".join(idat), rep)
    assert bad is None, "%s (%s, %s)%s: %s" % (name, COLOR[bpp], FILTER[adaptive], how, bad)
    im = Image.open(io.BytesIO(bytes(png)))
    assert im.mode == COLOR[bpp].upper() and np.array_equal(np.asarray(im), a[..., :bpp]), name + how
    return idat


def check_file(name, a, png, bpp=4, adaptive=False, how=""):
    check_stream(name, a, png, bpp, adaptive, how)
    assert bytes(png) == M.file_bytes_window(a, bpp, K.report(name, a, bpp, adaptive).stream, adaptive), name + how      # one slab, one IDAT: the whole file


def _file(t, n):
    got = t.cpu().numpy().tobytes()
    assert len(got) == n
    return got


def _device(a, bpp=4, adaptive=False, match="window", **kw):
    return _file(*ist.encode_png_device(torch.from_numpy(a).to(DEV), level=1, color=COLOR[bpp], row_filter=FILTER[adaptive], match=match, **kw))


def _run_file(a, bpp=4, adaptive=False):
    """the default setting's file from the references that existed before"""
    if adaptive:
        return F.file_bytes_adaptive(a, bpp)
    return R.file_bytes(a) if bpp == 4 else G.file_bytes_rgb(a)


@pytest.mark.parametrize("name", NAMES)
def test_encode_png_device_writes_the_reference_file(name):
    """every shape and content: no key below 4 bytes, one ragged span, two chunks, a short last chunk, pieces of a row, the RGB grid"""
    a = K.by_name()[name]
    check_file(name, a, _device(a, _bpp(a)), _bpp(a))


@pytest.mark.parametrize("name", ("match text 64x70", "match text|noise 64x70", "match text 720x12", "match text over photo 720x12"))
def test_window_with_rgb_and_adaptive_filters_together(name):
    a = K.by_name()[name]
    check_file(name, a, _device(a, 3, True), 3, True)


@pytest.mark.parametrize("bpp,adaptive", ((3, False), (4, True)))
def test_window_with_rgb_or_adaptive_filters_alone(bpp, adaptive):
    for name in ("match text 1x1", "match text 3x1", "match text 15x1", "match text 16x5", "match text 64x70", "match flat 720x12", "match text|noise 4200x3",
                 "match one distance 1024x1"):
        a = K.by_name()[name]
        check_file(name, a, _device(a, bpp, adaptive), bpp, adaptive)


def test_encode_png_device_on_a_pitched_canvas():
    name = "match text|noise 4200x3"
    a = K.by_name()[name]
    h, w = a.shape[:2]
    wide = torch.full((h, w + 13, 4), 0xEE, dtype=torch.uint8, device=DEV)
    wide[:, :w] = torch.from_numpy(a).to(DEV)
    check_file(name, a, _file(*ist.encode_png_device(wide[:, :w], level=1, match="window")), how=" (pitched)")


def test_host_path_on_every_case():
    """encode_png: the slabs' streams"""
    for name, a in K.shape_cases():
        bpp = _bpp(a)
        got = ist.encode_png(a, level=1, color=COLOR[bpp], match="window")
        check_stream(name, a, got, bpp, how=" (host path)")
        assert bytes(got) == M.host_file_bytes_window(a, bpp, K.report(name, a, bpp)), name


def _images():
    return [{"width": 90, "height": 60, "data": K.text_like(4900 + k, 60, 90)} for k in range(3)]


def test_stitch_png_host_images_and_bitmaps_with_and_without_preview():
    imgs = _images()
    bms = [ist.upload_bitmap(im) for im in imgs]
    for direction in ("vertical", "horizontal"):
        opts = {"gap": 3, "mode": "max"}
        canvas = np.ascontiguousarray(ist.stitch(imgs, direction, opts)["data"])
        name = "match stitch " + direction
        assert "form window" in K.regimes(K.report(name, canvas)) and len(K.report(name, canvas).chunks) >= 2
        form = dict(opts, pngMatch="window")
        for what, src in (("host images", imgs), ("bitmaps", bms)):
            got = ist.stitch_png(src, direction, form)
            assert (got["width"], got["height"]) == canvas.shape[:2][::-1]
            check_file(name, canvas, got["png"], how=", " + what)
            plain = ist.stitch_png(src, direction, dict(opts, preview=BOX))
            both = ist.stitch_png(src, direction, dict(form, preview=BOX))
            check_file(name, canvas, both["png"], how=", %s with a preview" % what)
            assert np.array_equal(both["preview"], plain["preview"])
            assert bytes(plain["png"]) == R.file_bytes(canvas)                          # (the default call in between is untouched)
    for b in bms:
        b.close()


def test_stitch_files_with_and_without_preview(tmp_path):
    from PIL import Image
    paths = []
    for k, (w, h) in enumerate(((120, 80), (96, 110))):
        p = tmp_path / ("in%d.png" % k)
        Image.fromarray(K.text_like(5000 + k, h, w)[..., :3]).save(p)
        paths.append(str(p))
    opts = {"gap": 2}
    plain = ist.stitch_files(paths, "vertical", dict(opts, preview=BOX))
    canvas = ist.decode_png(plain["png"])
    name = "match files"
    assert "form window" in K.regimes(K.report(name, canvas))
    got = ist.stitch_files(paths, "vertical", dict(opts, pngMatch="window"), out_path=str(tmp_path / "out.png"))
    check_stream(name, canvas, got["png"])
    assert open(tmp_path / "out.png", "rb").read() == bytes(got["png"]) and len(got["png"]) < len(plain["png"])
    both = ist.stitch_files(paths, "vertical", dict(opts, pngMatch="window", pngColor="rgb", pngFilter="adaptive", preview=BOX))
    check_stream(name, canvas, both["png"], 3, True, " with a preview")
    assert np.array_equal(both["preview"], plain["preview"])


@pytest.mark.parametrize("bpp,adaptive", ((4, False), (3, True)))
def test_encode_png_batch_device_mixes_window_and_run_canvases_in_one_launch(bpp, adaptive):
    cases = K.by_name()
    forms = set()
    before = L.lib.ist_debug_png_batch_launches()
    files = ist.encode_png_batch_device([torch.from_numpy(cases[n]).to(DEV) for n in K.BATCH], level=1, color=COLOR[bpp], row_filter=FILTER[adaptive], match="window")
    assert L.lib.ist_debug_png_batch_launches() == before + 1 and len(files) == len(K.BATCH)
    for n, (t, ln) in zip(K.BATCH, files):
        check_file(n, cases[n], _file(t, ln), bpp, adaptive, " (batch)")
        forms |= {c.form for c in K.report(n, cases[n], bpp, adaptive).chunks}
    assert forms == {"window", "huff", "stored"}


def test_stitch_png_batch_mixes_window_and_run_canvases_in_one_batch():
    cases = K.by_name()
    reqs = [([{"width": a.shape[1], "height": a.shape[0], "data": TG.K.opaque(a)}], "vertical") for a in (cases[n] for n in K.BATCH)]
    canvases = ist.stitch_batch(reqs)
    got = ist.stitch_png_batch(reqs, level=1, match="window")
    forms = set()
    for k, n in enumerate(K.BATCH):
        canvas = np.ascontiguousarray(canvases[k])
        assert canvas.shape == cases[n].shape and (got[k]["width"], got[k]["height"]) == canvas.shape[:2][::-1]
        check_file("match batch request of " + n, canvas, got[k]["png"])
        forms |= {c.form for c in K.report("match batch request of " + n, canvas).chunks}
    assert {"window", "huff"} <= forms
    plain = ist.stitch_png_batch(reqs, level=1)                            # the next batch without the option is the default form again
    for k in range(len(reqs)):
        assert bytes(plain[k]["png"]) == R.file_bytes(np.ascontiguousarray(canvases[k]))


def test_the_setter_accepts_its_two_values_only():
    import sys
    ctx = sys.modules["imagestitching_amd.stitch"]._ctx(0)
    assert L.lib.ist_ctx_set_png_match(ctx, 2) == -1 and L.lib.ist_ctx_set_png_match(ctx, -1) == -1      # IST_E_INVALID
    assert b"IST_PNG_MATCH_WINDOW" in L.lib.ist_last_error()
    assert L.lib.ist_ctx_set_png_match(ctx, 1) == L.IST_OK and L.lib.ist_ctx_set_png_match(ctx, 0) == L.IST_OK


def _live():
    out = (ctypes.c_int64 * 4)()
    assert L.lib.ist_debug_live_handles(out) == L.IST_OK
    return tuple(out)


def test_the_default_setting_writes_the_files_it_wrote_on_every_entry_point():
    """'run', given or not: one file per entry point against the references that existed before - selection did not leak"""
    name = "match text over photo 720x12"
    a = K.by_name()[name]
    dense = torch.from_numpy(a).to(DEV)
    want = R.file_bytes(a)
    assert want != M.file_bytes_window(a, 4, K.report(name, a).stream)
    assert _device(a, match="run") == want and _file(*ist.encode_png_device(dense, level=1)) == want
    assert _device(a, 3, True, match="run") == _run_file(a, 3, True)
    assert bytes(ist.encode_png(a, level=1, match="run")) == want == bytes(ist.encode_png(a, level=1))
    assert [_file(t, n) for t, n in ist.encode_png_batch_device([dense, dense], level=1, match="run")] == [want, want]
    img = {"width": a.shape[1], "height": a.shape[0], "data": a}
    canvas = np.ascontiguousarray(ist.stitch([img], "vertical")["data"])
    for opts in ({"pngMatch": "run"}, {}, {"pngMatch": "run", "preview": BOX}):
        assert bytes(ist.stitch_png([img], "vertical", opts)["png"]) == R.file_bytes(canvas), opts
    assert bytes(ist.stitch_png_batch([([img], "vertical")], level=1, match="run")[0]["png"]) == R.file_bytes(canvas)


def test_one_context_switched_between_the_settings_and_nothing_leaks():
    """the setting is read per call: window, run, window; no device block, pinned block, stream or event stays behind a call"""
    name = "match text 64x70"
    a = K.by_name()[name]
    dense = torch.from_numpy(a).to(DEV)
    want = {"window": M.file_bytes_window(a, 4, K.report(name, a).stream), "run": R.file_bytes(a)}
    assert len(want["window"]) < len(want["run"])
    live = allocs = None
    for m in ("window", "run", "window", "run", "window"):
        assert _file(*ist.encode_png_device(dense, level=1, match=m)) == want[m], m
        assert bytes(ist.encode_png(a, level=1, match=m)) == want[m], m + " (host path)"
        if live is None:
            live, allocs = _live(), L.lib.ist_debug_device_allocs()
    assert _live() == live and L.lib.ist_debug_device_allocs() == allocs
    assert _file(*ist.encode_png_device(dense, level=1)) == want["run"]    # no match given: runs, whatever the call before chose


def test_stored_form_refuses_window_and_the_context_recovers(tmp_path):
    from PIL import Image
    name = "match text 16x5"
    a = K.by_name()[name]
    dense = torch.from_numpy(a).to(DEV)
    img = {"width": 16, "height": 5, "data": a}
    path = str(tmp_path / "in.png")
    Image.fromarray(a[..., :3]).save(path)
    bm = ist.upload_bitmap(img)
    calls = {"encode_png_device": lambda lv: ist.encode_png_device(dense, level=lv, match="window"),
             "stitch_png": lambda lv: ist.stitch_png([img], "vertical", {"pngLevel": lv, "pngMatch": "window"}),
             "stitch_png with a preview": lambda lv: ist.stitch_png([img], "vertical", {"pngLevel": lv, "pngMatch": "window", "preview": BOX}),
             "stitch_png on bitmaps": lambda lv: ist.stitch_png([bm], "vertical", {"pngLevel": lv, "pngMatch": "window"}),
             "stitch_files": lambda lv: ist.stitch_files([path], "vertical", {"pngLevel": lv, "pngMatch": "window"}),
             "stitch_files with a preview": lambda lv: ist.stitch_files([path], "vertical", {"pngLevel": lv, "pngMatch": "window", "preview": BOX}),
             "encode_png_batch_device": lambda lv: ist.encode_png_batch_device([dense, dense], level=lv, match="window"),
             "encode_png": lambda lv: ist.encode_png(a, level=lv, match="window"),
             "stitch_png_batch": lambda lv: ist.stitch_png_batch([([img], "vertical")], level=lv, match="window")}
    ist.encode_png(a, level=1)                                            # (the context exists before the handles are counted)
    live = _live()
    for who, call in calls.items():
        with pytest.raises(ist.StitchError) as e:
            call(0)
        assert e.value.code == E_UNSUPPORTED and "pngLevel 1" in str(e.value), who
        assert _live() == live, who                                       # nothing was enqueued, nothing stays behind
    bm.close()
    want = M.file_bytes_window(a, 4, K.report(name, a).stream)             # the same context, set back to level 1
    assert _file(*ist.encode_png_device(dense, level=1, match="window")) == want
    assert [_file(t, n) for t, n in ist.encode_png_batch_device([dense, dense], level=1, match="window")] == [want, want]
    assert np.array_equal(ist.decode_png(ist.encode_png(a, level=0)), a)   # and the stored form still writes its file
