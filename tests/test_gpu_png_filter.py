"""The adaptive row filters of the compressing PNG export (pngFilter 'adaptive': ist_ctx_set_png_filter, IST_PNG_FILTER_ADAPTIVE) byte
for byte against their CPU statement (tests/png_filter_reference.py), in both colour forms, on every entry point that writes a PNG.
The inputs (tests/png_filter_cases.py) are judged on the CPU first (tests/test_png_filter_reference.py).  Reference anchor:
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
from tests import png_filter_cases as K
from tests import png_filter_reference as F
from tests import png_rgb_reference as G
from tests import png_stream_cases as C
from tests import test_gpu_png_rgb as TG
from tests import test_gpu_png_stream as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOX = (40, 60)
E_UNSUPPORTED = -7
COLOR = {4: "rgba", 3: "rgb"}
FORMS = [(bpp, name) for bpp in (4, 3) for name, _ in K.shape_cases(bpp)]


def check_stream(name, a, bpp, png, how=""):
    """the file's IDAT data is the reference's adaptive stream for canvas a, and PIL reads the file as the canvas; returns the IDATs"""
    from PIL import Image
    rep = K.report(name, a, bpp)
    h, w = a.shape[:2]
    idat = (T.walk if bpp == 4 else TG.walk)(png, w, h)
    bad = T.stream_difference(b"".join(idat), rep)
    assert bad is None, "%s (%s)%s: %s" % (name, COLOR[bpp], how, bad)
    im = Image.open(io.BytesIO(bytes(png)))
    assert im.mode == COLOR[bpp].upper() and np.array_equal(np.asarray(im), a[..., :bpp]), name + how
    return idat


def check_file(name, a, bpp, png, how=""):
    check_stream(name, a, bpp, png, how)
    assert bytes(png) == F.file_bytes_adaptive(a, bpp, K.report(name, a, bpp).stream), name + how      # one slab, one IDAT: the whole file


def _file(t, n):
    got = t.cpu().numpy().tobytes()
    assert len(got) == n
    return got


def _device(a, bpp, **kw):
    return _file(*ist.encode_png_device(torch.from_numpy(a).to(DEV), level=1, color=COLOR[bpp], row_filter="adaptive", **kw))


@pytest.mark.parametrize("bpp,name", FORMS)
def test_encode_png_device_writes_the_reference_file(bpp, name):
    """every form of the chunk grid and every filter type, one slab; rows of up to 1024 pixels take the pre-pass a wave per row, wider
    ones a workgroup per row"""
    K.check_regimes()
    a = dict(K.shape_cases(bpp))[name]
    check_file(name, a, bpp, _device(a, bpp))


@pytest.mark.parametrize("bpp", (4, 3))
def test_a_canvas_on_which_paeth_wins_every_row_gives_the_default_file(bpp):
    a = np.full((33, 64, 4), 255, np.uint8)
    assert _device(a, bpp) == (R.file_bytes(a) if bpp == 4 else G.file_bytes_rgb(a))


@pytest.mark.parametrize("bpp", (4, 3))
def test_encode_png_device_on_a_pitched_canvas(bpp):
    """row pitch > 4 w, and not a multiple of 16: the pre-pass's 16-byte loads are 4-byte aligned only"""
    cases = dict(K.shape_cases(bpp))
    for name in (("filter rows nunapppnuanppppppnu 257x19", "filter rows na 8191x2") if bpp == 4 else ("filter rows nunap 2730x5", "filter rows na 10923x2")):
        a = cases[name]
        h, w = a.shape[:2]
        wide = torch.full((h, w + 13, 4), 0xEE, dtype=torch.uint8, device=DEV)
        wide[:, :w] = torch.from_numpy(a).to(DEV)
        view = wide[:, :w]
        assert view.stride(0) == 4 * (w + 13)
        check_file(name, a, bpp, _file(*ist.encode_png_device(view, level=1, color=COLOR[bpp], row_filter="adaptive")), " (pitched)")


@pytest.mark.parametrize("bpp", (4, 3))
def test_host_path_on_every_shape(bpp):
    """encode_png: the slabs' streams, a table of row types per stream"""
    for name, a in K.shape_cases(bpp):
        got = ist.encode_png(a, level=1, color=COLOR[bpp], row_filter="adaptive")
        check_stream(name, a, bpp, got, " (host path)")
        assert bytes(got) == F.host_file_bytes_adaptive(a, bpp, K.report(name, a, bpp)), name


@pytest.mark.parametrize("bpp", (4, 3))
def test_host_path_with_the_slab_cut_inside_a_row(bpp):
    """775 chunks in slabs of 768 and 7: row 153 is cut between the two streams after its third piece, noise above and below it, and
    its type is Up"""
    name, a = K.slab_cut_case(bpp)
    rep = K.report(name, a, bpp)
    got = ist.encode_png(a, level=1, color=COLOR[bpp], row_filter="adaptive")
    idat = check_stream(name, a, bpp, got, " (host path)")
    assert [len(d) for d in idat] == R.idat_lengths([c.nbytes for c in rep.chunks], R.idat_limit(None), [768, 7])
    assert bytes(got) == F.host_file_bytes_adaptive(a, bpp, rep)
    img = {"width": a.shape[1], "height": a.shape[0], "data": TG.K.opaque(a)}
    big = {"maxSide": 32768, "maxPixels": 1e9}
    canvas = np.ascontiguousarray(ist.stitch([img], "vertical", big)["data"])
    assert np.array_equal(canvas[..., :3], a[..., :3])
    got = ist.stitch_png([img], "vertical", dict(big, pngColor=COLOR[bpp], pngFilter="adaptive"))
    check_stream(name + " stitched", canvas, bpp, got["png"], " (stitch_png)")


def _images():
    """three opaque images of one size (nothing is resampled) whose rows are of the same kinds, so that the stitched canvas has rows of
    several types in either direction"""
    return [{"width": 90, "height": 60, "data": TG.K.opaque(K.rows_of_kinds(60 + k, 90, "nunapppnuanp" * 5))} for k in range(3)]


@pytest.mark.parametrize("bpp", (4, 3))
def test_stitch_png_host_images_and_bitmaps_with_and_without_preview(bpp):
    imgs = _images()
    bms = [ist.upload_bitmap(im) for im in imgs]
    for direction in ("vertical", "horizontal"):
        opts = {"gap": 3, "mode": "max"}
        canvas = np.ascontiguousarray(ist.stitch(imgs, direction, opts)["data"])
        name = "filter stitch " + direction
        assert len(K.report(name, canvas, bpp).chunks) >= 2 and len(set(F.row_filters(canvas, bpp).tolist())) >= 2
        form = dict(opts, pngColor=COLOR[bpp], pngFilter="adaptive")
        for what, src in (("host images", imgs), ("bitmaps", bms)):
            got = ist.stitch_png(src, direction, form)
            assert (got["width"], got["height"]) == canvas.shape[:2][::-1]
            check_file(name, canvas, bpp, got["png"], ", " + what)
            plain = ist.stitch_png(src, direction, dict(opts, preview=BOX))
            both = ist.stitch_png(src, direction, dict(form, preview=BOX))
            check_file(name, canvas, bpp, both["png"], ", %s with a preview" % what)
            assert np.array_equal(both["preview"], plain["preview"])
            assert bytes(plain["png"]) == R.file_bytes(canvas)                          # (the default call in between is untouched)
    for b in bms:
        b.close()


def test_stitch_files_with_and_without_preview(tmp_path):
    from PIL import Image
    paths = []
    for k, (w, h) in enumerate(((120, 80), (96, 110))):
        p = tmp_path / ("in%d.png" % k)
        Image.fromarray(C.photo_like(70 + k, h, w)[..., :3]).save(p)
        paths.append(str(p))
    opts = {"gap": 2}
    plain = ist.stitch_files(paths, "vertical", dict(opts, preview=BOX))
    canvas = ist.decode_png(plain["png"])
    name = "filter files"
    got = ist.stitch_files(paths, "vertical", dict(opts, pngFilter="adaptive"), out_path=str(tmp_path / "out.png"))
    check_stream(name, canvas, 4, got["png"])
    assert open(tmp_path / "out.png", "rb").read() == bytes(got["png"]) and bytes(got["png"]) != bytes(plain["png"])
    both = ist.stitch_files(paths, "vertical", dict(opts, pngFilter="adaptive", pngColor="rgb", preview=BOX))
    check_stream(name, canvas, 3, both["png"], " with a preview")
    assert np.array_equal(both["preview"], plain["preview"])


# a 1 x 1, a whole-rows, a one-row and a pieces canvas in one launch (a workgroup per row in the pre-pass: the widest decides); and
# narrow canvases alone (a wave per row, rows of several files in one workgroup)
BATCHES = {4: (("filter photo 1x1", "filter rows nunapppnuanppppppnu 257x19", "filter rows na 4095x2", "filter rows nu 8191x2"),
               ("filter photo 1x1", "filter rows nunap 3x5", "filter rows nunapppnuanppppppnu 257x19", "filter flat 300x40")),
           3: (("filter photo 1x1", "filter rows nunap 2730x5", "filter rows nua 5461x3", "filter rows na 10923x2"),
               ("filter photo 1x1", "filter rows nunap 3x5", "filter rows nunapppnuanppppppnu 257x19", "filter flat 300x40"))}


def _batch_cases(bpp):
    return dict(K.shape_cases(4) + K.shape_cases(bpp))             # (the small canvases serve either colour form)


@pytest.mark.parametrize("bpp", (4, 3))
def test_encode_png_batch_device_with_every_grid_form_in_one_launch(bpp):
    cases = _batch_cases(bpp)
    for names in BATCHES[bpp]:
        before = L.lib.ist_debug_png_batch_launches()
        files = ist.encode_png_batch_device([torch.from_numpy(cases[n]).to(DEV) for n in names], level=1, color=COLOR[bpp], row_filter="adaptive")
        assert L.lib.ist_debug_png_batch_launches() == before + 1 and len(files) == len(names)
        for n, (t, ln) in zip(names, files):
            check_file(n, cases[n], bpp, _file(t, ln), " (batch)")


@pytest.mark.parametrize("bpp", (4, 3))
def test_stitch_png_batch_with_every_grid_form_in_one_batch(bpp):
    cases = _batch_cases(bpp)
    for names in BATCHES[bpp]:
        reqs = [([{"width": a.shape[1], "height": a.shape[0], "data": TG.K.opaque(a)}], "vertical") for a in (cases[n] for n in names)]
        canvases = ist.stitch_batch(reqs)
        got = ist.stitch_png_batch(reqs, level=1, color=COLOR[bpp], row_filter="adaptive")
        for k, n in enumerate(names):
            canvas = np.ascontiguousarray(canvases[k])
            assert canvas.shape == cases[n].shape and (got[k]["width"], got[k]["height"]) == canvas.shape[:2][::-1]
            check_file("filter batch request of " + n, canvas, bpp, got[k]["png"])
    plain = ist.stitch_png_batch(reqs, level=1)                            # the next batch without the option is the default form again
    for k in range(len(reqs)):
        assert bytes(plain[k]["png"]) == R.file_bytes(np.ascontiguousarray(canvases[k]))


def test_the_setter_accepts_its_two_values_only():
    import sys
    ctx = sys.modules["imagestitching_amd.stitch"]._ctx(0)
    assert L.lib.ist_ctx_set_png_filter(ctx, 2) == -1 and L.lib.ist_ctx_set_png_filter(ctx, -1) == -1      # IST_E_INVALID
    assert b"IST_PNG_FILTER_ADAPTIVE" in L.lib.ist_last_error()
    assert L.lib.ist_ctx_set_png_filter(ctx, 1) == L.IST_OK and L.lib.ist_ctx_set_png_filter(ctx, 0) == L.IST_OK


def _live():
    out = (ctypes.c_int64 * 4)()
    assert L.lib.ist_debug_live_handles(out) == L.IST_OK
    return tuple(out)


def test_one_context_switched_between_the_filters_and_nothing_leaks():
    """the setting is read per call: adaptive, paeth, adaptive; no device block, pinned block, stream or event stays behind a call"""
    cases = dict(K.shape_cases(4))
    name = "filter rows nunapppnuanppppppnu 257x19"
    a = cases[name]
    dense = torch.from_numpy(a).to(DEV)
    want = {"adaptive": F.file_bytes_adaptive(a, 4, K.report(name, a, 4).stream), "paeth": R.file_bytes(a)}
    assert want["adaptive"] != want["paeth"]
    live = allocs = None
    for rf in ("adaptive", "paeth", "adaptive", "paeth", "adaptive"):
        assert _file(*ist.encode_png_device(dense, level=1, row_filter=rf)) == want[rf], rf
        assert bytes(ist.encode_png(a, level=1, row_filter=rf)) == want[rf], rf + " (host path)"
        if live is None:
            live, allocs = _live(), L.lib.ist_debug_device_allocs()
    assert _live() == live and L.lib.ist_debug_device_allocs() == allocs
    assert _file(*ist.encode_png_device(dense, level=1)) == want["paeth"]  # no filter given: Paeth, whatever the call before chose


def test_stored_form_refuses_adaptive_and_the_context_recovers():
    cases = dict(K.shape_cases(4))
    name = "filter rows nunap 3x5"
    a = cases[name]
    dense = torch.from_numpy(a).to(DEV)
    img = {"width": 3, "height": 5, "data": TG.K.opaque(a)}
    calls = {"encode_png_device": lambda lv: ist.encode_png_device(dense, level=lv, row_filter="adaptive"),
             "stitch_png": lambda lv: ist.stitch_png([img], "vertical", {"pngLevel": lv, "pngFilter": "adaptive"}),
             "stitch_png with a preview": lambda lv: ist.stitch_png([img], "vertical", {"pngLevel": lv, "pngFilter": "adaptive", "preview": BOX}),
             "encode_png_batch_device": lambda lv: ist.encode_png_batch_device([dense, dense], level=lv, row_filter="adaptive"),
             "encode_png": lambda lv: ist.encode_png(a, level=lv, row_filter="adaptive"),
             "stitch_png_batch": lambda lv: ist.stitch_png_batch([([img], "vertical")], level=lv, row_filter="adaptive")}
    for who, call in calls.items():
        with pytest.raises(ist.StitchError) as e:
            call(0)
        assert e.value.code == E_UNSUPPORTED and "pngLevel 1" in str(e.value), who
    want = F.file_bytes_adaptive(a, 4, K.report(name, a, 4).stream)        # the same context, set back to level 1
    assert _file(*ist.encode_png_device(dense, level=1, row_filter="adaptive")) == want
    assert [_file(t, n) for t, n in ist.encode_png_batch_device([dense, dense], level=1, row_filter="adaptive")] == [want, want]
    assert np.array_equal(ist.decode_png(ist.encode_png(a, level=0)), a)   # and the stored form still writes its file
