"""The RGB form of the compressing PNG export (pngColor 'rgb': ist_ctx_set_png_color, IST_PNG_RGB) byte for byte against its CPU
statement (tests/png_rgb_reference.py), on every entry point that writes a PNG.  The inputs (tests/png_rgb_cases.py) are judged on the
CPU first (tests/test_png_rgb_reference.py).  Reference anchor: wx.canvasToTempFilePath({fileType: 'png'}) (utils/canvas.js:205-242,
pages/index/index.js:1577-1579) on a canvas the plan's white fillRect has made opaque - a file that decodes to the same colours."""
import io
import struct
import zlib

import numpy as np
import pytest
import torch

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests import png_deflate_reference as R
from tests import png_rgb_cases as K
from tests import png_rgb_reference as G
from tests import png_stream_cases as C
from tests import test_gpu_png_stream as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOX = (40, 60)
E_UNSUPPORTED = -7


def walk(png, w, h):
    """every chunk's CRC, the fixed head (signature, IHDR with colour type 2, the tEXt chunk) and the chunk order; returns the data of
    each IDAT chunk"""
    png = bytes(png)
    head = G.file_head_rgb(w, h)
    assert len(head) == 56 and png[:56] == head, "signature / IHDR / tEXt: %r" % png[:56]
    at, kinds, idat = 8, [], []
    while at < len(png):
        n, kind = struct.unpack(">I4s", png[at:at + 8])
        data = png[at + 8:at + 8 + n]
        assert len(data) == n and struct.unpack(">I", png[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + data) & 0xFFFFFFFF, (kind, at)
        kinds.append(kind)
        if kind == b"IDAT":
            idat.append(data)
        at += 12 + n
    assert at == len(png) and kinds == [b"IHDR", b"tEXt"] + [b"IDAT"] * len(idat) + [b"IEND"] and idat, kinds
    assert png.index(b"IDAT") + 4 == 64
    return idat


def check_stream(name, a, png, how=""):
    """the file's IDAT data is the reference's stream for canvas a, and PIL reads the file as the canvas's colours"""
    from PIL import Image
    rep = K.report(name, a)
    h, w = a.shape[:2]
    idat = walk(png, w, h)
    bad = T.stream_difference(b"".join(idat), rep)
    assert bad is None, "%s%s: %s" % (name, how, bad)
    im = Image.open(io.BytesIO(bytes(png)))
    assert im.mode == "RGB" and np.array_equal(np.asarray(im), a[..., :3]), name + how
    return idat


def check_file(name, a, png, how=""):
    check_stream(name, a, png, how)
    assert bytes(png) == G.file_bytes_rgb(a, K.report(name, a).stream), name + how       # one slab, one IDAT: the whole file


def _file(t, n):
    got = t.cpu().numpy().tobytes()
    assert len(got) == n
    return got


@pytest.mark.parametrize("name", [name for name, _ in K.all_cases()])
def test_encode_png_device_writes_the_reference_file(name):
    """every form of the chunk grid, photograph, flat and noise content, the 800 chunks of the slab case in one launch; a canvas with
    random alpha gives the file of the opaque canvas (alpha is neither read nor leaked)"""
    K.check_regimes()
    a = dict(K.all_cases())[name]
    png = _file(*ist.encode_png_device(torch.from_numpy(a).to(DEV), level=1, color="rgb"))
    check_file(name, a, png)
    if "random alpha" in name:
        assert _file(*ist.encode_png_device(torch.from_numpy(K.opaque(a)).to(DEV), level=1, color="rgb")) == png, name


def test_encode_png_device_on_a_pitched_canvas():
    for name, a in K.shape_cases()[2:8:5]:                                # 100 x 130 (rows per chunk) and 5462 x 2 (pieces)
        h, w = a.shape[:2]
        wide = torch.full((h, w + 13, 4), 0xEE, dtype=torch.uint8, device=DEV)
        wide[:, :w] = torch.from_numpy(a).to(DEV)
        view = wide[:, :w]
        assert view.stride(0) == 4 * (w + 13)
        check_file(name, a, _file(*ist.encode_png_device(view, level=1, color="rgb")), " (pitched)")


@pytest.mark.parametrize("limit", [None, "65536"])
def test_host_path_in_slabs(monkeypatch, limit):
    """encode_png: 800 chunks in slabs of 768 and 32, each its own IDAT; IST_PNG_IDAT_LIMIT moves IDAT boundaries only"""
    if limit:
        monkeypatch.setenv("IST_PNG_IDAT_LIMIT", limit)
    name, a = K.slab_case()
    rep = K.report(name, a)
    idat = check_stream(name, a, ist.encode_png(a, level=1, color="rgb"))
    want = R.idat_lengths([c.nbytes for c in rep.chunks], R.idat_limit(limit), R.host_slabs(800))
    assert [len(d) for d in idat] == want and len(idat) >= (2 if limit is None else 3)
    if limit:
        assert all(len(d) <= 65536 for d in idat)


def _images():
    return [{"width": w, "height": h, "data": C.photo_like(60 + k, h, w)} for k, (w, h) in enumerate(((90, 60), (60, 90), (75, 50)))]


def test_stitch_png_host_images_and_bitmaps_with_and_without_preview():
    imgs = _images()
    bms = [ist.upload_bitmap(im) for im in imgs]
    for direction in ("vertical", "horizontal"):
        opts = {"gap": 3, "mode": "max"}
        canvas = np.ascontiguousarray(ist.stitch(imgs, direction, opts)["data"])
        name = "rgb stitch " + direction
        assert len(K.report(name, canvas).chunks) >= 2
        for what, src in (("host images", imgs), ("bitmaps", bms)):
            got = ist.stitch_png(src, direction, dict(opts, pngColor="rgb"))
            assert (got["width"], got["height"]) == canvas.shape[:2][::-1]
            check_file(name, canvas, got["png"], ", " + what)
            rgba = ist.stitch_png(src, direction, dict(opts, preview=BOX))
            both = ist.stitch_png(src, direction, dict(opts, preview=BOX, pngColor="rgb"))
            check_file(name, canvas, both["png"], ", %s with a preview" % what)
            assert np.array_equal(both["preview"], rgba["preview"]) and both["preview"].shape[2] == 4
            assert np.array_equal(ist.decode_png(rgba["png"]), canvas)                  # (the RGBA call in between is untouched)
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
    rgba = ist.stitch_files(paths, "vertical", dict(opts, preview=BOX))
    canvas = ist.decode_png(rgba["png"])
    name = "rgb files"
    assert len(K.report(name, canvas).chunks) >= 2
    got = ist.stitch_files(paths, "vertical", dict(opts, pngColor="rgb"), out_path=str(tmp_path / "out.png"))
    check_stream(name, canvas, got["png"])
    assert open(tmp_path / "out.png", "rb").read() == bytes(got["png"])
    both = ist.stitch_files(paths, "vertical", dict(opts, pngColor="rgb", preview=BOX))
    check_stream(name, canvas, both["png"], " with a preview")
    assert np.array_equal(both["preview"], rgba["preview"])


BATCH = ("rgb photo 100x130, random alpha", "rgb photo 5462x2, random alpha", "rgb photo 1x1, random alpha")


def test_encode_png_batch_device_with_every_grid_form_in_one_launch():
    cases = dict(K.shape_cases())
    before = L.lib.ist_debug_png_batch_launches()
    files = ist.encode_png_batch_device([torch.from_numpy(cases[n]).to(DEV) for n in BATCH], level=1, color="rgb")
    assert L.lib.ist_debug_png_batch_launches() == before + 1 and len(files) == 3
    for n, (t, ln) in zip(BATCH, files):
        check_file(n, cases[n], _file(t, ln))


def test_stitch_png_batch_with_every_grid_form_in_one_batch():
    cases = dict(K.shape_cases())
    reqs = [([{"width": a.shape[1], "height": a.shape[0], "data": K.opaque(a)}], "vertical") for a in (cases[n] for n in BATCH)]
    canvases = ist.stitch_batch(reqs)
    got = ist.stitch_png_batch(reqs, level=1, color="rgb")
    for k, n in enumerate(BATCH):
        canvas = np.ascontiguousarray(canvases[k])
        assert canvas.shape == cases[n].shape and (got[k]["width"], got[k]["height"]) == canvas.shape[:2][::-1]
        check_file("rgb batch request %d" % k, canvas, got[k]["png"])
    plain = ist.stitch_png_batch(reqs, level=1)                            # the next batch without the option is RGBA again
    for k in range(3):
        assert np.array_equal(ist.decode_png(plain[k]["png"]), canvases[k])


def test_one_context_switched_between_the_forms():
    name, a = K.shape_cases()[2]                                           # 100 x 130
    dense = torch.from_numpy(a).to(DEV)
    want = {"rgba": R.file_bytes(a), "rgb": G.file_bytes_rgb(a, K.report(name, a).stream)}
    allocs = None
    for color in ("rgba", "rgb", "rgba", "rgb"):
        assert _file(*ist.encode_png_device(dense, level=1, color=color)) == want[color], color
        if color == "rgb" and allocs is None:
            allocs = L.lib.ist_debug_device_allocs()
    assert L.lib.ist_debug_device_allocs() == allocs                       # flat after the first pair
    assert _file(*ist.encode_png_device(dense, level=1)) == want["rgba"]   # no colour given: RGBA, whatever the call before chose


def test_stored_form_refuses_rgb_and_the_context_recovers():
    name, a = K.shape_cases()[1]                                           # 3 x 5
    dense = torch.from_numpy(a).to(DEV)
    img = {"width": 3, "height": 5, "data": K.opaque(a)}
    calls = {"encode_png_device": lambda lv: ist.encode_png_device(dense, level=lv, color="rgb"),
             "stitch_png": lambda lv: ist.stitch_png([img], "vertical", {"pngLevel": lv, "pngColor": "rgb"}),
             "encode_png_batch_device": lambda lv: ist.encode_png_batch_device([dense, dense], level=lv, color="rgb"),
             "encode_png": lambda lv: ist.encode_png(a, level=lv, color="rgb"),
             "stitch_png_batch": lambda lv: ist.stitch_png_batch([([img], "vertical")], level=lv, color="rgb")}
    for who, call in calls.items():
        with pytest.raises(ist.StitchError) as e:
            call(0)
        assert e.value.code == E_UNSUPPORTED and "pngLevel 1" in str(e.value), who
    want = G.file_bytes_rgb(a, K.report(name, a).stream)                   # the same context, set back to level 1
    assert _file(*ist.encode_png_device(dense, level=1, color="rgb")) == want
    assert bytes(ist.stitch_png([img], "vertical", {"pngLevel": 1, "pngColor": "rgb"})["png"]) == want
    assert [_file(t, n) for t, n in ist.encode_png_batch_device([dense, dense], level=1, color="rgb")] == [want, want]
    assert np.array_equal(ist.decode_png(ist.encode_png(a, level=0)), a)   # and the stored form still writes RGBA
