"""Resident bitmaps on the GPU (ist_bitmap_*, ist_stitch_bitmaps_*; Python host): images decoded or uploaded once and stitched again and
again from HBM give the host path's pixels byte for byte, decode nothing again, and give their memory back."""
import gc
import io

import numpy as np
import pytest
from PIL import Image

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests import util as U

pytestmark = pytest.mark.gpu


def _photo(seed, h, w):
    a = U.smooth_image(seed, h, w)[..., :3].astype(np.int32)
    a += np.random.default_rng(seed).integers(-20, 21, a.shape)
    return np.clip(a, 0, 255).astype(np.uint8)


def _save(im, fmt, **kw):
    b = io.BytesIO()
    im.save(b, fmt, **kw)
    return b.getvalue()


def _jpeg(a, orientation=None, **kw):
    if orientation:
        exif = Image.Exif()
        exif[0x0112] = orientation
        kw["exif"] = exif
    return _save(Image.fromarray(a), "JPEG", **kw)


def _pil(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))


def _block_bytes(w, h):
    """what one bitmap holds on the device: dense rows + the 256-byte tail of a staged source, 256-byte aligned"""
    return (w * 4 * h + 256 + 255) & ~255


def _host_twin(bitmaps):
    """the same pixels and descs as host images"""
    return [{"width": b.width, "height": b.height, "orientation": b.orientation, "opaque": b.opaque, "fileSize": b.file_size, "data": b.download()}
            for b in bitmaps]


def _mixed_files(h=96, w=128):
    """one file per decoder path: baseline JPEG 4:2:0 / 4:4:4 with and without restart intervals (GPU entropy decoder), progressive
    JPEG, PNG with alpha, BMP, GIF, lossy and lossless WebP"""
    rgba = U.smooth_image(5, h, w, opaque=False)
    files = [
        _jpeg(_photo(1, h, w), quality=88, subsampling=2),
        _jpeg(_photo(2, h + 7, w - 3), quality=90, subsampling=0),
        _jpeg(_photo(3, h, w + 5), quality=85, subsampling=2, restart_marker_blocks=3),
        _jpeg(_photo(4, h - 5, w), quality=85, subsampling=0, restart_marker_rows=1),
        _jpeg(_photo(6, h + 11, w), quality=80, subsampling=2, progressive=True),
        _save(Image.fromarray(rgba, "RGBA"), "PNG"),
        _save(Image.fromarray(_photo(7, h, w - 9)), "BMP"),
        _save(Image.fromarray(_photo(8, h - 13, w)).convert("P"), "GIF"),
        _save(Image.fromarray(_photo(9, h, w + 3)), "WEBP", quality=80),
        _save(Image.fromarray(rgba, "RGBA"), "WEBP", lossless=True),
    ]
    assert b"\xff\xdd" in files[2] and b"\xff\xdd" in files[3]
    return files


@pytest.mark.parametrize("w,h", [(1, 5), (2, 9), (3, 4), (4, 1), (5, 7), (6, 3), (7, 11), (1, 3000), (4032, 3024)])
def test_upload_and_download_round_trip_exactly(w, h):
    a = U.rand_image(w * 1000 + h, h, w, opaque=False)
    before = L.lib.ist_debug_bitmap_bytes()
    b = ist.upload_bitmap({"width": w, "height": h, "data": a, "orientation": 3, "fileSize": 12345, "opaque": False})
    assert (b.width, b.height, b.orientation, b.file_size, b.opaque) == (w, h, 3, 12345, False)
    assert L.lib.ist_debug_bitmap_bytes() - before == _block_bytes(w, h)
    assert np.array_equal(b.download(), a)
    # a source with padded rows (its pitch is not 4 * width) and a bare array
    wide = U.rand_image(w + h, h, w + 3, opaque=True)
    c = ist.upload_bitmap(wide[:, :w])
    assert (c.width, c.height, c.orientation, c.file_size) == (w, h, 1, 0)
    assert np.array_equal(c.download(), wide[:, :w])
    b.close()
    c.close()
    assert L.lib.ist_debug_bitmap_bytes() == before


def test_decoded_bitmaps_are_the_decoder_pixels_with_the_file_pipeline_desc():
    files = _mixed_files()
    bms = ist.decode_bitmaps(files)
    assert len(bms) == len(files)
    for k, (f, b) in enumerate(zip(files, bms)):
        w, h, o = ist.image_info(f)
        assert (b.width, b.height, b.orientation, b.file_size) == (w, h, o or 1, len(f)), k
        assert b.opaque == (f[:2] == b"\xff\xd8"), k
        assert np.array_equal(b.download(), ist.decode_image(f)), k
    for b in bms:
        b.close()


def test_decode_is_all_or_nothing(tmp_path):
    good = _jpeg(_photo(11, 40, 50), quality=90)
    p = tmp_path / "good.jpg"
    p.write_bytes(good)
    before = L.lib.ist_debug_bitmap_bytes()
    with pytest.raises(ist.StitchError) as e:
        ist.decode_bitmaps([str(p), good, good[:200]])
    assert e.value.code in (-6, -7) and "图片2解码异常" in str(e.value)
    assert L.lib.ist_debug_bitmap_bytes() == before
    bms = ist.decode_bitmaps([str(p), good])
    assert np.array_equal(bms[0].download(), bms[1].download())
    del bms
    gc.collect()
    assert L.lib.ist_debug_bitmap_bytes() == before


def _parity(bms, direction, opts, oracle=True):
    """stitch(bitmaps) == stitch(the same pixels and descs as host arrays), byte for byte; and within the oracle's tolerance"""
    got = ist.stitch(bms, direction, opts)
    host = _host_twin(bms)
    want = ist.stitch(host, direction, opts)
    assert (got["width"], got["height"]) == (want["width"], want["height"])
    assert np.array_equal(got["data"], want["data"]), (direction, opts)
    if oracle:
        ref, _, _ = U.oracle_stitch([h["data"] for h in host], direction, opts, orientations=[h["orientation"] for h in host])
        U.oracle_tolerance(got["data"], ref, exact=opts.get("filter") == "nearest" and not U.edge_aa_of(opts))
    return got


@pytest.mark.parametrize("filt", ["nearest", "bilinear", "area"])
@pytest.mark.parametrize("edge_aa", [False, True])
def test_stitch_from_bitmaps_is_the_host_path(filt, edge_aa):
    px = [U.rand_image(300, 61, 83), U.smooth_image(301, 97, 40), U.rand_image(302, 33, 120, opaque=False), U.smooth_image(303, 150, 151)]
    ori = [1, 6, 3, 8]
    bms = [ist.upload_bitmap({"width": a.shape[1], "height": a.shape[0], "orientation": o, "data": a}) for a, o in zip(px, ori)]
    for direction in ("vertical", "horizontal"):
        for mode in ("min", "max", "original"):
            _parity(bms, direction, {"filter": filt, "edgeAA": edge_aa, "mode": mode, "gap": 5})


def test_every_orientation_with_a_gap_in_every_mode():
    px = [U.smooth_image(400 + k, 30 + 7 * k, 50 - 3 * k) for k in range(8)]
    bms = [ist.upload_bitmap({"width": a.shape[1], "height": a.shape[0], "orientation": k + 1, "data": a}) for k, a in enumerate(px)]
    for direction in ("vertical", "horizontal"):
        for mode in ("min", "max", "original"):
            _parity(bms, direction, {"filter": "bilinear", "mode": mode, "gap": 7})


@pytest.mark.parametrize("platform", ["ios", "android"])
def test_phone_plans_and_a_big_task_from_the_file_size(platform):
    px = [U.smooth_image(500 + k, 300 + 40 * k, 400 - 30 * k) for k in range(3)]
    small = [ist.upload_bitmap({"width": a.shape[1], "height": a.shape[0], "orientation": 1 + 2 * k, "data": a}) for k, a in enumerate(px)]
    _parity(small, "vertical", {"platform": platform, "gap": 4})
    big = [ist.upload_bitmap({"width": a.shape[1], "height": a.shape[0], "fileSize": 30 << 20, "data": a}) for a in px]
    assert ist.plan(big, "horizontal", {"platform": platform}).big_task
    assert not ist.plan(small, "horizontal", {"platform": platform}).big_task
    _parity(big, "horizontal", {"platform": platform, "mode": "max"}, oracle=False)      # (the oracle's descs carry no file size)


def test_a_canvas_the_host_path_renders_in_row_bands():
    """>= 32 MB canvases go through the banded host path (uploads and downloads overlapped); the bitmap path renders them in one launch
    and must still give the same bytes"""
    px = [U.smooth_image(600 + k, 1500, 2000) for k in range(3)]
    bms = [ist.upload_bitmap(a) for a in px]
    before = L.lib.ist_debug_duplex_stitches()
    got = _parity(bms, "vertical", {"filter": "bilinear"}, oracle=False)
    assert L.lib.ist_debug_duplex_stitches() - before == 1          # (the host leg took the banded path)
    assert got["data"].nbytes >= 32 << 20
    assert np.array_equal(got["data"], np.concatenate(px, 0))
    got = _parity(bms, "horizontal", {"filter": "area", "mode": "original", "gap": 3}, oracle=False)


def test_stitch_png_from_decoded_bitmaps_is_stitch_files(tmp_path):
    files = _mixed_files(h=120, w=160)[:9]
    paths = []
    for k, f in enumerate(files):
        paths.append(str(tmp_path / ("f%d" % k)))
        open(paths[-1], "wb").write(f)
    bms = ist.decode_bitmaps(paths)
    _, descs = ist.decode_files_device(files)
    for opts in ({}, {"platform": "ios", "gap": 6, "filter": "area"}, {"mode": "original", "gap": 2}):
        for direction in ("vertical", "horizontal"):
            got = ist.stitch_png(bms, direction, opts)
            want = ist.stitch_files(paths, direction, opts)
            assert (got["width"], got["height"]) == (want["width"], want["height"])
            assert np.array_equal(_pil(got["png"]), _pil(want["png"])), (direction, opts)
            pb, pf = ist.plan(bms, direction, opts), ist.plan(descs, direction, opts)
            assert (pb.canvas_w, pb.canvas_h, pb.super_sample, pb.scale_down, pb.big_task, pb.rects) == \
                   (pf.canvas_w, pf.canvas_h, pf.super_sample, pf.scale_down, pf.big_task, pf.rects)


def test_restitch_decodes_nothing_again_and_allocates_nothing():
    photos = [_photo(700 + k, 300 + 20 * k, 400 - 10 * k) for k in range(5)]
    files = [_jpeg(a, quality=90, subsampling=2) for a in photos]
    entropy = L.lib.ist_debug_gpu_entropy_files()
    bms = ist.decode_bitmaps(files)
    assert L.lib.ist_debug_gpu_entropy_files() - entropy == len(files)          # (baseline JPEG: the GPU entropy decoder)
    entropy = L.lib.ist_debug_gpu_entropy_files()
    layouts = [
        ([bms[k] for k in (2, 0, 4, 1, 3)], "vertical", {"gap": 0}),
        (bms[::-1], "vertical", {"gap": 0}),
        (bms[::-1], "horizontal", {"gap": 0}),
        (bms[::-1], "horizontal", {"gap": 9, "mode": "max"}),
    ]
    first = []
    for imgs, direction, opts in layouts:
        first.append(_parity(imgs, direction, opts, oracle=False)["data"].copy())
    assert L.lib.ist_debug_gpu_entropy_files() == entropy
    for (imgs, direction, opts), want in zip(layouts, first):
        assert np.array_equal(ist.stitch(imgs, direction, opts)["data"], want)
        assert ist.stitch_png(imgs, direction, opts) is not None
    allocs = L.lib.ist_debug_device_allocs()          # (the PNG encoder's scratch is made by its first call above)
    for (imgs, direction, opts), want in zip(layouts, first):
        assert np.array_equal(ist.stitch(imgs, direction, opts)["data"], want)
        assert np.array_equal(_pil(ist.stitch_png(imgs, direction, opts)["png"]), want)
    assert L.lib.ist_debug_device_allocs() == allocs
    assert L.lib.ist_debug_gpu_entropy_files() == entropy


def test_memory_comes_back_on_close_and_on_collection():
    gc.collect()
    base = L.lib.ist_debug_bitmap_bytes()
    a = U.rand_image(800, 301, 257)
    b = ist.upload_bitmap(a)
    c = ist.decode_bitmaps([_jpeg(_photo(801, 64, 80), quality=90)])[0]
    assert L.lib.ist_debug_bitmap_bytes() == base + _block_bytes(257, 301) + _block_bytes(80, 64)
    b.close()
    b.close()                                                    # (again: nothing)
    with pytest.raises(ValueError):
        b.download()
    with pytest.raises(ValueError):
        ist.stitch([b, c], "vertical")
    assert L.lib.ist_debug_bitmap_bytes() == base + _block_bytes(80, 64)
    del c
    gc.collect()
    assert L.lib.ist_debug_bitmap_bytes() == base


def test_a_missing_bitmap_and_an_empty_request():
    b = ist.upload_bitmap(U.rand_image(900, 10, 10))
    with pytest.raises(ist.StitchError) as e:
        ist.stitch([b, None], "vertical")
    assert e.value.code == -6 and "图片1解码异常" in str(e.value)
    assert ist.stitch([], "vertical") is None
    with pytest.raises(ist.StitchError) as e:
        ist.upload_bitmap({"width": 0, "height": 4, "data": np.zeros((4, 0, 4), np.uint8)})
    assert e.value.code == -6


@pytest.mark.skipif(L.lib.ist_device_count() < 2, reason="needs two GPUs")
def test_a_bitmap_of_another_device_is_refused():
    b = ist.upload_bitmap(U.rand_image(901, 8, 8), device=1)
    with pytest.raises(ist.StitchError) as e:
        ist.stitch([b], "vertical", device=0)
    assert e.value.code == -1
