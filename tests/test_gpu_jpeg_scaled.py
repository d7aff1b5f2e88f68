"""Reduced-size JPEG decode on the GPU (scale= 2, 4, 8; csrc/ist_jpeg_scaled.hip): every decode is byte-equal to the numpy statement
of the contract (tests/jpeg_scaled_reference.py, itself pinned against Pillow's draft by tests/test_jpeg_scaled_reference.py).

The writer's size matrix (widths 1-17 x heights 1-17) at a scaled block of 4, 2 or 1 samples covers scaled widths 1-9, planes at most
2 samples wide (where h2v1 replicates) and partial blocks at every IDCT size; its coefficient-edge, 16-bit-table, multi-scan and
restart files cover both entropy paths; the large files span several workgroups of both kernels in x and y.  Files go through
decode_bitmaps 128 per call with one denominator per file."""
import ctypes as C
import functools
import io

import numpy as np
import pytest
from PIL import Image

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from imagestitching_amd.stitch import _ctx
from tests import jpeg_scaled_reference as R
from tests import jpeg_writer as JW
from tests import util as U

pytestmark = pytest.mark.gpu

LAYOUTS = ("grey", "444", "420", "422", "440", "rgb", "rgb420")
SCALES = (2, 4, 8)


def _launches():
    return L.lib.ist_debug_jpeg_scaled_launches()


def _gpu_files():
    return L.lib.ist_debug_gpu_entropy_files()


def _decode(datas, scales):
    """files -> downloaded pixels, 128 files per decode call; every bitmap's desc is checked on the way"""
    out = []
    for k in range(0, len(datas), 128):
        bms = ist.decode_bitmaps(datas[k:k + 128], scale=list(scales[k:k + 128]))
        for b, data, d in zip(bms, datas[k:k + 128], scales[k:k + 128]):
            w, h, _ = ist.image_info(data)
            assert (b.width, b.height) == (w, h), "the desc keeps the natural size"
            sw, sh = ist.scaled_size(w, h, d)
            assert b.shape == (sh, sw, 4), (b.shape, (w, h), d)
            if d > 1:
                assert (b._desc.bmp_width, b._desc.bmp_height) == (sw, sh)
            out.append(b.download())
            b.close()
    return out


def _check_cases(cases, scales=SCALES):
    """every case at every scale against the contract; returns how many files the GPU Huffman decoder took"""
    datas = [c["data"] for c in cases for _ in scales]
    ds = [d for _ in cases for d in scales]
    before = _gpu_files()
    got = _decode(datas, ds)
    taken = _gpu_files() - before
    k = 0
    for c in cases:
        for d in scales:
            want = R.decode_rgba(c["frame"], d)
            g = got[k]
            k += 1
            assert g.shape == want.shape, (c["name"], d, g.shape, want.shape)
            diff = np.abs(g.astype(np.int32) - want.astype(np.int32))
            assert diff.max() == 0, "%s at 1/%d: max diff %d in %d px, first at %s" % (
                c["name"], d, diff.max(), int((diff.max(-1) > 0).sum()), tuple(np.argwhere(diff.max(-1) > 0)[0]))
    return taken


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_small_size_at_every_scale(layout):
    cases = JW.size_cases(layout)
    assert _check_cases(cases) == len(SCALES) * sum(c["gpu"] for c in cases)


@pytest.mark.parametrize("layout", JW.VARIANT_LAYOUTS)
def test_coefficient_edges_wide_tables_and_both_entropy_paths(layout):
    """frame_edges coefficients, the SOF1 file with 16-bit tables, files the host entropy decoder takes (three tables, one scan per
    component) and restart-interval files on the GPU Huffman path"""
    cases = JW.variant_cases(layout)
    names = {c["name"][len(layout) + 1:] for c in cases}
    assert {"edges", "sof1_q16", "restart3"} <= names and (layout == "grey" or {"three_tables", "scans_cr_cb_y"} <= names)
    host = [c for c in cases if not c["gpu"]]
    assert layout == "grey" or host, "some files must take the host entropy path"
    assert _check_cases(cases) == len(SCALES) * sum(c["gpu"] for c in cases)


def test_a_restart_interval_file_takes_the_gpu_huffman_path():
    c = [c for c in JW.variant_cases("420") if c["name"] == "420_restart7"]
    assert len(c) == 1 and c[0]["gpu"]
    assert _check_cases(c) == len(SCALES), "ist_debug_gpu_entropy_files must move: no silent host decode"


def test_large_files_span_several_workgroups():
    cases = JW.large_cases()
    assert {(c["width"], c["height"]) for c in cases} == {(1000, 700), (4000, 64)}
    before = _launches()
    _check_cases(cases)
    assert _launches() > before


def _pillow_file(w, h, seed, **save):
    b = io.BytesIO()
    Image.fromarray(JW.photo(seed, h, w, 8)).save(b, "JPEG", **save)
    return b.getvalue()


def _draft(data, d):
    im = Image.open(io.BytesIO(data))
    w, h = im.size
    im.draft(im.mode, (w // d, h // d))
    assert im.size == ist.scaled_size(w, h, d), (im.size, d)
    return np.asarray(im.convert("RGBA"))


def test_a_progressive_pillow_file_against_draft():
    data = _pillow_file(203, 141, 5, quality=88, progressive=True)
    before = _gpu_files()
    got = _decode([data] * 3, list(SCALES))
    assert _gpu_files() == before                       # progressive: the host entropy decoder
    for g, d in zip(got, SCALES):
        assert np.array_equal(g, _draft(data, d)), d


@functools.lru_cache(maxsize=None)
def _photo_12mp():
    return _pillow_file(4032, 3024, 12, quality=90)


@pytest.mark.parametrize("d", SCALES)
def test_a_12_megapixel_photo_against_draft(d):
    data = _photo_12mp()
    (got,) = _decode([data], [d])
    want = _draft(data, d)
    assert got.shape == want.shape
    assert np.array_equal(got, want), int((got != want).any(-1).sum())


def _png(seed, h, w):
    b = io.BytesIO()
    Image.fromarray(U.rand_image(seed, h, w, opaque=False)).save(b, "PNG")
    return b.getvalue()


def _mixed_files():
    jp = [c["data"] for c in JW.size_cases("420") if c["name"] in ("420_17x16", "420_9x15", "420_16x17", "420_13x9")]
    assert len(jp) == 4
    return [jp[0], jp[1], _png(3, 21, 34), jp[2], jp[3]]


def test_a_mixed_call_with_a_png_among_the_files():
    files = _mixed_files()
    full = ist.decode_bitmaps(files)
    mixed = ist.decode_bitmaps(files, scale=[1, 2, 4, 8, 1])
    for i in (0, 2, 4):                                 # d = 1 and the PNG (which decodes at 1 / 1 whatever its denominator)
        assert np.array_equal(mixed[i].download(), full[i].download()), i
        assert bytes(mixed[i]._desc) == bytes(full[i]._desc), i
    assert (mixed[2]._desc.bmp_width, mixed[2]._desc.bmp_height) in ((0, 0), (34, 21))
    for i, d in ((1, 2), (3, 8)):
        w, h, _ = ist.image_info(files[i])
        assert (mixed[i].width, mixed[i].height) == (w, h)
        assert mixed[i].shape[:2] == ist.scaled_size(w, h, d)[::-1]
        assert np.array_equal(mixed[i].download(), ist.decode_image(files[i], scale=d))
    for b in full + mixed:
        b.close()


def test_an_all_one_call_makes_no_reduced_launch():
    files = _mixed_files()
    n = len(files)
    before = _launches()
    out = (C.c_void_p * n)()
    L.check(L.lib.ist_bitmaps_decode_scaled(_ctx(0), (C.c_char_p * n)(*files), (C.c_int64 * n)(*[len(f) for f in files]), n,
                                            (C.c_int32 * n)(*[1] * n), out))
    bms = [ist.Bitmap(out[i], 0) for i in range(n)]
    assert _launches() == before
    ref = ist.decode_bitmaps(files)
    for a, b in zip(bms, ref):
        assert np.array_equal(a.download(), b.download()) and bytes(a._desc) == bytes(b._desc)
    for b in bms + ref:
        b.close()
    b2 = ist.decode_bitmaps(files[:1], scale=2)
    assert _launches() > before
    b2[0].close()


def test_bad_denominators_fail_before_anything_is_decoded():
    files = _mixed_files()
    bytes_before, launches = L.lib.ist_debug_bitmap_bytes(), _launches()
    for bad in (0, 3, 16, -2):
        with pytest.raises(ist.StitchError) as e:
            ist.decode_bitmaps(files, scale=[1, 2, bad, 4, 8])
        assert e.value.code == -1 and "image 2" in str(e.value), str(e.value)
    n = len(files)
    out = (C.c_void_p * n)()
    rc = L.lib.ist_bitmaps_decode_scaled(_ctx(0), (C.c_char_p * n)(*files), (C.c_int64 * n)(*[len(f) for f in files]), n,
                                         (C.c_int32 * n)(1, 2, 4, 5, 1), out)
    assert rc == -1 and b"image 3" in L.lib.ist_last_error() and not any(out)
    with pytest.raises(ist.StitchError):
        ist.decode_image(files[0], scale=3)
    assert L.lib.ist_debug_bitmap_bytes() == bytes_before and _launches() == launches
    # all or nothing with a damaged file, as the unscaled call
    with pytest.raises(ist.StitchError) as e:
        ist.decode_bitmaps([files[0], files[1][:40]], scale=2)
    assert "图片1解码异常" in str(e.value)
    assert L.lib.ist_debug_bitmap_bytes() == bytes_before


def test_a_scaled_bitmap_holds_what_an_uploaded_one_of_its_size_holds():
    data = JW.large_cases()[0]["data"]                  # 1000 x 700
    base = L.lib.ist_debug_bitmap_bytes()
    for d in SCALES:
        (b,) = ist.decode_bitmaps([data], scale=d)
        held = L.lib.ist_debug_bitmap_bytes() - base
        sw, sh = ist.scaled_size(1000, 700, d)
        b.close()
        u = ist.upload_bitmap(np.zeros((sh, sw, 4), np.uint8))
        assert L.lib.ist_debug_bitmap_bytes() - base == held, d
        u.close()
    assert L.lib.ist_debug_bitmap_bytes() == base


def _handles():
    out = (C.c_int64 * 4)()
    assert L.lib.ist_debug_live_handles(out) == L.IST_OK
    return list(out)


def test_live_handles_are_steady_across_repeated_calls():
    files = _mixed_files()
    for b in ist.decode_bitmaps(files, scale=[2, 4, 8, 2, 1]):
        b.close()
    before = _handles()
    for _ in range(3):
        for b in ist.decode_bitmaps(files, scale=[2, 4, 8, 2, 1]):
            b.close()
        ist.decode_image(files[0], scale=4)
    assert _handles() == before


def test_decode_files_device_takes_the_scale_and_checks_the_scaled_capacity():
    import torch
    c = [c for c in JW.size_cases("422") if c["name"] == "422_17x9"][0]
    out, imgs = ist.decode_files_device([c["data"], c["data"]], scale=[2, 1])
    assert tuple(out[0].shape) == (5, 9, 4) and tuple(out[1].shape) == (9, 17, 4)
    assert (imgs[0]["width"], imgs[0]["height"], imgs[0]["bmpWidth"], imgs[0]["bmpHeight"]) == (17, 9, 9, 5) and "bmpWidth" not in imgs[1]
    assert np.array_equal(out[0].cpu().numpy(), R.decode_rgba(c["frame"], 2))
    assert np.array_equal(out[1].cpu().numpy(), R.decode_rgba(c["frame"], 1))
    small = [torch.empty((5, 8, 4), dtype=torch.uint8, device="cuda")]            # one column short of 9 x 5
    with pytest.raises(ist.StitchError) as e:
        ist.decode_files_device([c["data"]], out=small, scale=2)
    assert e.value.code == -1 and "9x5" in str(e.value)
    fits = [torch.empty((5, 9, 4), dtype=torch.uint8, device="cuda")]             # too small for 17 x 9, right for the scaled size
    ist.decode_files_device([c["data"]], out=fits, scale=2)
    assert np.array_equal(fits[0].cpu().numpy(), R.decode_rgba(c["frame"], 2))


@pytest.mark.parametrize("direction", ("vertical", "horizontal"))
def test_stitch_of_scaled_bitmaps_is_stitch_of_their_pixels_at_the_natural_size(direction):
    """a reduced bitmap is a drop-in: the plan and the canvas are those of the full-size bitmaps, the pixels those of host images that
    hold the scaled pixels under the natural width / height"""
    cases = JW.large_cases()[:1] + [c for c in JW.variant_cases("440") if c["name"] in ("440_std", "440_edges_optimal")]
    files = [c["data"] for c in cases]
    scales = [4, 2, 2]
    opts = {"gap": 3}
    full = ist.decode_bitmaps(files)
    red = ist.decode_bitmaps(files, scale=scales)
    p_full, p_red = ist.plan(full, direction, opts), ist.plan(red, direction, opts)
    assert (p_full.canvas_w, p_full.canvas_h, p_full.rects) == (p_red.canvas_w, p_red.canvas_h, p_red.rects)
    a = ist.stitch(red, direction, opts)
    f = ist.stitch(full, direction, opts)
    assert (a["width"], a["height"]) == (f["width"], f["height"]) == (p_full.canvas_w, p_full.canvas_h)
    host = [{"width": b.width, "height": b.height, "orientation": b.orientation, "opaque": b.opaque, "fileSize": b.file_size, "data": b.download()}
            for b in red]
    assert all(h["data"].shape[1] < h["width"] for h in host)
    h = ist.stitch(host, direction, opts)
    assert (h["width"], h["height"]) == (a["width"], a["height"])
    assert np.array_equal(np.asarray(a["data"]), np.asarray(h["data"]))
    for b in full + red:
        b.close()


@pytest.mark.parametrize("mode", ("fill", "fit"))
def test_thumbnails_from_files_are_thumbnails_of_bitmaps_at_the_chosen_scales(mode):
    big = JW.large_cases()
    files = [big[0]["data"], big[1]["data"], _png(9, 300, 200), _pillow_file(640, 480, 3, quality=85)]
    cell = (60, 40)
    infos = [ist.image_info(f) for f in files]
    items = ist.thumbnail_layout([(w, h, o or 1) for w, h, o in infos], cell, mode)
    scales = [ist.decode_scale_fit(w, h, t["width"], t["height"]) for (w, h, _), t in zip(infos, items)]
    assert max(scales) == 8 and len(set(scales)) > 1, scales      # (fill: 4000 x 64 cannot shrink, its height is all the cell shows)
    live = L.lib.ist_debug_bitmap_bytes()
    got = ist.thumbnails_from_files(files, cell, mode)
    assert L.lib.ist_debug_bitmap_bytes() == live, "the bitmaps are released"
    bms = ist.decode_bitmaps(files, scale=scales)
    want = ist.thumbnails(bms, cell, mode)
    assert len(got) == len(want) == len(files)
    for g, w_ in zip(got, want):
        assert np.array_equal(g, w_)
    for b in bms:
        b.close()


def test_thumbnails_from_files_map_the_thumbnail_to_the_stored_axes():
    """an EXIF-turned file (orientation 6: the stored pixels lie on their side): the thumbnail's width bounds the stored HEIGHT"""
    b = io.BytesIO()
    exif = Image.Exif()
    exif[0x0112] = 6
    Image.fromarray(JW.photo(4, 160, 1200, 8)).save(b, "JPEG", quality=85, exif=exif)
    data = b.getvalue()
    assert ist.image_info(data) == (1200, 160, 6)
    cell = (20, 150)                                    # upright the image is 160 x 1200
    (t,) = ist.thumbnail_layout([(1200, 160, 6)], cell, "fit")
    d = ist.decode_scale_fit(1200, 160, t["height"], t["width"])
    assert d == 8 and ist.decode_scale_fit(1200, 160, t["width"], t["height"]) == 1
    (bm,) = ist.decode_bitmaps([data], scale=d)
    (want,) = ist.thumbnails([bm], cell, "fit")
    bm.close()
    (got,) = ist.thumbnails_from_files([data], cell, "fit")
    assert got.shape == (t["height"], t["width"], 4) and np.array_equal(got, want)
