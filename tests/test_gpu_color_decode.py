"""profile='srgb' on the decode entry points: a file tagged with an ICC profile the colour contract takes lands in HBM converted to sRGB,
byte for byte tests/icc_reference.py applied to what the same call leaves with profile='ignore' - on each of the decoder's three ways
to place a bitmap (JPEG decoded on the GPU, JPEG from host coefficients, host-decoded file upload) and at a reduced scale.  Untagged,
sRGB-tagged and unsupported files stay as decoded; 'ignore' is every byte of the call without the argument."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import icc_reference as R
import icc_writer as W
import imagestitching_amd as ist
from imagestitching_amd import _lib as L

pytestmark = pytest.mark.gpu

P3 = W.fixtures()["p3_para3"]
TAB = R.tables(P3)
GRAY = W.profile(W.P3, W.para(0, 2.2), space=b"GRAY")


def _pixels(w, h, alpha=False):
    rng = np.random.default_rng(w * 1000 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([(xx * 255) // max(1, w - 1), (yy * 255) // max(1, h - 1), ((xx + yy) * 9) % 256], -1)
    a = (a + rng.integers(-12, 12, a.shape)).clip(0, 255).astype(np.uint8)
    if alpha:
        a = np.concatenate([a, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], -1)
    return a


def _file(fmt, w, h, icc=None, **kw):
    im = Image.fromarray(_pixels(w, h, kw.pop("alpha", False)))
    b = io.BytesIO()
    im.save(b, fmt, **({"icc_profile": icc} if icc else {}), **kw)
    return b.getvalue()


def _tagged_files():
    files = {}
    for w, h in ((48, 32), (65, 17)):
        for sub, sname in ((2, "420"), (0, "444")):
            for prog in (False, True):
                files["jpeg %dx%d %s %s" % (w, h, sname, "progressive" if prog else "baseline")] = _file("JPEG", w, h, P3, subsampling=sub, progressive=prog, quality=90)
        files["png %dx%d" % (w, h)] = _file("PNG", w, h, P3)
        files["png rgba %dx%d" % (w, h)] = _file("PNG", w, h, P3, alpha=True)
        files["webp %dx%d" % (w, h)] = _file("WEBP", w, h, P3, lossless=True)
        files["webp lossy %dx%d" % (w, h)] = _file("WEBP", w, h, P3, quality=85)
    return files


FILES = _tagged_files()


def _down(bitmaps):
    out = [b.download() for b in bitmaps]
    for b in bitmaps:
        b.close()
    return out


def test_every_tagged_file_is_found():
    assert all(ist.image_color(f) == "convert" for f in FILES.values())


def test_decode_bitmaps_converts_tagged_files():
    names, blobs = list(FILES), list(FILES.values())
    gpu_before = L.lib.ist_debug_gpu_entropy_files()
    plain = _down(ist.decode_bitmaps(blobs))
    assert L.lib.ist_debug_gpu_entropy_files() - gpu_before == 4          # the baseline JPEGs take the GPU decoder, the progressive ones the host's
    launches = L.lib.ist_debug_color_launches()
    conv = _down(ist.decode_bitmaps(blobs, profile="srgb"))
    assert L.lib.ist_debug_color_launches() - launches == len(blobs)      # one launch per image
    for n, p, c in zip(names, plain, conv):
        assert np.array_equal(c, R.convert(TAB, p)), n
        assert not np.array_equal(c, p), n
    again = _down(ist.decode_bitmaps(blobs, profile="ignore"))            # the setting does not outlive its call
    assert all(np.array_equal(a, p) for a, p in zip(again, plain))
    assert all(np.array_equal(a, p) for a, p in zip(_down(ist.decode_bitmaps(blobs)), plain))


def test_decode_bitmaps_at_a_reduced_scale():
    names = [n for n in FILES if n.startswith("jpeg")] + ["png 65x17"]
    blobs = [FILES[n] for n in names]
    plain = _down(ist.decode_bitmaps(blobs, scale=2))
    conv = _down(ist.decode_bitmaps(blobs, scale=2, profile="srgb"))
    for n, p, c in zip(names, plain, conv):
        assert p.shape[:2] == ((17, 65) if n == "png 65x17" else (16, 24) if "48x32" in n else (9, 33)), (n, p.shape)
        assert np.array_equal(c, R.convert(TAB, p)), n
    per_file = [1, 2, 4, 8, 1, 2, 4, 8, 1]
    plain = _down(ist.decode_bitmaps(blobs, scale=per_file))
    conv = _down(ist.decode_bitmaps(blobs, scale=per_file, profile="srgb"))
    assert all(np.array_equal(c, R.convert(TAB, p)) for p, c in zip(plain, conv))


def test_a_mixed_list_changes_only_the_convertible_image():
    srgb = W.fixtures()["srgb_para3"]
    blobs = [_file("JPEG", 48, 32), _file("JPEG", 48, 32, srgb), _file("JPEG", 48, 32, P3), _file("JPEG", 48, 32, GRAY),
             _file("PNG", 33, 9), W.png_with_chunks(_file("PNG", 33, 9), [(b"sRGB", b"\0")]), _file("PNG", 33, 9, P3), _file("PNG", 33, 9, GRAY),
             W.png_with_icc(_file("PNG", 33, 9), P3, corrupt=True), W.jpeg_with_icc(_file("JPEG", 65, 17), P3, chunks=3, order=(2, 3, 1)),
             W.jpeg_with_icc(_file("JPEG", 65, 17), P3, chunks=3, drop=3), _file("BMP", 20, 10), W.jpeg_with_icc(_file("JPEG", 65, 17), W.fixtures()["adobe_gamma"])]
    kinds = [ist.image_color(b) for b in blobs]
    assert kinds == ["none", "identity", "convert", "unsupported", "none", "identity", "convert", "unsupported", "none", "convert", "none", "none", "convert"]
    plain = _down(ist.decode_bitmaps(blobs))
    launches = L.lib.ist_debug_color_launches()
    conv = _down(ist.decode_bitmaps(blobs, profile="srgb"))
    assert L.lib.ist_debug_color_launches() - launches == kinds.count("convert")
    for k, (kind, p, c) in enumerate(zip(kinds, plain, conv)):
        tab = R.tables(W.fixtures()["adobe_gamma"]) if k == len(blobs) - 1 else TAB
        assert np.array_equal(c, R.convert(tab, p) if kind == "convert" else p), (k, kind)


def test_decode_files_device_into_caller_tensors():
    names, blobs = list(FILES), list(FILES.values())
    plain, descs = ist.decode_files_device(blobs)
    plain = [t.cpu().numpy() for t in plain]
    conv, descs2 = ist.decode_files_device(blobs, profile="srgb")
    assert descs == descs2
    for n, p, c in zip(names, plain, conv):
        assert np.array_equal(c.cpu().numpy(), R.convert(TAB, p)), n
    # caller tensors with padded rows: the padding is not touched
    outs, keep = [], []
    for p in plain:
        h, w = p.shape[:2]
        full = torch.full((h + 1, w + 5, 4), 0xA5, dtype=torch.uint8, device="cuda")
        keep.append(full)
        outs.append(full[:h, :w])
    ist.decode_files_device(blobs, out=outs, profile="srgb")
    for n, p, full in zip(names, plain, keep):
        h, w = p.shape[:2]
        got = full.cpu().numpy()
        assert np.array_equal(got[:h, :w], R.convert(TAB, p)), n
        assert (got[h:] == 0xA5).all() and (got[:, w:] == 0xA5).all(), n
    again, _ = ist.decode_files_device(blobs, scale=2, profile="srgb")
    half, _ = ist.decode_files_device(blobs, scale=2)
    assert all(np.array_equal(a.cpu().numpy(), R.convert(TAB, b.cpu().numpy())) for a, b in zip(again, half))


def test_decode_image_converts_jpeg_and_says_what_it_leaves():
    for n in ("jpeg 48x32 420 baseline", "jpeg 65x17 444 progressive"):
        plain = ist.decode_image(FILES[n])
        assert np.array_equal(ist.decode_image(FILES[n], profile="srgb"), R.convert(TAB, plain)), n
        half = ist.decode_image(FILES[n], scale=2)
        assert np.array_equal(ist.decode_image(FILES[n], scale=2, profile="srgb"), R.convert(TAB, half)), n
        assert np.array_equal(ist.decode_image(FILES[n]), plain)
    png = FILES["png 48x32"]                                 # decoded on the host into the caller's array: never on the device, not converted
    assert np.array_equal(ist.decode_image(png, profile="srgb"), ist.decode_image(png))


def test_thumbnails_from_files_take_the_profile():
    blobs = [FILES["jpeg 48x32 444 baseline"], FILES["png 65x17"]]
    plain = ist.thumbnails_from_files(blobs, (48, 32), mode="fit")
    conv = ist.thumbnails_from_files(blobs, (48, 32), mode="fit", profile="srgb")
    bitmaps = ist.decode_bitmaps(blobs, profile="srgb")
    want = ist.thumbnails(bitmaps, (48, 32), mode="fit")
    for b in bitmaps:
        b.close()
    assert all(np.array_equal(c, w) for c, w in zip(conv, want)) and not any(np.array_equal(c, p) for c, p in zip(conv, plain))
