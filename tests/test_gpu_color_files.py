"""opts['colorProfile'] = 'srgb' on stitch_files: the PNG decodes to the stitch of the converted bitmaps, on each way the file pipeline
brings an image into the canvas - reconstructed straight into its box (equal widths; and mode 'original', where a narrower image's
box starts at an X0 that is no multiple of 4 pixels, so its rows are not 16-byte aligned), and the band path (mode 'min')."""
import io

import numpy as np
import pytest
from PIL import Image

import icc_reference as R
import icc_writer as W
import imagestitching_amd as ist
from imagestitching_amd import _lib as L

pytestmark = pytest.mark.gpu

P3 = W.fixtures()["p3_para3"]
ADOBE = W.fixtures()["adobe_gamma"]


def _jpeg(path, w, h, icc, seed, **kw):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([(xx * 255) // (w - 1), (yy * 255) // (h - 1), ((xx + 2 * yy) * 5) % 256], -1)
    a = (a + rng.integers(-10, 10, a.shape)).clip(0, 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=92, **({"icc_profile": icc} if icc else {}), **kw)
    path.write_bytes(b.getvalue())
    return str(path)


def _expected(paths, direction, opts):
    """the stitch of the converted bitmaps: decode with profile='srgb' (pinned against the reference by test_gpu_color_decode.py), download,
    stitch the host pixels"""
    bitmaps = ist.decode_bitmaps(paths, profile="srgb")
    px = [b.download() for b in bitmaps]
    for b in bitmaps:
        b.close()
    return ist.stitch([{"width": a.shape[1], "height": a.shape[0], "data": a} for a in px], direction, opts)["data"], px


def _pil(png):
    return np.asarray(Image.open(io.BytesIO(png)).convert("RGBA"))


def test_equal_widths_are_converted_in_their_boxes_of_the_canvas(tmp_path):
    paths = [_jpeg(tmp_path / "a.jpg", 64, 40, P3, 1), _jpeg(tmp_path / "b.jpg", 64, 24, ADOBE, 2, subsampling=0), _jpeg(tmp_path / "c.jpg", 64, 33, P3, 3)]
    want, px = _expected(paths, "vertical", None)
    before, launches = L.lib.ist_debug_direct_images(), L.lib.ist_debug_color_launches()
    res = ist.stitch_files(paths, "vertical", {"colorProfile": "srgb"})
    assert L.lib.ist_debug_direct_images() - before == 3 and L.lib.ist_debug_color_launches() - launches == 3
    got = _pil(res["png"])
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(got[:40], px[0]) and np.array_equal(got[64:], px[2])
    # ... against the reference itself, from the unconverted bitmaps
    plain = _pil(ist.stitch_files(paths, "vertical")["png"])
    tabs = [R.tables(P3), R.tables(ADOBE), R.tables(P3)]
    ref = np.concatenate([R.convert(t, plain[y0:y1]) for t, (y0, y1) in zip(tabs, ((0, 40), (40, 64), (64, 97)))], 0)
    assert np.array_equal(got, ref) and not np.array_equal(got, plain)
    assert np.array_equal(_pil(ist.stitch_files(paths, "vertical", {"colorProfile": "ignore"})["png"]), plain)


def test_a_box_that_starts_between_16_byte_boundaries(tmp_path):
    paths = [_jpeg(tmp_path / "a.jpg", 64, 30, P3, 4), _jpeg(tmp_path / "n.jpg", 50, 21, P3, 5), _jpeg(tmp_path / "c.jpg", 64, 18, None, 6)]
    opts = {"mode": "original", "gap": 3}
    want, _ = _expected(paths, "vertical", opts)
    before, launches = L.lib.ist_debug_direct_images(), L.lib.ist_debug_color_launches()
    res = ist.stitch_files(paths, "vertical", dict(opts, colorProfile="srgb"))
    assert L.lib.ist_debug_direct_images() - before == 3 and L.lib.ist_debug_color_launches() - launches == 2
    got = _pil(res["png"])
    assert got.shape == want.shape == (75, 64, 4) and np.array_equal(got, want)
    assert (got[33:54, :7] == 255).all() and (got[33:54, 57:] == 255).all() and (got[30:33] == 255).all()      # the narrow image sits at X0 = 7; around it the canvas is white


def test_the_band_path(tmp_path):
    paths = [_jpeg(tmp_path / "a.jpg", 64, 30, P3, 7), _jpeg(tmp_path / "w.jpg", 96, 48, P3, 8), _jpeg(tmp_path / "c.jpg", 64, 18, ADOBE, 9, progressive=True)]
    want, _ = _expected(paths, "vertical", {"mode": "min"})
    launches = L.lib.ist_debug_color_launches()
    res = ist.stitch_files(paths, "vertical", {"mode": "min", "colorProfile": "srgb"})
    assert L.lib.ist_debug_color_launches() - launches == 3
    got = _pil(res["png"])
    assert got.shape == want.shape == (80, 64, 4) and np.array_equal(got, want)
    plain = _pil(ist.stitch_files(paths, "vertical", {"mode": "min"})["png"])
    assert not np.array_equal(got, plain)
