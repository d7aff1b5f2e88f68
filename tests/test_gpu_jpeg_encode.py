"""The JPEG export on the GPU: every file equals tests/jpeg_encode_reference.py byte for byte.

Shapes are the smallest that reach each thing that can go wrong: partial MCUs on both axes, an interval longer than a batch of the
entropy kernel, more than eight intervals (RSTn wraps), more than one slab, a pitched canvas.  Contents reach long codes and 0xFF
stuffing (noise), EOB and ZRL (a photo at quality 50), DC differences of category 11 (black and white blocks), all-EOB blocks (a
constant)."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import jpeg_encode_reference as R
from tests import jpeg_writer as JW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITIES = (1, 50, 90, 100)
LAYOUTS = ("420", "444")


@pytest.fixture(scope="module")
def ist():
    import imagestitching_amd
    return imagestitching_amd


def photo(w, h, seed=0, alpha=255):
    a = np.empty((h, w, 4), np.uint8)
    a[..., :3] = JW.photo(1000 * w + h + seed, h, w)
    a[..., 3] = alpha
    return a


def noise(w, h, seed=5):
    a = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    a[..., 3] = 255
    return a


def checker(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    v = ((((yy >> 3) + (xx >> 3)) & 1) * 255).astype(np.uint8)
    return np.stack([v, v, v, np.full_like(v, 255)], -1)


def first_difference(got, want):
    n = min(len(got), len(want))
    d = np.nonzero(np.frombuffer(got[:n], np.uint8) != np.frombuffer(want[:n], np.uint8))[0]
    return "lengths %d / %d, first difference at byte %s" % (len(got), len(want), d[0] if len(d) else "none")


def check(ist, a, quality, layout):
    got, want = ist.encode_jpeg(a, quality, layout), R.encode(a, quality, layout)
    assert got == want, "%dx%d Q%d %s: %s" % (a.shape[1], a.shape[0], quality, layout, first_difference(got, want))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("w,h", ((1, 1), (7, 9), (16, 16), (17, 33)))
def test_partial_mcus(ist, w, h, layout):
    for q in QUALITIES:
        check(ist, photo(w, h), q, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_an_interval_longer_than_a_batch(ist, layout):
    """4805 x 19: 301 MCUs of 6 blocks = 1806 blocks in one interval of the 4:2:0 file (1803 in 4:4:4): eight batches of 256"""
    a = photo(4805, 19)
    for q in QUALITIES:
        check(ist, a, q, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_rst_markers_wrap(ist, layout):
    a = photo(33, 170)
    want = R.encode(a, 50, layout)
    assert want.count(b"\xff\xd7") >= 1 and want.count(b"\xff\xd0") >= 2        # 11 / 22 intervals: RST0 comes round again
    for q in QUALITIES:
        check(ist, a, q, layout)


def test_slabs(tmp_path):
    """33 x 700 with 13 MCU rows per slab: 4 slabs in 4:2:0 (44 MCU rows), 7 in 4:4:4 (88).  The override is read once, in tuning
    mode, so the encodes run in a process of their own."""
    code = """
import sys
sys.path.insert(0, %r)
import numpy as np
import imagestitching_amd as ist
from imagestitching_amd import _lib as L
a = np.load(sys.argv[1])
before = L.lib.ist_debug_jpeg_encode_launches()
out = {}
for q in (1, 50, 90, 100):
    for layout in ("420", "444"):
        out["%%d_%%s" %% (q, layout)] = np.frombuffer(ist.encode_jpeg(a, q, layout), np.uint8)
print("launches", L.lib.ist_debug_jpeg_encode_launches() - before)
np.savez(sys.argv[2], **out)
""" % (ROOT,)
    a = photo(33, 700)
    np.save(tmp_path / "a.npy", a)
    env = dict(os.environ, IST_TUNING="1", IST_JPEG_ENC_ROWS="13")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "a.npy"), str(tmp_path / "out.npz")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "launches %d" % (4 * (4 + 7)) in r.stdout, r.stdout
    got = np.load(tmp_path / "out.npz")
    for q in QUALITIES:
        for layout in LAYOUTS:
            g, want = got["%d_%s" % (q, layout)].tobytes(), R.encode(a, q, layout)
            assert g == want, "Q%d %s: %s" % (q, layout, first_difference(g, want))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_pitched_canvas_on_the_device(ist, layout):
    import torch
    a = photo(37, 21)
    wide = torch.full((21, 37 + 13, 4), 0xEE, dtype=torch.uint8, device="cuda")
    wide[:, :37] = torch.from_numpy(a).cuda()
    canvas = wide[:, :37]
    assert canvas.stride(0) == 4 * (37 + 13)
    for q in QUALITIES:
        t, n = ist.encode_jpeg_device(canvas, q, layout)
        torch.cuda.synchronize()
        got, want = t.cpu().numpy().tobytes(), R.encode(a, q, layout)
        assert n == len(want) and got == want, "Q%d: %s" % (q, first_difference(got, want))


def test_alpha_is_not_read(ist):
    a = photo(23, 18)
    b = a.copy()
    b[..., 3] = np.random.default_rng(3).integers(0, 256, b.shape[:2], dtype=np.uint8)
    for layout in LAYOUTS:
        assert ist.encode_jpeg(a, 90, layout) == ist.encode_jpeg(b, 90, layout) == R.encode(a, 90, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_noise_long_codes_and_stuffing(ist, layout):
    a = noise(100, 150)
    assert b"\xff\x00" in R.encode(a, 100, layout)
    check(ist, a, 100, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_photo_eob_and_zrl(ist, layout):
    a = photo(100, 150)
    assert R.max_zero_run(R.frame(a, 50, layout)) >= 16
    check(ist, a, 50, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_black_and_white_blocks_dc_category_11(ist, layout):
    a = checker(48, 40)
    dc = R.frame(a, 100, layout).comps[0]["coef"][..., 0]
    assert np.abs(np.diff(dc, axis=1)).max() >= 1024
    check(ist, a, 100, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_constant_canvas(ist, layout):
    a = np.full((40, 50, 4), 200, np.uint8)
    for q in QUALITIES:
        check(ist, a, q, layout)


def test_our_files_take_the_gpu_huffman_decoder(ist):
    """one interleaved scan, two DC + two AC tables, intervals that tile the frame: the file pipeline's GPU entropy decoder takes the
    file, and the pixels are PIL's"""
    from PIL import Image
    from imagestitching_amd import _lib as L
    a = photo(150, 100)
    for layout in LAYOUTS:
        data = ist.encode_jpeg(a, 90, layout)
        want = np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))
        before = L.lib.ist_debug_gpu_entropy_files()
        tensors, _ = ist.decode_files_device([data])
        assert L.lib.ist_debug_gpu_entropy_files() == before + 1
        assert np.array_equal(tensors[0].cpu().numpy(), want)
        assert np.array_equal(ist.decode_image(data), want)


STITCHES = (("vertical", {}), ("horizontal", {}), ("vertical", {"gap": 5}), ("horizontal", {"gap": 3, "filter": "bilinear"}),
            ("vertical", {"filter": "bilinear", "mode": "max"}))


def three_images():
    return [photo(w, h, seed=k) for k, (w, h) in enumerate(((40, 30), (33, 47), (52, 21)))]


@pytest.mark.parametrize("direction,opts", STITCHES)
def test_stitch_jpeg_is_encode_jpeg_of_the_canvas(ist, direction, opts):
    imgs = three_images()
    canvas = ist.stitch(imgs, direction, opts)
    for q, layout in ((90, "420"), (50, "444")):
        res = ist.stitch_jpeg(imgs, direction, dict(opts, quality=q, subsampling=layout))
        assert (res["width"], res["height"]) == (canvas["width"], canvas["height"])
        assert res["jpeg"] == ist.encode_jpeg(canvas["data"], q, layout) == R.encode(canvas["data"], q, layout)


@pytest.mark.parametrize("direction,opts", STITCHES)
def test_stitch_jpeg_from_bitmaps(ist, direction, opts):
    imgs = three_images()
    bms = [ist.upload_bitmap(a) for a in imgs]
    try:
        canvas = ist.stitch(imgs, direction, opts)
        res = ist.stitch_jpeg(bms, direction, dict(opts, quality=75))
        assert res["jpeg"] == R.encode(canvas["data"], 75, "420")
    finally:
        for b in bms:
            b.close()


def test_steady_state_allocates_nothing_and_launches_are_counted(ist):
    import torch
    from imagestitching_amd import _lib as L
    a = photo(64, 48)
    canvas = torch.from_numpy(a).cuda()
    imgs = three_images()
    ist.encode_jpeg(a, 90, "420")
    ist.encode_jpeg_device(canvas, 90, "420")
    ist.stitch_jpeg(imgs, "vertical")
    allocs, launches = L.lib.ist_debug_device_allocs(), L.lib.ist_debug_jpeg_encode_launches()
    out = torch.empty(int(L.lib.ist_jpeg_bound(64, 48, 1)) + 16, dtype=torch.uint8, device="cuda")
    ist.encode_jpeg(a, 90, "420")
    ist.encode_jpeg_device(canvas, 90, "420", out=out)
    ist.stitch_jpeg(imgs, "vertical")
    assert L.lib.ist_debug_device_allocs() == allocs
    assert L.lib.ist_debug_jpeg_encode_launches() == launches + 3


def test_a_65536_wide_canvas_is_refused_before_any_launch(ist):
    import torch
    from imagestitching_amd import _lib as L
    canvas = torch.zeros((1, 65536, 4), dtype=torch.uint8, device="cuda")
    before = L.lib.ist_debug_jpeg_encode_launches()
    with pytest.raises(ist.StitchError) as e:
        ist.encode_jpeg_device(canvas)
    assert e.value.code == -7 and "width" in e.value.reason
    with pytest.raises(ist.StitchError) as e:
        ist.encode_jpeg(np.zeros((65536, 1, 4), np.uint8))
    assert e.value.code == -7 and "height" in e.value.reason
    assert L.lib.ist_debug_jpeg_encode_launches() == before
