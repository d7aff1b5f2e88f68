"""The numpy statement of the JPEG export contract (tests/jpeg_encode_reference.py) against PIL: its quantisation tables are
libjpeg's at every quality, PIL opens its files, and they are as close to the source as PIL's own at the same settings."""
import io

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_encode_reference as R
from tests import jpeg_writer as JW

SHAPES = ((1, 1), (7, 9), (17, 33), (48, 64), (100, 150))          # (width, height)
QUALITIES = (1, 50, 90, 100)
LAYOUTS = ("420", "444")


def source(w, h):
    a = np.empty((h, w, 4), np.uint8)
    a[..., :3] = JW.photo(100 * w + h, h, w)
    a[..., 3] = 255
    return a


def dqt_segments(data):
    """the payloads of a file's DQT segments, in file order"""
    out, p = [], 2
    while p < len(data) and data[p] == 0xFF and data[p + 1] != 0xDA:
        n = int.from_bytes(data[p + 2:p + 4], "big")
        if data[p + 1] == 0xDB:
            body = data[p + 4:p + 2 + n]
            while body:                                            # (PIL puts both tables into one segment)
                out.append(bytes(body[:65]))
                body = body[65:]
        p += 2 + n
    return out


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def test_fdct_matrix_is_the_rounded_cosine():
    exact = np.array([[8192 * (np.sqrt(1 / 8) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])
    assert np.array_equal(R.T, np.round(exact).astype(np.int64))
    assert np.min(np.abs(exact - np.floor(exact) - 0.5)) > 0.028   # no entry near a rounding tie


def test_colour_stays_in_range():
    rng = np.random.default_rng(1)
    px = rng.integers(0, 256, (4096, 4), dtype=np.uint8)
    ext = np.array([[r, g, b, 0] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    for p in R.planes(np.concatenate([px, ext])[None]):
        assert p.min() >= 0 and p.max() <= 255


@pytest.mark.parametrize("quality", range(1, 101))
def test_quant_tables_are_libjpegs(quality):
    ours = R.encode(source(8, 8), quality, "444")
    b = io.BytesIO()
    Image.fromarray(source(8, 8)[..., :3]).save(b, "JPEG", quality=quality, subsampling=0)
    assert dqt_segments(ours) == dqt_segments(b.getvalue())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("w,h", SHAPES)
def test_files_open_and_match_pil_quality(w, h, quality, layout):
    src = source(w, h)
    data = R.encode(src, quality, layout)
    im = Image.open(io.BytesIO(data))
    assert im.size == (w, h) and im.mode == "RGB"
    ours = psnr(np.asarray(im), src[..., :3])
    b = io.BytesIO()
    Image.fromarray(src[..., :3]).save(b, "JPEG", quality=quality, subsampling=0 if layout == "444" else 2)
    pil = psnr(np.asarray(Image.open(io.BytesIO(b.getvalue()))), src[..., :3])
    print("%dx%d Q%d %s: reference %.2f dB, PIL %.2f dB" % (w, h, quality, layout, ours, pil))
    assert ours >= pil - 0.5


def test_restart_interval_is_one_mcu_row():
    data = R.encode(source(33, 40), 50, "420")
    at = data.index(b"\xff\xdd")
    assert int.from_bytes(data[at + 4:at + 6], "big") == 3
    assert data.count(b"\xff\xd0") >= 1 and data.endswith(b"\xff\xd9")
