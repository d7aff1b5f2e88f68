"""The numpy statement of the reduced-size decode contract (tests/jpeg_scaled_reference.py, include/imagestitch.h) against Pillow's
Image.draft (libjpeg-turbo's scale_num / scale_denom), byte for byte: seven layouts x seven sizes x d in {2, 4, 8}, and d = 1 against a
plain Pillow decode.  Both sides of every size are >= 8, so Pillow takes every requested scale and no case is skipped.  CPU only."""
import io

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_scaled_reference as R
from tests import jpeg_writer as jw

LAYOUTS = ("grey", "444", "420", "422", "440", "rgb", "rgb420")
SIZES = ((16, 16), (17, 15), (33, 47), (61, 45), (64, 40), (129, 70), (1000, 700))


def _file(layout, w, h):
    f = jw.frame_from_pixels(jw.photo(w * 100 + h, h, w), layout, 0.5)
    return f, jw.write_jpeg(f, marker="jfif" if f.colour != "rgb" else "adobe0")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_contract_is_pillows_draft_byte_for_byte(layout, size):
    w, h = size
    f, data = _file(layout, w, h)
    full = np.asarray(Image.open(io.BytesIO(data))).astype(np.int64)
    assert np.array_equal(R.decode(f, 1), full), "d = 1 is the plain decode"
    for d in (2, 4, 8):
        n = 8 // d
        im = Image.open(io.BytesIO(data))
        im.draft(im.mode, (w * n // 8, h * n // 8))
        assert im.size == R.scaled_size(w, h, d), (d, im.size)
        ref = np.asarray(im).astype(np.int64)
        mine = R.decode(f, d)
        assert mine.shape == ref.shape, (d, mine.shape, ref.shape)
        assert np.array_equal(mine, ref), (layout, size, d, int(np.abs(mine - ref).max()), int((mine != ref).sum()))


def test_the_idct_sizes_and_upsampling_factors_of_every_layout():
    """what the contract says in words: 4:2:0 chroma at 2 N without upsampling, 4:2:2 keeps ux = 2, 4:4:0 keeps uy = 2"""
    for layout, want in (("420", {2: (8, 1, 1), 4: (4, 1, 1), 8: (2, 1, 1)}), ("422", {2: (4, 2, 1), 4: (2, 2, 1), 8: (1, 2, 1)}),
                         ("440", {2: (4, 1, 2), 4: (2, 1, 2), 8: (1, 1, 2)}), ("444", {2: (4, 1, 1), 4: (2, 1, 1), 8: (1, 1, 1)})):
        f = jw.frame_from_pixels(jw.photo(1, 16, 16), layout, 0.5)
        for d, (s, ux, uy) in want.items():
            g = R.geometry(f, d)
            assert g[0][0] == 8 // d and g[0][3:] == (1, 1), (layout, d, g)
            assert (g[1][0], g[1][3], g[1][4]) == (s, ux, uy) and g[1] == g[2], (layout, d, g)
    assert [R.scaled_size(w, 9, d) for w, d in ((1, 8), (7, 2), (8, 8), (9, 8), (65535, 4))] == [(1, 2), (4, 5), (1, 2), (2, 2), (16384, 3)]


def test_the_arithmetic_is_32_bit():
    assert int(R.descale(np.int64((1 << 31) - 1), 3)) == -(1 << 28)           # the rounding term wraps
    assert int(R.descale(np.int64(-5), 1)) == -2 and int(R.descale(np.int64(5), 1)) == 3      # arithmetic shift
