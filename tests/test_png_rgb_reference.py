"""The CPU statement of the RGB PNG export (tests/png_rgb_reference.py) must be right before it judges the kernel
(tests/test_gpu_png_rgb.py): zlib inflates its streams to the Paeth-filtered colour bytes, un-filtering them gives canvas[..., :3],
PIL reads its files as mode RGB, every input reaches the form of the chunk grid it was built for, and the inputs can tell the grid
from a near miss.  Reference anchor of the export: wx.canvasToTempFilePath({fileType: 'png'}) (utils/canvas.js:205-242) on a canvas
that the plan's white fillRect has made opaque."""
import io
import zlib

import numpy as np
import pytest

from tests import png_deflate_reference as R
from tests import png_rgb_cases as K
from tests import png_rgb_reference as G
from tests import png_stream_cases as C

NAMES = [name for name, _ in K.all_cases()]


@pytest.mark.parametrize("name", NAMES)
def test_stream_inflates_unfilters_and_the_file_decodes_as_rgb(name):
    from PIL import Image
    a = dict(K.all_cases())[name]
    rep = K.report(name, a)
    h, w = a.shape[:2]
    filt = G.filtered_rows_rgb(a)
    assert rep.filtered == filt.tobytes() and len(rep.filtered) == h * (3 * w + 1), name
    assert zlib.decompress(rep.stream) == rep.filtered, name
    assert sum(c.nbytes for c in rep.chunks) + 9 == len(rep.stream) and all(c.nbytes % 16 == 0 for c in rep.chunks), name
    assert np.array_equal(G.unfilter_rows_rgb(filt, a[..., :3]), a[..., :3]), name
    png = G.file_bytes_rgb(a, rep.stream)
    assert png.index(b"IDAT") + 4 == 64 and png[25] == 2 and png[24] == 8, name
    im = Image.open(io.BytesIO(png))
    assert im.mode == "RGB" and im.size == (w, h), name
    assert np.array_equal(np.asarray(im), a[..., :3]), name


def test_paeth_filter_against_a_scalar_statement():
    """PNG specification 9.4, byte by byte with a distance of 3 bytes between neighbours, on a small canvas with ties"""
    a = C.noise(3, 7, 9)
    a[2:4, 3:6] = a[1, 2]
    want = bytearray()
    for y in range(7):
        want.append(4)
        for x in range(9):
            for ch in range(3):
                left = int(a[y, x - 1, ch]) if x else 0
                up = int(a[y - 1, x, ch]) if y else 0
                ul = int(a[y - 1, x - 1, ch]) if x and y else 0
                p = left + up - ul
                pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
                pred = left if pa <= pb and pa <= pc else (up if pb <= pc else ul)
                want.append((int(a[y, x, ch]) - pred) & 255)
    assert G.filtered_rows_rgb(a).tobytes() == bytes(want)


def test_inputs_reach_their_regimes():
    K.check_regimes()
    assert R.host_slabs(800) == [768, 32]


def test_grid_numbers_are_the_grids():
    for w, h in K.SHAPES + K.BOUNDARY_SHAPES:
        n, rpc, ppr, px = G.grid_numbers_rgb(w, h)
        cells = G.make_grid_rgb(w, h)
        assert len(cells) == n and (ppr == 0) == (rpc > 0)
        assert max(c[1] for c in cells) == (min(rpc, h) if rpc else 1) and max(c[3] for c in cells) == (w if rpc else px)
        n4, rpc4, ppr4, px4 = G.grid_numbers_rgba(w, h)
        cells4 = R.make_grid(w, h)
        assert len(cells4) == n4 and max(c[3] for c in cells4) == (w if rpc4 else px4)
        assert n <= n4, (w, h)                                        # an RGB canvas never has more chunks than the RGBA one


def test_alpha_is_not_part_of_the_file():
    for name, a in K.shape_cases():
        if "random alpha" in name:
            assert len(np.unique(a[..., 3])) > 1 or a.shape[:2] == (1, 1)
            assert G.file_bytes_rgb(a, K.report(name, a).stream) == G.file_bytes_rgb(K.opaque(a)), name


# The 3 x 5 canvases: one stored chunk either way, 2 + 5 + 50 = 57 bytes against 2 + 5 + 65 = 72, and the pad rule (blocks of 5 bytes
# up to a multiple of 16) takes both to 112: eleven pad blocks against eight.  The framing of the reference alone, whatever the
# encoder does; these two are left out of the assertion BY NAME and their equality is asserted instead.
NOT_SHORTER = {"rgb photo 3x5, random alpha": (121, 121), "rgb flat 3x5": (121, 121)}


def test_rgb_stream_is_shorter_than_the_rgba_stream():
    """on every input but the two above, the 1 x 1 canvas included (16 + 9 bytes against 32 + 9: one pad block against four); and
    against the RGBA stream of the OPAQUE canvas too, which is the file a caller has today"""
    assert set(NOT_SHORTER) <= {name for name, _ in K.all_cases()}
    for name, a in K.all_cases():
        rgb, rgba, rgba_opaque = len(K.report(name, a).stream), len(R.encode(a).stream), len(R.encode(K.opaque(a)).stream)
        if name in NOT_SHORTER:
            assert (rgb, rgba_opaque) == NOT_SHORTER[name] and rgba >= rgb, (name, rgb, rgba, rgba_opaque)
        else:
            assert rgb < rgba_opaque <= rgba, (name, rgb, rgba, rgba_opaque)


def test_inputs_tell_the_grid_from_a_near_miss():
    """Pieces of 4095 pixels are told apart by 5462 x 2, and so is the whole RGBA grid (rows counted as 4 w + 1 bytes AND pieces of
    4095 pixels).  Rows counted as 4 w + 1 bytes with the RGB piece are NOT told apart by it - 16387 and 21849 bytes are both longer
    than a chunk, so both grids cut the same pieces - but by the shapes where the count decides how many rows share a chunk: 100 x 130
    (40 rows against 54) and 2730 x 5 (one row against two).  Either way the bent grid still gives a valid stream of the same filtered
    bytes."""
    cases = {a.shape[:2][::-1]: (name, a) for name, a in K.shape_cases() if "photo" in name}

    def differs(shape, **bent):
        name, a = cases[shape]
        w, h = shape
        true = K.report(name, a)
        other = G.encode_rgb(a, G.make_grid_rgb(w, h, **bent))
        assert zlib.decompress(other.stream) == true.filtered, name
        return other.stream != true.stream

    assert differs((5462, 2), piece_px=4095)
    assert differs((5462, 2), piece_px=4095, row_bytes=4 * 5462 + 1)
    assert not differs((5462, 2), row_bytes=4 * 5462 + 1)
    told = [s for s in K.SHAPES if differs(s, row_bytes=4 * s[0] + 1)]
    assert told == [(100, 130), (2730, 5)], told
