"""Row views of resident bitmaps (ist_bitmap_rows; Bitmap.rows): a view is the parent's rows where they are - every call that takes a
bitmap gives, for a view, byte for byte what it gives for a bitmap uploaded from the same rows - and it costs and leaks nothing."""
import ctypes as C
import gc
import io

import numpy as np
import pytest
from PIL import Image

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests import util as U

pytestmark = pytest.mark.gpu


def _live():
    v = (C.c_int64 * 4)()
    L.lib.ist_debug_live_handles(v)
    return list(v)


# (width, height, y0, rows): odd widths put row y0 at an address that is only 4-byte aligned; the last case ends at the parent's last row
CASES = [(33, 40, 7, 21), (130, 75, 1, 74), (64, 50, 0, 50), (5, 30, 11, 19), (611, 90, 13, 60)]


@pytest.mark.parametrize("w,h,y0,rows", CASES)
def test_a_view_downloads_as_the_slice(w, h, y0, rows):
    a = U.rand_image(w + h, h, w, opaque=False)
    b = ist.upload_bitmap({"width": w, "height": h, "data": a, "fileSize": 999, "opaque": False})
    held = L.lib.ist_debug_bitmap_bytes()
    allocs = L.lib.ist_debug_device_allocs()
    v = b.rows(y0, rows)
    assert (v.width, v.height, v.shape, v.orientation, v.file_size, v.opaque) == (w, rows, (rows, w, 4), 1, 0, False)
    assert L.lib.ist_debug_bitmap_bytes() == held and L.lib.ist_debug_device_allocs() == allocs      # nothing is copied or counted
    assert np.array_equal(v.download(), a[y0:y0 + rows])
    vv = v.rows(2, rows - 3)                                   # a view of a view
    assert np.array_equal(vv.download(), a[y0 + 2:y0 + rows - 1])
    for x in (vv, v, b):
        x.close()


def test_views_stitch_preview_and_thumbnail_like_uploads_of_the_slices():
    shapes = [(611, 90, 13, 60), (611, 70, 0, 33), (611, 81, 40, 41)]
    arrays = [U.smooth_image(k, h, w, opaque=(k != 1)) for k, (w, h, _, _) in enumerate(shapes)]
    parents = [ist.upload_bitmap(a) for a in arrays]
    views = [p.rows(y0, rows) for p, (_, _, y0, rows) in zip(parents, shapes)]
    twins = [ist.upload_bitmap(np.ascontiguousarray(a[y0:y0 + rows])) for a, (_, _, y0, rows) in zip(arrays, shapes)]
    for direction, opts in (("vertical", {"gap": 3}), ("horizontal", {"mode": "max"}), ("vertical", {"filter": "area", "maxSide": 300, "platform": "ios"})):
        got, want = ist.stitch(views, direction, opts), ist.stitch(twins, direction, opts)
        assert (got["width"], got["height"]) == (want["width"], want["height"])
        assert np.array_equal(got["data"], want["data"]), (direction, opts)
    got, want = ist.stitch_png(views, "vertical", {"preview": (120, 160)}), ist.stitch_png(twins, "vertical", {"preview": (120, 160)})
    assert got["png"] == want["png"] and np.array_equal(got["preview"], want["preview"])
    assert ist.stitch_jpeg(views, "vertical", {"quality": 85})["jpeg"] == ist.stitch_jpeg(twins, "vertical", {"quality": 85})["jpeg"]
    for v, t in zip(views, twins):
        assert np.array_equal(v.preview(50, 20), t.preview(50, 20))
    for mode in ("fill", "fit"):
        for g, w_ in zip(ist.thumbnails(views, (48, 32), mode), ist.thumbnails(twins, (48, 32), mode)):
            assert np.array_equal(g, w_), mode
    for x in views + twins + parents:
        x.close()


def test_the_parent_may_go_first_and_everything_comes_back():
    gc.collect()
    bytes0, live0 = L.lib.ist_debug_bitmap_bytes(), _live()
    a = U.rand_image(3, 64, 100, opaque=True)
    b = ist.upload_bitmap(a)
    held = L.lib.ist_debug_bitmap_bytes()
    assert held > bytes0
    v = b.rows(10, 40)
    vv = v.rows(5, 5)
    b.close()                                                  # the creator's reference goes: the views keep the block
    assert L.lib.ist_debug_bitmap_bytes() == held
    assert np.array_equal(v.download(), a[10:50])
    v.close()
    assert L.lib.ist_debug_bitmap_bytes() == held              # the view of the view holds the parent itself
    assert np.array_equal(vv.download(), a[15:20])
    out = ist.stitch([vv, vv], "vertical")
    assert np.array_equal(out["data"], np.concatenate([a[15:20], a[15:20]]))
    del out
    vv.close()
    gc.collect()
    assert L.lib.ist_debug_bitmap_bytes() == bytes0
    now = _live()
    assert now[0] <= live0[0] + 2 and now[2:] == live0[2:]     # (device blocks: at most the context's grow-only stitch scratch is new)
    # the other order: views first
    b = ist.upload_bitmap(a)
    v = b.rows(0, 64)
    v.close()
    b.close()
    assert L.lib.ist_debug_bitmap_bytes() == bytes0 and _live() == now


def test_refusals():
    a = U.rand_image(4, 20, 16, opaque=True)
    b = ist.upload_bitmap(a)
    for y0, rows in ((-1, 5), (0, 0), (0, 21), (20, 1), (15, 6)):
        with pytest.raises(ist.StitchError) as e:
            b.rows(y0, rows)
        assert e.value.code == -1
    turned = ist.upload_bitmap({"width": 16, "height": 20, "data": a, "orientation": 3})
    with pytest.raises(ist.StitchError) as e:
        turned.rows(0, 5)
    assert e.value.code == -7 and "orientation" in str(e.value)
    buf = io.BytesIO()
    Image.fromarray(U.smooth_image(1, 64, 64)[..., :3]).save(buf, "JPEG", quality=90)
    small = ist.decode_bitmaps([buf.getvalue()], scale=2)[0]
    assert small.shape == (32, 32, 4)
    with pytest.raises(ist.StitchError) as e:
        small.rows(0, 5)
    assert e.value.code == -7 and "reduced scale" in str(e.value)
    b.close()
    with pytest.raises(ValueError):
        b.rows(0, 5)                                           # a closed bitmap
    for x in (turned, small):
        x.close()
