"""The reduced-size JPEG decode at the C-ABI and in the Python host, CPU only: the two pure-CPU rules (ist_jpeg_scaled_size,
ist_decode_scale_fit) at their edges, bad denominators and NULLs, the entry points that need a context, and the agreement of the
header, the library's exports and the ctypes table.  (What needs a device is in tests/test_gpu_jpeg_scaled.py.)  Reference anchor: the
decoded bitmap that is smaller than the image (bmp.width against width, pages/index/index.js:1522-1523)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests import jpeg_scaled_reference as R
from tests import jpeg_writer as JW

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "imagestitch.h")
E_INVALID, E_NO_CONTEXT, E_UNSUPPORTED = -1, -4, -7
NEW = {
    "ist_jpeg_scaled_size": r"int ist_jpeg_scaled_size\(int32_t w, int32_t h, int32_t denom, int32_t\* sw, int32_t\* sh\);",
    "ist_decode_scale_fit": r"int ist_decode_scale_fit\(int32_t w, int32_t h, int32_t min_w, int32_t min_h\);",
    "ist_image_decode_rgba8_scaled": r"int ist_image_decode_rgba8_scaled\(ist_ctx\* ctx, const uint8_t\* file, int64_t len, int32_t denom, uint8_t\* out, size_t out_pitch,\s+int64_t out_rows\);",
    "ist_decode_files_device_scaled": r"int ist_decode_files_device_scaled\(ist_ctx\* ctx, const uint8_t\* const\* files, const int64_t\* lens, int n_images, const int32_t\* denom,\s+void\* const\* dst, const size_t\* dst_pitch, const int64_t\* dst_rows, ist_image_desc\* out_descs\);",
    "ist_bitmaps_decode_scaled": r"int ist_bitmaps_decode_scaled\(ist_ctx\* ctx, const uint8_t\* const\* files, const int64_t\* lens, int n, const int32_t\* denom, ist_bitmap\*\* out\);",
    "ist_debug_jpeg_scaled_launches": r"int64_t ist_debug_jpeg_scaled_launches\(void\);",
}


def _size(w, h, d):
    sw, sh = C.c_int32(-1), C.c_int32(-1)
    rc = L.lib.ist_jpeg_scaled_size(w, h, d, C.byref(sw), C.byref(sh))
    return rc, sw.value, sh.value


def test_scaled_size_at_the_edges():
    for w in (1, 7, 8, 9, 15, 16, 17, 4032, 65535):
        for h in (1, 7, 8, 9, 65535):
            for d in (1, 2, 4, 8):
                want = (-(-w // d), -(-h // d))                      # ceil(w N / 8) with N = 8 / d is ceil(w / d)
                assert want == R.scaled_size(w, h, d)
                assert _size(w, h, d) == (0,) + want, (w, h, d)
                assert ist.scaled_size(w, h, d) == want
    assert _size(1, 1, 8) == (0, 1, 1) and _size(7, 8, 8) == (0, 1, 1) and _size(9, 8, 8) == (0, 2, 1) and _size(65535, 65535, 2) == (0, 32768, 32768)


def test_scaled_size_argument_errors():
    for d in (0, 3, 5, 6, 7, 16, -1, -8):
        assert _size(10, 10, d)[0] == E_INVALID, d
    assert b"ist_jpeg_scaled_size" in L.lib.ist_last_error()
    assert _size(0, 10, 2)[0] == E_INVALID and _size(10, 0, 2)[0] == E_INVALID and _size(-4, 10, 2)[0] == E_INVALID
    one = C.c_int32(0)
    assert L.lib.ist_jpeg_scaled_size(10, 10, 2, None, C.byref(one)) == E_INVALID
    assert L.lib.ist_jpeg_scaled_size(10, 10, 2, C.byref(one), None) == E_INVALID
    with pytest.raises(ist.StitchError):
        ist.scaled_size(10, 10, 3)


def _fit_rule(w, h, mw, mh):
    for d in (8, 4, 2):
        if -(-w // d) >= mw and -(-h // d) >= mh:
            return d
    return 1


def test_scale_fit_at_the_edges_and_on_random_cases():
    fit = L.lib.ist_decode_scale_fit
    assert fit(1, 1, 1, 1) == 8                                      # ceil(1 / 8) = 1
    assert fit(7, 7, 1, 1) == 8 and fit(8, 8, 1, 1) == 8 and fit(9, 9, 2, 2) == 8 and fit(8, 8, 2, 2) == 4 and fit(7, 7, 2, 2) == 4
    assert fit(9, 9, 3, 3) == 4 and fit(9, 9, 5, 5) == 2 and fit(9, 9, 6, 5) == 1 and fit(9, 9, 10, 1) == 1      # (none qualifies: 1)
    assert fit(65535, 65535, 8192, 8192) == 8 and fit(65535, 65535, 8193, 1) == 4 and fit(65535, 1, 65535, 1) == 1
    assert fit(4032, 3024, 100, 100) == 8 and fit(4032, 3024, 1080, 100) == 2 and fit(4032, 3024, 100, 757) == 2 and fit(4032, 3024, 100, 756) == 4
    rng = np.random.default_rng(5)
    for _ in range(400):
        w, h, mw, mh = (int(v) for v in rng.integers(1, 70, 4))
        assert fit(w, h, mw, mh) == _fit_rule(w, h, mw, mh) == ist.decode_scale_fit(w, h, mw, mh), (w, h, mw, mh)


def test_scale_fit_argument_errors():
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (-3, 5, 1, 1), (5, 5, -1, 1)):
        assert L.lib.ist_decode_scale_fit(*bad) == E_INVALID, bad
    assert b"ist_decode_scale_fit" in L.lib.ist_last_error()
    with pytest.raises(ist.StitchError):
        ist.decode_scale_fit(0, 1, 1, 1)


def _one_file():
    data = JW.size_cases("420")[20]["data"]
    return data, (C.c_char_p * 1)(data), (C.c_int64 * 1)(len(data))


def test_the_entry_points_need_a_context():
    data, files, lens = _one_file()
    out = np.zeros((32, 32, 4), np.uint8)
    assert L.lib.ist_image_decode_rgba8_scaled(None, data, len(data), 2, out.ctypes.data, 128, 32) == E_NO_CONTEXT
    assert b"\xe6\x97\xa0\xe6\xb3\x95" in L.lib.ist_last_error()
    bm = (C.c_void_p * 1)()
    den = (C.c_int32 * 1)(2)
    assert L.lib.ist_bitmaps_decode_scaled(None, files, lens, 1, den, bm) == E_NO_CONTEXT
    dst, pitch, rows = (C.c_void_p * 1)(), (C.c_size_t * 1)(), (C.c_int64 * 1)()
    assert L.lib.ist_decode_files_device_scaled(None, files, lens, 1, den, dst, pitch, rows, None) == E_NO_CONTEXT
    assert L.lib.ist_decode_files_device_scaled(None, files, lens, 1, None, dst, pitch, rows, None) == E_NO_CONTEXT


def test_bad_denominators_and_nulls_behind_a_context():
    """the checks that come after the context and before any device work (the context is a non-NULL pointer that is never followed, as
    in tests/test_bitmap_abi.py)"""
    data, files, lens = _one_file()
    fake = C.c_void_p(8)
    bm = (C.c_void_p * 1)()
    assert L.lib.ist_bitmaps_decode_scaled(fake, None, None, 0, None, None) == 1                    # IST_NOTHING_TO_DO
    assert L.lib.ist_bitmaps_decode_scaled(fake, None, lens, 1, None, bm) == E_INVALID
    assert L.lib.ist_bitmaps_decode_scaled(fake, files, lens, 1, None, None) == E_INVALID
    many = (C.c_char_p * 129)(*[data] * 129)
    assert L.lib.ist_bitmaps_decode_scaled(fake, many, (C.c_int64 * 129)(*[len(data)] * 129), 129, None, (C.c_void_p * 129)()) == E_UNSUPPORTED
    dst, pitch, rows = (C.c_void_p * 1)(), (C.c_size_t * 1)(), (C.c_int64 * 1)()
    for d in (0, 3, 16, -2):
        den = (C.c_int32 * 1)(d)
        assert L.lib.ist_bitmaps_decode_scaled(fake, files, lens, 1, den, bm) == E_INVALID, d
        msg = L.lib.ist_last_error()
        assert b"image 0" in msg and str(d).encode() in msg, msg
        assert not bm[0]
        assert L.lib.ist_decode_files_device_scaled(fake, files, lens, 1, den, dst, pitch, rows, None) == E_INVALID, d
        assert b"image 0" in L.lib.ist_last_error()
        assert L.lib.ist_image_decode_rgba8_scaled(fake, data, len(data), d, None, 0, 0) == E_INVALID, d
    assert L.lib.ist_decode_files_device_scaled(fake, files, lens, 1, None, None, pitch, rows, None) == E_INVALID


def test_the_python_host_checks_scale_before_it_asks_for_a_device(monkeypatch):
    import sys
    S = sys.modules["imagestitching_amd.stitch"]
    data, _, _ = _one_file()

    def no_device(*a, **k):
        raise AssertionError("asked for a context")
    for bad in (0, 3, [2, 4], "2x"):
        with pytest.raises((ist.StitchError, ValueError)):
            S._scales(bad, [data], "decode_bitmaps")
    assert S._scales(4, [data, data], "t")[0] == [4, 4] and S._scales(1, [data], "t")[1] is None and S._scales([1, 8], [data, data], "t")[0] == [1, 8]
    monkeypatch.setattr(S, "_ctx", no_device)
    with pytest.raises(ist.StitchError) as e:
        ist.decode_image(data, scale=5)
    assert e.value.code == E_INVALID and "image 0" in str(e.value)
    with pytest.raises(ValueError):
        ist.decode_files_device([data], scale=[1, 2])
    assert ist.thumbnails_from_files([], (10, 10)) == []


def test_the_header_the_exports_and_the_ctypes_table_agree():
    text = open(HEADER, encoding="utf-8").read()
    table = {name: (res, args) for name, res, args in L.SYMBOLS}
    for name, decl in NEW.items():
        assert re.search(r"IST_API\s+" + decl, text), name
        assert name in table and hasattr(L.lib, name), name
    i32, p32, vp = C.c_int32, C.POINTER(C.c_int32), C.c_void_p
    assert table["ist_jpeg_scaled_size"] == (C.c_int, [i32, i32, i32, p32, p32])
    assert table["ist_decode_scale_fit"] == (C.c_int, [i32, i32, i32, i32])
    assert table["ist_debug_jpeg_scaled_launches"] == (C.c_int64, [])
    # the scaled twins take their unscaled twins' arguments with the denominator(s) put in where the header puts them
    a = list(table["ist_image_decode_rgba8"][1])
    assert table["ist_image_decode_rgba8_scaled"][1] == a[:3] + [i32] + a[3:]
    a = list(table["ist_decode_files_device"][1])
    assert table["ist_decode_files_device_scaled"][1] == a[:4] + [p32] + a[4:]
    a = list(table["ist_bitmaps_decode"][1])
    assert table["ist_bitmaps_decode_scaled"][1] == a[:4] + [p32] + a[4:]
    assert L.lib.ist_debug_jpeg_scaled_launches() == 0 or L.lib.ist_device_count() > 0
    for name in ("scaled_size", "decode_scale_fit", "thumbnails_from_files"):
        assert name in ist.__all__ and callable(getattr(ist, name))
