"""The colour conversion kernel (csrc/ist_color.hip) through convert_color_device, byte for byte against tests/icc_reference.py: every
way a row can be cut at its 16-byte boundaries (widths around the group and the workgroup sizes, base pointers 0 / 4 / 8 / 12 bytes off
a boundary, dense and padded pitches), with every byte around the box poisoned and required to stay; every code of every channel;
the corners of the cube, where P3 clips on both sides; alpha; identity and unsupported tables."""
import numpy as np
import pytest
import torch

import icc_reference as R
import icc_writer as W
import imagestitching_amd as ist
from imagestitching_amd import _lib as L

pytestmark = pytest.mark.gpu

P3 = W.fixtures()["p3_para3"]
TAB = R.tables(P3)
GUARD = 256                                   # poisoned bytes in front of and behind the box's rows


def _boxed(rng, w, h, extra, off):
    """a poisoned flat buffer and the h x w x 4 view of it whose first byte sits `off` bytes behind a 16-byte boundary, rows
    4 w + extra bytes apart; the pixels of the view are random"""
    pitch = 4 * w + extra
    flat = torch.from_numpy(rng.integers(0, 256, GUARD + off + pitch * h + GUARD, dtype=np.uint8)).cuda()
    assert flat.data_ptr() % 16 == 0
    view = torch.as_strided(flat, (h, w, 4), (pitch, 4, 1), GUARD + off)
    assert view.data_ptr() % 16 == off
    return flat, view


@pytest.mark.parametrize("w", [1, 3, 4, 5, 63, 64, 65, 257, 1021, 1030])
def test_every_row_cut_and_nothing_outside_the_box(w):
    rng = np.random.default_rng(w)
    cases = []
    for h in (1, 3) if w <= 257 else (33,):                 # (33 rows: three row bands; 1030 pixels: a second column of workgroups)
        for extra in (0, 48):
            for off in (0, 4, 8, 12):
                flat, view = _boxed(rng, w, h, extra, off)
                before = flat.cpu().numpy().copy()
                ist.convert_color_device(view, P3)
                cases.append((h, extra, off, flat, view, before))
    torch.cuda.synchronize()
    for h, extra, off, flat, view, before in cases:
        want = torch.from_numpy(before.copy())
        box = torch.as_strided(want, (h, w, 4), (4 * w + extra, 4, 1), GUARD + off)
        box.copy_(torch.from_numpy(R.convert(TAB, box.numpy().copy())))
        assert np.array_equal(flat.cpu().numpy(), want.numpy()), (w, h, extra, off)


def test_every_code_of_every_channel():
    yy, xx = np.mgrid[0:256, 0:256]
    for planes in ((xx, yy, (xx + yy) % 256), (yy, (xx * 7 + yy) % 256, xx), (255 - xx, xx, yy)):
        a = np.stack(list(planes) + [(xx ^ yy)], -1).astype(np.uint8)
        assert all(len(np.unique(a[..., c])) == 256 for c in range(3))
        t = torch.from_numpy(a).cuda()
        ist.convert_color_device(t, P3)
        assert np.array_equal(t.cpu().numpy(), R.convert(TAB, a))


def test_the_corners_of_the_cube_clip_and_alpha_is_copied():
    rng = np.random.default_rng(8)
    corners = np.array([[r, g, b, 0] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    a = np.concatenate([corners, rng.integers(0, 256, (56, 4), dtype=np.uint8)]).reshape(4, 16, 4)
    a[..., 3] = rng.integers(0, 256, (4, 16), dtype=np.uint8)
    t = torch.from_numpy(a).cuda()
    ist.convert_color_device(t, P3)
    got = t.cpu().numpy()
    assert np.array_equal(got, R.convert(TAB, a)) and np.array_equal(got[..., 3], a[..., 3])
    red = got.reshape(-1, 4)[4]                              # P3 (255, 0, 0): outside sRGB on both sides
    assert a.reshape(-1, 4)[4, :3].tolist() == [255, 0, 0] and red[0] == 255 and red[1] == 0
    assert got.reshape(-1, 4)[0, :3].tolist() == [0, 0, 0] and got.reshape(-1, 4)[7, :3].tolist() == [255, 255, 255]


@pytest.mark.parametrize("name", ["adobe_gamma", "p3_gamma18", "p3_para1", "p3_para2", "p3_curv0"])
def test_other_profiles(name):
    icc = W.fixtures()[name]
    a = np.random.default_rng(3).integers(0, 256, (37, 129, 4), dtype=np.uint8)
    t = torch.from_numpy(a).cuda()
    ist.convert_color_device(t, icc)
    assert np.array_equal(t.cpu().numpy(), R.convert(R.tables(icc), a))


def test_identity_tables_launch_nothing_and_unsupported_tables_are_refused():
    a = np.random.default_rng(4).integers(0, 256, (9, 33, 4), dtype=np.uint8)
    t = torch.from_numpy(a).cuda()
    before = L.lib.ist_debug_color_launches()
    ist.convert_color_device(t, W.fixtures()["srgb_para3"])
    assert L.lib.ist_debug_color_launches() == before and np.array_equal(t.cpu().numpy(), a)
    with pytest.raises(ist.StitchError) as e:
        ist.convert_color_device(t, W.profile(W.P3, W.para(0, 2.2), space=b"GRAY"))
    assert e.value.code == -1 and np.array_equal(t.cpu().numpy(), a)
    ist.convert_color_device(t, P3)
    assert L.lib.ist_debug_color_launches() == before + 1


def test_argument_errors_on_the_device():
    import ctypes as C
    import sys
    S = sys.modules["imagestitching_amd.stitch"]             # (the package's `stitch` attribute is the function)
    t = torch.zeros((4, 8, 4), dtype=torch.uint8, device="cuda")
    tab = S._icc_tables(P3)
    ctx = S._ctx(0)
    call = L.lib.ist_color_convert_device
    assert call(ctx, None, 32, 8, 4, C.byref(tab), None) == -1 and call(ctx, t.data_ptr(), 32, 8, 4, None, None) == -1
    assert call(ctx, t.data_ptr(), 28, 8, 4, C.byref(tab), None) == -1          # a short pitch
    assert call(ctx, t.data_ptr(), 34, 8, 4, C.byref(tab), None) == -1          # a pitch that is no multiple of 4
    assert call(ctx, t.data_ptr() + 2, 32, 7, 4, C.byref(tab), None) == -1      # an unaligned pointer
    assert call(ctx, t.data_ptr(), 32, 0, 4, C.byref(tab), None) == -1 and call(ctx, t.data_ptr(), 32, 8, 0, C.byref(tab), None) == -1
    torch.cuda.synchronize()
    assert not t.any()
