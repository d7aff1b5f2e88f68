"""The preview and thumbnail reduce (ist_preview.hip) in every regime of its geometry: each case of tests/preview_reference.py sits
beside a boundary of preview_geometry - per_group, sub, column rounds, passes, chunks, chunk_rows - and first asserts, through
ist_debug_preview_geometry, that it runs the regime it claims, and, through ist_debug_preview_launches, that the reduce ran and not the
job path.

Content is per-pixel noise confined to 0..127 inside a window of a larger tensor filled with 255, at a column offset of 1 to 3 pixels
and a row offset of 1: the base is only 4-byte aligned, as thumbnail windows are, and any pixel read from outside the window raises a
sum.  Two rules (tests/preview_reference.py; tests/test_preview_reference.py shows on the CPU that each rejects a dropped column, a seam
column given to the neighbour, a skipped pass or chunk, a chunk moved by a row, an end weight from the wrong side and a column past the
window):

  exact        integer odd kx and ky: every weight is 1.0 and every partial sum an integer below 2^24; where the replay of the fp32
               finish agrees with the integer rule for every possible sum (exact_ok), the bytes are known and must be equal.
  consistent   every byte is a correct rounding of the fp64 reference v to within EPS = 0.01 LSB, a bound derived from the number
               of fp32 roundings (at most 150 * 2^-24 relative = 2.3e-3 LSB), not from what the kernel gives.

Measured on an MI355X, the largest |got - v| - 0.5 over the colour bytes under the opaque hint (how far the worst byte is beyond a
perfect rounding; negative: no byte is):
  regime (cases)                                                              worst margin
  per_group > 1, two column rounds, sub 4 .. 64 (kx 3, 5, 7, 9, 17, 33)       -5.1e-03
  per_group > 1, one column round (kx 15, 31, 63, 125)                         -5.4e-03
  a box wider than sub, the strided column loop (kx 65)                        -2.6e-03
  per_group 1, one pass (kx 127, 253)                                          -1.2e-02
  two passes (kx 255, 509)                                                     -1.6e-02
  three passes (kx 511, 513)                                                   -1.2e-02
  one chunk (ky 13, 15, 17, 61)                                                -2.7e-03
  two chunks (ky 63, 65; fractional ky 63.67)                                  -2.6e-03
  three chunks (ky 127, 129)                                                   -1.4e-02
  22 chunks (ky 1365)                                                          -2.6e-02
  64 chunks of 64 rows (ky 4093)                                               -1.6e-02
  chunk_rows 68 / 132 (ky 4095 / 8191)                                         -1.2e-02 / -1.6e-02
  kx 126.4 / 126.5 / 126.6 (per_group 2 -> 1)                                  -1.4e-03 / -1.5e-02 / -3.2e-02
  kx 252.9 / 253.1 (passes 1 -> 2)                                             -1.1e-02 / -5.7e-03
  four column rounds (kx 1.004 / 1.31)                                         +4.1e-13 / -2.6e-05
  kx 2.2 x ky 2.2 / kx 13 x ky 8.1                                             -2.6e-05 / -1.2e-04
  the batch twin at k = 253 (the one item not held to equality)                -1.8e-04

No byte of any case lies beyond a perfect rounding by more than 4.1e-13 (kx 1.004: an exact tie, rounded half up, that the fp64 reference
holds as x.5 - 4e-13), against the derived bound of 2.3e-03.  A margin says how close the INPUT comes to a tie where the kernel is
right; it would be positive, by the size of the error, where the kernel is wrong.
"""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests import preview_reference as PR
from tests import util as U
from tests.test_thumbs_abi import turned

pytestmark = pytest.mark.gpu

S = importlib.import_module("imagestitching_amd.stitch")


def _window(img, dx, dy=1):
    """the image as a window of a larger device tensor filled with 255: dx pixels from the left (the base is 4 * dx bytes past a
    16-byte boundary), dy rows from the top"""
    h, w = img.shape[:2]
    wide = (w + dx + 1 + 3) & ~3
    buf = torch.full((h + dy + 1, wide, 4), 255, dtype=torch.uint8, device="cuda")
    buf[dy:dy + h, dx:dx + w] = torch.from_numpy(img).cuda()
    win = buf[dy:dy + h, dx:dx + w]
    assert win.data_ptr() % 16 == 4 * dx and 1 <= dx <= 3
    return win


def _preview(img, pw, ph, opaque, dx):
    out = ist.preview_device(_window(img, dx), pw, ph, opaque=opaque)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_regime(c):
    out = (C.c_int32 * 6)()
    assert L.lib.ist_debug_preview_geometry(c.w, c.h, c.pw, c.ph, out) == 0
    per_group, groups, passes, sub, chunk_rows, chunks = out
    column_rounds = -(-min(per_group, c.pw) // (256 // sub))
    assert (per_group, sub, column_rounds, passes, chunks, chunk_rows) == tuple(c[4:10]), "the case no longer reaches its regime"
    assert groups == -(-c.pw // per_group)


@pytest.fixture(scope="module")
def rare():
    r = U.RareDiff()
    yield r
    print(r)
    r.check()                    # the second net: fewer than 1 % of the solid channel bytes differ from the rounded reference, no drift


@pytest.fixture(scope="module")
def margins():
    m = {}
    yield m
    for name, v in m.items():
        print("margin %-18s %+.2e" % (name, v))
    if m:
        print("margin worst %+.2e (derived bound %.1e)" % (max(m.values()), PR.ROUNDOFF_BOUND))


# ---- a. integer boxes -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", PR.INTEGER_CASES, ids=PR.case_id)
def test_integer_boxes_give_the_integer_rule(c, margins):
    _assert_regime(c)
    k = PR.INTEGER_CASES.index(c)
    n = PR.integer_n(c)
    before = L.lib.ist_debug_preview_launches()
    img = PR.case_image(c)
    want = PR.exact_bytes(img, c.pw, c.ph)
    v = PR.unrounded(img, c.pw, c.ph, True)
    got = _preview(img, c.pw, c.ph, True, 1 + k % 3)
    margins[PR.case_id(c)] = PR.margin(got, v)
    print("%s kx %d ky %d: margin %+.2e" % (PR.case_id(c), c.w // c.pw, c.h // c.ph, margins[PR.case_id(c)]))
    if c.rule == "exact":
        assert np.array_equal(got, want)
    else:
        assert PR.consistent(got, v, PR.EPS, True).all()
    # the same pixels without the hint: the alpha bytes are then weights like any others.  (n > 257: the premultiplied sums are no
    # integers in fp32; the seeds keep every mean farther than EPS from a tie, so the bytes are still the only correct ones)
    got = _preview(img, c.pw, c.ph, False, 1 + (k + 1) % 3)
    if c.rule == "exact":
        assert np.array_equal(got, want)
    else:
        assert PR.consistent(got, PR.unrounded(img, c.pw, c.ph, False), PR.EPS, False).all()
    calls = 2
    if n <= 257:                 # translucent noise: the premultiplied sums stay integers below 2^24, and 255 n is odd - no tie
        soft = PR.case_image(c, opaque=False)
        got = _preview(soft, c.pw, c.ph, False, 1 + (k + 2) % 3)
        assert np.array_equal(got, PR.exact_bytes_translucent(soft, c.pw, c.ph))
        calls = 3
    assert L.lib.ist_debug_preview_launches() == before + calls


def test_the_integer_cases_reach_every_regime():
    cs = PR.INTEGER_CASES
    assert {c.w % 4 for c in PR.KX_SWEEP} == {0, 1, 2, 3}
    assert {c.sub for c in cs} == {4, 8, 16, 32, 64} and {c.rounds for c in cs} == {1, 2}
    assert {c.passes for c in cs} == {1, 2, 3} and {c.chunks for c in cs} >= {1, 2, 3, 22, 64}
    assert {c.chunk_rows for c in cs} == {64, 68, 132}
    assert any(c.per_group == 1 for c in cs) and any(c.per_group > 1 for c in cs) and any(c.w // c.pw > c.sub for c in cs)
    assert sum(PR.integer_n(c) <= 257 for c in cs) >= 10       # the cases that also run translucent noise


# ---- b. fractional boxes --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", PR.FRACTIONAL_CASES, ids=PR.case_id)
def test_fractional_boxes_round_the_reference(c, rare, margins):
    _assert_regime(c)
    k = PR.FRACTIONAL_CASES.index(c)
    before = L.lib.ist_debug_preview_launches()
    img = PR.case_image(c)
    v = PR.unrounded(img, c.pw, c.ph, True)
    got = _preview(img, c.pw, c.ph, True, 1 + k % 3)
    margins[PR.case_id(c)] = PR.margin(got, v)
    print("%s kx %.3f ky %.3f: margin %+.2e" % (PR.case_id(c), c.w / c.pw, c.h / c.ph, margins[PR.case_id(c)]))
    bad = ~PR.consistent(got, v, PR.EPS, True)
    assert not bad.any(), "%d pixels are no rounding of the reference, the first at %s" % (bad.sum(), np.argwhere(bad)[0])
    rare.add(U.oracle_tolerance(got, PR.finish(v, True)))
    # without the hint: the same pixels, then translucent noise
    v = PR.unrounded(img, c.pw, c.ph, False)
    got = _preview(img, c.pw, c.ph, False, 1 + (k + 1) % 3)
    bad = ~PR.consistent(got, v, PR.EPS, False)
    assert not bad.any(), "no hint: %d pixels are no rounding of the reference, the first at %s" % (bad.sum(), np.argwhere(bad)[0])
    rare.add(U.oracle_tolerance(got, PR.finish(v, False)))
    soft = PR.case_image(c, opaque=False)
    v = PR.unrounded(soft, c.pw, c.ph, False)
    got = _preview(soft, c.pw, c.ph, False, 1 + (k + 2) % 3)
    bad = ~PR.consistent(got, v, PR.EPS, False)
    assert not bad.any(), "translucent: %d pixels are no rounding of the reference, the first at %s" % (bad.sum(), np.argwhere(bad)[0])
    U.oracle_tolerance(got, PR.finish(v, False))
    assert L.lib.ist_debug_preview_launches() == before + 3


# ---- c. the destination ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,pw,ph", [(507, 15, 169, 5), (1527, 15, 3, 5), (21, 195, 7, 3)])
def test_a_padded_destination_keeps_its_padding(w, h, pw, ph):
    (c,) = [c for c in PR.INTEGER_CASES if (c.w, c.h, c.pw, c.ph) == (w, h, pw, ph)]
    _assert_regime(c)
    img = PR.case_image(c)
    want = PR.exact_bytes(img, pw, ph)
    src = _window(img, 3)
    pitch = 4 * pw + 12
    ctx = S._ctx(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    before = L.lib.ist_debug_preview_launches()
    for opaque in (1, 0):
        buf = torch.full((ph + 2, pitch), 0xA5, dtype=torch.uint8, device="cuda")     # a guard row before and one after
        L.check(L.lib.ist_preview_device(ctx, C.c_void_p(src.data_ptr()), src.stride(0), w, h, opaque,
                                         C.c_void_p(buf.data_ptr() + pitch), pitch, pw, ph, stream))
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.array_equal(host[1:1 + ph, :4 * pw].reshape(ph, pw, 4), want)
        assert (host[0] == 0xA5).all() and (host[-1] == 0xA5).all() and (host[:, 4 * pw:] == 0xA5).all()
    assert L.lib.ist_debug_preview_launches() == before + 2


# ---- d. the batch twin ----------------------------------------------------------------------------------------------------------

def test_the_batch_twin_runs_every_regime_like_the_single_path():
    items = [(k, True) for k in PR.BATCH_KS] + [(3, False), (15, False)]
    imgs = [PR.noise(200 + i, 5 * k, 5 * k, opaque) for i, (k, opaque) in enumerate(items)]
    devs = [_window(a, 1 + i % 3) for i, a in enumerate(imgs)]
    orient = [1 + i % 8 for i in range(len(items))]
    hints = [opaque for _, opaque in items]
    out = (C.c_int32 * 6)()
    for k, _ in items:
        assert L.lib.ist_debug_preview_geometry(5 * k, 5 * k, 5, 5, out) == 0
        assert (out[0], out[3], out[2], out[5]) == PR.BATCH_REGIMES[k], k
    for t in ist.thumbnail_layout([(5 * k, 5 * k, o) for (k, _), o in zip(items, orient)], (5, 5), "fit"):
        assert (t["width"], t["height"]) == (5, 5) and t["window"][:2] == (0, 0) and t["window"][2] == t["window"][3]
    pairs, single = L.lib.ist_debug_thumb_launches(), L.lib.ist_debug_preview_launches()
    got = [t.cpu().numpy() for t in ist.thumbnails_device(devs, (5, 5), "fit", orientations=orient, opaque=hints)]
    assert L.lib.ist_debug_thumb_launches() == pairs + 2      # the opaque items in one launch pair, the translucent ones in another
    assert L.lib.ist_debug_preview_launches() == single
    for i, (k, opaque) in enumerate(items):
        one = ist.preview_device(devs[i], 5, 5, opaque=opaque).cpu().numpy()
        assert np.array_equal(got[i], turned(one, orient[i])), "item %d (k = %d) differs from the single-image path" % (i, k)
        if not opaque:
            assert np.array_equal(got[i], turned(PR.exact_bytes_translucent(imgs[i], 5, 5), orient[i])), k
        elif k in PR.BATCH_EXACT:
            assert np.array_equal(got[i], turned(PR.exact_bytes(imgs[i], 5, 5), orient[i])), k
        else:
            v = PR.unrounded(imgs[i], 5, 5, True)
            print("batch k %d: margin %+.2e" % (k, PR.margin(one, v)))
            assert PR.consistent(one, v, PR.EPS, True).all(), k
    assert L.lib.ist_debug_preview_launches() == single + len(items)
    # the items in reverse order: every workgroup's item lookup lands elsewhere, the bytes per item are the same
    back = [t.cpu().numpy() for t in ist.thumbnails_device(devs[::-1], (5, 5), "fit", orientations=orient[::-1], opaque=hints[::-1])]
    assert L.lib.ist_debug_thumb_launches() == pairs + 4
    for a, b in zip(got, back[::-1]):
        assert np.array_equal(a, b)
