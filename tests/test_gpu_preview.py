"""Previews on the GPU (ist_preview_device, the four *_png_preview entry points, ist_bitmap_preview; Python host).  The contract is
not new: a preview of a w x h image at pw x ph is what a fresh transparent pw x ph canvas reads back after ONE drawImage(img, 0, 0, w,
h, 0, 0, pw, ph) under filter 'area' - the oracle's render_ops of that draw, under the op-list tolerance of tests/util.py.  Reference
anchor: the redraw into the preview node, pages/index/index.js:1597-1603."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from oracle import oracle as O
from tests import util as U
from tests.test_gpu_bitmaps import _jpeg, _photo

pytestmark = pytest.mark.gpu

S = importlib.import_module("imagestitching_amd.stitch")      # (the package exports the function `stitch` under the module's name)

BOX = (343, 457)


def oracle_preview(img, pw, ph):
    h, w = img.shape[:2]
    draw = {"kind": "draw", "image": 0, "m": [1, 0, 0, 1, 0, 0], "s": [0, 0, w, h], "d": [0, 0, pw, ph]}
    return O.render_ops(pw, ph, [draw], [{"width": w, "height": h}], [img], filter="area", clear=(0, 0, 0, 0))


def _device(img, pad=0):
    """the image in HBM, its rows `pad` pixels apart from dense (the padding holds 0xEE bytes the preview must never read as pixels)"""
    h, w = img.shape[:2]
    buf = torch.full((h, w + pad, 4), 0xEE, dtype=torch.uint8, device="cuda")
    buf[:, :w] = torch.from_numpy(img).cuda()
    return buf[:, :w]


def _preview(img, pw, ph, opaque, pad=0):
    out = ist.preview_device(_device(img, pad), pw, ph, opaque=opaque)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# (w, h, pw, ph): the shrink factors the issue lists; widths 601 and 4033, odd heights
SHAPES = [
    (601, 777, 462, 598),        # 1.3
    (601, 777, 273, 353),        # 2.2
    (4033, 1001, 611, 152),      # 6.6
    (4033, 1001, 345, 86),       # 11.7
    (4033, 2737, 68, 46),        # 59.3 x 59.5: the streamed box path's narrowest tile
    (600, 36000, 8, 457),        # 75 x 79: past the streamed path's |ky| limit of 64
    (4536, 378, 343, 29),        # 13 x 13
    (40, 200000, 1, 457),        # 40 x 438, one output column
    (601, 5001, 200, 100),       # 3 x 50
    (5001, 601, 100, 200),       # 50 x 3
    (1300, 3, 1, 1),             # one output pixel, several 256-column passes over its box
]


@pytest.fixture(scope="module")
def rare():
    r = U.RareDiff()
    yield r
    r.check()                    # fewer than 1 % of the solid channel bytes differ from the oracle, unbiased


@pytest.mark.parametrize("w,h,pw,ph", SHAPES)
def test_preview_device_matches_the_oracle(w, h, pw, ph, rare):
    before = L.lib.ist_debug_preview_launches()
    solid = U.smooth_image(w + h, h, w, opaque=True)
    got = _preview(solid, pw, ph, opaque=True)
    ref = oracle_preview(solid, pw, ph)
    stats = U.oracle_tolerance(got, ref)
    print("%dx%d -> %dx%d opaque: %d of %d bytes differ, signed sum %d" % ((w, h, pw, ph) + stats))
    rare.add(stats)
    # the same pixels without the hint, rows padded: the alpha bytes are then weights like any others
    got2 = _preview(solid, pw, ph, opaque=False, pad=3)
    stats = U.oracle_tolerance(got2, ref)
    print("%dx%d -> %dx%d no hint, padded: %d of %d bytes differ, signed sum %d" % ((w, h, pw, ph) + stats))
    rare.add(stats)
    soft = U.smooth_image(w + h + 1, h, w, opaque=False)
    got3 = _preview(soft, pw, ph, opaque=False, pad=5)
    U.oracle_tolerance(got3, oracle_preview(soft, pw, ph))
    assert L.lib.ist_debug_preview_launches() == before + 3          # every one of them took the reduce


def test_ties_and_noise():
    """noise averages to 128 and hides wrong weights, but it probes rounding ties: 2 x 2 boxes of bytes land on .0 / .25 / .5 / .75"""
    a = U.rand_image(3, 600, 802, opaque=True)
    got = _preview(a, 401, 300, opaque=True)
    exact = ((a.astype(np.uint32).reshape(300, 2, 401, 2, 4).sum(axis=(1, 3)) * 2 + 4) // 8).astype(np.uint8)     # round half up
    assert np.array_equal(got, exact)
    U.oracle_tolerance(got, oracle_preview(a, 401, 300))
    b = U.rand_image(4, 333, 1001, opaque=False)
    U.oracle_tolerance(_preview(b, 77, 41, opaque=False, pad=1), oracle_preview(b, 77, 41))


@pytest.mark.parametrize("k,bw,bh", [(2, 37, 23), (3, 37, 23), (7, 37, 23), (64, 9, 7), (65, 9, 7), (300, 5, 3)])
def test_block_images_shrink_to_their_blocks_exactly(k, bw, bh):
    blocks = U.rand_image(k, bh, bw, opaque=True)
    img = np.repeat(np.repeat(blocks, k, axis=0), k, axis=1)
    before = L.lib.ist_debug_preview_launches()
    assert np.array_equal(_preview(img, bw, bh, opaque=True), blocks)
    assert np.array_equal(_preview(img, bw, bh, opaque=False, pad=2), blocks)
    assert L.lib.ist_debug_preview_launches() == before + 2


def test_the_same_call_gives_the_same_bytes():
    img = U.smooth_image(9, 36000, 600, opaque=False)
    dev = _device(img, 1)
    a = ist.preview_device(dev, 8, 457).cpu().numpy()
    b = ist.preview_device(dev, 8, 457).cpu().numpy()
    assert np.array_equal(a, b)
    noise = _device(U.rand_image(10, 2737, 4033, opaque=False))
    outs = [ist.preview_device(noise, 68, 46).cpu().numpy() for _ in range(3)]
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def test_two_streams_do_not_share_partial_sums():
    """the partial sums are the context's: a reduce on another stream is ordered behind the one before it by an event.  Without the
    event the outcome is a race, so the test is shaped to lose it: a LONG reduce (640 MB of source, ~0.1 ms) goes out first and a
    short one of the same output shape - whose first stage takes a few microseconds and writes the same scratch - right behind it on
    another stream, four times over, so that unordered the short one's partial sums land under the long one's second stage."""
    rng = np.random.default_rng(5)
    long_src = [torch.from_numpy(rng.integers(0, 256, (20000, 8000, 4), dtype=np.uint8)).cuda() for _ in range(2)]
    short_src = [_device(U.smooth_image(20 + k, 1201, 401, opaque=False)) for k in range(2)]
    want_long = [ist.preview_device(t, 100, 300).cpu().numpy() for t in long_src]
    want_short = [ist.preview_device(t, 100, 300).cpu().numpy() for t in short_src]
    torch.cuda.synchronize()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    for rep in range(4):
        k = rep & 1
        out_long = torch.zeros((300, 100, 4), dtype=torch.uint8, device="cuda")
        out_short = torch.zeros((300, 100, 4), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ist.preview_device(long_src[k], 100, 300, out=out_long, stream=a)
        ist.preview_device(short_src[k], 100, 300, out=out_short, stream=b)
        torch.cuda.synchronize()
        assert np.array_equal(out_long.cpu().numpy(), want_long[k]), rep
        assert np.array_equal(out_short.cpu().numpy(), want_short[k]), rep


@pytest.mark.parametrize("w,h,pw,ph", [(100, 120, 343, 412), (1000, 100, 250, 200), (300, 200, 300, 50)])
def test_a_draw_that_does_not_shrink_on_both_axes_takes_the_job_path(w, h, pw, ph):
    if (w, h) == (100, 120):
        assert ist.preview_fit(w, h, *BOX) == (pw, ph)       # a result smaller than its box is enlarged, like the reference's
    before = L.lib.ist_debug_preview_launches()
    for opaque in (True, False):
        img = U.smooth_image(w, h, w, opaque=opaque)
        U.oracle_tolerance(_preview(img, pw, ph, opaque=opaque), oracle_preview(img, pw, ph))
    assert L.lib.ist_debug_preview_launches() == before


def test_argument_errors_on_the_device():
    """(one error of the list cannot be provoked on one GPU: a bitmap of another device than the context's, IST_E_INVALID, is the check
    of ist_bitmap_preview that mirrors take_bitmaps in ist_bitmap.cpp; it is untested, like that one)"""
    t = _device(U.rand_image(1, 40, 50))
    for pw, ph in [(0, 5), (5, 0), (-3, 5)]:
        with pytest.raises(ist.StitchError) as e:
            ist.preview_device(t, pw, ph)
        assert e.value.code == -1
    ctx = S._ctx(0)
    # the Python host checks what the library cannot see of a tensor: shape, dtype, pixel stride and device of `out`, a host source
    for bad in [torch.empty((9, 10, 4), dtype=torch.uint8, device="cuda"), torch.empty((10, 10, 4), dtype=torch.int8, device="cuda"),
                torch.empty((10, 10, 3), dtype=torch.uint8, device="cuda"), torch.empty((10, 10, 8), dtype=torch.uint8, device="cuda")[..., ::2],
                torch.empty((10, 10, 4), dtype=torch.uint8)]:
        with pytest.raises(TypeError, match="out must be"):
            ist.preview_device(t, 10, 10, out=bad)
    with pytest.raises(TypeError, match="CUDA tensor"):
        ist.preview_device(t.cpu(), 10, 10)
    assert ist.preview_device(t, 10, 10, out=torch.empty((10, 16, 4), dtype=torch.uint8, device="cuda")[:, :10]).shape == (10, 10, 4)      # padded rows are fine
    for rc_of in (lambda pv: L.lib.ist_stitch_png_preview(ctx, None, None, None, 1, 0, 0, 0.0, None, 1, None, None, None, C.byref(pv)),
                  lambda pv: L.lib.ist_stitch_bitmaps_png_preview(ctx, None, 1, 0, 0, 0.0, None, 1, None, None, None, C.byref(pv))):
        pv = L.Preview(343.0, 457.0, 5, 6, C.cast(1, C.POINTER(C.c_uint8)))
        assert rc_of(pv) == -1 and not pv.pixels and (pv.width, pv.height) == (0, 0)      # NULL outputs: the struct is cleared first
    out = torch.empty((10, 10, 4), dtype=torch.uint8, device="cuda")
    args = lambda sp, dp: L.lib.ist_preview_device(ctx, t.data_ptr(), sp, 50, 40, 0, out.data_ptr(), dp, 10, 10, None)  # noqa: E731
    assert args(199, 40) == -1 and args(202, 40) == -1 and args(200, 36) == -1 and args(200, 42) == -1
    assert L.lib.ist_preview_device(ctx, None, 200, 50, 40, 0, out.data_ptr(), 40, 10, 10, None) == -1
    img = U.rand_image(2, 40, 50)
    for box in [(0, 457), (343, float("nan")), (float("inf"), 457), (-1, 5)]:
        with pytest.raises(ist.StitchError) as e:
            ist.stitch_png([img], "vertical", {"preview": box})
        assert e.value.code == -1
    b = ist.upload_bitmap(img)
    small = np.empty((4, 4, 4), np.uint8)
    assert L.lib.ist_bitmap_preview(ctx, C.c_void_p(b.handle()), 0, 4, small.ctypes.data, 16) == -1
    assert L.lib.ist_bitmap_preview(ctx, C.c_void_p(b.handle()), 4, 4, small.ctypes.data, 15) == -1
    assert L.lib.ist_bitmap_preview(ctx, None, 4, 4, small.ctypes.data, 16) == -1
    b.close()


# ---- end to end: the four entry points -------------------------------------------------------------------------------------------

def _files(sizes, seed):
    return [_jpeg(_photo(seed + k, h, w), quality=90) for k, (w, h) in enumerate(sizes)]


def _check_end_to_end(without, with_preview, rare=None):
    """the file is the one the call without `preview` returns; the preview is the oracle's shrink of the file's own pixels"""
    assert "preview" not in without and bytes(with_preview["png"]) == bytes(without["png"])
    canvas = ist.decode_png(with_preview["png"])
    assert canvas.shape[:2] == (with_preview["height"], with_preview["width"])
    pw, ph = ist.preview_fit(canvas.shape[1], canvas.shape[0], *BOX)
    pv = with_preview["preview"]
    assert pv.shape == (ph, pw, 4) and pv.dtype == np.uint8
    stats = U.oracle_tolerance(pv, oracle_preview(canvas, pw, ph))
    if rare is not None:
        rare.add(stats)
    return stats


def _files_call(blobs, direction, box):
    """ist_stitch_files_png / ist_stitch_files_png_preview (the Python host binds the paths form)"""
    n = len(blobs)
    files = (C.c_char_p * n)(*blobs)
    lens = (C.c_int64 * n)(*[len(b) for b in blobs])
    lim = L.Limits()
    L.lib.ist_limits_unlimited(C.byref(lim))
    plan, out, ln = L.Plan(), C.POINTER(C.c_uint8)(), C.c_int64(0)
    ctx = S._ctx_png(0, None)
    if box is None:
        L.check(L.lib.ist_stitch_files_png(ctx, files, lens, n, S._DIRECTIONS[direction], 0, 0.0, C.byref(lim), 1, C.byref(plan), C.byref(out), C.byref(ln)))
    else:
        pv = L.Preview(float(box[0]), float(box[1]), 0, 0, None)
        L.check(L.lib.ist_stitch_files_png_preview(ctx, files, lens, n, S._DIRECTIONS[direction], 0, 0.0, C.byref(lim), 1, C.byref(plan), C.byref(out),
                                                   C.byref(ln), C.byref(pv)))
    res = {"width": int(plan.canvas_w), "height": int(plan.canvas_h), "png": S._take_png(out, ln)}
    L.lib.ist_plan_free(C.byref(plan))
    if box is not None:
        res["preview"] = S._take_preview(pv)
    return res


@pytest.mark.parametrize("direction", ["vertical", "horizontal"])
@pytest.mark.parametrize("big", [False, True])
def test_every_png_entry_point_returns_the_same_file_and_its_preview(tmp_path, direction, big, rare):
    # big: a canvas above 32 MB (the banded render of the host path, the per-image bands of the file pipeline)
    sizes = [(2000, 1500), (2000, 1400), (2000, 1600)] if big else [(400, 300), (380, 320), (420, 280)]
    if big and direction == "horizontal":
        sizes = [(h, w) for w, h in sizes]
    blobs = _files(sizes, 70 + (10 if big else 0))
    paths = []
    for k, b in enumerate(blobs):
        paths.append(str(tmp_path / ("p%d.jpg" % k)))
        open(paths[-1], "wb").write(b)
    host = [{"width": a.shape[1], "height": a.shape[0], "data": a, "opaque": True} for a in (ist.decode_image(b) for b in blobs)]
    bitmaps = ist.decode_bitmaps(blobs)
    opts = {"gap": 6, "preview": BOX}
    plain = {"gap": 6}
    calls = {
        "stitch_png": (lambda o: ist.stitch_png(host, direction, o)),
        "stitch_png(bitmaps)": (lambda o: ist.stitch_png(bitmaps, direction, o)),
        "stitch_files": (lambda o: ist.stitch_files(paths, direction, o)),
    }
    for name, call in calls.items():
        before, banded = L.lib.ist_debug_preview_launches(), L.lib.ist_debug_duplex_stitches()
        without = call(plain)
        assert L.lib.ist_debug_preview_launches() == before, name       # no preview asked for: nothing new is launched
        got = call(opts)
        assert L.lib.ist_debug_preview_launches() == before + 1, name
        if big:
            assert got["width"] * got["height"] * 4 > 32 << 20
        banded = L.lib.ist_debug_duplex_stitches() - banded
        print(name, direction, "banded renders:", banded)
        if big and direction == "vertical" and name == "stitch_png":
            # the host path rendered this canvas band by band, each band behind the encoder's request for its rows (render_png_banded):
            # the preview was queued behind the LAST band, not behind one launch of the whole canvas
            assert banded == 2, banded
        print(name, direction, "big" if big else "small", _check_end_to_end(without, got, rare))
    before = L.lib.ist_debug_preview_launches()
    without = _files_call(blobs, direction, None)
    assert L.lib.ist_debug_preview_launches() == before
    got = _files_call(blobs, direction, BOX)
    assert L.lib.ist_debug_preview_launches() == before + 1
    print("files", direction, "big" if big else "small", _check_end_to_end(without, got, rare))
    # both PNG forms carry the preview
    stored = ist.stitch_png(host, direction, dict(opts, pngLevel=0))
    assert np.array_equal(stored["preview"], ist.stitch_png(host, direction, opts)["preview"])
    assert np.array_equal(ist.decode_png(stored["png"]), ist.decode_png(ist.stitch_png(host, direction, plain)["png"]))
    for b in bitmaps:
        b.close()


def test_a_canvas_smaller_than_the_box_gets_an_enlarged_preview():
    img = U.smooth_image(5, 120, 100, opaque=True)
    before = L.lib.ist_debug_preview_launches()
    r = ist.stitch_png([img], "vertical", {"preview": BOX})
    assert r["preview"].shape == (412, 343, 4) and L.lib.ist_debug_preview_launches() == before      # the job path
    U.oracle_tolerance(r["preview"], oracle_preview(ist.decode_png(r["png"]), 343, 412))


def test_bitmap_preview_is_the_shrink_of_its_download():
    before = L.lib.ist_debug_preview_launches()
    for seed, (w, h), opaque in [(1, (1203, 901), False), (2, (640, 4801), True)]:
        img = U.smooth_image(seed, h, w, opaque=opaque)
        b = ist.upload_bitmap({"width": w, "height": h, "data": img, "opaque": opaque, "orientation": 6})
        pw, ph = ist.preview_fit(w, h, *BOX)
        pv = b.preview(*BOX)
        assert pv.shape == (ph, pw, 4)                       # the stored pixels: orientation 6 does not turn them
        U.oracle_tolerance(pv, oracle_preview(b.download(), pw, ph))
        b.close()
    assert L.lib.ist_debug_preview_launches() == before + 2
    photo = ist.decode_bitmaps([_jpeg(_photo(3, 900, 1200), quality=90)])[0]
    U.oracle_tolerance(photo.preview(100, 100), oracle_preview(photo.download(), 100, 75))
    photo.close()


def test_the_steady_state_allocates_nothing():
    img = _device(U.smooth_image(6, 2001, 1501, opaque=False))
    out = torch.empty((200, 150, 4), dtype=torch.uint8, device="cuda")
    host = [U.smooth_image(30 + k, 300, 400) for k in range(3)]
    bm = ist.upload_bitmap(host[0])
    small = _device(U.smooth_image(7, 120, 100))
    big_out = torch.empty((412, 343, 4), dtype=torch.uint8, device="cuda")

    def once():
        ist.preview_device(img, 150, 200, out=out)
        ist.preview_device(small, 343, 412, out=big_out)      # the job path keeps its job
        torch.cuda.synchronize()
        ist.stitch_png(host, "vertical", {"preview": BOX})
        bm.preview(*BOX)

    once()
    allocs = L.lib.ist_debug_device_allocs()
    for _ in range(3):
        once()
    assert L.lib.ist_debug_device_allocs() == allocs
    bm.close()
