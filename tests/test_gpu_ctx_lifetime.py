"""What a context (and a device group) asks the HIP runtime for, it gives back: ist_debug_live_handles counts the device blocks, the
pinned blocks outside the result pool, the streams and the events the library holds.  Every feature that keeps state between calls runs
twice on a context of the test's own - the second pass must leave all four counts where the first left them - and destroying the
context must return them to where they were before it was made.  Results are checked for shape only: pixels are the other suites'
business."""
import ctypes as C
import gc
import sys

import pytest

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests import util as U

S = sys.modules["imagestitching_amd.stitch"]      # (the package's attribute `stitch` is the function)

pytestmark = pytest.mark.gpu


def live():
    out = (C.c_int64 * 4)()
    assert L.lib.ist_debug_live_handles(out) == L.IST_OK
    return tuple(int(v) for v in out)


@pytest.fixture(scope="module")
def small():
    return [U.rand_image(4100 + k, 48, 64, opaque=(k == 0)) for k in range(3)]


@pytest.fixture(scope="module")
def big():
    return [U.rand_image(4110 + k, 2048, 2048) for k in range(2)]


@pytest.fixture(scope="module")
def jpeg_paths(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("lifetime")
    rgb = U.smooth_image(4120, 32, 48)[..., :3]
    paths = [str(d / "baseline.jpg"), str(d / "progressive.jpg")]
    Image.fromarray(rgb).save(paths[0], quality=90, subsampling="4:2:0")
    Image.fromarray(rgb).save(paths[1], quality=90, subsampling="4:2:0", progressive=True)
    return paths


def every_feature(small, big, jpeg_paths):
    """one call of everything that owns state in a context; nothing it made is alive when it returns"""
    import torch
    two = small[:2]
    for filt in ("nearest", "bilinear"):
        assert ist.stitch(two, "vertical", {"filter": filt})["data"].shape == (96, 64, 4)
    before = L.lib.ist_debug_duplex_stitches()
    assert ist.stitch(big, "vertical")["data"].shape == (4096, 2048, 4)            # exactly 32 MiB: the banded path
    assert L.lib.ist_debug_duplex_stitches() == before + 1
    for opts in ({"pngLevel": 0}, {"pngLevel": 1}, {"pngLevel": 1, "pngColor": "rgb"}, {"pngLevel": 1, "preview": (32, 32)}):
        got = ist.stitch_png(two, "vertical", opts)
        assert (got["width"], got["height"]) == (64, 96) and got["png"][:4] == b"\x89PNG"
        assert "preview" not in opts or got["preview"].shape == (32, 21, 4)
    got = ist.stitch_jpeg(two, "vertical", {"optimize": True})
    assert (got["width"], got["height"]) == (64, 96) and got["jpeg"][:2] == b"\xff\xd8"
    reqs = [(two, "vertical"), (two, "horizontal")]
    assert [a.shape for a in ist.stitch_batch(reqs)] == [(96, 64, 4), (48, 128, 4)]
    assert [(r["width"], r["height"]) for r in ist.stitch_png_batch(reqs)] == [(64, 96), (128, 48)]
    assert [(r["width"], r["height"]) for r in ist.stitch_jpeg_batch(reqs)] == [(64, 96), (128, 48)]
    files = L.lib.ist_debug_gpu_entropy_files()
    got = ist.stitch_files(jpeg_paths, "vertical")
    assert (got["width"], got["height"]) == (48, 64)
    assert L.lib.ist_debug_gpu_entropy_files() == files + 1                        # (the baseline file; the progressive one is the host's)
    bms = [ist.upload_bitmap(small[0])] + ist.decode_bitmaps(jpeg_paths[:1])
    assert ist.stitch(bms, "vertical")["data"].shape == (68, 48, 4)
    assert bms[0].preview(16, 16).shape == (12, 16, 4)
    assert [t.shape for t in ist.thumbnails(bms, (16, 16))] == [(16, 16, 4)] * 2
    for b in bms:
        b.close()
    st = ist.Stitcher(0)
    side = torch.cuda.Stream()
    for direction in ("vertical", "horizontal"):
        p, job = st.compile([{"width": 64, "height": 48}] * 2, direction, {"filter": "bilinear"})
        srcs = [torch.from_numpy(a).cuda() for a in two]
        out = torch.empty((p.canvas_h, p.canvas_w, 4), dtype=torch.uint8, device="cuda")
        side.wait_stream(torch.cuda.current_stream())
        job.launch(srcs, out, stream=side)
        side.synchronize()
        job.close()


def test_a_context_returns_every_handle_it_made(monkeypatch, small, big, jpeg_paths):
    gc.collect()                   # (what earlier tests left to the collector goes now, not between the readings)
    L.lib.ist_pool_trim()
    start = live()
    ctx = L.lib.ist_ctx_create(0)
    assert ctx
    monkeypatch.setitem(S._ctx_cache, 0, ctx)
    try:
        every_feature(small, big, jpeg_paths)
        gc.collect()
        first = live()
        every_feature(small, big, jpeg_paths)
        gc.collect()
        second = live()
    finally:
        monkeypatch.undo()
        L.lib.ist_ctx_destroy(ctx)
        L.lib.ist_pool_trim()
    print("live handles (device blocks, pinned blocks, streams, events): start", start, "first pass", first, "second pass", second, "end", live())
    assert first[0] > start[0] and first[1] > start[1] and first[2] > start[2] and first[3] > start[3]      # (the counts do count)
    assert second == first
    assert live() == start


def test_a_device_group_returns_every_handle_it_made(small):
    import torch
    gc.collect()                   # (what earlier tests left to the collector goes now, not between the readings)
    L.lib.ist_pool_trim()
    start = live()
    g = ist.StitchGroup([0, 0, 0])
    try:
        job = g.compile(U.hip_images(small), "vertical", {"filter": "bilinear", "split": "band"})
        out = torch.empty((job.plan.canvas_h, job.plan.canvas_w, 4), dtype=torch.uint8, device="cuda")
        full = [torch.from_numpy(a).cuda() for a in small]
        job.launch([full[p["image"]] for p in job.parts], out)                      # device sink
        g.sync()
        assert tuple(out.shape) == (144, 64, 4)
        job.close()
        o = S._merge({"filter": "bilinear"})
        descs, ptrs, pitches, keep = S._host_sources(small)
        cplan, pixels = L.Plan(), C.POINTER(C.c_uint8)()
        sunk = L.lib.ist_debug_host_sink_stitches()
        rc = L.check(L.lib.ist_group_stitch_rgba8(g._h, descs, ptrs, pitches, len(small), *S._plan_args("vertical", o), S._SPLITS["rows"],
                                                  C.byref(cplan), C.byref(pixels)))
        assert L.lib.ist_debug_host_sink_stitches() == sunk + 1                      # host sink
        assert S._take_pixels(pixels, *S._plan_size(rc, cplan)).shape == (144, 64, 4)
        held = live()
    finally:
        g.close()
        gc.collect()
        L.lib.ist_pool_trim()
    print("live handles (device blocks, pinned blocks, streams, events): start", start, "in use", held, "end", live())
    assert held[0] > start[0] and held[2] > start[2]
    assert live() == start
