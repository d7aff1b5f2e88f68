"""JPEG export with the file's own Huffman tables (IST_JPEG_OPTIMIZE, optimize=True) on the GPU: every file equals the numpy contract
byte for byte - tests/jpeg_writer.py write_jpeg(huff="optimal") over the coefficients of tests/jpeg_encode_reference.py, one restart
interval per MCU row.

Shapes are those of tests/test_gpu_jpeg_encode.py, for the same reasons, and for what is new here: tables of one or two symbols (1 x 1), counts
that cross the entropy kernel's batches and the histogram's parts and trees deeper than 16 (4805 x 19 at quality 100), counts that
accumulate over slabs, chroma tables that hold only size 0 and EOB (a grey ramp), batches that mix optimised and standard files in
one round and over several."""
import functools
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import jpeg_encode_reference as R
from tests import jpeg_writer as JW
from tests.test_gpu_jpeg_encode import LAYOUTS, QUALITIES, STITCHES, checker, first_difference, noise, photo, three_images

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ist():
    import imagestitching_amd
    return imagestitching_amd


def _lib():
    from imagestitching_amd import _lib as L
    return L


def reference(a, quality, layout):
    return JW.write_jpeg(R.frame(a, quality, layout), sof=0, marker="jfif", huff="optimal", restart=R.mcus_per_row(a.shape[1], layout))


@functools.lru_cache(maxsize=None)
def reference_of_photo(w, h, quality, layout, seed=0):
    return reference(photo(w, h, seed), quality, layout)


def _same(got, want, what):
    assert got == want, "%s: %s" % (what, first_difference(got, want))


def check(ist, a, quality, layout, want=None):
    got = ist.encode_jpeg(a, quality, layout, optimize=True)
    _same(got, reference(a, quality, layout) if want is None else want, "%dx%d Q%d %s" % (a.shape[1], a.shape[0], quality, layout))
    return got


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("w,h", ((1, 1), (7, 9), (16, 16), (17, 33)))
def test_partial_mcus(ist, w, h, layout):
    for q in QUALITIES:
        check(ist, photo(w, h), q, layout, reference_of_photo(w, h, q, layout))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_an_interval_longer_than_a_batch(ist, layout):
    """4805 x 19: 1806 (1803) blocks in one interval: eight batches of the entropy kernel, fifteen parts of the histogram; at quality 100
    the trees are deeper than 16 (tests/test_jpeg_optimize_abi.py asserts it of the contract)"""
    a = photo(4805, 19)
    for q in QUALITIES:
        check(ist, a, q, layout, reference_of_photo(4805, 19, q, layout))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_rst_markers_wrap(ist, layout):
    a = photo(33, 170)
    for q in QUALITIES:
        got = check(ist, a, q, layout, reference_of_photo(33, 170, q, layout))
    assert got.count(b"\xff\xd7") >= 1 and got.count(b"\xff\xd0") >= 2


@pytest.mark.parametrize("layout", LAYOUTS)
def test_pitched_canvas_on_the_device(ist, layout):
    import torch
    a = photo(37, 21)
    wide = torch.full((21, 37 + 13, 4), 0xEE, dtype=torch.uint8, device="cuda")
    wide[:, :37] = torch.from_numpy(a).cuda()
    canvas = wide[:, :37]
    assert canvas.stride(0) == 4 * (37 + 13)
    for q in QUALITIES:
        t, n = ist.encode_jpeg_device(canvas, q, layout, optimize=True)
        torch.cuda.synchronize()
        got, want = t.cpu().numpy().tobytes(), reference_of_photo(37, 21, q, layout)
        assert n == len(want)
        _same(got, want, "Q%d" % q)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_noise_long_codes_and_stuffing(ist, layout):
    got = check(ist, noise(100, 150), 100, layout)
    assert b"\xff\x00" in got


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


def grey_ramp(w=61, h=45):
    yy, xx = np.mgrid[0:h, 0:w]
    v = ((3 * xx + 2 * yy) % 256).astype(np.uint8)
    return np.stack([v, v, v, np.full_like(v, 255)], -1)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_grey_ramp_chroma_tables_of_size_zero_and_eob(ist, layout):
    a = grey_ramp()
    f = R.frame(a, 90, layout)
    assert not f.comps[1]["coef"].any() and not f.comps[2]["coef"].any() and f.comps[0]["coef"][..., 1:].any()
    for q in QUALITIES:
        check(ist, a, q, layout)


def test_slabs(ist, tmp_path):
    """33 x 700 with 13 MCU rows per slab: 4 slabs in 4:2:0 (44 MCU rows), 7 in 4:4:4 (88): the counts accumulate over the slabs and
    every slab is transformed twice.  The override is read once, in tuning mode, so the encodes run in a process of their own."""
    code = """
import sys
sys.path.insert(0, %r)
import numpy as np
import imagestitching_amd as ist
from imagestitching_amd import _lib as L
a = np.load(sys.argv[1])
before = L.lib.ist_debug_jpeg_encode_launches(), L.lib.ist_debug_jpeg_histogram_launches()
out = {}
for q in (1, 50, 90, 100):
    for layout in ("420", "444"):
        out["%%d_%%s" %% (q, layout)] = np.frombuffer(ist.encode_jpeg(a, q, layout, optimize=True), np.uint8)
print("launches", L.lib.ist_debug_jpeg_encode_launches() - before[0], L.lib.ist_debug_jpeg_histogram_launches() - before[1])
np.savez(sys.argv[2], **out)
""" % (ROOT,)
    a = photo(33, 700)
    np.save(tmp_path / "a.npy", a)
    env = dict(os.environ, IST_TUNING="1", IST_JPEG_ENC_ROWS="13")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "a.npy"), str(tmp_path / "out.npz")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "launches %d %d\n" % (2 * 4 * (4 + 7), 4 * (4 + 7)) in r.stdout, r.stdout
    got = np.load(tmp_path / "out.npz")
    L = _lib()
    for q in QUALITIES:
        for layout in LAYOUTS:
            want = reference_of_photo(33, 700, q, layout)
            _same(got["%d_%s" % (q, layout)].tobytes(), want, "Q%d %s" % (q, layout))
            # ... and as one slab: the coefficients are kept, one transform launch
            before = L.lib.ist_debug_jpeg_encode_launches()
            _same(ist.encode_jpeg(a, q, layout, optimize=True), want, "one slab, Q%d %s" % (q, layout))
            assert L.lib.ist_debug_jpeg_encode_launches() == before + 1


def test_alpha_is_not_read(ist):
    a = photo(23, 18)
    b = a.copy()
    b[..., 3] = np.random.default_rng(3).integers(0, 256, b.shape[:2], dtype=np.uint8)
    for layout in LAYOUTS:
        assert ist.encode_jpeg(a, 90, layout, optimize=True) == ist.encode_jpeg(b, 90, layout, optimize=True) == reference_of_photo(23, 18, 90, layout)


def test_round_trip_through_the_gpu_huffman_decoder(ist):
    """the library's own GPU entropy decoder takes the optimised file; its pixels are those of the standard file and PIL's"""
    from PIL import Image
    L = _lib()
    a = photo(150, 100)
    for layout in LAYOUTS:
        data, plain = ist.encode_jpeg(a, 90, layout, optimize=True), ist.encode_jpeg(a, 90, layout)
        assert len(data) < len(plain)
        want = np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))
        before = L.lib.ist_debug_gpu_entropy_files()
        tensors, _ = ist.decode_files_device([data])
        assert L.lib.ist_debug_gpu_entropy_files() == before + 1
        got = tensors[0].cpu().numpy()
        assert np.array_equal(got, want)
        assert np.array_equal(got, ist.decode_files_device([plain])[0][0].cpu().numpy())
        assert np.array_equal(ist.decode_image(data), want)


@pytest.mark.parametrize("direction,opts", STITCHES)
def test_stitch_jpeg_is_encode_jpeg_of_the_canvas(ist, direction, opts):
    imgs = three_images()
    canvas = ist.stitch(imgs, direction, opts)
    bms = [ist.upload_bitmap(a) for a in imgs]
    try:
        for q, layout in ((90, "420"), (50, "444")):
            want = reference(canvas["data"], q, layout)
            o = dict(opts, quality=q, subsampling=layout, optimize=True)
            res = ist.stitch_jpeg(imgs, direction, o)
            assert (res["width"], res["height"]) == (canvas["width"], canvas["height"])
            assert res["jpeg"] == ist.encode_jpeg(canvas["data"], q, layout, optimize=True) == want
            assert ist.stitch_jpeg(bms, direction, o)["jpeg"] == want
    finally:
        for b in bms:
            b.close()


# (pixels, quality, layout, optimize): different sizes, qualities and layouts, optimised and standard mixed; 33 x 700 is the file that
# spans rounds under BATCH_BUDGET
def batch_files():
    return [(photo(33, 700), 90, "420", True), (photo(7, 9), 50, "444", False), (noise(100, 150), 100, "444", True),
            (photo(1, 1), 1, "420", True), (photo(100, 150), 50, "420", False), (checker(48, 40), 100, "444", True)]


BATCH_BUDGET = 40000


def _want(a, q, layout, optimize):
    return reference(a, q, layout) if optimize else R.encode(a, q, layout)


def test_batch_mixes_optimised_and_standard_files_in_one_round(ist):
    import torch
    L = _lib()
    files = batch_files()
    cans = [torch.from_numpy(a).cuda() for a, _, _, _ in files]
    before = L.lib.ist_debug_jpeg_batch_launches(), L.lib.ist_debug_jpeg_histogram_launches()
    res = ist.encode_jpeg_batch_device(cans, [f[1] for f in files], [f[2] for f in files], optimize=[f[3] for f in files])
    torch.cuda.synchronize()
    assert L.lib.ist_debug_jpeg_batch_launches() == before[0] + 1          # one round: transformed once
    assert L.lib.ist_debug_jpeg_histogram_launches() == before[1] + 1
    for k, ((a, q, layout, o), (t, n), c) in enumerate(zip(files, res, cans)):
        got = t.cpu().numpy().tobytes()
        assert len(got) == n
        _same(got, _want(a, q, layout, o), "file %d against the reference" % k)
        s, _ = ist.encode_jpeg_device(c, q, layout, optimize=o)
        torch.cuda.synchronize()
        _same(got, s.cpu().numpy().tobytes(), "file %d against encode_jpeg_device" % k)


def test_batch_rounds(tmp_path):
    """a 40 000 byte budget: the optimised 33 x 700 file spans rounds, and rounds hold optimised and standard pieces.  The override is
    read once, in tuning mode, so the batch runs in a process of its own."""
    import ctypes as C
    code = """
import sys
sys.path.insert(0, %r)
import numpy as np
import torch
import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests.test_gpu_jpeg_optimize import batch_files
files = batch_files()
cans = [torch.from_numpy(a).cuda() for a, _, _, _ in files]
before = L.lib.ist_debug_jpeg_batch_launches()
res = ist.encode_jpeg_batch_device(cans, [f[1] for f in files], [f[2] for f in files], optimize=[f[3] for f in files])
torch.cuda.synchronize()
print("launches", L.lib.ist_debug_jpeg_batch_launches() - before)
np.savez(sys.argv[1], **{"f%%d" %% k: t.cpu().numpy() for k, (t, n) in enumerate(res)})
""" % (ROOT,)
    L = _lib()
    files = batch_files()
    n = len(files)
    w, h = (C.c_int64 * n)(*[f[0].shape[1] for f in files]), (C.c_int64 * n)(*[f[0].shape[0] for f in files])
    ss = (C.c_int * n)(*[{"444": 0, "420": 1}[f[2]] | (0x100 if f[3] else 0) for f in files])
    count = L.lib.ist_jpeg_batch_layout(w, h, ss, n, BATCH_BUDGET, None, 0)
    buf = (C.c_int32 * (4 * count))()
    assert L.lib.ist_jpeg_batch_layout(w, h, ss, n, BATCH_BUDGET, C.cast(buf, C.c_void_p), count) == count
    pieces = [tuple(buf[4 * p:4 * p + 4]) for p in range(count)]
    rounds = pieces[-1][1] + 1
    assert len({r for f, r, _, _ in pieces if f == 0}) > 1                  # the optimised 33 x 700 spans rounds
    env = dict(os.environ, IST_TUNING="1", IST_JPEG_ENC_BUDGET=str(BATCH_BUDGET))
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "out.npz")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    launches = int(r.stdout.split("launches")[1].split()[0])
    assert rounds < launches <= 2 * rounds, (launches, rounds)
    got = np.load(tmp_path / "out.npz")
    for k, (a, q, layout, o) in enumerate(files):
        _same(got["f%d" % k].tobytes(), _want(a, q, layout, o), "file %d" % k)


def test_stitch_jpeg_batch_with_optimize_per_request(ist):
    imgs = three_images()
    reqs = [(imgs, "vertical", {"quality": 90, "optimize": True}), (imgs[:2], "horizontal", {"gap": 3, "subsampling": "444"}),
            ([], "vertical", {"optimize": True}), (imgs[1:], "horizontal", {"quality": 50, "subsampling": "444", "optimize": True}),
            ([imgs[2]], "vertical", {"optimize": False})]
    got = ist.stitch_jpeg_batch(reqs)
    assert got[2] is None
    for k, (im, direction, o) in enumerate(reqs):
        if not im:
            continue
        plain = {key: v for key, v in o.items() if key not in ("quality", "subsampling", "optimize")}
        canvas = ist.stitch(im, direction, plain)["data"]
        want = _want(canvas, o.get("quality", 90), o.get("subsampling", "420"), o.get("optimize", False))
        _same(got[k]["jpeg"], want, "request %d against the reference" % k)
        _same(got[k]["jpeg"], ist.stitch_jpeg(im, direction, o)["jpeg"], "request %d against stitch_jpeg" % k)


def test_steady_state_allocates_nothing_and_histograms_are_counted_on_flagged_calls_only(ist):
    import torch
    L = _lib()
    a = photo(64, 48)
    canvas = torch.from_numpy(a).cuda()
    imgs = three_images()
    cans = [torch.from_numpy(photo(w, h)).cuda() for w, h in ((64, 48), (7, 9), (100, 30))]
    reqs = [(imgs, "vertical", {"optimize": True}), (imgs[:2], "horizontal", {})]

    def calls(optimize):
        ist.encode_jpeg(a, 90, "420", optimize=optimize)
        ist.encode_jpeg_device(canvas, 90, "444", optimize=optimize)
        ist.stitch_jpeg(imgs, "vertical", {"optimize": optimize})
        ist.encode_jpeg_batch_device(cans, optimize=[optimize, False, optimize])
        ist.stitch_jpeg_batch(reqs if optimize else [(r[0], r[1], {}) for r in reqs])
        torch.cuda.synchronize()

    calls(True)
    calls(False)
    allocs, hist = L.lib.ist_debug_device_allocs(), L.lib.ist_debug_jpeg_histogram_launches()
    calls(False)
    assert L.lib.ist_debug_jpeg_histogram_launches() == hist
    calls(True)
    assert L.lib.ist_debug_jpeg_histogram_launches() == hist + 5
    assert L.lib.ist_debug_device_allocs() == allocs
