"""join_jpeg on the GPU: a strip of compatible JPEG files becomes one JPEG in the coefficient domain (include/imagestitch.h,
'lossless JPEG joins').  The file equals tests/jpeg_join_reference.py::expected_file byte for byte, with the Annex K tables and with
the file's own, for every case of the reference's list (the smallest shapes at which the kernel can go wrong: one MCU per image, a
single file, partial last columns and rows, image boundaries inside a workgroup's 32 blocks, rows of 33, 36 and 96 blocks, 128
images), through every route into the coefficient planes (GPU entropy decoder with and without restart intervals, sparse entries of
host-decoded sequential files, the dense planes of a progressive file, all of them in one join), across slabs, at the edge of the
coefficient range; the launch counters show that no transform, reconstruction or stitch launch is made.

jpeg_writer writes sequential scans only (its sof=2 is a frame marker over sequential scan headers, which no decoder takes), so the
progressive source is Pillow's; its Frame is built from the coefficients the library's GPU decoder reads from the file's baseline
twin (ist_debug_jpeg_gpu_coefficients, pinned against jpeg_writer by tests/test_gpu_jpeg_conformance.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import jpeg_join_reference as JR
from tests.jpeg_encode_reference import quant_tables
from tests.jpeg_writer import _new_frame, frame_from_pixels, photo, write_jpeg
from tests.test_gpu_jpeg_encode import first_difference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ist():
    import imagestitching_amd
    return imagestitching_amd


def lib():
    from imagestitching_amd import _lib
    return _lib


def same_file(got, want, what):
    assert got == want, "%s: %s" % (what, first_difference(got, want))


def counters():
    L = lib()
    return {"join": L.lib.ist_debug_jpeg_join_launches(), "transform": L.lib.ist_debug_jpeg_encode_launches(),
            "histogram": L.lib.ist_debug_jpeg_histogram_launches(), "gpu_files": L.lib.ist_debug_gpu_entropy_files(),
            "scaled": L.lib.ist_debug_jpeg_scaled_launches(), "batch": L.lib.ist_debug_batch_launches(),
            "direct": L.lib.ist_debug_direct_images()}


def moved(before):
    return {k: v - before[k] for k, v in counters().items() if v != before[k]}


@pytest.mark.parametrize("optimize", (False, True))
@pytest.mark.parametrize("name", JR.CASE_NAMES)
def test_a_case_equals_the_reference_byte_for_byte(ist, name, optimize):
    _, layout, direction, _, _ = next(c for c in JR.CASES if c[0] == name)
    frames = JR.case_frames(name)
    before = counters()
    got = ist.join_jpeg([write_jpeg(f) for f in frames], direction, optimize=optimize)
    same_file(got, JR.expected_file(frames, direction, optimize), "%s, %s tables" % (name, "optimised" if optimize else "Annex K"))
    # one slab: one join launch (the coefficients are kept for the optimised file), every source through the GPU entropy decoder,
    # and no transform, reduced-size reconstruction or stitch launch
    want = {"join": 1, "gpu_files": len(frames)}
    if optimize:
        want["histogram"] = 1
    assert moved(before) == want


def test_a_single_file_is_rewritten_in_the_exports_form(ist):
    for name in ("single file 420", "single file 444"):
        _, layout, direction, _, _ = next(c for c in JR.CASES if c[0] == name)
        f, = JR.case_frames(name)
        from tests.jpeg_encode_reference import mcus_per_row
        want = write_jpeg(f, sof=0, marker="jfif", huff="std", restart=mcus_per_row(f.width, layout))
        same_file(ist.join_jpeg([write_jpeg(f, huff="optimal", restart=3)], direction), want, name)


# ---- every route into the planes -------------------------------------------------------------------------------------------------
def q85_frames(layout):
    """48 wide, heights 32, 16, 48 (whole MCUs: a non-interleaved scan then carries every block of the planes), libjpeg's tables of
    quality 85 - the tables of the Pillow sources below"""
    ql, qc = quant_tables(85)
    return [frame_from_pixels(photo(300 + k, h, 48), layout, qtabs=[ql, qc, qc]) for k, h in enumerate((32, 16, 48))]


ROUTES = {"gpu": {}, "gpu restart": {"restart": 2}, "host sparse, non-interleaved": {"scans": [[0], [1], [2]]},
          "host sparse, three tables": {"huff": "optimal", "dc_slots": (0, 1, 2), "ac_slots": (0, 1, 2)}}


@pytest.mark.parametrize("layout", ("420", "444"))
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_sequential_sources_by_every_route(ist, layout, route):
    frames = q85_frames(layout)
    want = JR.expected_file(frames, "vertical")
    before = counters()
    same_file(ist.join_jpeg([write_jpeg(f, **ROUTES[route]) for f in frames], "vertical"), want, route)
    assert moved(before).get("gpu_files", 0) == (3 if route.startswith("gpu") else 0), route


def pillow_frame(ist, rgb, subsampling, layout):
    """the Frame of Pillow's file of these pixels: the coefficients the GPU decoder reads from the baseline file"""
    data = JR.pillow_file(rgb, subsampling)
    got = ist.debug_jpeg_gpu_coefficients(data)
    assert got["ok"]
    ql, qc = quant_tables(85)
    f = _new_frame(rgb.shape[1], rgb.shape[0], layout, [ql, qc, qc])
    for c, p in zip(f.comps, got["planes"]):
        assert c["coef"].shape == p.shape
        c["coef"] = p.astype(np.int64)
    return f


@pytest.mark.parametrize("layout,subsampling", (("420", 2), ("444", 0)))
def test_a_progressive_source_and_all_four_routes_in_one_join(ist, layout, subsampling):
    pytest.importorskip("PIL")
    rgb = photo(77, 32, 48)
    fp = pillow_frame(ist, rgb, subsampling, layout)
    progressive = JR.pillow_file(rgb, subsampling, progressive=True)
    assert b"\xff\xc2" in progressive
    for optimize in (False, True):
        before = counters()
        same_file(ist.join_jpeg([progressive], "vertical", optimize=optimize), JR.expected_file([fp], "vertical", optimize), "progressive alone")
        assert moved(before).get("gpu_files", 0) == 0
    f = q85_frames(layout)
    files = [write_jpeg(f[0]), write_jpeg(f[1], restart=2), progressive, write_jpeg(f[2], scans=[[0], [1], [2]])]
    frames = [f[0], f[1], fp, f[2]]
    for direction in ("vertical",):
        before = counters()
        same_file(ist.join_jpeg(files, direction), JR.expected_file(frames, direction), "four routes")
        assert moved(before) == {"join": 1, "gpu_files": 2}
    # side by side (equal heights): progressive | GPU | host sparse
    g = frame_from_pixels(photo(78, 32, 32), layout, qtabs=[c["q"] for c in fp.comps])
    files = [progressive, write_jpeg(f[0]), write_jpeg(g, scans=[[1], [0], [2]])]
    same_file(ist.join_jpeg(files, "horizontal", optimize=True), JR.expected_file([fp, f[0], g], "horizontal", True), "three routes, horizontal")


@pytest.mark.parametrize("subsampling,layout", ((0, "444"), (2, "420")))
@pytest.mark.parametrize("direction", ("vertical", "horizontal"))
def test_pillow_made_sources_join_to_what_pillow_sees_side_by_side(ist, subsampling, layout, direction):
    """no Frame exists for them: Pillow's decode of the joined file is Pillow's decodes of the sources side by side (for 4:2:0 but
    for the one row or column on each side of each seam: tests/test_jpeg_join_reference.py)"""
    pytest.importorskip("PIL")
    sizes = [(h, 48) if direction == "vertical" else (48, h) for h in (32, 16, 48)]
    sources = [JR.pillow_file(photo(500 + k, h, w), subsampling, progressive=(k == 1)) for k, (h, w) in enumerate(sizes)]
    for optimize in (False, True):
        joined = ist.join_jpeg(sources, direction, optimize=optimize)
        differing, allowed = JR.witness_mismatch(joined, sources, direction, layout)
        assert set(differing) <= allowed, (differing, sorted(allowed))
    assert len(joined) < sum(len(s) for s in sources)      # (one header, and tables made for the whole strip)


# ---- slabs -------------------------------------------------------------------------------------------------------------------------
SLAB_SETS = {"seams inside slabs": ("420", 40, (16, 32, 9)), "seams on slab edges": ("420", 40, (32, 32, 16)), "444": ("444", 33, (8, 24, 3))}

CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
import imagestitching_amd as ist
from imagestitching_amd import _lib as L
src = np.load(sys.argv[1])
out = {}
for name in sorted(set(k.split("/")[0] for k in src.files)):
    files = [src[k].tobytes() for k in sorted(src.files) if k.split("/")[0] == name]
    for optimize in (False, True):
        before = L.lib.ist_debug_jpeg_join_launches(), L.lib.ist_debug_jpeg_encode_launches()
        out["%%s/%%d" %% (name, optimize)] = np.frombuffer(ist.join_jpeg(files, "vertical", optimize=optimize), np.uint8)
        print("launches", name, int(optimize), L.lib.ist_debug_jpeg_join_launches() - before[0], L.lib.ist_debug_jpeg_encode_launches() - before[1])
np.savez(sys.argv[2], **out)
""" % (ROOT,)


@pytest.mark.parametrize("rows", (1, 2))
def test_slabs_of_one_and_two_mcu_rows_in_a_child_process(tmp_path, rows):
    """IST_TUNING=1 IST_JPEG_ENC_ROWS cuts the small files into slabs: a seam on a slab edge, a seam inside a slab, three and more
    slabs; with optimised tables every slab is filled twice (the join launch count doubles) and the bytes are still the reference's"""
    frames = {name: [frame_from_pixels(photo(900 + k, h, w), layout, 0.6) for k, h in enumerate(heights)]
              for name, (layout, w, heights) in SLAB_SETS.items()}
    np.savez(tmp_path / "src.npz", **{"%s/%d" % (name, k): np.frombuffer(write_jpeg(f), np.uint8) for name, fs in frames.items() for k, f in enumerate(fs)})
    env = dict(os.environ, IST_TUNING="1", IST_JPEG_ENC_ROWS=str(rows))
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "src.npz"), str(tmp_path / "out.npz")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(tmp_path / "out.npz")
    for name, (layout, w, heights) in SLAB_SETS.items():
        mcu = 16 if layout == "420" else 8
        mcu_rows = -(-sum(heights) // mcu)
        slabs = -(-mcu_rows // rows)
        assert slabs >= (3 if rows == 1 or name != "seams inside slabs" else 2)
        for optimize in (False, True):
            same_file(got["%s/%d" % (name, optimize)].tobytes(), JR.expected_file(frames[name], "vertical", optimize), "%s, %d rows per slab, optimize %s" % (name, rows, optimize))
            assert "launches %s %d %d 0\n" % (name, optimize, slabs * (2 if optimize else 1)) in r.stdout, r.stdout


# ---- the coefficient range ---------------------------------------------------------------------------------------------------------
def range_frames(layout, dc=(-1024, 1023), ac=(-1023, 1023)):
    ones = np.ones(64, np.int64)
    out = []
    for k in range(2):
        f = _new_frame(32, 16, layout, [ones] * 3)
        rng = np.random.default_rng(40 + k)
        for c in f.comps:
            co = c["coef"]
            co[..., 0] = rng.choice(dc, co.shape[:2])
            co.reshape(-1, 64)[0, 0], co.reshape(-1, 64)[1, 0] = dc          # both ends, and the largest difference between them
            for z in (1, 5, 63):
                co[..., z] = rng.choice(ac + (0,), co.shape[:2])
        out.append(f)
    return out


@pytest.mark.parametrize("layout", ("420", "444"))
def test_the_ends_of_the_coefficient_range_join_byte_for_byte(ist, layout):
    frames = range_frames(layout)
    for optimize in (False, True):
        for opts in ({}, {"scans": [[0], [1], [2]]}):
            same_file(ist.join_jpeg([write_jpeg(f, **opts) for f in frames], "vertical", optimize=optimize),
                      JR.expected_file(frames, "vertical", optimize), "range ends, optimize %s, %s" % (optimize, opts))


@pytest.mark.parametrize("dc", (1024, -1025))
def test_a_dc_outside_the_range_is_refused_and_nothing_is_returned(ist, dc):
    """jpeg_writer can state such a file: the DC DIFFERENCE stays within +-2047 (category 11), which the Annex K table codes.  An AC
    outside +-1023 needs category 11, which no baseline AC table has: jpeg_writer cannot state that one."""
    L = lib()
    good, bad = range_frames("420")
    bad.comps[1]["coef"][0, 1, 0] = dc
    bad.comps[1]["coef"][0, 0, 0] = 0                      # (differences within +-2047)
    ctx = sys.modules["imagestitching_amd.stitch"]._ctx(0)
    ist.join_jpeg([write_jpeg(good), write_jpeg(good)], "vertical")      # (scratch of this shape exists)
    handles = (C.c_int64 * 4)()
    L.lib.ist_debug_live_handles(handles)
    before, live = counters(), list(handles)
    for opts in ({}, {"scans": [[0], [1], [2]]}):
        blobs = [write_jpeg(good), write_jpeg(bad, **opts)]
        n = len(blobs)
        files, lens = (C.c_char_p * n)(*blobs), (C.c_int64 * n)(*[len(b) for b in blobs])
        info, out, m = L.JpegJoinInfo(), C.POINTER(C.c_uint8)(), C.c_int64(-1)
        rc = L.lib.ist_jpeg_join_files(ctx, files, lens, n, 0, 0, C.byref(info), C.byref(out), C.byref(m))
        assert rc == -7 and L.JOIN_REASONS[info.reason] == "range" and info.image == -1, L.last_error()
        assert not out and m.value == 0
        with pytest.raises(L.StitchError, match="lossless"):
            ist.join_jpeg(blobs, "vertical", optimize=True)
    L.lib.ist_debug_live_handles(handles)
    assert list(handles) == live
    assert moved(before).get("transform", 0) == 0
    # the context is as good as before
    frames = [good, good]
    same_file(ist.join_jpeg([write_jpeg(f) for f in frames], "vertical"), JR.expected_file(frames, "vertical"), "after a refusal")


# ---- book-keeping ------------------------------------------------------------------------------------------------------------------
def test_a_repeated_shape_allocates_nothing_and_leaves_no_handle(ist):
    L = lib()
    frames = JR.case_frames("partial column and row 420")
    files = [write_jpeg(f) for f in frames]
    want = JR.expected_file(frames, "vertical", True)
    same_file(ist.join_jpeg(files, "vertical", optimize=True), want, "first call")
    handles = (C.c_int64 * 4)()
    L.lib.ist_debug_live_handles(handles)
    allocs, live, before = L.lib.ist_debug_device_allocs(), list(handles), counters()
    for _ in range(3):
        same_file(ist.join_jpeg(files, "vertical", optimize=True), want, "repeated call")
    L.lib.ist_debug_live_handles(handles)
    assert L.lib.ist_debug_device_allocs() == allocs and list(handles) == live
    assert moved(before) == {"join": 3, "histogram": 3, "gpu_files": 9}


def test_a_refused_set_and_a_damaged_scan_leave_no_file_and_no_held_block(ist):
    L = lib()
    frames = JR.case_frames("partial column and row 420")
    files = [write_jpeg(f) for f in frames]
    ist.join_jpeg(files, "vertical")
    handles = (C.c_int64 * 4)()
    L.lib.ist_debug_live_handles(handles)
    live, before = list(handles), counters()
    with pytest.raises(L.StitchError, match="image 1: .*last image") as e:
        ist.join_jpeg([files[0], files[2], files[1]], "vertical")        # a height of 9 in the middle
    assert e.value.code == -7
    with pytest.raises(L.StitchError, match="image 1: .*layout differs"):
        ist.join_jpeg([files[0], write_jpeg(frame_from_pixels(photo(1, 16, 40), "444", 0.6))], "vertical")
    assert moved(before) == {}
    whole = write_jpeg(frames[1], restart=1)
    cut = whole[:whole.index(b"\xff\xd0")]                                # eligible by its headers; its scan ends in front of RST0
    with pytest.raises(L.StitchError) as e:
        ist.join_jpeg([files[0], cut, files[2]], "vertical")
    assert e.value.code == -6 and "图片1解码异常" in str(e.value), str(e.value)
    L.lib.ist_debug_live_handles(handles)
    assert list(handles) == live
    same_file(ist.join_jpeg(files, "vertical"), JR.expected_file(frames, "vertical"), "after the failures")
