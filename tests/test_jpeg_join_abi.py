"""ist_jpeg_join_check (include/imagestitch.h, 'lossless JPEG joins'): which sets of JPEG files can be joined in the coefficient
domain, decided from their headers alone, on the CPU.  One eligible set per layout and direction; one set per refusal reason, each
reporting the reason and the first failing image that tests/jpeg_join_reference.py::refusal states; the joined size equals
ist_plan_compute's canvas for the same images (mode 'min', gap 0, unlimited caps); the argument errors of both entry points, which
are raised before a context is touched.  No device is needed."""
import ctypes as C
import struct

import numpy as np
import pytest

from imagestitching_amd import _lib as L
from tests import jpeg_join_reference as JR
from tests.jpeg_writer import frame_from_pixels, photo, quant_table, write_jpeg

INVALID, NO_CONTEXT, UNSUPPORTED = -1, -4, -7
DIRS = {"vertical": L.VERTICAL, "horizontal": L.HORIZONTAL}
PNG = b"\x89PNG\r\n\x1a\n" + b"\x00" * 32


def check(blobs, direction):
    n = len(blobs)
    files = (C.c_char_p * n)(*blobs)
    lens = (C.c_int64 * n)(*[len(b) for b in blobs])
    info = L.JpegJoinInfo()
    rc = L.lib.ist_jpeg_join_check(files, lens, n, DIRS[direction], C.byref(info))
    return rc, info, L.last_error()


def frame(seed, h, w, layout="420", scale=0.6, **kw):
    return frame_from_pixels(photo(seed, h, w), layout, scale, **kw)


def with_orientation(data, orientation):
    """the file with an EXIF APP1 segment (little-endian TIFF, one IFD entry: tag 0x0112) behind SOI"""
    tiff = b"II*\x00" + struct.pack("<I", 8) + struct.pack("<H", 1) + struct.pack("<HHIHH", 0x0112, 3, 1, orientation, 0) + struct.pack("<I", 0)
    body = b"Exif\x00\x00" + tiff
    return data[:2] + b"\xff\xe1" + struct.pack(">H", len(body) + 2) + body + data[2:]


def with_height(data, height):
    """the file with another height in its frame header (the check reads headers only)"""
    at = data.index(b"\xff\xc0")
    return data[:at + 5] + struct.pack(">H", height) + data[at + 7:]


def plan_canvas(sizes, direction):
    n = len(sizes)
    descs = (L.ImageDesc * n)()
    for d, (h, w) in zip(descs, sizes):
        d.width, d.height, d.orientation, d.opaque = w, h, 1, 1
    lim = L.Limits()
    L.lib.ist_limits_unlimited(C.byref(lim))
    plan = L.Plan()
    assert L.lib.ist_plan_compute(descs, n, DIRS[direction], 0, 0.0, C.byref(lim), C.byref(plan)) == 0, L.last_error()
    try:
        assert plan.super_sample == 1.0
        return int(plan.canvas_w), int(plan.canvas_h)
    finally:
        L.lib.ist_plan_free(C.byref(plan))


@pytest.mark.parametrize("name", [n for n in JR.CASE_NAMES if "128" not in n] + ["128 images of one MCU, vertical 444"])
def test_every_case_of_the_list_is_eligible_and_its_size_is_the_planners_canvas(name):
    case = next(c for c in JR.CASES if c[0] == name)
    _, layout, direction, _, _ = case
    frames = JR.case_frames(name)
    rc, info, _ = check([write_jpeg(f) for f in frames], direction)
    assert rc == 0 and (info.reason, info.image) == (0, -1)
    assert JR.refusal([JR.describe(f) for f in frames], direction) == ("ok", -1)
    J = JR.join(frames, direction)
    assert (info.width, info.height) == (J.width, J.height) == plan_canvas(JR.case_sizes(case), direction)
    assert info.subsampling == {"444": 0, "420": 1}[layout]


def test_eligibility_reads_no_entropy_coded_byte_and_takes_every_scan_form():
    """non-interleaved, restart intervals, tables in front of their scans, optimal tables: all eligible; so are a progressive file
    and its baseline twin (Pillow's: jpeg_writer writes sequential scans only), and a file whose scan is cut off behind its header
    (the damage shows when the join decodes it)"""
    f = frame(1, 32, 48)
    forms = [write_jpeg(f), write_jpeg(f, scans=[[0], [1], [2]]), write_jpeg(f, restart=2),
             write_jpeg(f, scans=[[0], [2, 1]], tables="scan", huff="optimal"), write_jpeg(f, huff="optimal", fill=2, noise=True)]
    rc, info, _ = check(forms, "vertical")
    assert rc == 0 and (info.width, info.height) == (48, 32 * len(forms))
    pytest.importorskip("PIL")
    twins = [JR.pillow_file(photo(5, 32, 48), 2, progressive=p) for p in (True, False, True)]
    assert b"\xff\xc2" in twins[0] and b"\xff\xc2" not in twins[1]
    rc, info, _ = check(twins, "vertical")
    assert rc == 0 and (info.width, info.height, info.subsampling) == (48, 96, 1)
    whole = write_jpeg(f)
    cut = whole[:whole.index(b"\xff\xda") + 14 + 5]
    assert check([whole, cut], "vertical")[0] == 0


def refusals():
    a, b = frame(1, 32, 48), frame(2, 16, 48)
    out = {}
    add = lambda name, blobs, records, direction="vertical": out.__setitem__(name, (blobs, records, direction))
    J, D = write_jpeg, JR.describe
    add("a PNG", [J(a), PNG], [D(a), D(None, jpeg=False)])
    g = frame(3, 16, 48, "grey")
    add("a grey file", [J(a), J(g)], [D(a), D(g)])
    r = frame(4, 16, 48, "rgb")
    add("an rgb colour-space file", [J(r, marker="adobe0"), J(a)], [D(r), D(a)])
    s = frame(5, 16, 48, "422")
    add("4:2:2", [J(a), J(b), J(s)], [D(a), D(b), D(s)])
    f444 = frame(6, 16, 48, "444")
    add("mixed 4:4:4 / 4:2:0", [J(f444), J(frame(7, 16, 48, "444")), J(b)], [D(f444), D(f444), D(b)])
    other = frame(8, 16, 48, scale=0.5)
    add("a differing luma table", [J(a), J(other)], [D(a), D(other)])
    cbcr = frame(9, 16, 48, qtabs=[quant_table(0, 0.6), quant_table(1, 0.6), quant_table(1, 0.7)], tq=(0, 1, 2))
    add("Cb and Cr tables differ", [J(cbcr), J(a)], [D(cbcr), D(a)])
    late = frame(9, 16, 48, qtabs=[quant_table(0, 0.6), quant_table(1, 0.6), quant_table(1, 0.7)], tq=(0, 1, 2))
    add("Cb and Cr tables differ in a later image", [J(a), J(late)], [D(a), D(late)])
    wide = frame(10, 16, 48, qtabs=[quant_table(0, 6.0), quant_table(1, 0.6), quant_table(1, 0.6)])
    add("a 16-bit table", [J(wide, sof=1)], [D(wide)])
    narrow = frame(11, 16, 40)
    add("a width mismatch", [J(a), J(narrow)], [D(a), D(narrow)])
    tall = frame(12, 24, 48)
    add("a height mismatch, horizontal", [J(a), J(tall)], [D(a), D(tall)], "horizontal")
    add("a non-last height of 24 in 4:2:0", [J(a), J(tall), J(b)], [D(a), D(tall), D(b)])
    add("a non-last width of 24 in 4:2:0, horizontal", [J(frame(13, 32, 24)), J(a)], [D(frame(13, 32, 24)), D(a)], "horizontal")
    add("orientation 6", [J(a), with_orientation(J(b), 6)], [D(a), D(b, orientation=6)])
    one = frame(14, 8, 8, "444")
    add("129 files", [J(one)] * 129, [D(one)] * 129)
    big, heights = frame(15, 8, 8, "444"), (40000, 25528, 16)      # 65528 after two images, 65544 after three
    huge, recs = [with_height(J(big), h) for h in heights], []
    for h in heights:
        d = frame(15, 8, 8, "444")
        d.height = h
        recs.append(D(d))
    add("a joined height above 65535", huge, recs)
    return out


REFUSALS = refusals()
WANT = {"a PNG": ("not_jpeg", 1), "a grey file": ("layout", 1), "an rgb colour-space file": ("layout", 0), "4:2:2": ("layout", 2),
        "mixed 4:4:4 / 4:2:0": ("mixed", 2), "a differing luma table": ("tables", 1), "Cb and Cr tables differ": ("tables", 0),
        "Cb and Cr tables differ in a later image": ("tables", 1), "a 16-bit table": ("tables", 0), "a width mismatch": ("size", 1),
        "a height mismatch, horizontal": ("size", 1), "a non-last height of 24 in 4:2:0": ("align", 1),
        "a non-last width of 24 in 4:2:0, horizontal": ("align", 0), "orientation 6": ("orient", 1), "129 files": ("limit", 128),
        "a joined height above 65535": ("limit", 2)}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_a_refusal_names_its_reason_and_the_first_failing_image(name):
    blobs, records, direction = REFUSALS[name]
    want = WANT[name]
    assert JR.refusal(records, direction) == want, "the reference's own restatement"
    rc, info, msg = check(blobs, direction)
    assert rc == UNSUPPORTED
    assert (L.JOIN_REASONS[info.reason], info.image) == want
    assert (info.width, info.height) == (0, 0)
    assert msg.startswith("image %d: " % want[1]), msg


def test_the_decoders_message_is_kept_for_a_file_it_refuses():
    a = frame(1, 32, 48)
    twelve = bytearray(write_jpeg(a))
    at = bytes(twelve).index(b"\xff\xc0")
    twelve[at + 4] = 12                                   # sample precision
    rc, info, msg = check([write_jpeg(a), bytes(twelve)], "vertical")
    assert rc == UNSUPPORTED and (L.JOIN_REASONS[info.reason], info.image) == ("not_jpeg", 1)
    assert "only 8-bit JPEG is supported" in msg, msg
    rc, info, msg = check([write_jpeg(a)[:40]], "vertical")
    assert rc == UNSUPPORTED and L.JOIN_REASONS[info.reason] == "not_jpeg" and info.image == 0


def test_the_python_check_returns_the_record():
    import imagestitching_amd as ist
    frames = JR.case_frames("horizontal 420")
    got = ist.jpeg_join_check([write_jpeg(f) for f in frames], "horizontal")
    assert got == {"ok": True, "reason": "ok", "image": -1, "width": 57, "height": 24, "subsampling": "420"}
    blobs, _, direction = REFUSALS["orientation 6"]
    got = ist.jpeg_join_check(blobs, direction)
    assert got == {"ok": False, "reason": "orient", "image": 1, "width": 0, "height": 0, "subsampling": "420"}
    with pytest.raises(ValueError):
        ist.jpeg_join_check(blobs, "diagonal")
    with pytest.raises(ValueError):
        ist.jpeg_join_check([], "vertical")
    with pytest.raises(TypeError):
        ist.join_jpeg(blobs, "vertical", optimize=1)


def test_argument_errors_of_both_entry_points_need_no_device():
    blob = write_jpeg(frame(1, 16, 16))
    files = (C.c_char_p * 1)(blob)
    lens = (C.c_int64 * 1)(len(blob))
    info = L.JpegJoinInfo()
    chk = lambda f=files, ln=lens, n=1, d=0, o=C.byref(info): L.lib.ist_jpeg_join_check(f, ln, n, d, o)
    assert chk() == 0
    assert chk(o=None) == 0                               # (the record is optional)
    for bad in (dict(f=None), dict(ln=None), dict(n=0), dict(n=-3), dict(d=2), dict(d=-1)):
        assert chk(**bad) == INVALID and "ist_jpeg_join_check: bad argument" in L.last_error(), bad
    fake = C.c_void_p(8)                                  # (never dereferenced: every argument is checked before the context is used)
    out, m = C.POINTER(C.c_uint8)(), C.c_int64(7)
    join = lambda ctx=fake, f=files, ln=lens, n=1, d=0, flags=0, o=C.byref(out), mm=C.byref(m): \
        L.lib.ist_jpeg_join_files(ctx, f, ln, n, d, flags, C.byref(info), o, mm)
    assert join(ctx=None) == NO_CONTEXT
    assert join(ctx=None, flags=5, f=None) == NO_CONTEXT   # the context is looked at first
    for flags in (1, 0x101, 0x200, -1):
        assert join(flags=flags) == INVALID and "unknown flags" in L.last_error(), flags
    assert join(flags=3, f=None) == INVALID and "unknown flags" in L.last_error()      # ... then the flags
    for bad in (dict(f=None), dict(ln=None), dict(n=0), dict(d=7)):
        assert join(**bad) == INVALID and "ist_jpeg_join_files: bad argument" in L.last_error(), bad
    assert join(o=None) == INVALID and "NULL output" in L.last_error()
    assert join(mm=None) == INVALID and "NULL output" in L.last_error()
    # an ineligible set is refused before the context is used, the record is filled, and nothing is returned
    png = (C.c_char_p * 1)(PNG)
    launches = L.lib.ist_debug_jpeg_join_launches()
    assert join(f=png, ln=(C.c_int64 * 1)(len(PNG)), flags=0x100) == UNSUPPORTED
    assert (L.JOIN_REASONS[info.reason], info.image) == ("not_jpeg", 0) and not out and m.value == 0
    assert L.lib.ist_debug_jpeg_join_launches() == launches


def test_the_host_side_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the eligibility rule, the per-image table and the slab walk of the kernel's block mapping in a stand-alone program on the CPU
    (tools/run_fuzz.sh jpegjoin): seeded random sets with one defect or none, files with random damage, every walk checked"""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, IST_FUZZ_BIN=str(tmp_path / "check_jpeg_join_host"))
    r = subprocess.run([os.path.join(root, "tools", "run_fuzz.sh"), "jpegjoin", "300", "7"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "300 iterations" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    eligible, refused = int(re.search(r"(\d+) eligible", r.stdout).group(1)), int(re.search(r"(\d+) refused", r.stdout).group(1))
    assert eligible > 100 and refused > 30
