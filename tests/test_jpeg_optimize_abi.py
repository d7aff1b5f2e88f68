"""The CPU side of the JPEG export's optimised Huffman tables (IST_JPEG_OPTIMIZE): ist_jpeg_optimal_table against
tests/jpeg_writer.py::optimal_table, the bound and the batch layout with the flag, every entry point's argument checks without a device,
the option checks of the Python and Node hosts, and what the numpy contract itself promises for the inputs of the GPU tests."""
import ctypes as C
import io
import json
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests import jpeg_encode_reference as R
from tests import jpeg_writer as JW
from tests.test_gpu_jpeg_encode import checker, noise, photo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "node", "imagestitch.node")
needs_node = pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
J444, J420, OPT = 0, 1, 0x100
INVALID, NO_CONTEXT, UNSUPPORTED = -1, -4, -7


def table(freq):
    f = (C.c_int64 * 256)(*[int(x) for x in freq])
    bits, vals, n = (C.c_uint8 * 16)(), (C.c_uint8 * 256)(), C.c_int(-1)
    assert L.lib.ist_jpeg_optimal_table(f, bits, vals, C.byref(n)) == 0
    return list(bits), list(vals)[:n.value]


def check_table(freq, what):
    freq = np.asarray(freq, dtype=object)
    bits, vals = table(freq)
    want_bits, want_vals = JW.optimal_table([int(x) for x in freq])
    assert bits == list(want_bits) and vals == list(want_vals), what
    # one value per counted symbol, lengths 1..16 by construction of BITS; with the reserved point the Kraft sum is at most 1, and no
    # code is all ones: the canonical code after the last one is still inside its length
    assert sorted(vals) == [s for s in range(256) if freq[s] > 0] and sum(bits) == len(vals), what
    kraft = sum(Fraction(n, 1 << (l + 1)) for l, n in enumerate(bits))
    if vals:
        longest = max(l + 1 for l, n in enumerate(bits) if n)
        assert kraft + Fraction(1, 1 << longest) <= 1, what
        code = 0
        for l in range(1, 17):
            code = (code + bits[l - 1]) << 1
            assert bits[l - 1] == 0 or (code >> 1) - 1 < (1 << l) - 1, (what, l)      # the last code of length l is not all ones
    else:
        assert bits == [0] * 16
    return bits, vals


def vec(pairs):
    f = [0] * 256
    for s, n in pairs:
        f[s] = n
    return f


def test_optimal_table_equals_the_reference_on_chosen_vectors():
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    cases = {
        "one symbol": vec([(5, 7)]),
        "one symbol, the last": vec([(255, 1)]),
        "two equal counts": vec([(0, 9), (1, 9)]),
        "162 equal counts": vec([(s, 3) for s in range(162)]),
        "256 symbols": [1 + (s * 37) % 101 for s in range(256)],
        "256 equal": [5] * 256,
        "fibonacci": vec(list(enumerate(fib))),
        "geometric": vec([(s, 2 ** s) for s in range(25)]),
        "geometric, descending": vec([(s, 3 ** (24 - s)) for s in range(25)]),
        "many ties": vec([(s, 1 + s // 40) for s in range(0, 256, 2)]),
        "near 2^40": vec([(s, (1 << 40) - s * s) for s in range(200)]),
        "near 2^40 and ones": vec([(s, (1 << 40) + s) for s in range(100)] + [(s, 1) for s in range(100, 256)]),
        "empty": [0] * 256,
    }
    for what, f in cases.items():
        bits, vals = check_table(f, what)
        if what == "fibonacci":
            assert bits[15] > 0 and sum(bits) == 30                          # depth 29: the limit of step 4 was applied
        if what == "empty":
            assert (bits, vals) == ([0] * 16, [])
    assert table(vec([(5, 7)])) == ([1] + [0] * 15, [5])


def test_optimal_table_equals_the_reference_on_seeded_random_vectors():
    rng = np.random.default_rng(2024)
    for t in range(300):
        k = int(rng.integers(1, 257))
        f = np.zeros(256, np.int64)
        idx = rng.choice(256, k, replace=False)
        kind = t % 4
        if kind == 0:
            f[idx] = rng.integers(1, 1000, k)
        elif kind == 1:
            f[idx] = rng.integers(1, 4, k)                                     # ties everywhere
        elif kind == 2:
            f[idx] = 1 << rng.integers(0, 33, k)                               # deep trees (at most 34 + log2(256): under the reference's 39)
        else:
            f[idx] = rng.integers(1, 1 << 40, k)
        check_table(f, "random %d" % t)


def test_optimal_table_is_not_limited_to_depth_39():
    """Fibonacci counts over 60 symbols: a tree of depth 59, which the reference cannot build (its arrays end at 39); the table is
    still a valid one for exactly these symbols"""
    fib = [1, 1]
    while len(fib) < 60:
        fib.append(fib[-1] + fib[-2])
    f = vec(list(enumerate(fib)))
    with pytest.raises(IndexError):
        JW.optimal_table(f)
    bits, vals = table(f)
    assert sorted(vals) == list(range(60)) and sum(bits) == 60
    assert sum(Fraction(n, 1 << (l + 1)) for l, n in enumerate(bits)) + Fraction(1, 1 << 16) <= 1
    # HUFFVAL is ordered by the size BEFORE the limit: the tree is a chain (each count outweighs all smaller ones together), symbol 59
    # at depth 1 down to symbol 2, then symbols 0 and 1 (merged first, with the reserved symbol joining them next) at the bottom
    assert vals == list(range(59, 1, -1)) + [0, 1]


def test_optimal_table_rejects_bad_arguments():
    f = (C.c_int64 * 256)(*([1] * 256))
    bits, vals, n = (C.c_uint8 * 16)(), (C.c_uint8 * 256)(), C.c_int(0)
    assert L.lib.ist_jpeg_optimal_table(None, bits, vals, C.byref(n)) == INVALID
    assert L.lib.ist_jpeg_optimal_table(f, None, vals, C.byref(n)) == INVALID
    assert L.lib.ist_jpeg_optimal_table(f, bits, None, C.byref(n)) == INVALID
    assert L.lib.ist_jpeg_optimal_table(f, bits, vals, None) == INVALID
    f[200] = -1
    assert L.lib.ist_jpeg_optimal_table(f, bits, vals, C.byref(n)) == INVALID and "negative" in L.last_error()


def test_flagged_bound():
    bound = L.lib.ist_jpeg_bound
    for ss in (J444, J420):
        for w, h in ((1, 1), (7, 9), (17, 33), (4805, 19), (65535, 65535)):
            m = 16 if ss == J420 else 8
            mx, my = -(-w // m), -(-h // m)
            blocks = mx * (6 if ss == J420 else 3)
            assert bound(w, h, ss | OPT) == 1024 + my * (blocks * 417 + 16) >= bound(w, h, ss) == 1024 + my * (blocks * 415 + 16)
        for w in (1, 8, 9, 16, 17, 1000, 65535):
            assert bound(min(w + 1, 65535), 40, ss | OPT) >= bound(w, 40, ss | OPT) > 0
            assert bound(40, min(w + 1, 65535), ss | OPT) >= bound(40, w, ss | OPT) > 0
        prev = 0
        for side in range(1, 70):
            b = bound(side, side, ss | OPT)
            assert b >= prev
            prev = b
    for w, h, ss in ((0, 1, J420 | OPT), (1, 0, J420 | OPT), (-3, 5, J444 | OPT), (65536, 1, J420 | OPT), (1, 65536, J444 | OPT),
                     (8, 8, 0x200), (8, 8, 0x102), (8, 8, OPT | 2), (8, 8, 2), (8, 8, 3), (8, 8, 7), (8, 8, -1), (8, 8, 0x201), (8, 8, 0x300)):
        assert bound(w, h, ss) < 0, (w, h, ss)


@pytest.mark.parametrize("layout,ss", (("420", J420), ("444", J444)))
def test_flagged_bound_holds_for_the_worst_contents(layout, ss):
    for w, h in ((1, 1), (7, 9), (17, 33), (48, 64), (100, 150)):
        for make in (noise, checker):
            n = len(reference(make(w, h), 100, layout))
            assert L.lib.ist_jpeg_bound(w, h, ss | OPT) >= n, (w, h, layout, make.__name__)


class Piece(C.Structure):
    _fields_ = [("file", C.c_int32), ("round", C.c_int32), ("mcu_row0", C.c_int32), ("mcu_rows", C.c_int32)]


def layout_of(sizes, budget):
    n = len(sizes)
    w, h, ss = (C.c_int64 * n)(*[s[0] for s in sizes]), (C.c_int64 * n)(*[s[1] for s in sizes]), (C.c_int * n)(*[s[2] for s in sizes])
    count = L.lib.ist_jpeg_batch_layout(w, h, ss, n, budget, None, 0)
    if count < 0:
        return count
    buf = (Piece * count)()
    assert L.lib.ist_jpeg_batch_layout(w, h, ss, n, budget, C.cast(buf, C.c_void_p), count) == count
    return [(p.file, p.round, p.mcu_row0, p.mcu_rows) for p in buf]


def test_batch_layout_costs_a_flagged_row_at_the_417_byte_slot():
    def cost(w, ss):
        m = 16 if (ss & 1) else 8
        blocks = -(-w // m) * (6 if (ss & 1) else 3)
        return blocks * 128 + ((blocks * (417 if ss & OPT else 415) + 2 + 15) & ~15)

    for ss in (J420, J444):
        w = 1000
        plain, flagged = cost(w, ss), cost(w, ss | OPT)
        assert flagged > plain
        # a budget of exactly three flagged rows: three rows a round with the flag; a byte less: two
        assert [p[3] for p in layout_of([(w, 200, ss | OPT)], 3 * flagged)][:2] == [3, 3]
        assert [p[3] for p in layout_of([(w, 200, ss | OPT)], 3 * flagged - 1)][:2] == [2, 2]
        assert [p[3] for p in layout_of([(w, 200, ss)], 3 * flagged - 1)][:2] == [3, 3]
    # mixed files follow the greedy rule with each file's own cost
    sizes = [(33, 170, J444 | OPT), (7, 9, J420), (33, 700, J420 | OPT), (17, 33, J444)]
    budget = 40000
    want, rnd, used = [], 0, 0
    for f, (w, h, ss) in enumerate(sizes):
        rows, c, r = -(-h // (16 if ss & 1 else 8)), cost(w, ss), 0
        while r < rows:
            if used > 0 and used + c > budget:
                rnd, used = rnd + 1, 0
            take = min(max(1, (budget - used) // c), rows - r)
            want.append((f, rnd, r, take))
            used, r = used + take * c, r + take
    assert layout_of(sizes, budget) == want
    for bad in (0x200, 0x102, OPT | 2, 2, -1):
        assert layout_of([(16, 16, J420), (16, 16, bad)], 0) < 0


def test_every_entry_point_accepts_the_flag_as_far_as_the_checks_without_a_device():
    fake = C.c_void_p(8)                                   # (never dereferenced: every argument is checked before the context is used)
    px = np.zeros((4, 4, 4), np.uint8)
    p, buf = px.ctypes.data, C.c_void_p(4096)              # (a 16-byte aligned "device" address, never dereferenced either)
    n, out, plan = C.c_int64(0), C.POINTER(C.c_uint8)(), L.Plan()
    before = L.lib.ist_debug_jpeg_encode_launches(), L.lib.ist_debug_jpeg_batch_launches(), L.lib.ist_debug_jpeg_histogram_launches()
    unknown = (0x200, 0x102, OPT | 2, OPT | 7, 2, 3, 7, -1)
    for flagged in (J420 | OPT, J444 | OPT):
        dev = lambda ctx=fake, canvas=p, pitch=16, w=4, h=4, q=90, ss=flagged, o=buf, cap=1 << 20, ln=C.byref(n): \
            L.lib.ist_jpeg_encode_device(ctx, canvas, pitch, w, h, q, ss, o, cap, ln, None)
        assert dev(ctx=None) == NO_CONTEXT
        assert dev(q=0) == dev(q=101) == INVALID
        assert all(dev(ss=s) == INVALID and "unknown subsampling" in L.last_error() for s in unknown)
        assert dev(canvas=None) == dev(o=None) == dev(ln=None) == dev(w=0) == dev(h=0) == dev(pitch=12) == INVALID
        # the bound that is asked for is the flagged one
        assert dev(cap=L.lib.ist_jpeg_bound(4, 4, flagged) - 1) == INVALID and "ist_jpeg_bound" in L.last_error()
        assert L.lib.ist_jpeg_bound(4, 4, flagged) - 1 >= L.lib.ist_jpeg_bound(4, 4, flagged & 1)
        assert dev(o=C.c_void_p(4100)) == INVALID and "aligned" in L.last_error()
        assert dev(w=65536, pitch=4 * 65536) == UNSUPPORTED and "width" in L.last_error()
        assert dev(h=65536) == UNSUPPORTED and "height" in L.last_error()

        host = lambda ctx=fake, pixels=p, pitch=16, w=4, h=4, q=90, ss=flagged, o=C.byref(out), ln=C.byref(n): \
            L.lib.ist_jpeg_encode_rgba8(ctx, pixels, pitch, w, h, q, ss, o, ln)
        assert host(ctx=None) == NO_CONTEXT
        assert host(q=0) == host(pixels=None) == host(w=0) == host(pitch=8) == host(o=None) == host(ln=None) == INVALID
        assert all(host(ss=s) == INVALID for s in unknown)
        assert host(h=65536) == UNSUPPORTED

        descs = (L.ImageDesc * 1)(L.ImageDesc(4, 4, 1, 0, 0, 0, 0))
        ptrs, pitches = (C.c_void_p * 1)(p), (C.c_size_t * 1)(16)
        st = lambda ctx=fake, q=90, ss=flagged, pl=C.byref(plan), o=C.byref(out), ln=C.byref(n): \
            L.lib.ist_stitch_jpeg(ctx, descs, ptrs, pitches, 1, 0, 0, 0.0, None, 1, q, ss, pl, o, ln)
        assert st(ctx=None) == NO_CONTEXT
        assert st(q=0) == st(q=101) == st(pl=None) == st(o=None) == st(ln=None) == INVALID
        assert all(st(ss=s) == INVALID for s in unknown)
        bms = (C.c_void_p * 1)()
        sb = lambda ctx=fake, nb=1, q=90, ss=flagged, pl=C.byref(plan), o=C.byref(out), ln=C.byref(n): \
            L.lib.ist_stitch_bitmaps_jpeg(ctx, bms, nb, 0, 0, 0.0, None, 1, q, ss, pl, o, ln)
        assert sb(ctx=None) == NO_CONTEXT
        assert sb(q=0) == sb(pl=None) == sb(o=None) == INVALID
        assert all(sb(ss=s) == INVALID for s in unknown)
        assert sb(nb=0) == 1                                   # IST_NOTHING_TO_DO
        assert sb() == -6                                      # a NULL bitmap (the flag passed the option check): '图片0解码异常'

        # the batch encoder: file 1 carries the flag
        def batch(ctx=fake, q1=90, ss1=flagged, cap1=1 << 20, o1=4096 + 4096):
            cv, pt = (C.c_void_p * 2)(p, p), (C.c_size_t * 2)(16, 16)
            w, h = (C.c_int64 * 2)(4, 4), (C.c_int64 * 2)(4, 4)
            q, ss = (C.c_int * 2)(90, q1), (C.c_int * 2)(J420, ss1)
            o, cap, ln = (C.c_void_p * 2)(4096, o1), (C.c_int64 * 2)(1 << 20, cap1), (C.c_int64 * 2)()
            return L.lib.ist_jpeg_encode_batch_device(ctx, cv, pt, w, h, q, ss, 2, o, cap, ln, None)
        assert batch(ctx=None) == NO_CONTEXT
        assert batch(q1=0) == INVALID and "file 1" in L.last_error()
        assert all(batch(ss1=s) == INVALID and "file 1" in L.last_error() for s in unknown)
        assert batch(cap1=L.lib.ist_jpeg_bound(4, 4, flagged) - 1) == INVALID and "file 1" in L.last_error() and "ist_jpeg_bound" in L.last_error()
        assert batch(o1=4100) == INVALID and "aligned" in L.last_error()

        # the stitch batch: the options are checked before the context
        reqs = (L.StitchRequest * 1)()
        plans, outs, lens = (L.Plan * 1)(), (C.POINTER(C.c_uint8) * 1)(), (C.c_int64 * 1)()
        sj = lambda ctx=fake, q=90, ss=flagged: L.lib.ist_stitch_jpeg_batch(ctx, reqs, 1, (C.c_int * 1)(q), (C.c_int * 1)(ss), plans, outs, lens)
        assert sj(ctx=None) == NO_CONTEXT
        assert sj(q=0) == INVALID and "request 0" in L.last_error()
        assert all(sj(ss=s) == INVALID and "request 0" in L.last_error() for s in unknown)
    assert before == (L.lib.ist_debug_jpeg_encode_launches(), L.lib.ist_debug_jpeg_batch_launches(), L.lib.ist_debug_jpeg_histogram_launches())


def test_debug_counts_refuses_bad_arguments_without_a_device():
    """ist_debug_jpeg_counts: every argument is checked before the context is used (what the block holds needs a context: that refusal is
    in tests/test_gpu_jpeg_encode_regimes.py)"""
    fake = C.c_void_p(8)                                   # (never dereferenced)
    out = (C.c_int64 * 1088)()
    before = L.lib.ist_debug_jpeg_encode_launches(), L.lib.ist_debug_jpeg_histogram_launches()
    assert L.lib.ist_debug_jpeg_counts(None, out, 544) == NO_CONTEXT
    assert L.lib.ist_debug_jpeg_counts(fake, None, 544) == INVALID
    for n in (-544, -1, 1, 16, 272, 543, 545, 1087):
        assert L.lib.ist_debug_jpeg_counts(fake, out, n) == INVALID and "544" in L.last_error(), n
    assert before == (L.lib.ist_debug_jpeg_encode_launches(), L.lib.ist_debug_jpeg_histogram_launches())
    header = open(os.path.join(ROOT, "include", "imagestitch.h")).read()
    assert "IST_API int ist_debug_jpeg_counts(ist_ctx* ctx, int64_t* out, int64_t n);" in header


def test_python_wrappers_check_optimize():
    px = np.zeros((4, 4, 4), np.uint8)
    for bad in (1, 0, "yes", None, np.bool_(True), [True]):
        with pytest.raises(TypeError, match="optimize"):
            ist.encode_jpeg(px, optimize=bad)
        with pytest.raises(TypeError, match="optimize"):
            ist.stitch_jpeg([px], "vertical", {"optimize": bad})
        with pytest.raises(TypeError, match="request 0: optimize"):
            ist.stitch_jpeg_batch([([px], "vertical", {"optimize": bad})])
    # the device entry points check the option before they look at a canvas: no GPU is needed to be refused
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="optimize"):
            ist.encode_jpeg_device(px, optimize=bad)
        with pytest.raises(TypeError, match="file 0: optimize"):
            ist.encode_jpeg_batch_device([px, px], optimize=bad)
    with pytest.raises(TypeError, match="file 1: optimize"):
        ist.encode_jpeg_batch_device([px, px], optimize=[True, 1])
    with pytest.raises(TypeError, match="file 1: optimize"):
        ist.encode_jpeg_batch_device([px, px], optimize=(False, "yes"))
    with pytest.raises(ValueError, match="optimize"):
        ist.encode_jpeg_batch_device([px, px], optimize=[True])          # a sequence of the wrong length
    with pytest.raises(TypeError, match="request 1: optimize"):
        ist.stitch_jpeg_batch([([px], "vertical", {"optimize": True}), ([px], "vertical", {"optimize": 1})])
    with pytest.raises(TypeError, match="unknown"):
        ist.stitch_jpeg([px], "vertical", {"optimize": True, "nonsense": 1})
    with pytest.raises(ValueError):
        ist.stitch_jpeg([px], "vertical", {"optimize": True, "quality": 0})
    assert ist.stitch_jpeg([], "vertical", {"optimize": True}) is None
    assert "optimize" not in ist.DEFAULT_OPTS                              # the other hosts keep refusing it
    with pytest.raises(TypeError, match="unknown"):
        ist.plan([{"width": 4, "height": 4}], "vertical", {"optimize": True})
    # after the existing parameters: positional callers are unaffected
    import inspect
    assert list(inspect.signature(ist.encode_jpeg).parameters) == ["pixels", "quality", "subsampling", "device", "optimize"]
    assert list(inspect.signature(ist.encode_jpeg_device).parameters) == ["canvas", "quality", "subsampling", "out", "stream", "optimize"]
    assert list(inspect.signature(ist.encode_jpeg_batch_device).parameters) == ["canvases", "quality", "subsampling", "outs", "stream", "optimize"]


@needs_node
def test_node_option_checks():
    code = """
const api = require('%s/node/index.js');
const out = {errors: []};
const px = new Uint8Array(64);
for (const o of [{optimize: 1}, {optimize: 'yes'}, {optimize: 0}])
  try { api.encodeJpeg(px, 4, 4, o); out.errors.push('accepted'); } catch (e) { out.errors.push(e.constructor.name + ':' + e.message); }
const img = [{width: 4, height: 4, data: px}];
const name = (p) => p.then(() => 'accepted', (e) => e.constructor.name + ':' + e.message);
Promise.all([{optimize: 1}, {optimize: 'yes'}, {optimize: true, nonsense: 1}, {optimize: true, quality: 0}].map((o) => name(api.stitchJpeg(img, 'vertical', o)))
  .concat([name(api.stitchJpegBatch([{images: img, direction: 'vertical', opts: {optimize: 'yes'}}])),
           name(api.stitchJpegBatch([{images: img, direction: 'vertical', opts: {optimize: true, nonsense: 1}}]))]))
  .then((r) => { out.rejected = r; return api.stitchJpeg([], 'vertical', {optimize: true}); })
  .then((r) => { out.empty = r; console.log(JSON.stringify(out)); });
""" % ROOT
    r = subprocess.run([NODE, "-e", code], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert all(e.startswith("TypeError:") and "optimize" in e for e in out["errors"]), out
    rej = out["rejected"]
    assert rej[0].startswith("TypeError:") and "optimize" in rej[0] and rej[1].startswith("TypeError:") and "optimize" in rej[1]
    assert rej[2].startswith("TypeError:") and "unknown" in rej[2] and "nonsense" in rej[2] and "optimize" not in rej[2]
    assert rej[3].startswith("RangeError:")
    assert rej[4].startswith("TypeError:") and "request 0" in rej[4] and "optimize" in rej[4]
    assert rej[5].startswith("TypeError:") and "nonsense" in rej[5]
    assert out["empty"] is None
    assert "optimize?: boolean" in open(os.path.join(ROOT, "node", "index.d.ts")).read()


# ---- the contract itself, numpy only: what tests/test_gpu_jpeg_optimize.py compares the GPU with ----
def reference(a, quality, layout):
    return JW.write_jpeg(R.frame(a, quality, layout), sof=0, marker="jfif", huff="optimal", restart=R.mcus_per_row(a.shape[1], layout))


def grey_ramp(w=61, h=45):
    yy, xx = np.mgrid[0:h, 0:w]
    v = ((3 * xx + 2 * yy) % 256).astype(np.uint8)
    return np.stack([v, v, v, np.full_like(v, 255)], -1)


def pil_pixels(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def header_length(data):
    """bytes up to and including the SOS segment, found by walking the segments"""
    at = 2
    while True:
        assert data[at] == 0xFF
        n = int.from_bytes(data[at + 2:at + 4], "big")
        if data[at + 1] == 0xDA:
            return at + 2 + n
        at += 2 + n


# every canvas tests/test_gpu_jpeg_optimize.py encodes directly (the stitched canvases of its STITCHES tests need the GPU to exist)
PHOTOS = ((1, 1), (7, 9), (16, 16), (17, 33), (4805, 19), (33, 170), (37, 21), (33, 700), (23, 18), (150, 100), (100, 150), (64, 48), (61, 45))
CONTENTS = [("photo %dx%d" % s, lambda s=s: photo(*s)) for s in PHOTOS] + [
    ("noise 100x150", lambda: noise(100, 150)), ("checker 48x40", lambda: checker(48, 40)),
    ("constant 50x40", lambda: np.full((40, 50, 4), 200, np.uint8)), ("grey ramp", grey_ramp)]


@pytest.mark.parametrize("layout", ("420", "444"))
def test_contract_files_are_strictly_shorter_and_decode_to_the_same_pixels(layout):
    """every shape and content of the GPU tests, both layouts, quality 1 / 50 / 90 / 100 - photo(4805, 19) at 100, the file whose
    trees take the length limit, and photo(33, 700), the slab and batch file, included: the optimal file is strictly shorter than the
    standard one, its header is no longer, and PIL decodes both to identical pixels"""
    for what, make in CONTENTS:
        a = make()
        for q in (1, 50, 90, 100):
            opt, std = reference(a, q, layout), R.encode(a, q, layout)
            assert len(opt) < len(std), (what, q, layout, len(opt), len(std))
            assert header_length(std) == 629 and header_length(opt) <= 629, (what, q, layout)
            assert np.array_equal(pil_pixels(opt), pil_pixels(std)), (what, q, layout)


def _tree_depth(freq):
    """the deepest leaf of the tree of steps 1-2 (before the limit), by the reference's rule"""
    import heapq
    heap = [(int(f), s, 0) for s, f in enumerate(list(freq[:256]) + [1]) if f > 0]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), max(a[2], b[2]) + 1))
    return heap[0][2]


@pytest.mark.parametrize("layout,depth", (("420", 17), ("444", 18)))
def test_the_long_interval_at_quality_100_reaches_the_length_limit(layout, depth):
    """photo(4805, 19) at quality 100 builds a tree deeper than 16, so the GPU test of that shape exercises step 4 inside a real file"""
    f = R.frame(photo(4805, 19), 100, layout)
    (cls, comp, sym, _, _), _, _ = JW._symbols(f, [0, 1, 2], R.mcus_per_row(4805, layout))
    deepest = 0
    for tc in (0, 1):
        for comps in ((0,), (1, 2)):
            freq = np.zeros(257, np.int64)
            np.add.at(freq, sym[(cls == tc) & np.isin(comp, comps)], 1)
            deepest = max(deepest, _tree_depth(freq))
    assert deepest == depth


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_table_builder_and_header_writer_under_sanitizers(tmp_path):
    """the host code of an optimised file that needs no device, driven by a stand-alone program built with ASan + UBSan
    (tools/run_fuzz.sh jpegoptimize): seeded random and adversarial count vectors, the invariants of every table and header"""
    env = dict(os.environ, IST_FUZZ_BIN=str(tmp_path / "check_jpeg_optimize_host"))
    r = subprocess.run([os.path.join(ROOT, "tools", "run_fuzz.sh"), "jpegoptimize", "400", "3"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "400 files" in r.stdout and r.stdout.rstrip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
