"""Bilinear resampling in every tile form the compiler can pick (ist_compile.cpp, cell classification; tests/bilinear_forms.py restates it):
SAMPLE_LDS 256 wide at every stage height and 128 wide, SAMPLE_STREAM 256 / 128 / 64 wide, the direct gather, SWAP_LDS 64 / 32 / 16 high and
the per-pixel general path.  Every case is ONE draw over an opaque fill, or an opaque-hinted draw over a transparent canvas, on a canvas of
two whole tiles and a ragged third (13 pixels across, 5 rows down: a ragged last stage and a last tile shorter than 4 rows); before it is
launched its compiled form is asserted with ist_debug_cells, so a case that no longer reaches its form fails instead of quietly testing
another kernel.

  a. form sweep: the two scales (adjacent doubles of the source span) on either side of every boundary of the rule, crossed with five
     sub-pixel offsets, the four flips, an opaque-hinted and a translucent draw, and a source rectangle cropped out of a larger bitmap or
     reaching 3 px past it on every side - against the fp64 oracle under the op-list rule (solid pixels within 1 LSB), with one RareDiff per
     form: fewer than 1 % of the solid channel bytes differ, signed drift within 0.001 LSB per byte plus three standard deviations;
  b. known answers at integer ratios (every tap weight a multiple of 1/4: exact in fp32), all eight transforms;
  c. the same bytes whatever the tile walk: a child process compiled without the tile table (IST_NO_TILE_TABLE: the band / cell prefix
     search production uses above 4 Mi tiles) renders every case of (a) and three multi-draw strips whose bands mix cells of different tile
     widths; byte equality with the production renders;
  d. the same bytes whatever the kernel: a child process with IST_NO_LDS renders every axis-aligned case through the direct gather, which
     the kernel comments claim does identical IEEE operations per channel: byte equality.  Turned draws fall to the general path there,
     whose arithmetic is not claimed identical: the child holds them to (a)'s rule.

Measured on an MI355X, per form: cases, differing solid channel bytes, mean signed difference in LSB (also in LAB_NOTES.md):
  DIRECT       384 cases   24612 of  51672576 bytes (4.76e-04)  +4.74e-04 LSB
  GENERAL      160 cases    1078 of  12001920 bytes (8.98e-05)  +8.85e-05 LSB
  LDS-128/4    320 cases     994 of   7230720 bytes (1.37e-04)  +1.32e-04 LSB
  LDS-128/8    320 cases     399 of  12739840 bytes (3.13e-05)  +3.01e-05 LSB
  LDS-256/12   640 cases    2298 of  71232000 bytes (3.23e-05)  +3.19e-05 LSB
  LDS-256/16   640 cases    2241 of  92736000 bytes (2.42e-05)  +2.32e-05 LSB
  LDS-256/20   640 cases   46971 of 114240000 bytes (4.11e-04)  +4.01e-04 LSB
  LDS-256/24   480 cases    1842 of 101808000 bytes (1.81e-05)  +1.79e-05 LSB
  LDS-256/28   480 cases    1892 of 117936000 bytes (1.60e-05)  +1.57e-05 LSB
  LDS-256/32   264 cases    1450 of  69517344 bytes (2.09e-05)  +1.96e-05 LSB
  LDS-256/4    480 cases    4076 of  21168000 bytes (1.93e-04)  +1.88e-04 LSB
  LDS-256/8    640 cases    3046 of  49728000 bytes (6.13e-05)  +6.01e-05 LSB
  STREAM-128   320 cases     168 of   7230720 bytes (2.32e-05)  +2.21e-05 LSB
  STREAM-256   264 cases    1999 of  12077088 bytes (1.66e-04)  +1.64e-04 LSB
  STREAM-64    160 cases     345 of   1895040 bytes (1.82e-04)  +1.78e-04 LSB
  SWAP-16      320 cases    1726 of   6677760 bytes (2.58e-04)  +2.51e-04 LSB
  SWAP-32      320 cases    1676 of  12453120 bytes (1.35e-04)  +1.33e-04 LSB
  SWAP-64      160 cases    1337 of  12001920 bytes (1.11e-04)  +1.08e-04 LSB
Every difference but a handful is +1: what is left are blends whose exact value is a rounding tie x.5 (the swept axis sits on a rational
boundary scale, and the draw (3, 0.3) has weights in steps of 1/20 on y and 1/4 on x: LDS-256/20), which fp32 sees as the tie and rounds
half up while the fp64 oracle sees x.5 -+ 1e-11 - see tests/bilinear_forms.py, SWEEP_LINES.  The tile walk without a table (c) and the
direct gather (d) wrote the same bytes as production in every one of the 6995 / 6032 cases compared.  Under IST_NO_LDS the turned cases
(general path): GENERAL 1078 of 12001920 (+8.85e-05), SWAP-16 1726 of 6677760 (+2.51e-04), SWAP-32 1676 of 12453120 (+1.33e-04), SWAP-64
1337 of 12001920 (+1.08e-04) - the same counts as production, so there too the bytes are most likely equal (not asserted: not claimed)."""
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from oracle import oracle as O
from tests import bilinear_forms as B
from tests import util as U

pytestmark = pytest.mark.gpu

OFFSETS = [0.0, 0.25, 0.5 - 1e-6, 0.5, 0.999]
MODE = "production"            # a child process sets "walk" (no tile table) or "direct" (IST_NO_LDS) before it renders
SWEEP_LINES = B.SWEEP_LINES    # the lines of the (|kx|, |ky|) plane whose boundaries the sweep straddles


def _m(t, e, f):
    """one of the 8 axis-aligned transforms: bit 0 flips x, bit 1 flips y, bit 2 turns a quarter"""
    sx, sy = (-1.0 if t & 1 else 1.0), (-1.0 if t & 2 else 1.0)
    return [0, sx, sy, 0, e, f] if t & 4 else [sx, 0, 0, sy, e, f]


def _c_ops(ops_o):
    ops = (L.Op * len(ops_o))()
    for i, o in enumerate(ops_o):
        ops[i].m[:] = o["m"]
        if o["kind"] == "fill":
            ops[i].kind = 0; ops[i].image = -1; ops[i].d[:] = o["rect"]; ops[i].rgba[:] = o["rgba"]
        else:
            ops[i].kind = 1; ops[i].image = o["image"]; ops[i].s[:] = o["s"]; ops[i].d[:] = o["d"]
    return ops


# ------------------------------------------------------------------------------------------------ the cases
def _scales():
    """[(id, turned, form, span_x, span_y, cw, ch)]: for every boundary of every sweep line the last source span below it and the first
    above it, each on the canvas of its own form; then the two draws that enlarge on one axis and shrink on the other"""
    out = []
    for line in SWEEP_LINES:
        lname, turned, axis, other = line
        for k_lo, k_hi, fa, fb in B.boundaries(line):
            for side, f in (("below", fa), ("above", fb)):
                cw, ch = 2 * f[1] + 13, 2 * f[2] + 5
                dw, dh = (ch, cw) if turned else (cw, ch)
                ext = dw if axis == "x" else dh
                s_lo, s_hi = B.bisect_span(lambda k: B.line_form(line, k), ext, k_lo * (1 - 1e-9), k_hi * (1 + 1e-9))
                span = s_lo if side == "below" else s_hi
                sx, sy = (span, other * dh) if axis == "x" else (other * dw, span)
                assert B.form(sx / dw, sy / dh, turned) == f
                out.append(("%s:%s-%s-%s" % (lname, B.name(fa), B.name(fb), side), turned, f, sx, sy, cw, ch))
    for kx, ky in ((0.25, 3.0), (3.0, 0.3)):
        f = B.form(kx, ky)
        cw, ch = 2 * f[1] + 13, 2 * f[2] + 5
        out.append(("mixed:%g,%g-%s" % (kx, ky, B.name(f)), False, f, kx * cw, ky * ch, cw, ch))
    return out


SCALES = _scales()


def _draw_case(sid, turned, f, sx, sy, cw, ch, off, flip, opaque, past, seed):
    """one draw over the whole canvas: opaque-hinted over a transparent canvas, or translucent over an opaque fill"""
    dw, dh = (ch, cw) if turned else (cw, ch)
    if past:       # the source rectangle starts 3 pixels before the bitmap and ends 3 after it: taps clamp at cx0 / cx1, the last source row is the bitmap's
        w, h = max(2, int(math.ceil(sx)) - 6 + 1), max(2, int(math.ceil(sy)) - 6 + 1)
        s = [-3.0 + off, -3.0 + off, sx, sy]
    else:          # cropped out of a larger bitmap at an offset that is not a multiple of 4 pixels
        w, h = int(math.ceil(sx)) + 9, int(math.ceil(sy)) + 9
        s = [5.0 + off, 5.0 + off, sx, sy]
    t = (4 | flip) if turned else flip
    e, f_ = ((cw if t & 2 else 0), (ch if t & 1 else 0)) if turned else ((cw if t & 1 else 0), (ch if t & 2 else 0))
    ops = [{"kind": "draw", "image": 0, "m": _m(t, e, f_), "s": s, "d": [0, 0, dw, dh]}]
    if not opaque:
        ops.insert(0, {"kind": "fill", "m": [1, 0, 0, 1, 0, 0], "rect": [0, 0, cw, ch], "rgba": (seed % 251, seed % 241, seed % 239, 255)})
    return {"name": "%s/o%g/f%d/%s/%s" % (sid, off, flip, "opaque" if opaque else "translucent", "past" if past else "crop"), "form": f, "turned": turned,
            "cw": cw, "ch": ch, "ops": ops, "specs": [(seed, h, w, opaque)], "hints": [opaque]}


def _scale_cases(n):
    sid, turned, f, sx, sy, cw, ch = SCALES[n]
    out = []
    for opaque in (True, False):
        for past in (False, True):
            seed = 40000 + 8 * n + 2 * opaque + past                 # one bitmap per (scale, hint, rectangle), shared by its 20 cases
            for off in OFFSETS:
                for flip in range(4):
                    out.append(_draw_case(sid, turned, f, sx, sy, cw, ch, off, flip, opaque, past, seed))
    return out


def _thin_cases():
    """sources 1 and 2 pixels wide or high.  One pixel has no second tap on that axis: the direct path whatever the scale; two pixels
    are a footprint like any other and take the staged forms"""
    out = []
    for n, (iw, ih) in enumerate([(1, 97), (2, 97), (301, 1), (301, 2), (1, 700), (2, 700), (1, 1)]):
        for cw, ch in ((525, 69), (141, 37)):
            degenerate = iw == 1 or ih == 1
            f = B.form(iw / cw, ih / ch, degenerate=degenerate)
            assert (f[0] == B.SAMPLE) == degenerate or ih / ch >= 2.0
            for flip in range(4):
                for opaque in (True, False):
                    c = _draw_case("thin:%dx%d->%dx%d" % (iw, ih, cw, ch), False, f, float(iw), float(ih), cw, ch, 0.0, flip, opaque, False, 49000 + 2 * n + opaque)
                    c["ops"][-1]["s"] = [0.0, 0.0, float(iw), float(ih)]
                    c["specs"] = [(49000 + 2 * n + opaque, ih, iw, opaque)]
                    out.append(c)
    return out


def _strip_cases():
    """multi-draw strips over a white fill: draws side by side, each as high as the canvas, so that ONE band of tiles holds cells of
    different paths and tile widths (cells of one tile height that follow each other share a band), and the bands are re-sorted by weight"""
    def strip(name, H, parts, gap):
        ops = [{"kind": "fill", "m": [1, 0, 0, 1, 0, 0], "rect": [0, 0, 0, H], "rgba": (255, 255, 255, 255)}]
        specs, hints, paths, x = [], [], [], 0
        for i, (w, kx, ky, turned, opaque, want) in enumerate(parts):
            if i and gap:
                paths.append((B.FILL, 256, 8)); x += gap
            dw, dh = (H, w) if turned else (w, H)
            sx, sy = kx * dw, ky * dh
            specs.append((48000 + 16 * len(name) + i, int(math.ceil(sy)) + 2, int(math.ceil(sx)) + 2, opaque))
            hints.append(opaque)
            ops.append({"kind": "draw", "image": i, "m": _m(4 if turned else 0, x, 0), "s": [0, 0, sx, sy] if want == B.COPY else [1.25, 0.5, sx, sy], "d": [0, 0, dw, dh]})
            paths.append(want if isinstance(want, tuple) else (want,) + {B.COPY: (256, 8), B.GENERAL: (64, 64)}[want])
            x += w
        ops[0]["rect"][2] = x
        return {"name": "strip:" + name, "paths": paths, "turned": False, "cw": x, "ch": H, "ops": ops, "specs": specs, "hints": hints}
    LDS, STREAM, SWAP, DIRECT = B.SAMPLE_LDS, B.SAMPLE_STREAM, B.SWAP_LDS, B.SAMPLE
    return [
        # one band of tiles 8 rows high: COPY (256 wide), LDS-256/4, STREAM-128, FILL, STREAM-64, COPY
        strip("eight-row-band", 45, [(300, 1, 1, False, True, B.COPY), (270, 2.6, 1.0, False, True, (LDS, 256, 8)), (141, 4, 4, False, False, (STREAM, 128, 8)),
                                     (77, 8, 8, False, True, (STREAM, 64, 8)), (259, 1, 1, False, False, B.COPY)], 0),
        # one band of tiles 64 rows high: LDS-256/32 (256 wide) next to GENERAL and SWAP-64 (64 wide)
        strip("tall-band", 133, [(300, 0.5, 0.5, False, True, (LDS, 256, 64)), (70, 9, 9, True, True, B.GENERAL), (130, 1.2, 1.2, True, False, (SWAP, 64, 64)),
                                 (100, 0.5, 0.5, False, False, (LDS, 256, 64))], 0),
        # many bands, re-sorted: copies and fills go behind the resampling bands
        strip("sorted-bands", 45, [(259, 1, 1, False, True, B.COPY), (70, 9, 9, True, True, B.GENERAL), (300, 2.2, 2.2, False, True, (STREAM, 256, 8)),
                                   (280, 1.5, 1.5, False, False, (LDS, 256, 16)), (90, 17, 17, False, True, (DIRECT, 256, 32)), (300, 1, 1, False, True, B.COPY),
                                   (150, 1.3, 1.3, True, True, (SWAP, 64, 64))], 3),
    ]


def _all_cases():
    out = []
    for n in range(len(SCALES)):
        out += _scale_cases(n)
    return out + _thin_cases() + _strip_cases()


# ------------------------------------------------------------------------------------------------ rendering
_BITMAPS = {}
DIGESTS = {}                   # case name -> sha1 of the canvas as this process's mode rendered it


def _bitmap(spec):
    """(host array, device tensor) of a bitmap spec (seed, h, w, opaque): made once, shared by the cases that draw it"""
    if spec not in _BITMAPS:
        if len(_BITMAPS) >= 16:
            _BITMAPS.clear()
        a = U.rand_image(*spec)
        _BITMAPS[spec] = (a, torch.from_numpy(a).cuda())
    return _BITMAPS[spec]


def _assert_form(case, cells, kind, table):
    got = [(c["path"], c["tile_w"], c["tile_h"], c["sub_h"]) for c in cells]
    assert table == (MODE != "walk"), (case["name"], MODE, table)
    if "paths" in case:
        assert MODE != "direct"
        assert [g[:3] for g in got] == case["paths"], (case["name"], got)
        return
    assert len(cells) == 1 and (cells[0]["X0"], cells[0]["Y0"], cells[0]["X1"], cells[0]["Y1"]) == (0, 0, case["cw"], case["ch"]), (case["name"], cells)
    want = case["form"]
    if MODE == "direct":
        want = (B.GENERAL, 64, 64, 0) if case["turned"] else (B.SAMPLE, 256, 32, 0)
    assert got[0] == want, "%s compiles to %s, not to %s" % (case["name"], B.name(got[0]), B.name(want))


def _render(case):
    """asserts the compiled form, then one launch on device tensors into a poisoned canvas"""
    px = [_bitmap(s) for s in case["specs"]]
    ops = _c_ops(case["ops"])
    descs = (L.ImageDesc * len(px))(*[L.ImageDesc(a.shape[1], a.shape[0], 1, 0, 0, int(h), 0) for (a, _), h in zip(px, case["hints"])])
    cw, ch = case["cw"], case["ch"]
    cells, kind, table = ist.debug_cells(cw, ch, ops, len(case["ops"]), descs, len(px), "bilinear")
    _assert_form(case, cells, kind, table)
    job = ist.Stitcher(0).compile_ops(cw, ch, ops, len(case["ops"]), descs, len(px), "bilinear")
    out = torch.full((ch, cw, 4), 0x5A, dtype=torch.uint8, device="cuda")
    job.launch([t for _, t in px], out)
    torch.cuda.synchronize()
    job.close()
    got = out.cpu().numpy()
    DIGESTS[case["name"]] = hashlib.sha1(got.tobytes()).hexdigest()
    return got


def _oracle(case):
    px = [_bitmap(s)[0] for s in case["specs"]]
    return O.render_ops(case["cw"], case["ch"], case["ops"], [{"width": a.shape[1], "height": a.shape[0]} for a in px], px, "bilinear")


class FormStats:
    """one RareDiff per form"""

    def __init__(self):
        self.by_form = {}

    def add(self, form_name, stats):
        r = self.by_form.setdefault(form_name, [U.RareDiff(), 0])
        r[0].add(stats)
        r[1] += 1

    def lines(self):
        return ["  %-11s %5d cases, %s" % (k, n, r) for k, (r, n) in sorted(self.by_form.items())]

    def check(self):
        print("\n".join(["bilinear forms against the oracle:"] + self.lines()))
        failed = []
        for k, (r, n) in sorted(self.by_form.items()):
            try:
                r.check()
            except AssertionError as e:
                failed.append("%s: %s" % (k, e))
        assert not failed, "\n".join(failed)


@pytest.fixture(scope="module")
def forms():
    f = FormStats()
    yield f
    f.check()                  # per form: fewer than 1 % of the solid channel bytes differ from the oracle, unbiased


def _check_cases(cases, forms):
    for case in cases:
        got = _render(case)
        try:
            forms.add(B.name(case["form"]), U.oracle_tolerance(got, _oracle(case)))
        except AssertionError as e:
            raise AssertionError("%s: %s" % (case["name"], e))


# ------------------------------------------------------------------------------------------------ a. form sweep
@pytest.mark.parametrize("n", range(len(SCALES)), ids=[s[0] for s in SCALES])
def test_form_sweep_against_the_oracle(n, forms):
    """one scale on one side of a boundary: 5 offsets x 4 flips x (opaque-hinted | translucent) x (cropped | past the bitmap)"""
    cases = _scale_cases(n)
    assert len(cases) == 80
    _check_cases(cases, forms)


def test_sources_one_and_two_pixels_wide_or_high(forms):
    _check_cases(_thin_cases(), forms)


def test_every_form_was_swept():
    """the sweep reaches every form the compiler can pick in production (test_cell_paths.py pins that set)"""
    swept = {s[2] for s in SCALES}
    want = {(B.SAMPLE_LDS, 256, 2 * s, s) for s in range(4, 33, 4)} | {(B.SAMPLE_LDS, 128, 8, 4), (B.SAMPLE_LDS, 128, 16, 8)} | \
           {(B.SAMPLE_STREAM, w, 8, 2) for w in (256, 128, 64)} | {(B.SAMPLE, 256, 32, 0)} | {(B.SWAP_LDS, 64, h, 0) for h in (64, 32, 16)} | \
           {(B.GENERAL, 64, 64, 0)}
    assert swept == want, (sorted(swept - want), sorted(want - swept))


# ------------------------------------------------------------------------------------------------ b. known answers
def _dyadic_taps(k, n, length):
    """bilinear taps of canvas coordinates 0..n-1 at scale k into a rectangle of `length` source pixels that starts on a pixel: (first
    index, second index, weight of the second in quarters), clamped as the kernels clamp (both taps on the edge pixel)"""
    f = k * (np.arange(n) + 0.5) - 0.5
    i0 = np.floor(f)
    q = np.round((f - i0) * 4).astype(np.int64)
    assert np.array_equal(q / 4.0, f - i0)                    # every weight is a multiple of 1/4
    i0 = i0.astype(np.int64)
    return np.clip(i0, 0, length - 1), np.clip(i0 + 1, 0, length - 1), q


def _known_answer(R, kx, ky, W, H):
    """the exact bilinear resample of rectangle R (h x w x 4, opaque) to W x H when every weight is a multiple of 1/4: the weighted sum
    is an integer number of sixteenths, rounded half up - for |k| even (a + b + c + d + 2) // 4, for |k| odd the centre pixel, for
    |k| = 1/2 (9a + 3b + 3c + d + 8) // 16"""
    R = R.astype(np.int64)
    x0, x1, qx = _dyadic_taps(kx, W, R.shape[1])
    y0, y1, qy = _dyadic_taps(ky, H, R.shape[0])
    qx, qy = qx[None, :, None], qy[:, None, None]
    top = (4 - qx) * R[y0][:, x0] + qx * R[y0][:, x1]
    bot = (4 - qx) * R[y1][:, x0] + qx * R[y1][:, x1]
    return (((4 - qy) * top + qy * bot + 8) // 16).astype(np.uint8)


KNOWN = [(2, 2), (4, 4), (6, 6), (8, 8), (16, 16), (18, 18), (32, 32), (3, 3), (5, 5), (7, 7), (17, 17), (0.5, 0.5), (3, 1), (4, 1), (0.5, 2), (2, 0.5)]


@pytest.mark.parametrize("kx,ky", KNOWN, ids=["%gx%g" % k for k in KNOWN])
def test_integer_ratios_give_the_exact_weighted_sum(kx, ky):
    """opaque draws at integer ratios (and 1/2) aligned to the bitmap's pixels, all eight transforms: STREAM at every width, the direct
    path, LDS, and - turned - SWAP at every height and the general path; exact in fp32, so the bytes are equal"""
    seen = set()
    for turned in (False, True):
        f = B.form(kx, ky, turned)
        # (canvas W x H in the draw's own frame: source x runs along W)
        H = 21 if not turned else 2 * 64 + 13
        W = max(9, min(2 * (f[2] if turned else f[1]) + 13, int(3.0e6 / (kx * ky * H))))          # (sources of at most ~3 MP)
        sw, sh = int(kx * 2 * (W // 2)), int(ky * 2 * (H // 2))
        W, H = 2 * (W // 2), 2 * (H // 2)                  # even, so that k = 1/2 covers whole source pixels
        bmp = U.rand_image(int(1000 * kx + 10 * ky) + turned, sh + 9, sw + 11, opaque=True)
        want_b = _known_answer(bmp[3:3 + sh, 5:5 + sw], kx, ky, W, H)
        for flip in range(4):
            t = (4 | flip) if turned else flip
            cw, ch = (H, W) if turned else (W, H)
            e, f_ = ((cw if t & 2 else 0), (ch if t & 1 else 0)) if turned else ((cw if t & 1 else 0), (ch if t & 2 else 0))
            want = want_b.transpose(1, 0, 2) if turned else want_b
            # bit 0 mirrors source x, which runs along canvas y when turned; bit 1 mirrors source y
            if t & 1:
                want = want[::-1] if turned else want[:, ::-1]
            if t & 2:
                want = want[:, ::-1] if turned else want[::-1]
            case = {"name": "known:%gx%g/t%d" % (kx, ky, t), "form": f, "turned": turned, "cw": cw, "ch": ch,
                    "ops": [{"kind": "draw", "image": 0, "m": _m(t, e, f_), "s": [5, 3, sw, sh], "d": [0, 0, W, H]}],
                    "specs": [("known", kx, ky, turned)], "hints": [True]}
            _BITMAPS[case["specs"][0]] = (bmp, torch.from_numpy(bmp).cuda())
            got = _render(case)
            bad = (got != want).any(axis=-1)
            assert not bad.any(), (case["name"], B.name(f), int(bad.sum()), U.max_abs_diff(got, np.ascontiguousarray(want)))
            seen.add(B.name(f))
    print("known answers %gx%g:" % (kx, ky), sorted(seen))


# ------------------------------------------------------------------------------------------------ c, d. child processes
def child(mode, production_json, report_json):
    """entry point of the knob processes: render every case in this process's mode, compare the digests with the production ones"""
    global MODE
    MODE = mode
    production = json.load(open(production_json))
    stats = FormStats()
    different, compared, n = [], 0, 0
    for case in _all_cases():
        if mode == "direct" and "paths" in case:
            continue
        got = _render(case)
        n += 1
        if mode == "direct" and case["turned"]:          # the general path: not claimed identical, held to the oracle rule
            stats.add(B.name(case["form"]), U.oracle_tolerance(got, _oracle(case)))
            continue
        compared += 1
        if DIGESTS[case["name"]] != production[case["name"]]:
            different.append(case["name"])
    json.dump({"rendered": n, "compared": compared, "different": different, "stats": stats.lines()}, open(report_json, "w"))
    if stats.by_form:
        stats.check()


def _run_child(mode, env_knob, tmp_path):
    cases = _all_cases()
    for case in cases:                                       # the production renders (made once per process: the sweep leaves them behind)
        if case["name"] not in DIGESTS:
            _render(case)
    prod, report = tmp_path / "production.json", tmp_path / "report.json"
    prod.write_text(json.dumps({c["name"]: DIGESTS[c["name"]] for c in cases}))
    code = "import sys; sys.path.insert(0, %r); from tests import test_gpu_bilinear_forms as T; T.child(%r, %r, %r); print('child ok')" % (
        U.ROOT, mode, str(prod), str(report))
    env = dict(os.environ, IST_TUNING="1")
    env[env_knob] = "1"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    rep = json.loads(report.read_text())
    print("\n".join(["%s child: %d rendered, %d compared byte for byte, %d differ" % (mode, rep["rendered"], rep["compared"], len(rep["different"]))] + rep["stats"]))
    return cases, rep


def test_the_tile_walk_without_a_table_writes_the_same_bytes(tmp_path):
    """IST_NO_TILE_TABLE: run_tile finds a tile's cell by binary search over the band and cell prefixes instead of reading the per-tile
    table - the same tile functions, so the same bytes without exception, also where one band holds cells of different tile widths"""
    assert MODE == "production"
    cases, rep = _run_child("walk", "IST_NO_TILE_TABLE", tmp_path)
    assert rep["rendered"] == rep["compared"] == len(cases)
    assert not rep["different"], "%d of %d canvases differ without the tile table: %s" % (len(rep["different"]), len(cases), rep["different"][:20])


def test_the_direct_gather_writes_the_same_bytes_as_every_staged_form(tmp_path):
    """IST_NO_LDS: every axis-aligned case runs tile_sample; tile_sample_lds<NP> and tile_sample_stream<NP> do the same IEEE operations per
    channel on the same taps, so their canvases are equal byte for byte.  Turned cases run the general path there (oracle rule, in the child)."""
    assert MODE == "production"
    cases, rep = _run_child("direct", "IST_NO_LDS", tmp_path)
    single = [c for c in cases if "paths" not in c]
    assert rep["rendered"] == len(single) and rep["compared"] == sum(not c["turned"] for c in single)
    assert not rep["different"], "%d canvases differ between the direct gather and the staged forms: %s" % (len(rep["different"]), rep["different"][:20])
