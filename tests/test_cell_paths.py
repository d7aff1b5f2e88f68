"""Which kernel form a bilinear draw compiles to (no GPU): ist_debug_cells against the Python restatement of the rule in
tests/bilinear_forms.py - over the whole (|kx|, |ky|) plane, under all eight transforms, on either side of every boundary of the rule - and
the set of forms production can reach at all.  The GPU tests (test_gpu_bilinear_forms.py) take their scales from the same restatement and
assert the form of every case before they launch it, so a compiler edit that silently moves a boundary, or stops choosing a form, fails here
first."""
import pytest

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests import bilinear_forms as B

CW, CH = 41, 23            # the draw covers the whole canvas: one cell


def _m(t, e, f):
    """one of the 8 axis-aligned transforms: bit 0 flips x, bit 1 flips y, bit 2 turns a quarter"""
    sx, sy = (-1.0 if t & 1 else 1.0), (-1.0 if t & 2 else 1.0)
    return [0, sx, sy, 0, e, f] if t & 4 else [sx, 0, 0, sy, e, f]


def _ops(t, span_x, span_y, cw=CW, ch=CH, fill=None, s0=(5.25, 3.5)):
    """[fill,] one draw over the whole canvas whose source rectangle is span_x x span_y; returns (ops array, n, |kx|, |ky| as the library
    computes them: span / destination extent)"""
    dw, dh = (ch, cw) if t & 4 else (cw, ch)          # the user-space rectangle: a quarter turn swaps the canvas axes
    if t & 4:
        e, f = (cw if t & 2 else 0), (ch if t & 1 else 0)
    else:
        e, f = (cw if t & 1 else 0), (ch if t & 2 else 0)
    ops = (L.Op * 2)()
    n = 0
    if fill is not None:
        ops[0].kind = 0; ops[0].image = -1; ops[0].m[:] = [1, 0, 0, 1, 0, 0]; ops[0].d[:] = [0, 0, cw, ch]; ops[0].rgba[:] = fill
        n = 1
    ops[n].kind = 1; ops[n].image = 0; ops[n].m[:] = _m(t, e, f); ops[n].s[:] = [s0[0], s0[1], span_x, span_y]; ops[n].d[:] = [0, 0, dw, dh]
    return ops, n + 1, span_x / dw, span_y / dh


def _desc(w, h, opaque):
    return (L.ImageDesc * 1)(L.ImageDesc(int(w), int(h), 1, 0, 0, int(opaque), 0))


def _one_cell(ops, n, descs, filt, clear, cw=CW, ch=CH):
    cells, kind, table = ist.debug_cells(cw, ch, ops, n, descs, 1, filt, clear=clear)
    assert len(cells) == 1 and (cells[0]["X0"], cells[0]["Y0"], cells[0]["X1"], cells[0]["Y1"]) == (0, 0, cw, ch), cells
    c = cells[0]
    assert c["tiles"] == -(-cw // c["tile_w"]) * -(-ch // c["tile_h"]), c
    return (c["path"], c["tile_w"], c["tile_h"], c["sub_h"]), kind, table


def _library_form(t, kx, ky, filt="bilinear", opaque=True, fill=None, clear=(0, 0, 0, 0), cw=CW, ch=CH):
    dw, dh = (ch, cw) if t & 4 else (cw, ch)
    ops, n, akx, aky = _ops(t, kx * dw, ky * dh, cw, ch, fill)
    got, kind, table = _one_cell(ops, n, _desc(kx * dw + 12, ky * dh + 12, opaque), filt, clear, cw, ch)
    return got, akx, aky, kind, table


def test_constants_match_the_header():
    assert (B.FILL, B.COPY, B.SAMPLE, B.GENERAL, B.SAMPLE_LDS, B.SWAP_LDS, B.SAMPLE_STREAM) == \
        (L.PATH_FILL, L.PATH_COPY, L.PATH_SAMPLE, L.PATH_GENERAL, L.PATH_SAMPLE_LDS, L.PATH_SWAP_LDS, L.PATH_SAMPLE_STREAM)


@pytest.mark.parametrize("filt", ["bilinear", "nearest"])
@pytest.mark.parametrize("t", range(8))
def test_the_whole_scale_plane_under_every_transform(t, filt):
    """a log grid of (|kx|, |ky|) from 0.2 to 150: opaque-hinted and translucent draws over a transparent canvas, an opaque clear colour
    and an opaque fill.  Only a translucent draw over a transparent canvas leaves the fast forms."""
    grid = B.log_grid()
    for kx in grid:
        for ky in grid:
            for opaque, fill, clear in ((True, None, (0, 0, 0, 0)), (False, None, (0, 0, 0, 0)), (False, None, (9, 8, 7, 255)),
                                        (False, (1, 2, 3, 255), (0, 0, 0, 0)), (True, (1, 2, 3, 255), (0, 0, 0, 0))):
                got, akx, aky, kind, table = _library_form(t, kx, ky, filt, opaque, fill, clear)
                fast = opaque or fill is not None or clear[3] == 255
                want = B.form(akx, aky, bool(t & 4), filt, fast=fast)
                assert got == want, (t, filt, kx, ky, opaque, fill, clear, B.name(got), B.name(want))
                assert table and kind == (1 if want[0] in (B.SAMPLE, B.SAMPLE_LDS, B.SAMPLE_STREAM) else 2), (kind, table, B.name(want))


@pytest.mark.parametrize("line", B.LINES + B.SWEEP_LINES, ids=[ln[0] for ln in B.LINES + B.SWEEP_LINES])
def test_the_form_switches_exactly_at_every_boundary(line):
    """along a line of the plane, every change of form the restatement has: the library shows the one form at the last double of the source
    span below it and the other form at the next double"""
    _, turned, axis, other = line
    found = B.boundaries(line)
    assert found
    for k_lo, k_hi, fa, fb in found:
        assert fa != fb
        for t in ((4, 5, 6, 7) if turned else (0, 1, 2, 3)):
            for f_side in (fa, fb):
                # a canvas of two tiles and a ragged third of the form on this side, as the GPU sweep draws it
                cw = 2 * f_side[1] + 13
                ch = 2 * f_side[2] + 5
                dw, dh = (ch, cw) if turned else (cw, ch)
                ext = dw if axis == "x" else dh
                s_lo, s_hi = B.bisect_span(lambda k: B.line_form(line, k), ext, k_lo * (1 - 1e-9), k_hi * (1 + 1e-9))
                for span, want in ((s_lo, fa), (s_hi, fb)):
                    sx, sy = (span, other * dh) if axis == "x" else (other * dw, span)
                    ops, n, akx, aky = _ops(t, sx, sy, cw, ch)
                    assert B.form(akx, aky, turned) == want
                    got, kind, table = _one_cell(ops, n, _desc(sx + 12, sy + 12, True), "bilinear", (0, 0, 0, 0), cw, ch)
                    assert got == want, (line[0], t, span / ext, B.name(got), B.name(want))


def test_the_boundaries_are_where_the_design_says():
    """the figures DESIGN.md quotes, from the restatement (which the tests above tie to the library)"""
    steps = [round(b[0], 2) for b in B.boundaries(B.LINES[0])]
    assert steps == [0.70, 0.79, 0.92, 1.07, 1.33, 1.70, 2.39, 4.00], steps           # LDS-256 stage heights 32 -> 4 at |ky| = 1, then direct
    stream = [(round(b[0], 1), B.name(b[3])) for b in B.boundaries(B.LINES[3])]
    assert stream == [(3.0, "STREAM-128"), (6.0, "STREAM-64"), (16.2, "DIRECT")], stream
    swap = [(round(b[0], 2), B.name(b[3])) for b in B.boundaries(B.LINES[7])]
    assert swap == [(1.90, "SWAP-32"), (3.87, "SWAP-16"), (8.0, "GENERAL")], swap


@pytest.mark.parametrize("t", range(8))
def test_degenerate_sources_and_deeper_stacks(t):
    """a source whose clamp box is one pixel wide or high has no second tap: the direct path (the general one when turned) at every scale;
    two pixels are enough for the staged forms.  More than one draw in a cell's stack is the general path."""
    turned = bool(t & 4)
    dw, dh = (CH, CW) if turned else (CW, CH)
    for kx, ky in ((0.5, 0.5), (1.3, 1.3), (2.5, 2.5), (3.5, 1.5), (7.0, 3.0)):
        for iw, ih, s in ((1, 4000, [0, 0, 1, ky * dh]), (4000, 1, [0, 0, kx * dw, 1]), (1, 1, [0, 0, 1, 1]),
                          (4000, 4000, [3.2, 0, 0.5, ky * dh]), (4000, 4000, [0, 7.5, kx * dw, 0.5])):     # (a rectangle inside one column / row of a larger bitmap)
            ops, n, _, _ = _ops(t, s[2], s[3])
            ops[0].s[:] = s
            got, _, _ = _one_cell(ops, n, _desc(iw, ih, True), "bilinear", (0, 0, 0, 0))
            assert got == B.form(s[2] / dw, s[3] / dh, turned, degenerate=True), (t, kx, ky, iw, ih, B.name(got))
            assert got[0] == (B.GENERAL if turned else B.SAMPLE)
        for iw, ih, s in ((2, 4000, [0, 0, 2, ky * dh]), (4000, 2, [0, 0, kx * dw, 2])):
            ops, n, _, _ = _ops(t, s[2], s[3])
            ops[0].s[:] = s
            got, _, _ = _one_cell(ops, n, _desc(iw, ih, True), "bilinear", (0, 0, 0, 0))
            assert got == B.form(s[2] / dw, s[3] / dh, turned), (t, kx, ky, iw, ih, B.name(got))
            assert kx > 2.5 or got[0] in (B.SAMPLE_LDS, B.SAMPLE_STREAM, B.SWAP_LDS)       # (the other axis may still be too strong a shrink)
        # two translucent draws over an opaque fill: stack_len == 2; an opaque draw on top hides what is under it: one draw again
        for top_opaque in (False, True):
            ops2 = (L.Op * 3)()
            one, _, akx, aky = _ops(t, kx * dw, ky * dh, fill=(1, 2, 3, 255))
            ops2[0], ops2[1], ops2[2] = one[0], one[1], one[1]
            ops2[2].image = 1
            descs = (L.ImageDesc * 2)(L.ImageDesc(4000, 4000, 1, 0, 0, 0, 0), L.ImageDesc(4000, 4000, 1, 0, 0, int(top_opaque), 0))
            cells, kind, table = ist.debug_cells(CW, CH, ops2, 3, descs, 2, "bilinear")
            assert len(cells) == 1
            got = (cells[0]["path"], cells[0]["tile_w"], cells[0]["tile_h"], cells[0]["sub_h"])
            assert got == B.form(akx, aky, turned, fast=top_opaque), (t, kx, ky, top_opaque, B.name(got))


def test_copies_and_fills_carry_no_tile_table():
    ops, n, _, _ = _ops(0, CW, CH, fill=(1, 2, 3, 255), s0=(0, 0))
    cells, kind, table = ist.debug_cells(CW, CH, ops, n, _desc(CW, CH, True), 1, "bilinear")
    assert [c["path"] for c in cells] == [B.COPY] and kind == 0 and not table
    cells, kind, table = ist.debug_cells(CW, CH, ops, 1, _desc(CW, CH, True), 1, "bilinear")
    assert [c["path"] for c in cells] == [B.FILL] and kind == 0 and not table
    cells, kind, table = ist.debug_cells(CW, CH, ops, n, _desc(CW, CH, True), 1, "bilinear", clip=(3, 2, 10, 5))
    assert [(c["X0"], c["Y0"], c["X1"], c["Y1"], c["tiles"]) for c in cells] == [(3, 2, 13, 7, 1)]
    n_cells = L.C.c_int(0)
    assert L.lib.ist_debug_cells(CW, CH, None, ops, n, _desc(CW, CH, True), 1, 1, None, None, 0, L.C.byref(n_cells), None, None) == 0 and n_cells.value == 1
    assert L.lib.ist_debug_cells(CW, CH, None, ops, n, _desc(CW, CH, True), 1, 1, None, None, 0, None, None, None) == -1


def test_the_forms_production_can_reach():
    """a dense survey of the plane (120 x 120, straight and turned): the set of (path, tile_w, tile_h, sub_h) the library compiles is
    exactly the one below.  SAMPLE_LDS 64 pixels wide is absent: a 128-wide stage of 4 rows fits the budget at every |kx| <= 4, |ky| < 2,
    so the narrowest staged tile only exists under the tuning knob that pins the width."""
    seen = set()
    grid = B.log_grid(n=120)
    for t in (0, 4):
        for kx in grid:
            for ky in grid:
                got, akx, aky, _, _ = _library_form(t, kx, ky)
                assert got == B.form(akx, aky, bool(t & 4)), (t, kx, ky)
                seen.add(got)
    print("forms seen (path, tile_w, tile_h, sub_h):", sorted(seen), sorted(B.name(f) for f in seen))
    want = {(B.SAMPLE_LDS, 256, 2 * s, s) for s in range(4, 33, 4)} | {(B.SAMPLE_LDS, 128, 8, 4), (B.SAMPLE_LDS, 128, 16, 8)} | \
           {(B.SAMPLE_STREAM, w, 8, 2) for w in (256, 128, 64)} | {(B.SAMPLE, 256, 32, 0)} | {(B.SWAP_LDS, 64, h, 0) for h in (64, 32, 16)} | \
           {(B.GENERAL, 64, 64, 0)}
    assert seen == want, (sorted(seen - want), sorted(want - seen))
    assert not any(f[0] == B.SAMPLE_LDS and f[1] == 64 for f in seen)
