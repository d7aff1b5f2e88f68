"""The cell classification of ist_compile.cpp under filter 'cubic' restated in Python (test infrastructure, no GPU), and what the streamed
cubic kernel (tile_cubic_stream, ist_kernels.hip) does with one tile: which template instance it runs and how many rounds its chunk
loop takes.  tests/test_cubic_cells.py holds the first against ist_debug_cells; tests/test_gpu_cubic_regimes.py takes its scales from
here and labels its cases with the second.

A cell with ONE draw that is not turned, over an opaque colour (or an opaque-hinted draw over anything), becomes by (|kx|, |ky|):

  |kx| <= 1 and |ky| <= 1    CUBIC_STREAM, tiles 256 x 32 - unless the draw is 1:1 at an integer offset and stays inside its clamp box:
                             the cubic weights are (0, 1, 0, 0) there, and the cell is a COPY
  |kx| >  1 and |ky| >  1    AREA_STREAM while |ky| <= 64 (the box filter; its tile shape is restated in area_tile), beyond that GENERAL
  one axis each way          GENERAL, the per-pixel stack under the cubic rule

and everything else - quarter turns (there is no SWAP form under cubic), a translucent draw over a transparent canvas, a stack of more
than one draw - is GENERAL.  With IST_NO_LDS neither streamed form is compiled: GENERAL, except copies.

kernel_kind of a cubic job: 6 when it holds a per-pixel cell, 5 when it holds a streamed cubic cell and none per pixel, and otherwise
what the same cells launch under 'area': 3 for streamed box cells alone, 0 for copies and fills."""
import math

FILL, COPY, SAMPLE, GENERAL, AREA_STREAM, CUBIC_STREAM = 0, 1, 2, 3, 7, 8
NAMES = {FILL: "FILL", COPY: "COPY", GENERAL: "GENERAL", AREA_STREAM: "AREA", CUBIC_STREAM: "CUBIC"}
FLAT = (256, 8)               # tile of a FILL / COPY cell


def area_tile(akx, aky):
    """(tile_w, tile_h) of a streamed box-filter cell, or None where no tile fits (then GENERAL)"""
    bwx = max(akx, 1.0)

    def foot_px(w):
        return (math.ceil((w - 1) * akx + bwx) + 2 + 3) & ~3

    tw = 0
    room = 256.0 - 3.0 - bwx
    if room >= 0.0:
        w = int(min(128.0, math.floor(room / max(akx, 1e-9)) + 1.0))
        if w >= 24:
            tw = w
    if not tw and akx <= 200.0:
        for w in (16, 8, 4, 2, 1):
            if foot_px(w) <= 768:
                tw = w
                break
    if not tw:
        return None
    box_rows = math.ceil(max(aky, 1.0)) + 1
    return tw, (32 if box_rows <= 4 else 8 if box_rows <= 6 else 4)


def form(akx, aky, turned=False, fast=True, copy=False, no_lds=False):
    """(path, tile_w, tile_h, sub_h) of a cell that holds one draw under filter 'cubic'.  fast: the canvas under the draw is opaque or the
    draw carries the opaque hint; copy: the draw is 1:1 at an integer offset and the cell lies inside its clamp box"""
    general = (GENERAL, 64, 64, 0)
    if akx > 1.0 or aky > 1.0:
        if turned or not fast or no_lds or not (akx > 1.0 and aky > 1.0) or aky > 64.0:
            return general
        t = area_tile(akx, aky)
        return (AREA_STREAM, t[0], t[1], 0) if t else general
    if turned or not fast:
        return general
    if copy and akx == 1.0 and aky == 1.0:
        return (COPY,) + FLAT + (0,)
    return general if no_lds else (CUBIC_STREAM, 256, 32, 0)


def kernel_kind(paths):
    """of a cubic job whose cells have these paths"""
    paths = set(paths)
    if GENERAL in paths:
        return 6
    if CUBIC_STREAM in paths:
        return 5
    return 3 if AREA_STREAM in paths else 0


def name(f):
    return "%s-%d" % (NAMES[f[0]], f[1]) if f[0] == AREA_STREAM else NAMES[f[0]]


# ------------------------------------------------------------------------------------------------ inside tile_cubic_stream
def sp_of(akx):
    """source pixels per lane of the row pass: the template instance"""
    return 4 if akx > 0.5 else 2 if akx > 0.25 else 1


def tile_row(kx, ox, X0, X1):
    """(SP, wl, chunks, rounds) of the tile [X0, X1) of a draw whose source x is kx (X + 0.5) + ox: wl source pixels per LDS row - the
    taps floor(f) - 1 .. floor(f) + 2 of the tile's first and last column, rounded up to 4 -, wl / SP chunks, 64 of them per round"""
    fa = (kx * (X0 + 0.5) + ox) - 0.5
    fb = (kx * ((X1 - 1) + 0.5) + ox) - 0.5
    fx0, fx1 = math.floor(min(fa, fb)) - 1, math.floor(max(fa, fb)) + 2
    wl = (fx1 - fx0 + 1 + 3) & ~3
    sp = sp_of(abs(kx))
    chunks = wl // sp
    return sp, wl, chunks, -(-chunks // 64)


def host_row(akx):
    """the source pixels per LDS row the compiler provides for (lds_words = 16 times this); every tile_row(...)[1] must fit"""
    return (math.floor(255.0 * akx) + 5 + 3) & ~3


def rounds_of(kx, ox, cw, x0=0):
    """the most rounds any 256-pixel tile of the canvas columns [x0, cw) takes, and the chunk counts of its tiles"""
    tiles = [tile_row(kx, ox, X, min(X + 256, cw)) for X in range(x0, cw, 256)]
    return max(t[3] for t in tiles), [t[2] for t in tiles]


def regime(kx, ox, cw, opaque):
    """'SP4/opaque/2r': the label of a one-draw case"""
    return "SP%d/%s/%dr" % (sp_of(abs(kx)), "opaque" if opaque else "translucent", rounds_of(kx, ox, cw)[0])


REGIMES = ["SP%d/%s/%dr" % (sp, o, r) for sp in (4, 2, 1) for o in ("opaque", "translucent") for r in (1, 2)]


def bisect_span(pred, ext, k_lo, k_hi):
    """pred(k_lo) and not pred(k_hi): the two adjacent doubles (s_lo, s_hi) of the source span between which pred(span / ext) - the scale
    as the library computes it for a destination of `ext` pixels - turns false"""
    a, b = k_lo * ext, k_hi * ext
    assert pred(a / ext) and not pred(b / ext)
    while True:
        m = 0.5 * (a + b)
        if m <= a or m >= b:
            return a, b
        if pred(m / ext):
            a = m
        else:
            b = m


# the thresholds of the rule on |kx| (and 1.0 on |ky|): (name, threshold); the side at or below it and the side above it differ
THRESHOLDS = [("quarter", 0.25), ("half", 0.5), ("one", 1.0)]


def spans_at(threshold, ext):
    """(last span whose quotient span / ext is <= threshold, first span above it)"""
    return bisect_span(lambda k: k <= threshold, ext, threshold * 0.99, threshold * 1.01)
