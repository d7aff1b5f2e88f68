"""The bilinear cell classification of ist_compile.cpp restated in Python (test infrastructure, no GPU), and the scales that sit on
either side of every boundary of that rule.

A cell with ONE draw over an opaque colour (or an opaque-hinted draw over anything) becomes, by (|kx|, |ky|) alone:

  axis-aligned   |ky| >= 2   SAMPLE_STREAM, the widest of 256 / 128 / 64 pixels whose ring (4 waves x 2 pairs x 2 rows of the tile's
                             x footprint) fits 12288 words, 16384 for the narrowest; beyond that (|kx| > ~16.2) the direct SAMPLE path
                 |ky| <  2   SAMPLE_LDS while |kx| <= 4: 256 wide with the tallest stage of 32, 28, ... 4 rows whose footprint fits 6144
                             words, else 128 wide (64 is never needed: a 128-wide stage of 4 rows always fits); direct above |kx| = 4
  quarter turn               SWAP_LDS, 64 wide and 64 / 32 / 16 high by fw * (fh | 1) <= 8192 with fw = floor((th - 1) |kx|) + 3 source
                             columns (driven by canvas y) and fh = floor(63 |ky|) + 3 source rows; else, or past 128 on an axis, GENERAL

A source one pixel wide or high (an empty second tap: cx1 == cx0 or cy1 == cy0) takes the direct path (GENERAL when turned), filter
'nearest' always does, and a translucent draw over a transparent canvas, or a stack of more than one draw, is GENERAL.  test_cell_paths.py
checks all of this against ist_debug_cells; the GPU tests take their scales from boundaries() below."""
import math

FILL, COPY, SAMPLE, GENERAL, SAMPLE_LDS, SWAP_LDS, SAMPLE_STREAM = 0, 1, 2, 3, 4, 5, 6
NAMES = {FILL: "FILL", COPY: "COPY", SAMPLE: "DIRECT", GENERAL: "GENERAL", SAMPLE_LDS: "LDS", SWAP_LDS: "SWAP", SAMPLE_STREAM: "STREAM"}
LDS_BUDGET, STREAM_CAP, STREAM_MAX, RING, STREAM_H, STREAM_MIN_K, SWAP_WORDS = 6144, 12288, 16384, 2, 8, 2.0, 8192


def _row_px(tw, akx):
    """pixels per LDS row of a tile tw canvas pixels wide"""
    return (math.floor((tw - 1) * akx) + 3 + 3) & ~3


def form(akx, aky, turned=False, filt="bilinear", degenerate=False, fast=True, no_lds=False):
    """(path, tile_w, tile_h, sub_h) of a cell that holds one draw which is no 1:1 copy.  degenerate: the clamp box is one pixel wide or
    high; fast: the canvas under the draw is opaque or the draw carries the opaque hint (otherwise the paint stack runs per pixel)"""
    if not fast:
        return (GENERAL, 64, 64, 0)
    if turned:
        if filt == "bilinear" and not degenerate and not no_lds and akx <= 128.0 and aky <= 128.0:
            for th in (64, 32, 16):
                fw, fh = math.floor((th - 1) * akx) + 3, math.floor(63.0 * aky) + 3
                if fw * (fh | 1) <= SWAP_WORDS:
                    return (SWAP_LDS, 64, th, 0)
        return (GENERAL, 64, 64, 0)
    if filt != "bilinear" or degenerate or no_lds:
        return (SAMPLE, 256, 32, 0)
    if aky >= STREAM_MIN_K and akx <= 64.0:
        for tw in (256, 128, 64):
            need = 4 * 2 * RING * _row_px(tw, akx)
            if (need > STREAM_CAP and tw > 64) or need > STREAM_MAX:
                continue
            return (SAMPLE_STREAM, tw, STREAM_H, RING)
    if akx <= 4.0 and aky <= 8.0:
        for tw in (256, 128, 64):
            for t in range(32, 0, -4):
                if _row_px(tw, akx) * (math.floor((t - 1) * aky) + 3) <= LDS_BUDGET:
                    return (SAMPLE_LDS, tw, 2 * t, t)
    return (SAMPLE, 256, 32, 0)


def name(f):
    """LDS-256/12, STREAM-128, SWAP-32, DIRECT, GENERAL"""
    if f[0] == SAMPLE_LDS:
        return "LDS-%d/%d" % (f[1], f[3])
    if f[0] == SAMPLE_STREAM:
        return "STREAM-%d" % f[1]
    if f[0] == SWAP_LDS:
        return "SWAP-%d" % f[2]
    return NAMES[f[0]]


def log_grid(lo=0.2, hi=150.0, n=25):
    return [lo * (hi / lo) ** (i / (n - 1.0)) for i in range(n)]


def bisect_span(f_of_k, ext, k_lo, k_hi):
    """f_of_k(k_lo) != f_of_k(k_hi): the two adjacent doubles (s_lo, s_hi) of the source span between which f(span / ext) - the scale as
    the library computes it for a destination of `ext` pixels - changes"""
    a, b = k_lo * ext, k_hi * ext
    fa = f_of_k(a / ext)
    assert fa != f_of_k(b / ext)
    while True:
        m = 0.5 * (a + b)
        if m <= a or m >= b:
            return a, b
        if f_of_k(m / ext) == fa:
            a = m
        else:
            b = m


# the lines of the (|kx|, |ky|) plane the sweeps walk: (name, turned, swept source axis, the other axis' scale)
LINES = [
    ("x@ky1", False, "x", 1.0),         # every LDS-256 stage height, then direct at |kx| = 4
    ("x@ky1.5", False, "x", 1.5),       # ... LDS-256 -> LDS-128 -> direct
    ("x@ky1.9", False, "x", 1.9),
    ("x@ky2.5", False, "x", 2.5),       # STREAM-256 -> 128 -> 64 -> direct
    ("y@kx1", False, "y", 1.0),         # every LDS stage height along y, then STREAM at |ky| = 2
    ("y@kx3.5", False, "y", 3.5),       # LDS-256 -> LDS-128 -> STREAM-128
    ("y@kx5", False, "y", 5.0),         # direct below |ky| = 2, STREAM-128 from there
    ("tx@ky1", True, "x", 1.0),         # SWAP 64 -> 32 -> 16 -> GENERAL
    ("ty@kx1", True, "y", 1.0),
]

# The lines the GPU sweep draws: the same walks with the other axis at an irrational scale.  On noise, a scale with a small denominator
# on both axes (1, 1.5, 2.5, but also 1.03 or 5.1: weights in steps of 1/100 or 1/20) makes a good share of all blends land EXACTLY on a
# rounding tie x.5.  The fp64 oracle sees such a value as x.5 -+ 1e-11, whichever way the rounding of 5.1 fell, and rounds it accordingly;
# fp32 cannot resolve that (ulp 1.5e-5 at 255), sees the tie and rounds half up - so half of the ties differ, all by +1, and a form looked
# biased by up to +0.02 LSB when the sweep ran on such lines (every differing byte's exact value was within 1e-10 of a tie, or within 1.4e-5
# under the offset 0.5 - 1e-6).  That measures the input, not the arithmetic.  With one axis irrational the blends are spread evenly between
# the integers, and what is left are the incidental near-ties the 1 % / 0.001 LSB rule allows for; exact ties are held to equality by the
# known-answer test.
_R = math.sqrt
SWEEP_LINES = [
    ("x@ky1.03", False, "x", _R(1.06)), ("x@ky1.47", False, "x", _R(2.16)), ("x@ky2.53", False, "x", _R(6.4)),
    ("y@kx1.03", False, "y", _R(1.06)), ("y@kx3.46", False, "y", _R(12.0)), ("y@kx5.1", False, "y", _R(26.0)),
    ("tx@ky1.03", True, "x", _R(1.06)), ("ty@kx1.03", True, "y", _R(1.06)),
]


def line_form(line, k, **kw):
    _, turned, axis, other = line
    return form(k, other, turned, **kw) if axis == "x" else form(other, k, turned, **kw)


def boundaries(line, grid=None):
    """every change of form along a line: [(k_below, k_above, form_below, form_above)], found on the log grid and narrowed by bisection
    on the restatement (in plain scales; the sweeps narrow further to adjacent doubles of the span they draw)"""
    grid = grid or log_grid(n=400)
    out = []
    for a, b in zip(grid, grid[1:]):
        fa, fb = line_form(line, a), line_form(line, b)
        while fa != fb:                  # (a grid step may hold more than one change: peel them off from the left)
            lo, hi = a, b
            for _ in range(200):
                m = 0.5 * (lo + hi)
                if m <= lo or m >= hi:
                    break
                if line_form(line, m) == fa:
                    lo = m
                else:
                    hi = m
            out.append((lo, hi, fa, line_form(line, hi)))
            a, fa = hi, line_form(line, hi)
    return out
