"""The adaptive row filters of the compressing PNG export (ist_ctx_set_png_filter, IST_PNG_FILTER_ADAPTIVE; pngFilter 'adaptive')
restated on the CPU, byte for byte.

Only the filter is stated here; the grid, spans, tokens, the code rule, stored against Huffman, framing and pads, the Adler-32 over
the filtered stream, the slabs of the host path and the IDAT layout are those of tests/png_deflate_reference.py (RGBA, bpp 4) and
tests/png_rgb_reference.py (RGB, bpp 3: the alpha byte is not read), used unchanged.  The IHDR is unchanged too: filter method 0
allows a type per row.

  residuals  PNG specification 9.2 - 9.4, per byte: None x, Sub x - left, Up x - up, Average x - ((left + up) >> 1) on the unwrapped
             0..255 values, Paeth x - the neighbour closest to left + up - upper left (ties: left, up, upper left).  left / up /
             upper left are the same channel of the neighbouring PIXEL, zero outside the image.
  cost       cost_f(y) = sum over the row's bpp w residual bytes r of (r < 128 ? r : 256 - r); the filter byte is not counted.
  choice     row y gets the type of least cost; ties go to the first of 4, 1, 2, 3, 0 - Paeth wins ties, so flat rows stay type 4, and
             on row 0, where Sub is Paeth and None is Up, neither Sub nor None is ever chosen.
             The choice is a function of row y and row y - 1 alone: not of the chunk grid, not of the slabs.

RULE is the design; a test may pass a bent copy (RULE._replace) to show that its inputs tell the design from a near miss: the tie
order 0, 1, 2, 3, 4, or the cost taken as the unsigned residual r.  Plain Python / numpy; nothing is imported from the package
under test."""
import collections
import struct
import zlib

import numpy as np

from tests import png_deflate_reference as R
from tests import png_rgb_reference as G

NONE, SUB, UP, AVERAGE, PAETH = range(5)
FilterRule = collections.namedtuple("FilterRule", "tie_order signed_cost")
RULE = FilterRule(tie_order=(4, 1, 2, 3, 0), signed_cost=True)
NEAR_MISSES = {"tie order 0,1,2,3,4": RULE._replace(tie_order=(0, 1, 2, 3, 4)), "unsigned cost": RULE._replace(signed_cost=False)}


def residuals(rgba, bpp):
    """5 x h x (bpp w) uint8: the residual bytes of every row under each of the five filter types"""
    a = np.asarray(rgba)
    assert a.ndim == 3 and a.shape[2] == 4 and a.dtype == np.uint8 and bpp in (3, 4)
    h, w = a.shape[:2]
    a = a[..., :bpp].astype(np.int32)
    left, up, ul = np.zeros_like(a), np.zeros_like(a), np.zeros_like(a)
    left[:, 1:] = a[:, :-1]
    up[1:] = a[:-1]
    ul[1:, 1:] = a[:-1, :-1]
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    preds = (np.zeros_like(a), left, up, (left + up) >> 1, paeth)
    return np.stack([((a - q) & 255).astype(np.uint8).reshape(h, bpp * w) for q in preds])


def row_costs(rgba, bpp, rule=RULE):
    """h x 5 int64: cost_f(y)"""
    r = residuals(rgba, bpp).astype(np.int64)
    c = np.where(r < 128, r, 256 - r) if rule.signed_cost else r
    return c.sum(axis=2).T


def row_filters(rgba, bpp, rule=RULE):
    """h uint8: the filter type of every row"""
    cost = row_costs(rgba, bpp, rule)
    best = np.full(cost.shape[0], rule.tie_order[0], np.int64)
    for f in rule.tie_order[1:]:
        better = cost[:, f] < cost[np.arange(cost.shape[0]), best]
        best[better] = f
    return best.astype(np.uint8)


def filtered_rows_adaptive(rgba, bpp, rule=RULE):
    """h x (bpp w + 1) uint8: per row its filter byte and the residuals of that type"""
    res = residuals(rgba, bpp)
    types = row_filters(rgba, bpp, rule)
    h = res.shape[1]
    out = np.empty((h, res.shape[2] + 1), np.uint8)
    out[:, 0] = types
    out[:, 1:] = res[types, np.arange(h)]
    return out


def _grid(w, h, bpp):
    return R.make_grid(w, h) if bpp == 4 else G.make_grid_rgb(w, h)


def encode_adaptive(rgba, bpp, rule=RULE):
    """the whole zlib stream of a canvas with the per-chunk report (png_deflate_reference.Encoded)"""
    h, w = rgba.shape[:2]
    filt = filtered_rows_adaptive(rgba, bpp, rule)
    cut = R.chunk_bytes if bpp == 4 else G.chunk_bytes_rgb
    parts, chunks, at = [], [], 0
    for k, cell in enumerate(_grid(w, h, bpp)):
        b, rep = R.encode_chunk(cut(filt, cell), k == 0, R.RULES, at)
        parts.append(b)
        chunks.append(rep)
        at += len(b)
    raw = filt.tobytes()
    parts.append(b"\x01\x00\x00\xff\xff" + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF))
    return R.Encoded(b"".join(parts), chunks, raw)


def file_head(w, h, bpp):
    return R.file_head(w, h) if bpp == 4 else G.file_head_rgb(w, h)


def file_bytes_adaptive(rgba, bpp, stream=None, rule=RULE):
    """the file of one slab and one IDAT (the device entry points without an IDAT limit)"""
    h, w = rgba.shape[:2]
    data = encode_adaptive(rgba, bpp, rule).stream if stream is None else stream
    return file_head(w, h, bpp) + R.png_chunk(b"IDAT", data) + R.png_chunk(b"IEND", b"")


def host_file_bytes_adaptive(rgba, bpp, rep=None, limit=None):
    """the file of the host path (encode_png, stitch_png): slabs of 768 and then 4096 chunks, an IDAT per slab"""
    h, w = rgba.shape[:2]
    rep = encode_adaptive(rgba, bpp) if rep is None else rep
    sizes = [c.nbytes for c in rep.chunks]
    out, at = file_head(w, h, bpp), 0
    for n in R.idat_lengths(sizes, R.idat_limit(limit), R.host_slabs(len(sizes))):
        out += R.png_chunk(b"IDAT", rep.stream[at:at + n])
        at += n
    assert at == len(rep.stream)
    return out + R.png_chunk(b"IEND", b"")
