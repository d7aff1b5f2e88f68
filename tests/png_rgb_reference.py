"""The RGB form of the compressing PNG export (ist_ctx_set_png_color, IST_PNG_RGB; pngColor 'rgb') restated on the CPU, byte for byte.

Only what differs from the RGBA form (tests/png_deflate_reference.py) is stated here; everything behind the filter - spans, tokens, the
code rule, the block header, stored against Huffman and its tie, framing and pads, the Adler-32 over the filtered stream, the slabs
of the host path and the IDAT layout - is that module's, used unchanged:

  pixels   R, G and B as stored; the alpha byte of the canvas is NOT read.
  filter   Paeth on every row (filter byte 4) over the 3 w colour bytes; left / up / upper left are the same channel of the
           neighbouring PIXEL (3 bytes back), zero outside the image, ties in that order.
  grid     R = 3 w + 1 filtered bytes per row.  R <= 16384: a chunk is 16384 // R whole rows (the last chunk may hold fewer);
           otherwise a chunk is a piece of one row of at most (16384 - 1) // 3 = 5461 pixels, the filter byte travelling with the
           piece at x = 0.
  file     IHDR with colour type 2, 8 bit; the tEXt chunk and the rest as in the RGBA form.

Plain Python / numpy; nothing is imported from the package under test.  make_grid_rgb takes the two numbers of the grid as
arguments so that a test can show that its inputs tell the design from a near miss (piece_px = 4095, or rows of 4 w + 1)."""
import struct
import zlib

import numpy as np

from tests import png_deflate_reference as R

BPP = 3
PIECE_PX = (R.CH - 1) // BPP        # 5461


def filtered_rows_rgb(rgba):
    """h x (3 w + 1) uint8: per row the filter byte 4 and the Paeth residuals of R, G, B (PNG specification, 9.4)"""
    a = np.asarray(rgba)
    assert a.ndim == 3 and a.shape[2] == 4 and a.dtype == np.uint8
    h, w = a.shape[:2]
    a = a[..., :3].astype(np.int32)
    left, up, ul = np.zeros_like(a), np.zeros_like(a), np.zeros_like(a)
    left[:, 1:] = a[:, :-1]
    up[1:] = a[:-1]
    ul[1:, 1:] = a[:-1, :-1]
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    out = np.empty((h, BPP * w + 1), np.uint8)
    out[:, 0] = 4
    out[:, 1:] = ((a - pred) & 255).reshape(h, BPP * w)
    return out


def unfilter_rows_rgb(filt, rgb):
    """The inverse of the filter, column by column: row y is rebuilt from its residuals, its own rebuilt left neighbours and row
    y - 1 of `rgb` (zeros above row 0).  If the result equals `rgb`, then by induction over the rows a decoder that un-filters from
    the top gets `rgb`: row 0 has nothing above it, and row y is rebuilt from a row y - 1 that is already known to be right.
    (All rows at once, so that a canvas of two million pixels takes w steps, not w h.)"""
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    filt = np.asarray(filt, np.uint8).reshape(h, BPP * w + 1)
    assert (filt[:, 0] == 4).all()
    res = filt[:, 1:].reshape(h, w, BPP).astype(np.int32)
    up = np.zeros((h, w + 1, BPP), np.int32)                 # column 0: the zero left of the image
    up[1:, 1:] = rgb[:-1].astype(np.int32)
    out = np.zeros((h, w + 1, BPP), np.int32)
    for x in range(1, w + 1):
        left, b, ul = out[:, x - 1], up[:, x], up[:, x - 1]
        p = left + b - ul
        pa, pb, pc = np.abs(p - left), np.abs(p - b), np.abs(p - ul)
        pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, b, ul))
        out[:, x] = (res[:, x - 1] + pred) & 255
    return out[:, 1:].astype(np.uint8)


def make_grid_rgb(w, h, piece_px=PIECE_PX, row_bytes=None):
    """[(y0, rows, x0, pixels)]: the canvas region of every chunk, in stream order.  piece_px / row_bytes: the design's values
    unless a test bends them"""
    row = BPP * w + 1 if row_bytes is None else row_bytes
    if row <= R.CH:
        rpc = max(1, R.CH // row)
        return [(y, min(rpc, h - y), 0, w) for y in range(0, h, rpc)]
    return [(y, 1, x, min(piece_px, w - x)) for y in range(h) for x in range(0, w, piece_px)]


def grid_numbers_rgb(w, h):
    """(n_chunks, rows_per_chunk (0: pieces), pieces_per_row, piece_px): the four numbers ist_debug_png_grid reports"""
    row = BPP * w + 1
    if row <= R.CH:
        rpc = R.CH // row
        return (-(-h // rpc), rpc, 0, 0)
    ppr = -(-w // PIECE_PX)
    return (h * ppr, 0, ppr, PIECE_PX)


def grid_numbers_rgba(w, h):
    """the same four numbers of the RGBA grid (R = 4 w + 1, pieces of 4095 pixels), from png_deflate_reference's constants"""
    row = 4 * w + 1
    if row <= R.CH:
        rpc = R.CH // row
        return (-(-h // rpc), rpc, 0, 0)
    ppr = -(-w // R.PIECE_PX)
    return (h * ppr, 0, ppr, R.PIECE_PX)


def chunk_bytes_rgb(filt, cell):
    y0, rows, x0, px = cell
    if x0 == 0:
        return filt[y0:y0 + rows, :1 + BPP * px].reshape(-1)
    return filt[y0, 1 + BPP * x0:1 + BPP * (x0 + px)]


def encode_rgb(rgba, grid=None):
    """the whole zlib stream of a canvas in the RGB form with the per-chunk report (png_deflate_reference.Encoded)"""
    h, w = rgba.shape[:2]
    filt = filtered_rows_rgb(rgba)
    parts, chunks, at = [], [], 0
    for k, cell in enumerate(make_grid_rgb(w, h) if grid is None else grid):
        b, rep = R.encode_chunk(chunk_bytes_rgb(filt, cell), k == 0, R.RULES, at)
        parts.append(b)
        chunks.append(rep)
        at += len(b)
    raw = filt.tobytes()
    parts.append(b"\x01\x00\x00\xff\xff" + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF))
    return R.Encoded(b"".join(parts), chunks, raw)


def file_head_rgb(w, h):
    return b"\x89PNG\r\n\x1a\n" + R.png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + R.png_chunk(b"tEXt", b"Software\x00is")


def file_bytes_rgb(rgba, stream=None):
    """the file of one slab and one IDAT (the device entry points without an IDAT limit)"""
    h, w = rgba.shape[:2]
    return file_head_rgb(w, h) + R.png_chunk(b"IDAT", encode_rgb(rgba).stream if stream is None else stream) + R.png_chunk(b"IEND", b"")
