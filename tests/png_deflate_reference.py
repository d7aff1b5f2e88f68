"""The compressing PNG export (ist_png_deflate.hip, pngLevel 1) restated on the CPU, byte for byte.

The encoder is deterministic by design - one chunk grid, one tokeniser, one code rule, fixed framing - so this module predicts
every byte of its files from the stream design documented at the top of ist_png_deflate.hip and in DESIGN.md (PNG export).
Plain Python / numpy, integer arithmetic only, nothing imported from the package under test:

  filter   Paeth on every row (filter byte 4); left / up / upper left are zero outside the image, ties in that order.
  grid     R = 4 w + 1 filtered bytes per row.  R <= 16384: a chunk is 16384 // R whole rows (the last chunk may hold fewer);
           otherwise a chunk is a piece of one row of at most 4095 pixels, the filter byte travelling with the piece at x = 0.
  tokens   the chunk in spans of 64 bytes (the last one ragged).  Inside a span a run of R >= 4 equal bytes is its first byte as
           a literal + ONE match of R - 1 bytes at distance 1; shorter runs are literals; no run continues across a span
           boundary, so match lengths are 3..63.  Length symbols and extra bits: RFC 1951, 3.2.5.
  code     histogram over the 286 literal/length symbols (+ 1 for end-of-block); a symbol with count c gets the length
           ceil(log2(ceil(total / c))) clamped to 1..15; then up to 16 rounds: for l = 2..15 ascending, the first
           min(class size, slack // 2^(15-l)) symbols of length l, in symbol order, lose one bit.  Slack left after 16
           rounds: the chunk is stored.  Canonical codes (RFC 1951, 3.2.2).
  block    BFINAL 0, BTYPE 2, HLIT 29, HDIST 0, HCLEN 15; the nineteen code-length-code lengths 0, 0, 0, 4 x 16 (so the code
           of code length v is v in 4 bits); 286 literal/length lengths and the one distance length (1); the tokens, a match
           followed by one zero bit for its distance; end-of-block; an empty stored block that re-aligns to a byte.
  stored   taken when the Huffman form is not smaller (a tie is stored): 00 LEN NLEN and the bytes.
  framing  78 01 in front of chunk 0 only; every chunk padded with 00 00 00 FF FF blocks to a multiple of 16 bytes; after the
           last chunk 01 00 00 FF FF and the big-endian Adler-32 of the filtered stream.
  file     signature, IHDR (8 bit, colour type 6), the 11-byte tEXt chunk "Software\\0is" (which puts the IDAT data at offset
           64), the IDAT chunks, IEND.

encode() also reports, per chunk, its form, pad count, byte count, tokens and the rounds its code took: the tests use these to
assert that an input reaches the regime it was built for.  RULES is the design; a test may pass a mutated copy (Rules._replace)
to show that its inputs can tell the design from a near miss."""
import collections
import struct
import zlib

import numpy as np

CH = 16384                      # most filtered-stream bytes in one chunk
SPAN = 64                       # bytes per span
PIECE_PX = (CH - 1) // 4        # pixels in a piece of a row that is longer than a chunk
NSYM = 286
EOB = 256
MATCH = 256                     # a token t < 256 is the literal t; t >= 256 is a match of t - 256 bytes at distance 1
FIRST_SLAB = 768                # the host path (encode_png, stitch_png) compresses in slabs of chunks: 768, then 4096 each
SLAB = 4096

Rules = collections.namedtuple("Rules", "matches min_run cross_span tie_stored slack_reverse extra_pads grid_late")
RULES = Rules(matches=True, min_run=4, cross_span=False, tie_stored=True, slack_reverse=False, extra_pads=0, grid_late=False)


# ---- RFC 1951, 3.2.5: the length symbols -------------------------------------------------------------------------------------
def _length_table():
    base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    extra = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    table = {}
    for k in range(len(base) - 1, -1, -1):                 # (258 is symbol 285, not 284 + 31)
        for v in range(1 << extra[k]):
            table.setdefault(base[k] + v, (257 + k, extra[k], v))
    return table


LENGTH = _length_table()        # match length -> (symbol, extra-bit count, extra-bit value)


def symbol_of(token):
    return token if token < MATCH else LENGTH[token - MATCH][0]


def format_tokens(tokens):
    """'L4 L0 M62 ...'"""
    return " ".join(("L%d" % t) if t < MATCH else ("M%d" % (t - MATCH)) for t in tokens)


# ---- filter -------------------------------------------------------------------------------------------------------------------
def filtered_rows(rgba):
    """h x (4 w + 1) uint8: per row the filter byte 4 and the Paeth residuals (PNG specification, 9.4)"""
    a = np.asarray(rgba)
    assert a.ndim == 3 and a.shape[2] == 4 and a.dtype == np.uint8
    h, w = a.shape[:2]
    a = a.astype(np.int32)
    left, up, ul = np.zeros_like(a), np.zeros_like(a), np.zeros_like(a)
    left[:, 1:] = a[:, :-1]
    up[1:] = a[:-1]
    ul[1:, 1:] = a[:-1, :-1]
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    out = np.empty((h, 4 * w + 1), np.uint8)
    out[:, 0] = 4
    out[:, 1:] = ((a - pred) & 255).reshape(h, 4 * w)
    return out


# ---- chunk grid ---------------------------------------------------------------------------------------------------------------
def make_grid(w, h, rules=RULES):
    """[(y0, rows, x0, pixels)]: the canvas region of every chunk, in stream order"""
    R = 4 * w + 1
    if R <= CH + (4 if rules.grid_late else 0):
        rpc = max(1, CH // R)
        return [(y, min(rpc, h - y), 0, w) for y in range(0, h, rpc)]
    return [(y, 1, x, min(PIECE_PX, w - x)) for y in range(h) for x in range(0, w, PIECE_PX)]


def chunk_bytes(filt, cell):
    y0, rows, x0, px = cell
    if x0 == 0:
        return filt[y0:y0 + rows, :1 + 4 * px].reshape(-1)
    return filt[y0, 1 + 4 * x0:1 + 4 * (x0 + px)]


# ---- tokens -------------------------------------------------------------------------------------------------------------------
def tokenise(data, rules=RULES):
    """a chunk's bytes -> its tokens (numpy int array: literals 0..255, MATCH + length)"""
    data = np.asarray(data, np.uint8)
    n = len(data)
    if n == 0:
        return np.zeros(0, np.int64)
    new = np.ones(n, bool)
    new[1:] = data[1:] != data[:-1]
    if not rules.cross_span:
        new[::SPAN] = True
    starts = np.flatnonzero(new)
    lens = np.diff(np.append(starts, n))
    vals = data[starts].astype(np.int64)
    if rules.cross_span:                                   # (a mutation only: matches of up to 258 bytes, the rest as it comes)
        out = []
        for v, run in zip(vals.tolist(), lens.tolist()):
            out.append(v)
            rest = run - 1
            if not rules.matches or run < rules.min_run:
                out.extend([v] * rest)
                continue
            while rest > 0:
                m = min(rest, 258)
                out.extend([MATCH + m] if m >= 3 else [v] * m)
                rest -= m
        return np.asarray(out, np.int64)
    is_match = (lens >= rules.min_run) if rules.matches else np.zeros(len(lens), bool)
    counts = np.where(is_match, 2, lens)
    tokens = np.repeat(vals, counts)
    last = np.cumsum(counts) - 1
    tokens[last[is_match]] = MATCH + lens[is_match] - 1
    return tokens


def histogram(tokens):
    counts = [0] * NSYM
    lit = tokens[tokens < MATCH]
    for s, c in enumerate(np.bincount(lit, minlength=256).tolist()):
        counts[s] = c
    for t, c in zip(*np.unique(tokens[tokens >= MATCH], return_counts=True)):
        counts[LENGTH[int(t) - MATCH][0]] += int(c)
    counts[EOB] += 1
    return counts


# ---- code ---------------------------------------------------------------------------------------------------------------------
def code_lengths(counts, rules=RULES, max_rounds=16):
    """(lengths per symbol or None when the code is not complete after max_rounds, rounds used)"""
    total = sum(counts)
    length = [0] * len(counts)
    for s, c in enumerate(counts):
        if c:
            r = (total + c - 1) // c                       # ceil(total / c)
            length[s] = min(15, max(1, (r - 1).bit_length()))      # ceil(log2(r))
    slack = (1 << 15) - sum(1 << (15 - l) for l in length if l)
    assert slack >= 0
    rounds = 0
    while slack > 0 and rounds < max_rounds:
        rounds += 1
        for l in range(2, 16):
            cls = [s for s, v in enumerate(length) if v == l]
            cost = 1 << (15 - l)
            take = min(len(cls), slack // cost)
            for s in (cls[len(cls) - take:] if rules.slack_reverse else cls[:take]):
                length[s] = l - 1
            slack -= take * cost
    return (length if slack == 0 else None), rounds


def canonical_codes(length):
    """RFC 1951, 3.2.2: per symbol the code as a string of bits in the order they are sent (most significant first)"""
    bl_count = [0] * 17
    for l in length:
        if l:
            bl_count[l] += 1
    next_code, code = [0] * 17, 0
    for bits in range(1, 17):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    out = [None] * len(length)
    for s, l in enumerate(length):
        if l:
            out[s] = format(next_code[l], "0%db" % l)
            assert len(out[s]) == l
            next_code[l] += 1
    return out


def _lsb(value, bits):
    """a header field or extra bits: least significant bit first"""
    return format(value, "0%db" % bits)[::-1] if bits else ""


def _pack(bits):
    """a string of bits in sending order -> bytes (bit k of the stream is bit k % 8 of byte k // 8); zero bits to the boundary"""
    bits += "0" * (-len(bits) % 8)
    return int(bits[::-1], 2).to_bytes(len(bits) // 8, "little") if bits else b""


HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + (NSYM + 1) * 4


def huffman_body(tokens, length):
    """the chunk as one dynamic-Huffman block + the empty stored block that re-aligns to a byte (without the lead bytes)"""
    code = canonical_codes(length)
    head = _lsb(0, 1) + _lsb(2, 2) + _lsb(NSYM - 257, 5) + _lsb(0, 5) + _lsb(19 - 4, 4)
    head += "".join(_lsb(v, 3) for v in [0, 0, 0] + [4] * 16)
    head += "".join(format(l, "04b") for l in length) + format(1, "04b")
    assert len(head) == HEADER_BITS
    table = {}
    for t in set(tokens.tolist()):
        if t < MATCH:
            table[t] = code[t]
        else:
            sym, eb, ev = LENGTH[t - MATCH]
            table[t] = code[sym] + _lsb(ev, eb) + "0"
    bits = head + "".join(map(table.__getitem__, tokens.tolist())) + code[EOB] + "000"
    return _pack(bits) + b"\x00\x00\xff\xff"


def huffman_size(tokens, length):
    """len(huffman_body(...)) from the token bits alone"""
    cost = {}
    for t, c in zip(*np.unique(tokens, return_counts=True)):
        t = int(t)
        cost[t] = int(c) * (length[t] if t < MATCH else length[LENGTH[t - MATCH][0]] + LENGTH[t - MATCH][1] + 1)
    return (HEADER_BITS + sum(cost.values()) + length[EOB] + 3 + 7) // 8 + 4


def stored_body(data):
    n = len(data)
    assert n <= 0xFFFF
    return b"\x00" + struct.pack("<HH", n, n ^ 0xFFFF) + bytes(data)


PAD = b"\x00\x00\x00\xff\xff"
Chunk = collections.namedtuple("Chunk", "form pads nbytes tokens rounds data huff_size stored_size offset")


def chunk_form(data, rules=RULES):
    """(tokens, lengths or None, rounds, Huffman size or None, stored size) of a chunk's bytes, lead bytes not counted (they are
    the same two bytes in either form)"""
    tokens = tokenise(data, rules)
    length, rounds = code_lengths(histogram(tokens), rules)
    return tokens, length, rounds, (None if length is None else huffman_size(tokens, length)), 5 + len(data)


def encode_chunk(data, first, rules=RULES, offset=0):
    """(bytes of the chunk in the stream, Chunk report)"""
    tokens, length, rounds, hsize, ssize = chunk_form(data, rules)
    stored = length is None or (hsize >= ssize if rules.tie_stored else hsize > ssize)
    body = stored_body(data) if stored else huffman_body(tokens, length)
    assert len(body) == (ssize if stored else hsize)
    out = (b"\x78\x01" if first else b"") + body
    pads = 0
    while (len(out) + 5 * pads) % 16:
        pads += 1
    out += PAD * (pads + rules.extra_pads)
    return out, Chunk("stored" if stored else "huff", pads, len(out), tokens, rounds, data, hsize, ssize, offset)


Encoded = collections.namedtuple("Encoded", "stream chunks filtered")


def encode(rgba, rules=RULES):
    """the whole zlib stream of a canvas with the per-chunk report"""
    h, w = rgba.shape[:2]
    filt = filtered_rows(rgba)
    parts, chunks, at = [], [], 0
    for k, cell in enumerate(make_grid(w, h, rules)):
        b, rep = encode_chunk(chunk_bytes(filt, cell), k == 0, rules, at)
        parts.append(b)
        chunks.append(rep)
        at += len(b)
    raw = filt.tobytes()
    parts.append(b"\x01\x00\x00\xff\xff" + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF))
    return Encoded(b"".join(parts), chunks, raw)


def zlib_stream(rgba):
    return encode(rgba).stream


# ---- file ---------------------------------------------------------------------------------------------------------------------
def png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def file_head(w, h):
    return b"\x89PNG\r\n\x1a\n" + png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + png_chunk(b"tEXt", b"Software\x00is")


def file_bytes(rgba, stream=None):
    """the file of one slab and one IDAT (the device entry points without an IDAT limit)"""
    h, w = rgba.shape[:2]
    return file_head(w, h) + png_chunk(b"IDAT", zlib_stream(rgba) if stream is None else stream) + png_chunk(b"IEND", b"")


def idat_limit(setting=None):
    """IST_PNG_IDAT_LIMIT as the encoder reads it"""
    v = int(setting) if setting else 0
    return (v & ~15) if v >= 4096 else 1 << 30


def host_slabs(n_chunks):
    """chunks per slab on the host path: the first slab is short, the others 4096 chunks"""
    out = [min(n_chunks, FIRST_SLAB)]
    while sum(out) < n_chunks:
        out.append(min(SLAB, n_chunks - sum(out)))
    return out


def idat_lengths(chunk_sizes, limit=1 << 30, slabs=None):
    """the data length of every IDAT (FileLayout::slab): a slab starts an IDAT of its own; inside a slab a chunk that would
    take a non-empty IDAT beyond limit - 9 starts the next one; the 9 trailer bytes go into the last"""
    slabs = slabs or [len(chunk_sizes)]
    assert sum(slabs) == len(chunk_sizes)
    out, k = [], 0
    for s in slabs:
        cur = 0
        for size in chunk_sizes[k:k + s]:
            if cur > 0 and cur + size + 9 > limit:
                out.append(cur)
                cur = 0
            cur += size
        out.append(cur)
        k += s
    out[-1] += 9
    return out
