"""The window matches of the compressing PNG export (ist_ctx_set_png_match, IST_PNG_MATCH_WINDOW; pngMatch 'window') restated on
the CPU, byte for byte.

Only the encoding of ONE CHUNK's bytes is stated here.  The filter (Paeth, or a type per row), the colour form, the chunk grid, the
64-byte spans, the code rule (Shannon lengths + slack rounds), the stored form, the lead bytes, the pads to 16 bytes, the Adler-32,
the slabs of the host path, the IDAT layout and the IHDR are those of tests/png_deflate_reference.py, tests/png_rgb_reference.py and
tests/png_filter_reference.py, used unchanged.

  candidates  a chunk of n bytes b.  Every position p with p + 4 <= n has a key, the little-endian 32-bit word b[p..p+3], and
              H(p) = ((key * 2654435761) mod 2^32) >> 20, 12 bits.  cand(p) is the GREATEST q that has a key, H(q) == H(p) and
              q < 64 * (p // 64): the most recent position of that hash in an EARLIER span; -1 when there is none or p has no key.
              A function of the chunk's bytes alone.
  parse       every span on its own, from its first byte.  At p:  run = the bytes from p on that equal b[p], inside the span;
              m = the number of i with b[cand(p) + i] == b[p + i] from i = 0 on, at most 63 and not past the span's end, 0 without a
              candidate (the source may run into the destination span: deflate's overlapping copy; a hash collision is m == 0 or
              some m < 4).  m >= 4 and m >= run: ONE match of m bytes at distance p - cand(p).  Otherwise run >= 4: the run form's
              pair, the literal b[p] + one match of run - 1 bytes at distance 1.  Otherwise the literal b[p].
  codes       literal/length: png_deflate_reference.code_lengths over the 286 symbols, as in the run form.  Distance: the same rule
              over the 30 distance symbols (RFC 1951, 3.2.5; a chunk reaches symbol 27).  Exactly one distance symbol in use: it
              gets length 1 (an incomplete code of one 1-bit code, which inflate accepts); none in use: symbol 0 gets length 1, as
              the run form's header says.  Either code incomplete after the rule's 16 rounds: no window form for this chunk.
  block       as the run form's, but HDIST = the highest distance symbol in use, and the HDIST + 1 distance code lengths follow
              the 286 literal/length lengths in the same fixed 4-bit code.  A match is its length code, the length's extra bits,
              its distance code, the distance's extra bits.
  choice      first the default setting's choice, unchanged: stored unless the run form's body is smaller.  The window form replaces
              it only where its CHUNK - lead bytes and the pads to 16 bytes included - is smaller; a tie keeps the default setting's
              bytes.  (The pads are not monotone in the body: a body of 234 bytes pads to 304, one of 236 to 256; so the chunks are
              compared, not the bodies.)  So every chunk, and every file, is at most as large as the default setting's.

encode_chunk() reports per chunk its form ('stored', 'huff' = run form, 'window'), the sizes of the three forms, the window parse and
the rounds of both its codes.  RULE is the design; a test may pass a bent copy (RULE._replace) to show that its inputs tell the
design from a near miss: the first candidate instead of the latest, a candidate in the position's own span, a minimum match of 3,
ties to the window form.  Plain Python / numpy; nothing is imported from the package under test."""
import collections
import struct
import zlib

import numpy as np

from tests import png_deflate_reference as R
from tests import png_filter_reference as F
from tests import png_rgb_reference as G

HASH_MUL = 2654435761
HASH_BITS = 12
MAX_MATCH = 63
NDIST = 30

MatchRule = collections.namedtuple("MatchRule", "latest earlier_span min_match tie_window")
RULE = MatchRule(latest=True, earlier_span=True, min_match=4, tie_window=False)
NEAR_MISSES = {"first candidate": RULE._replace(latest=False), "candidate in the own span": RULE._replace(earlier_span=False),
               "minimum 3": RULE._replace(min_match=3), "ties to window": RULE._replace(tie_window=True)}


# ---- RFC 1951, 3.2.5: the distance symbols ------------------------------------------------------------------------------------
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def dist_code(d):
    """distance -> (symbol, extra-bit count, extra-bit value)"""
    assert 1 <= d <= 32768
    s = max(k for k in range(NDIST) if DIST_BASE[k] <= d)
    return s, DIST_EXTRA[s], d - DIST_BASE[s]


# ---- candidates ---------------------------------------------------------------------------------------------------------------
def hashes(data):
    """H(p) of every position with a key (the first max(0, n - 3))"""
    b = np.asarray(data, np.uint8).astype(np.uint64)
    if len(b) < 4:
        return np.zeros(0, np.int64)
    key = b[:-3] | (b[1:-2] << np.uint64(8)) | (b[2:-1] << np.uint64(16)) | (b[3:] << np.uint64(24))
    return (((key * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HASH_BITS)).astype(np.int64)


def keys(data):
    b = np.asarray(data, np.uint8).astype(np.int64)
    return b[:-3] | (b[1:-2] << 8) | (b[2:-1] << 16) | (b[3:] << 24) if len(b) >= 4 else np.zeros(0, np.int64)


def candidates(data, rule=RULE):
    """cand(p) of every position of the chunk (-1: none)"""
    n = len(data)
    H = hashes(data)
    cand = np.full(n, -1, np.int64)
    table = {}
    if rule.earlier_span:
        for s in range(0, len(H), R.SPAN):             # a span looks everything up, then inserts itself
            hs = H[s:s + R.SPAN].tolist()
            for i, h in enumerate(hs):
                cand[s + i] = table.get(h, -1)
            for i, h in enumerate(hs):
                if rule.latest or h not in table:
                    table[h] = s + i
    else:
        for p, h in enumerate(H.tolist()):
            cand[p] = table.get(h, -1)
            if rule.latest or h not in table:
                table[h] = p
    return cand


# ---- parse --------------------------------------------------------------------------------------------------------------------
LIT, PAIR, WIN = 0, 1, 2
Token = collections.namedtuple("Token", "kind pos value length dist")      # LIT: value; PAIR: value, then length at distance 1; WIN: length, dist


def parse(data, rule=RULE):
    """a chunk's bytes -> its window-form tokens"""
    b = np.asarray(data, np.uint8)
    n = len(b)
    cand = candidates(b, rule).tolist()
    bl = b.tolist()
    out = []
    for s in range(0, n, R.SPAN):
        end = min(n, s + R.SPAN)
        p = s
        while p < end:
            run = 1
            while p + run < end and bl[p + run] == bl[p]:
                run += 1
            m, c = 0, cand[p]
            if c >= 0:
                cap = min(MAX_MATCH, end - p)
                while m < cap and bl[c + m] == bl[p + m]:
                    m += 1
            if m >= rule.min_match and m >= run:
                out.append(Token(WIN, p, None, m, p - c))
                p += m
            elif run >= 4:
                out.append(Token(PAIR, p, bl[p], run - 1, 1))
                p += run
            else:
                out.append(Token(LIT, p, bl[p], 0, 0))
                p += 1
    return out


def histograms(tokens):
    ll, dd = [0] * R.NSYM, [0] * NDIST
    for t in tokens:
        if t.kind != WIN:
            ll[t.value] += 1
        if t.kind != LIT:
            ll[R.LENGTH[t.length][0]] += 1
            dd[dist_code(t.dist)[0]] += 1
    ll[R.EOB] += 1
    return ll, dd


def dist_lengths(dd):
    """(lengths of the 30 distance symbols or None, rounds)"""
    used = [s for s, c in enumerate(dd) if c]
    if len(used) <= 1:
        out = [0] * NDIST
        out[used[0] if used else 0] = 1
        return out, 0
    return R.code_lengths(dd)


def window_body(tokens, ll_len, d_len):
    """the chunk as one dynamic-Huffman block with a distance code + the empty stored block that re-aligns to a byte"""
    code, dcode = R.canonical_codes(ll_len), R.canonical_codes(d_len)
    hdist = max(s for s, l in enumerate(d_len) if l)
    head = R._lsb(0, 1) + R._lsb(2, 2) + R._lsb(R.NSYM - 257, 5) + R._lsb(hdist, 5) + R._lsb(19 - 4, 4)
    head += "".join(R._lsb(v, 3) for v in [0, 0, 0] + [4] * 16)
    head += "".join(format(l, "04b") for l in ll_len) + "".join(format(l, "04b") for l in d_len[:hdist + 1])
    bits = [head]
    for t in tokens:
        if t.kind != WIN:
            bits.append(code[t.value])
        if t.kind != LIT:
            sym, eb, ev = R.LENGTH[t.length]
            ds, deb, dev = dist_code(t.dist)
            bits.append(code[sym] + R._lsb(ev, eb) + dcode[ds] + R._lsb(dev, deb))
    bits.append(code[R.EOB] + "000")
    return R._pack("".join(bits)) + b"\x00\x00\xff\xff"


def window_size(tokens, ll_len, d_len):
    """len(window_body(...)) from the token bits alone"""
    hdist = max(s for s, l in enumerate(d_len) if l)
    total = R.HEADER_BITS + 4 * hdist
    for t in tokens:
        if t.kind != WIN:
            total += ll_len[t.value]
        if t.kind != LIT:
            sym, eb, _ = R.LENGTH[t.length]
            ds, deb, _ = dist_code(t.dist)
            total += ll_len[sym] + eb + d_len[ds] + deb
    return (total + ll_len[R.EOB] + 3 + 7) // 8 + 4


def padded(nbytes):
    """a chunk of nbytes (lead bytes included) after its 5-byte pads to a multiple of 16"""
    while nbytes % 16:
        nbytes += 5
    return nbytes


MChunk = collections.namedtuple("MChunk", "form pads nbytes tokens rounds data huff_size stored_size offset win_tokens win_size ll_rounds dist_rounds dist_symbols")


def encode_chunk(data, first, rule=RULE, offset=0):
    """(bytes of the chunk in the stream, MChunk report)"""
    data = np.asarray(data, np.uint8)
    run_tokens, run_len, rounds, hsize, ssize = R.chunk_form(data)
    toks = parse(data, rule)
    ll, dd = histograms(toks)
    ll_len, ll_rounds = R.code_lengths(ll)
    d_len, d_rounds = dist_lengths(dd)
    wsize = None if ll_len is None or d_len is None else window_size(toks, ll_len, d_len)
    lead = 2 if first else 0
    form, best = "stored", ssize
    if hsize is not None and hsize < best:
        form, best = "huff", hsize
    if wsize is not None and (padded(lead + wsize) <= padded(lead + best) if rule.tie_window else padded(lead + wsize) < padded(lead + best)):
        form, best = "window", wsize
    body = {"stored": lambda: R.stored_body(data), "huff": lambda: R.huffman_body(run_tokens, run_len), "window": lambda: window_body(toks, ll_len, d_len)}[form]()
    assert len(body) == best
    out = (b"\x78\x01" if first else b"") + body
    pads = 0
    while (len(out) + 5 * pads) % 16:
        pads += 1
    out += R.PAD * pads
    return out, MChunk(form, pads, len(out), run_tokens, rounds, data, hsize, ssize, offset, toks, wsize, ll_rounds, d_rounds, [s for s, c in enumerate(dd) if c])


def filtered(rgba, bpp=4, adaptive=False):
    if adaptive:
        return F.filtered_rows_adaptive(rgba, bpp)
    return R.filtered_rows(rgba) if bpp == 4 else G.filtered_rows_rgb(rgba)


def encode_window(rgba, bpp=4, adaptive=False, rule=RULE):
    """the whole zlib stream of a canvas with the per-chunk report (png_deflate_reference.Encoded of MChunks)"""
    h, w = rgba.shape[:2]
    filt = filtered(rgba, bpp, adaptive)
    cut = R.chunk_bytes if bpp == 4 else G.chunk_bytes_rgb
    parts, chunks, at = [], [], 0
    for k, cell in enumerate(F._grid(w, h, bpp)):
        b, rep = encode_chunk(cut(filt, cell), k == 0, rule, at)
        parts.append(b)
        chunks.append(rep)
        at += len(b)
    raw = filt.tobytes()
    parts.append(b"\x01\x00\x00\xff\xff" + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF))
    return R.Encoded(b"".join(parts), chunks, raw)


def encode_run(rgba, bpp=4, adaptive=False):
    """the default setting's stream of the same canvas (pngMatch 'run'), from the other references"""
    if adaptive:
        return F.encode_adaptive(rgba, bpp)
    return R.encode(rgba) if bpp == 4 else G.encode_rgb(rgba)


def file_bytes_window(rgba, bpp=4, stream=None, adaptive=False):
    """the file of one slab and one IDAT (the device entry points without an IDAT limit)"""
    h, w = rgba.shape[:2]
    data = encode_window(rgba, bpp, adaptive).stream if stream is None else stream
    return F.file_head(w, h, bpp) + R.png_chunk(b"IDAT", data) + R.png_chunk(b"IEND", b"")


def host_file_bytes_window(rgba, bpp=4, rep=None, limit=None, adaptive=False):
    """the file of the host path (encode_png, stitch_png): slabs of 768 and then 4096 chunks, an IDAT per slab"""
    h, w = rgba.shape[:2]
    rep = encode_window(rgba, bpp, adaptive) if rep is None else rep
    sizes = [c.nbytes for c in rep.chunks]
    out, at = F.file_head(w, h, bpp), 0
    for n in R.idat_lengths(sizes, R.idat_limit(limit), R.host_slabs(len(sizes))):
        out += R.png_chunk(b"IDAT", rep.stream[at:at + n])
        at += n
    assert at == len(rep.stream)
    return out + R.png_chunk(b"IEND", b"")
